// Host-side launch helpers shared by the env families' launchers: the launch
// geometry, the run-kernel modes, and runtime-to-compile-time dispatch.  No
// device code.
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace invsim {

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// LDS a workgroup can request on gfx950
constexpr size_t LDS_LIMIT_BYTES = 160 * 1024;

// the policy argument of a kernel that takes one by value: the caller's, or zeros
inline const PolicyIO POLICY_NONE{};
inline const PolicyIO &pol_or_none(const PolicyIO *pol) { return pol ? *pol : POLICY_NONE; }

// The lock-step NEXT_STEP reset launch (one open-loop step at t_u >= T, the
// horizon): it resets every env and draws nothing, so it neither reads the
// generator state nor moves the demand stream.
template <class IO>
inline bool lockstep_reset_launch(const PolicyIO *pol, const IO &io, int t_u, int T) {
    return !pol && io.K == 1 && t_u >= T;
}

// What a family's run kernel (nv_run_kernel, im_run_kernel, net_spec_kernel,
// net_run_kernel) is launched for: one open-loop step, K of them, or K steps
// of an in-kernel policy -- the plain instantiation, or one of its compile-time
// variants.  A mode stands for the (ONE, POL, RND, EXT, LVL) template arguments
// that occur; no other combination can be written.
enum class Run { STEP, STEPS, POLICY, RANDOM, EXTERNAL, LEVELS };
template <Run R>
struct RunMode {
    static constexpr bool ONE = R == Run::STEP, POL = R >= Run::POLICY;
    static constexpr bool RND = R == Run::RANDOM, EXT = R == Run::EXTERNAL, LVL = R == Run::LEVELS;
};
inline Run run_mode(const PolicyIO *pol, int K) { return pol ? Run::POLICY : K == 1 ? Run::STEP : Run::STEPS; }
// ... with the policy variants, which are template arguments in every family
// (InvMgmt's variant instantiations are held by objects of their own, each of
// which dispatches over its own mode alone: the end of invmgmt.hip).
// levels_kind: the family's per-env levels policy, or POL_NONE when it has none.
inline Run run_mode_variant(const PolicyIO *pol, int K, int levels_kind) {
    if (pol && pol->kind == POL_RANDOM) return Run::RANDOM;
    if (pol && pol->kind == POL_EXTERNAL) return Run::EXTERNAL;
    if (pol && levels_kind != POL_NONE && pol->kind == levels_kind) return Run::LEVELS;
    return run_mode(pol, K);
}

// Runtime value -> compile-time constant: f(Const<V>{}) for the V of the list
// that equals v, otherwise() when none does.  f and otherwise return hipError_t.
// (In f, read the constant as decltype(c)::value: a type, so nested lambdas need
// no capture of it.)
template <auto V>
using Const = std::integral_constant<decltype(V), V>;
template <auto... Vs>
struct Values {
    template <class T>
    static constexpr bool has(T v) {
        return ((v == Vs) || ...);
    }
};
template <auto... Vs, class T, class F, class Else>
hipError_t dispatch(Values<Vs...>, T v, F &&f, Else &&otherwise) {
    hipError_t e = hipSuccess;
    const bool found = ((v == Vs && ((e = f(Const<Vs>{})), true)) || ...);
    return found ? e : otherwise();
}
template <class F>
hipError_t dispatch_bool(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
inline hipError_t invalid_value() { return hipErrorInvalidValue; }

}  // namespace invsim
