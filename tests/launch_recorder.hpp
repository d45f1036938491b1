// Force-included (-include) into a host-only compile of the csrc/ launchers by
// tests/test_launch_choice.py: every hipLaunchKernelGGL becomes a record of the
// kernel instantiation, the launch geometry and the arguments, appended to one
// process-wide text buffer that tests/launch_cases.hip reads after each call.
// Nothing is launched and no HIP runtime function is called.
#pragma once
#include <hip/hip_runtime.h>

#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <typeinfo>

namespace launch_rec {

inline std::string &buf() {
    static std::string b;
    return b;
}

template <auto K>
struct RecTag {};

// "launch_rec::RecTag<&invsim::(anonymous namespace)::nv_step1_kernel<5, true, true, invsim::Pcg>>"
// -> "nv_step1_kernel<5, true, true, Pcg>"
template <auto K>
std::string kernel_name() {
    int st = 0;
    char *d = abi::__cxa_demangle(typeid(RecTag<K>).name(), nullptr, nullptr, &st);
    std::string n = d ? d : typeid(RecTag<K>).name();
    free(d);
    const size_t lt = n.find('<');
    if (lt != std::string::npos && !n.empty() && n.back() == '>') n = n.substr(lt + 1, n.size() - lt - 2);
    if (!n.empty() && n[0] == '&') n.erase(0, 1);
    for (const char *cut : {"invsim::(anonymous namespace)::", "invsim::", "__device_stub__"}) {
        const std::string c(cut);
        for (size_t at; (at = n.find(c)) != std::string::npos;) n.erase(at, c.size());
    }
    // an instantiation of a template prints as "(void name<...>(parameter types))"
    if (n.rfind("(void ", 0) == 0) {
        n.erase(0, 6);
        int depth = 0;
        for (size_t i = 0; i < n.size(); i++) {
            depth += n[i] == '<';
            depth -= n[i] == '>';
            if (n[i] == '(' && depth == 0) {
                n.erase(i);
                break;
            }
        }
    }
    return n;
}

// One argument.  Scalars and pointers print their value; a parameter block
// prints the one field a launcher edits in its copy (P<ahead>), a StepIO its K
// (io<K>), a policy its kind (pol<kind>).  (Members are detected, so this header names no project type.)
template <class T, class = void> struct has_ahead : std::false_type {};
template <class T> struct has_ahead<T, std::void_t<decltype(std::declval<T>().ahead)>> : std::true_type {};
template <class T, class = void> struct has_k : std::false_type {};
template <class T> struct has_k<T, std::void_t<decltype(std::declval<T>().K)>> : std::true_type {};
template <class T, class = void> struct has_kind : std::false_type {};
template <class T> struct has_kind<T, std::void_t<decltype(std::declval<T>().kind)>> : std::true_type {};

template <class T>
void put(std::string &o, const T &v) {
    char t[64];
    if constexpr (std::is_pointer_v<T>) {
        snprintf(t, sizeof t, "%llx", (unsigned long long)(uintptr_t)v);
        o += '@';
        o += t;
    } else if constexpr (std::is_floating_point_v<T>) {
        snprintf(t, sizeof t, "%.17g", (double)v);
        o += t;
    } else if constexpr (std::is_unsigned_v<T>) {
        snprintf(t, sizeof t, "%lluu", (unsigned long long)v);
        o += t;
    } else if constexpr (std::is_integral_v<T>) {
        snprintf(t, sizeof t, "%lld", (long long)v);
        o += t;
    } else if constexpr (has_ahead<T>::value) {
        o += "P";
        put(o, v.ahead);
    } else if constexpr (has_k<T>::value) {
        o += "io";
        put(o, v.K);
    } else if constexpr (has_kind<T>::value) {
        o += "pol";
        put(o, v.kind);
    } else {
        o += '?';
    }
}

template <auto K, class... A>
void rec_launch(dim3 g, dim3 b, size_t lds, hipStream_t, const A &...args) {
    std::string &o = buf();
    char t[96];
    o += " | ";
    o += kernel_name<K>();
    snprintf(t, sizeof t, " g=%u b=%u lds=%zu (", g.x, b.x, lds);
    o += t;
    int i = 0;
    ((o += (i++ ? "," : ""), put(o, args)), ...);
    o += ')';
}

}  // namespace launch_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, ...) ::launch_rec::rec_launch<&k>(dim3(g), dim3(b), size_t(l), __VA_ARGS__)
#define hipGetLastError() hipSuccess
