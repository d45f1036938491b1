// InvManagementMasterEnv.step / reset (inventory_management.py:186-352) as
// HIP kernels for gfx950, templated on M1 = m-1 inventory stages (register
// arrays), backlog vs lost sales, and whether the episode period is lock-step
// uniform (TU).
//
// Work layout: one wave = 16 envs x 4 lanes (group_rng.hpp).  The 4 lanes of
// an env run the (cheap, integer) dynamics redundantly, evaluate 4 Poisson
// candidates in parallel, split the observation-window copy, and only the
// group leader writes state.  Observation rows are assembled in an LDS tile
// and written with 16-byte coalesced stores.
//
// Per-env HBM state (SoA rows of Npad, int64 like the reference):
//   I[M1]            on-hand inventory at the start of the period   (:203)
//   B[M1+1]          backlog carried into the period (backlog only)  (:208)
//   Rring[sum L_i]   fulfilled orders R; stage i keeps its last L_i in a ring,
//                    slot t mod L_i = R[t-L_i] = this period's arrival (:275)
//   alog32[D][Npad][M1] requested orders (action_log) ring of D = lt_max rows, 32-bit,
//                    an env's row contiguous
//                    (alog: int64 ring for the rare entries >= 2^32 - 1):
//                    exactly the observation window (:380)
//   period (only when not lock-step), PCG64
// Ring entries older than the episode are masked by the period counter, as the
// reference's zeroed history would be, so reset writes only I, B, period.
//
// A launch runs K >= 1 consecutive steps (invsim_step: K = 1; invsim_rollout:
// K) with PCG64, I, B and the period in registers.
#include "kernels.hpp"
#include "launch.hpp"

// The in-kernel policy variants are trailing template arguments of the policy
// kernels (launch.hpp RunMode), false in every other instantiation:
//   RND  RANDOM (RandomAgent, kernels.hpp ActGen): the dynamics code draws each
//        launch step's order from the env's action generator -- before the
//        reset / overrun branches, so every launch step draws -- instead of
//        asking an agent.  im_run_kernel and the fused rollouts.
//   EXT  EXTERNAL (invsim_rollout_metrics): the policy bookkeeping (metrics,
//        optional outputs) with the caller's action rows (io.act), read as the
//        open-loop path reads them.  im_run_kernel only: the fused rollout
//        kernels have no EXT variant.
//   LVL  LEVELS: BaseStock's inventory position against the env's own
//        order-up-to levels (and optional reorder points) from the attached
//        device arrays instead of one (L + 1) * mu * sf target.  im_run_kernel
//        and the fused rollouts.
// Which instantiations an object holds is decided where the launchers are
// defined, at the end of this file.

namespace invsim {
namespace {

#ifdef INVSIM_TIMING
__device__ uint64_t g_tbuf[TB_WAVES * TB_PROBES];
// im_split_kernel: the time at which a wave holds its first kernel-argument
// values, g_targ[workgroup][0 window wave / lookahead workgroup, 1 dynamics
// wave].  `dep` is an argument-derived scalar: the empty asm needs it in an
// SGPR, so the timestamp follows the wait on the argument loads (if any).
// g_targ[workgroup][2]: when the dynamics wave had issued its state stores.
__device__ uint64_t g_targ[TB_WAVES * 3];
#define TPROBE_ARGS(col, tid, dep)                                                             \
    do {                                                                                       \
        asm volatile("" ::"s"(dep));                                                           \
        if (threadIdx.x == (tid) && blockIdx.x < TB_WAVES)                                     \
            g_targ[blockIdx.x * 3 + (col)] = __builtin_amdgcn_s_memrealtime();                 \
    } while (0)
#define TPROBE_STORES(tid)                                                                     \
    do {                                                                                       \
        if (threadIdx.x == (tid) && blockIdx.x < TB_WAVES)                                     \
            g_targ[blockIdx.x * 3 + 2] = __builtin_amdgcn_s_memrealtime();                     \
    } while (0)
#else
#define TPROBE_ARGS(col, tid, dep) do {} while (0)
#define TPROBE_STORES(tid) do {} while (0)
#endif

// obs-window entries per lane kept in registers: the (lt_max - 1) * M1 entries
// of lt_max <= 10, capped at 36 (longer windows are copied ring -> LDS directly)
// Requested orders are >= 0 (np.maximum(action, 0), :250) and, for any sane
// policy, far below 2^32: the action_log ring keeps 4 bytes per entry, with a
// sentinel sending the rare wider value to the int64 ring (halves the step's
// largest read, the observation window)
constexpr uint32_t IM_WIDE = 0xFFFFFFFFu;

__device__ __forceinline__ int64_t alog_get(const ImParams &P, int64_t idx) {
    const uint32_t v = P.alog32[idx];
    return v == IM_WIDE ? P.alog[idx] : (int64_t)v;
}

constexpr int im_wlane(int m1) { return m1 * (9 < 36 / m1 ? 9 : 36 / m1); }   // whole rows

// numpy int64 array arithmetic wraps around (two's complement)
__device__ __forceinline__ int64_t wrap_add(int64_t a, int64_t b) {
    return (int64_t)((uint64_t)a + (uint64_t)b);
}
__device__ __forceinline__ int64_t wrap_sub(int64_t a, int64_t b) {
    return (int64_t)((uint64_t)a - (uint64_t)b);
}

// np.minimum(int64, float64).astype(int64) for the supplier-inventory cap (:265)
__device__ __forceinline__ int64_t min_via_f64(int64_t a, int64_t sup) {
    const double x = (double)a, y = (double)sup;
    return (int64_t)((x <= y) ? x : y);
}

// The period update (inventory_management.py:250-322), bit-exact, in the three
// pieces the kernels need (im_split_kernel has a barrier between the first two
// and runs the third behind its tile copy): im_orders, im_sales, im_profit.
// im_step_regs and the dynamics waves of im_split_kernel, im_roll3_kernel and
// im_roll3o_kernel all step through these.
//
// Orders (:250-277, :295-304): what does not depend on the demand.  req is
// clamped in place; arrival(i) is R[t - L_i] (0 while t < L_i) and l0(i) says
// whether L_i = 0 (the order arrives in its own period), each kernel's own way:
// ring loads and P.L, or register windows and compile-time lead times.
// Out: R, Icur (before sales), Sv[1..], U[1..].
template <int M1, class ArrF, class L0F>
__device__ __forceinline__ void im_orders(const ImParams &P, int64_t (&req)[M1], const int64_t (&I)[M1],
                                          const int64_t (&B)[M1 + 1], ArrF arrival, L0F l0, int64_t (&R)[M1],
                                          int64_t (&Icur)[M1], int64_t (&Sv)[M1 + 1], int64_t (&U)[M1 + 1]) {
    int64_t ordreq[M1];
#pragma unroll
    for (int i = 0; i < M1; i++) req[i] = req[i] > 0 ? req[i] : 0;  // :250
#pragma unroll
    for (int i = 0; i < M1; i++) {
        ordreq[i] = wrap_add(req[i], B[i + 1]);                     // :253-255
        const int64_t r = ordreq[i] < P.c[i] ? ordreq[i] : P.c[i];  // :263
        // :260-265 np.minimum(., [I[t,1:], inf]) in float64, then astype(int64):
        // the last stage's cap is +inf but the f64 round trip still rounds |r| > 2^53
        R[i] = (i + 1 < M1) ? min_via_f64(r, I[i + 1]) : (int64_t)(double)r;
    }
#pragma unroll
    for (int i = 0; i < M1; i++) Icur[i] = wrap_add(I[i], l0(i) ? R[i] : arrival(i));   // :271-277
#pragma unroll
    for (int i = 1; i < M1; i++) Icur[i] = wrap_sub(Icur[i], R[i]); // :300 (reference quirk, kept)
#pragma unroll
    for (int i = 0; i < M1; i++) {
        Sv[i + 1] = R[i];                                           // :295
        U[i + 1] = wrap_sub(ordreq[i], R[i]);                       // :304
    }
}

// Sales (:284-303): the demand d and the retailer's backlog against its stock
__device__ __forceinline__ void im_sales(int64_t d, int64_t B0, int64_t &Icur0, int64_t &Sv0, int64_t &U0) {
    const int64_t dfill = wrap_add(d, B0);                          // :284-286
    const int64_t s0 = Icur0 < dfill ? Icur0 : dfill;               // :288
    Icur0 = wrap_sub(Icur0, s0);
    Sv0 = s0;
    U0 = wrap_sub(dfill, s0);                                       // :303
}

// Profit (:315-321), undiscounted: the caller multiplies by alpha ** t (:322)
template <int M1>
__device__ __forceinline__ double im_profit(const ImParams &P, const int64_t (&Sv)[M1 + 1], const int64_t (&U)[M1 + 1],
                                            const int64_t (&Icur)[M1]) {
    double term[M1 + 1];
#pragma unroll
    for (int q = 0; q <= M1; q++) {
        const double Sj = (double)Sv[q];
        const int64_t inv = (q < M1) ? Icur[q] : 0;
        const double hold = P.hc[q] * (double)(inv > 0 ? inv : 0);
        term[q] = ((P.up[q] * Sj - P.uc[q] * Sj) - hold) - P.kc[q] * (double)U[q];
    }
    return np_sum<double>(M1 + 1, [&](int q) { return term[q]; });
}

// Step info (:334-345) into the env's record rr: S[t], U[t], then the f64 bits
// of the period_profit, revenue, procurement, holding and penalty sums
template <int M1>
__device__ __forceinline__ void im_info_record(const ImParams &P, int64_t *rr, const int64_t (&Sv)[M1 + 1],
                                               const int64_t (&U)[M1 + 1], const int64_t (&Icur)[M1], double profit) {
#pragma unroll
    for (int q = 0; q <= M1; q++) {
        rr[q] = Sv[q];
        rr[M1 + 1 + q] = U[q];
    }
    const double rev = np_sum<double>(M1 + 1, [&](int q) { return P.up[q] * (double)Sv[q]; });
    const double pro = np_sum<double>(M1 + 1, [&](int q) { return P.uc[q] * (double)Sv[q]; });
    const double hol = np_sum<double>(M1 + 1, [&](int q) {
        const int64_t inv = (q < M1) ? Icur[q] : 0;
        return P.hc[q] * (double)(inv > 0 ? inv : 0);
    });
    const double pen = np_sum<double>(M1 + 1, [&](int q) { return P.kc[q] * (double)U[q]; });
    rr[2 * (M1 + 1) + 0] = __double_as_longlong(profit);
    rr[2 * (M1 + 1) + 1] = __double_as_longlong(rev);
    rr[2 * (M1 + 1) + 2] = __double_as_longlong(pro);
    rr[2 * (M1 + 1) + 3] = __double_as_longlong(hol);
    rr[2 * (M1 + 1) + 4] = __double_as_longlong(pen);
}

// evaluate_agent's per-step sums (benchmark_InvManagementBacklogEnv.py:378-399);
// the caller adds the reward (met[0]) and the step count (met[1])
template <int M1>
__device__ __forceinline__ void im_metric_sums(double *met, int64_t d, int64_t Sv0, int64_t U0,
                                               const int64_t (&Icur)[M1]) {
    met[2] += (double)d;                                            // demand_realized
    met[3] += (double)Sv0;                                          // sales[0]
    met[4] += (double)U0;                                           // unfulfilled[0]
    int64_t es = 0;                                                 // sum(max(0, ending_inventory))
#pragma unroll
    for (int i = 0; i < M1; i++) es = wrap_add(es, Icur[i] > 0 ? Icur[i] : 0);
    met[5] += (double)es;
}

// BaseStockAgent.get_action (benchmark_InvManagementBacklogEnv.py:152-198) for
// one stage: order up to (L + 1) * mu * sf over the inventory position pos (on
// hand + the requested orders of the last L periods, summed by the caller), in
// float64, clipped to [0, c], truncated to int64
__device__ __forceinline__ int64_t im_base_stock_order(const PolicyIO &pol, int L, int64_t pos, int64_t c) {
    const double target = ((double)(L + 1) * pol.mu) * pol.sf;      // (lead_times + 1) * mu * sf
    double x = target - (double)pos;
    x = (x > 0) ? x : 0.0;                                          // np.maximum(0, .)
    x = (x < 0.0) ? 0.0 : x;                                        // np.clip(., low = 0, high = c)
    x = (x > (double)c) ? (double)c : x;
    return (int64_t)x;                                              // astype(int64)
}

// INVSIM_POLICY_LEVELS for one stage (invsim.h): order up to the env's level lv
// over the inventory position pos, only while pos is below the reorder point ro
// (the strict < of the reference's sSPolicyAgent; +inf without reorder points,
// which every (double)pos is below), clipped to [0, c] and truncated as
// im_base_stock_order.  A NaN level or reorder point orders 0.
__device__ __forceinline__ int64_t im_levels_order(double lv, double ro, int64_t pos, int64_t c) {
    double x = lv - (double)pos;
    x = ((double)pos < ro) ? x : 0.0;
    x = (x > 0) ? x : 0.0;
    x = (x > (double)c) ? (double)c : x;
    return (int64_t)x;
}

// An env's row of the attached arrays (row: the env, clamped to N - 1 by the
// caller: the arrays are [N][M1], not padded).  Only a LVL instantiation loads
// it; elsewhere the unused local costs nothing.
template <int M1>
struct ImLevels {
    double lv[M1], ro[M1];
    __device__ __forceinline__ void load(const PolicyIO &pol, int64_t row) {
#pragma unroll
        for (int i = 0; i < M1; i++) lv[i] = pol.levels[row * M1 + i];
#pragma unroll
        for (int i = 0; i < M1; i++) ro[i] = pol.reorder ? pol.reorder[row * M1 + i] : __builtin_huge_val();
    }
};
// Where the row lives in the fused rollout kernels follows the compiler's
// resource report: im_roll3o_kernel's dynamics wave has the registers to keep
// it over the launch's K steps (200 VGPRs at most, no scratch); im_roll3_kernel,
// at its 256-VGPR cap (waves_per_eu(2)), would spill 4 VGPRs (20 B of scratch)
// to hold it, so it reads the row again at the top of every step (cache
// resident after the first) and is back at 254 VGPRs without scratch.

// The PTRS right-hand-side table (or, without one, any valid words) into a
// TableStage bound for dst in LDS: a fixed count of clamped loads, issued in
// front of the caller's other loads and flushed to LDS once those are in flight
__device__ __forceinline__ TableStage im_stage_table(const ImParams &P, double *dst, int lane, bool has_tab) {
    TableStage ts;
    ts.dst = dst;
    const double *tsrc = has_tab ? P.rhs : P.alpha_pow;             // any valid pointer
    const int qm = has_tab ? P.pc.nk - 1 : 0;
#pragma unroll
    for (int u = 0; u < TableStage::NT; u++) ts.v[u] = tsrc[min(lane + u * WAVE, qm)];
    return ts;
}

// The step's state stores (ring rows, action_log row, I, B; ImPending holds the
// first two).  vmcnt counts stores as well as loads on gfx9, so a wait for a
// load issued after a store also waits for that store; the multi-step kernels
// issue the state stores after the obs tile store, where no load follows.
// im_split_kernel's EARLY instantiation (launches of more than
// IM_EARLY_STORES_MIN_N envs) issues them (im_store_rows, as im_flush_pending) as
// soon as the integer dynamics are done, in front of the tile barrier, where
// it would otherwise wait for the window wave, and the f64 reward chain, which
// the tile does not need, runs behind the tile copy.  In the generated gfx950
// code no vmcnt wait stands between the first of those stores and the last
// tile store, except inside the exec-guarded branch that fetches a wide
// entry; the compiler reuses the stores' address and data registers right
// after them with no wait.  Two properties make the early stores safe, and a
// change to the kernel has to keep them:
//   - the window rows whose values are used are ring slots (t+1-n .. t-1) mod D
//     and the action_log row written is slot t mod D, never among them.  The
//     straight-line loads of rows past the last logged one (clamped to rmax:
//     t = 0, or D = 1) may touch slot t mod D, but their values are discarded
//     (entries >= nw are never read from the registers, nor tested for
//     IM_WIDE), whatever they return;
//   - Rring slot t mod L_i is read (this period's arrival) and written (R[t])
//     by the same lane of the same wave, and the load has returned before the
//     dynamics that produce R[t] run (the wave waits for I and B, loaded
//     after the arrivals, and gfx9 loads return in order).  I and B rows
//     likewise: one lane reads, then writes.
template <int M1>
struct ImPending {
    int64_t R[M1], req[M1];
    int t;
};

template <int M1, bool BACKLOG, class G = Pcg>
struct ImState {
    G g;
    uint64_t u32;        // PCG64 32-bit buffer (dist 3 only)
    int64_t I[M1];
    int64_t B[M1 + 1];
};
// ... of a RND instantiation of im_run_kernel: with the env's action generator
// (loaded and stored once per launch, as g) and the launch step's draw.  A
// type of its own and not locals that the other instantiations leave unused:
// an unused local, in the kernel or in im_launch_step, changed the code the
// compiler generates for some of them (register numbers, instruction order).
template <int M1, bool BACKLOG, class G>
struct ImStateRnd : ImState<M1, BACKLOG, G> {
    ActGen ag;
    int64_t act[M1];
};

// reset (:197-220): I = I0, B = 0; obs row = [I0, 0...] (lane j of the group
// writes every 4th element)
template <int M1, bool BACKLOG, class G = Pcg>
__device__ __forceinline__ void im_reset_regs(const ImParams &P, ImState<M1, BACKLOG, G> &s,
                                              int64_t *orow, int j) {
#pragma unroll
    for (int i = 0; i < M1; i++) s.I[i] = P.I0[i];
#pragma unroll
    for (int q = 0; q <= M1; q++) s.B[q] = 0;
    if (orow) {
        const int O = M1 * (P.lt_max + 1);
        for (int q = j; q < O; q += LPE) orow[q] = (q < M1) ? P.I0[q] : 0;
    }
}

// One step (:224-352) at period t < periods.  Returns truncated.
template <int M1, bool BACKLOG, bool NPD, class G = Pcg>
__device__ __forceinline__ bool im_step_regs(const ImParams &P, int64_t e, bool valid, int j, int t,
                                             ImState<M1, BACKLOG, G> &s,
                                             const int64_t *__restrict__ arow, int64_t *orow,
                                             const double *rhs, TableStage *ts, double apow, int64_t udem,
                                             double &reward, int64_t &dem_out, double *met, int64_t *irec,
                                             ImPending<M1> &pend) {
    const int64_t S = P.cm.Npad;
    const int D = P.lt_max;
    const bool leader = valid && j == 0;   // state writes
    // Phase A: every load of the step up front (actions, arrivals, this lane's
    // share of the observation window) so the latency overlaps the demand draw
    int64_t req[M1], R[M1], arr[M1];
#pragma unroll
    for (int i = 0; i < M1; i++) req[i] = arow[i];
#pragma unroll
    for (int i = 0; i < M1; i++) {                                  // arrivals R[t-L_i] (:271-277)
        // unconditional load (row 0 when L = 0: the ring always has a row) so the
        // step's loads are straight-line and their waits exact; masked below
        const int L = P.L[i];
        const int row = L > 0 ? P.ring_off[i] + (int)((uint32_t)t % (uint32_t)L) : 0;
        arr[i] = P.Rring[(int64_t)row * S + e];
        if (!(L > 0 && t >= L)) arr[i] = 0;
    }
    // window rows t+1-n .. t-1 of the action_log ring (:380): nw entries, lane j
    // takes entries q = j, j+4, ...
    const int t1 = t + 1;
    const int n = D > 0 ? (t1 < D ? t1 : D) : 0;
    const int nw = n > 0 ? (n - 1) * M1 : 0;
    const int slot0 = D > 0 ? (int)((uint32_t)(t1 - n) % (uint32_t)D) : 0;
    // action_log ring layout [slot][env][stage]: one env's row of a slot is M1
    // contiguous words, so a window row is one vector load (dwordx3 at M1 = 3)
    auto wrow = [&](int r) -> int64_t {
        int slot = slot0 + r;
        slot = slot >= D ? slot - D : slot;
        return ((int64_t)slot * S + e) * M1;
    };
    auto widx = [&](int q) -> int64_t {
        const int r = q / M1, i = q - r * M1;
        return wrow(r) + i;
    };
    constexpr int WL = im_wlane(M1);
    const bool wreg = orow && (D - 1) * M1 <= WL * LPE;   // launch-uniform
    uint32_t wv[WL];
#ifndef INVSIM_ABL_NO_WINDOW
    {   // unconditional (straight-line loads, exact vmcnt waits): entries past nw
        // (start of an episode) re-read the last valid one, or entry 0, always a
        // valid ring row; unused when !wreg
        static_assert(LPE == 1, "window rows are loaded whole per lane");
        const int rmax = nw > 0 ? nw / M1 - 1 : 0;   // last valid window row
#pragma unroll
        for (int r = 0; r < WL / M1; r++) {
            const uint32_t *src = P.alog32 + wrow(r < rmax ? r : rmax);
#pragma unroll
            for (int i = 0; i < M1; i++) wv[r * M1 + i] = src[i];
        }
    }
#endif
    TPROBE(1);   // step loads issued
    if (ts) ts->flush((int)threadIdx.x);
    // Phase B: demand, a function of the RNG stream only (:172, :280)
#ifdef INVSIM_ABL_NO_POISSON  // profiling ablation build only (wrong results)
    int64_t d = 20 + (int64_t)(s.g.lo & 3);
#else
    s.g.sub(0);
    if constexpr (G::kCounter) s.u32 = 0;    // fast stream: no 32-bit half carried between steps
    int64_t d = NPD ? np_demand(s.g, s.u32, P.nd) : (P.dist == 5) ? udem : env_poisson(s.g, P.pc, rhs);
#endif
    if (d < 0) d = 0;
    TPROBE(2);
    // Phase C: dynamics (identical in the 4 lanes)
    int64_t Icur[M1], Sv[M1 + 1], U[M1 + 1];
    im_orders<M1>(P, req, s.I, s.B, [&](int i) { return arr[i]; }, [&](int i) { return P.L[i] == 0; }, R, Icur, Sv, U);
#pragma unroll
    for (int i = 0; i < M1; i++) pend.R[i] = R[i];                  // ring slot t mod L <- R[t] (:267)
    pend.t = t;
    im_sales(d, s.B[0], Icur[0], Sv[0], U[0]);
    const double profit = im_profit<M1>(P, Sv, U, Icur);
    reward = apow * profit;                                         // :322
    TPROBE(6);
#pragma unroll
    for (int i = 0; i < M1; i++) s.I[i] = Icur[i];                  // :326
#pragma unroll
    for (int q = 0; q <= M1; q++) s.B[q] = BACKLOG ? U[q] : 0;      // :307-312
    dem_out = d;
    if (irec) im_info_record<M1>(P, irec + e * (2 * (M1 + 1) + 5), Sv, U, Icur, profit);
    if (met) im_metric_sums<M1>(met, d, Sv[0], U[0], Icur);
    if (orow) {                                                     // :354-391
        int64_t *w = orow + M1;
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < M1; i++) orow[i] = Icur[i];
        }
        if (D > 0) {
            if (wreg) {
                // branch-free: the WL = (D-1)*M1 oldest slots get the window or 0,
                // then the tail slots are cleared before an early-episode newest row
                bool wide = false;
#pragma unroll
                for (int u = 0; u < WL; u++) {
                    const int q = j + u * LPE;
                    if (q < (D - 1) * M1) w[q] = (q < nw) ? (int64_t)wv[u] : 0;
                    wide |= (q < nw) && wv[u] == IM_WIDE;
                }
                if (wide) {   // rare: entries >= 2^32 - 1 come from the int64 ring
#pragma unroll
                    for (int u = 0; u < WL; u++) {
                        const int q = j + u * LPE;
                        if (q < nw && wv[u] == IM_WIDE) w[q] = P.alog[widx(q)];
                    }
                }
                if (n < D)
                    for (int q = (D - 1) * M1 + j; q < D * M1; q += LPE) w[q] = 0;
            } else {
#ifndef INVSIM_ABL_NO_WINDOW
                for (int q = j; q < nw; q += LPE) w[q] = alog_get(P, widx(q));
#endif
                for (int q = n * M1 + j; q < D * M1; q += LPE) w[q] = 0;
            }
        }
        if (j == 0 && D > 0) {
#pragma unroll
            for (int i = 0; i < M1; i++) w[(n - 1) * M1 + i] = req[i];   // newest row last (:380)
        }
    }
#pragma unroll
    for (int i = 0; i < M1; i++) pend.req[i] = req[i];              // action_log[t] (:268)
    TPROBE(3);
    return t1 >= P.periods;                                         // :350
}

// im_flush_pending's stores with the rows given (im_split_kernel's EARLY
// order works them out during its load phase): R[i] to ring row srow[i] (< 0:
// no ring store, L_i = 0), the requested orders to action_log slot wslot (with
// the int64 side ring for entries >= 2^32 - 1).  The stores are streamed
// (kernels.hpp wt_store), so each is whole lines per wave instruction: a ring
// row 8 B per lane, the action_log row as one store of the env's whole row
// (12 B per lane at M1 = 3, 768 contiguous bytes per wave), the sentinel
// already in place; the side ring's entries, single words of a line under
// their own exec mask, follow as cached stores.  im_flush_pending keeps its
// own body: built on this helper, the run and rollout kernels that use it came
// out with other register and spill figures.  A change to the ring layout has
// to reach both.
template <int M1>
__device__ __forceinline__ void im_store_rows(int64_t *Rring, uint32_t *alog32, int64_t *alog, int64_t S, int D,
                                              const int (&srow)[M1], int wslot, const int64_t (&R)[M1],
                                              const int64_t (&req)[M1], int64_t e) {
#pragma unroll
    for (int i = 0; i < M1; i++)
        if (srow[i] >= 0) wt_store(Rring + (int64_t)srow[i] * S + e, R[i]);
    if (D > 0) {
        uint32_t lo[M1];
        bool wide = false;
#pragma unroll
        for (int i = 0; i < M1; i++) {
            const bool w = req[i] >= (int64_t)IM_WIDE;
            lo[i] = w ? IM_WIDE : (uint32_t)req[i];
            wide |= w;
        }
        const int64_t idx = ((int64_t)wslot * S + e) * M1;
        wt_store_row<M1>(alog32 + idx, lo);
        if (wide) {   // rare, and single words of a line: cached (the row above holds IM_WIDE for them)
#pragma unroll
            for (int i = 0; i < M1; i++)
                if (lo[i] == IM_WIDE) st_store(alog + idx + i, req[i]);
        }
    }
}

template <int M1>
__device__ __forceinline__ void im_flush_pending(const ImParams &P, const ImPending<M1> &pend, int64_t e) {
    const int64_t S = P.cm.Npad;
    const int t = pend.t;
#pragma unroll
    for (int i = 0; i < M1; i++) {
        const int L = P.L[i];
        if (L > 0) st_store(P.Rring + (int64_t)(P.ring_off[i] + (int)((uint32_t)t % (uint32_t)L)) * S + e, pend.R[i]);
    }
    const int D = P.lt_max;
    if (D > 0) {
        const int wslot = (int)((uint32_t)t % (uint32_t)D);
#pragma unroll
        for (int i = 0; i < M1; i++) {
            const int64_t idx = ((int64_t)wslot * S + e) * M1 + i;
            const bool wide = pend.req[i] >= (int64_t)IM_WIDE;
            st_store(P.alog32 + idx, wide ? IM_WIDE : (uint32_t)pend.req[i]);
            if (wide) st_store(P.alog + idx, pend.req[i]);
        }
    }
}

// BaseStockAgent.get_action with the inventory position summed from the
// action_log ring: on hand + the requested orders of the last L_i periods
// (action_log[max(0, t - L_i) : t, i]).  LVL: against the env's own levels.
template <int M1, bool BACKLOG, bool LVL, class G>
__device__ __forceinline__ void im_base_stock(const ImParams &P, const PolicyIO &pol, const ImState<M1, BACKLOG, G> &st,
                                              int t, int64_t e, int64_t (&act)[M1]) {
    const int64_t S = P.cm.Npad;
    const int D = P.lt_max;
    ImLevels<M1> lvl;                                               // (lanes past N: the last env's row)
    if constexpr (LVL) lvl.load(pol, e < P.cm.N ? e : P.cm.N - 1);
#pragma unroll
    for (int i = 0; i < M1; i++) {
        const int L = P.L[i];
        int64_t pos = st.I[i];                                      // observation[:M1] = I[t]
        if (L > 0) {
            int64_t pipe = 0;
            for (int a = 1; a <= L; a++) {
                const int tau = t - a;
                if (tau >= 0)
                    pipe = wrap_add(pipe, alog_get(P, ((int64_t)((uint32_t)tau % (uint32_t)D) * S + e) * M1 + i));
            }
            pos = wrap_add(pos, pipe);
        }
        if constexpr (LVL) act[i] = im_levels_order(lvl.lv[i], lvl.ro[i], pos, P.c[i]);
        else act[i] = im_base_stock_order(pol, L, pos, P.c[i]);
    }
}

// Step k of a launch for the wave's envs: step (or NEXT_STEP reset) into the
// LDS obs tile, SAME_STEP final-obs/reset, then the tile's coalesced store.
// ST: ImState, or ImStateRnd in a RND instantiation.
template <int M1, bool BACKLOG, bool STEP_ONLY, bool POL, bool NPD, bool RND, bool EXT, bool LVL, class ST>
__device__ __forceinline__ void im_launch_step(const ImParams &P, const StepIO<int64_t, int64_t> &io, int k,
                                               int64_t e, int64_t e0, int lane, bool valid, int nvalid,
                                               ST &st, int &t, bool &fault,
                                               int64_t *tile, int64_t *trow, const double *rhs,
                                               TableStage *ts, const double *pre_apow, const int64_t *pre_udem,
                                               const PolicyIO &pol, double *met) {
    const int j = lane & (LPE - 1);
    const bool leader = j == 0;
    const int64_t N = P.cm.N;
    const int O = M1 * (P.lt_max + 1);
    const int64_t oi = (int64_t)k * N + e;
    bool tr = false;
    bool stepped = false;
    double rew = 0.0;
    int64_t dem = 0;
    ImPending<M1> pend;
    if constexpr (RND) {
#pragma unroll
        for (int i = 0; i < M1; i++) st.act[i] = act_draw(st.ag.g, pol.ci[i]);
        if (valid && leader && pol.act_out) {
#pragma unroll
            for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, st.act[i]);
        }
    }
    if (!STEP_ONLY && ts) {   // all lanes write the table before the divergent branch
        ts->flush(lane);
        ts = nullptr;
    }
    if (!STEP_ONLY && t >= P.periods) {
        if (P.cm.autoreset == AR_NEXT_STEP) {
            im_reset_regs<M1, BACKLOG>(P, st, trow, j);
            if (valid && leader && (!POL || io.rew)) {
                out_store(io.rew + oi, 0.0);
                out_store(io.term + oi, (uint8_t)0);
                out_store(io.trunc + oi, (uint8_t)0);
            }
            t = 0;
        } else {
            fault = true;  // stepping past the horizon (reference: IndexError)
        }
    } else {
        // every lane steps (lanes past N read padded state columns and the last
        // env's actions); only valid lanes store
        double r;
        int64_t d;
        const int64_t ea = valid ? oi : (int64_t)k * N + (N - 1);
        // per-period scalars (alpha**t, user_D[t]: always a valid table), loaded
        // before any store of the step (vmcnt counts stores too) unless preloaded
        const double apow = pre_apow ? *pre_apow : P.alpha_pow[t];
        const int64_t udem = pre_udem ? *pre_udem : P.user_D[t];
        const int64_t *arow = io.act + ea * M1;
        int64_t pact[M1];
        if constexpr (RND) {
            arow = st.act;
        } else if constexpr (EXT) {
            // the caller's row, as without a policy
        } else if (POL) {
            if (LVL || pol.kind == POL_BASE_STOCK) {
                im_base_stock<M1, BACKLOG, LVL>(P, pol, st, t, e, pact);
            } else {
#pragma unroll
                for (int i = 0; i < M1; i++) pact[i] = pol.ci[i];
            }
            if (valid && pol.act_out) {
#pragma unroll
                for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, pact[i]);
            }
            arow = pact;
        }
        tr = im_step_regs<M1, BACKLOG, NPD>(P, e, valid, j, t, st, arow, trow, rhs, ts, apow, udem, r, d,
                                            POL ? met : nullptr,
                                            (valid && leader && k == io.K - 1) ? (int64_t *)P.cm.info_rec : nullptr,
                                            pend);
        stepped = true;
        if (POL) {
            met[0] += r;                                            // episode_reward += reward
            met[1] += 1.0;                                          // episode_steps
        }
        rew = r;
        dem = d;
        t += 1;
    }
    wave_lds_sync();
    if (P.cm.autoreset == AR_SAME_STEP) {        // final obs out, then the reset obs in
        if (valid && tr && io.fobs)
            for (int q = j; q < O; q += LPE) io.fobs[e * O + q] = trow[q];
        wave_lds_sync();
        if (tr) {
            im_reset_regs<M1, BACKLOG>(P, st, trow, j);
            t = 0;
        }
        wave_lds_sync();
    }
#ifndef INVSIM_ABL_NO_OBS  // profiling ablation build only
    // obs tile: at most 64 * M1 * 11 int64 in register-window configurations
    if (!POL || io.obs)
        store_tile<(M1 * 11 * EPW * 8 + 16 * WAVE - 1) / (16 * WAVE)>(tile, io.obs + ((int64_t)k * N + e0) * O,
                                                                     (int64_t)nvalid * O, lane);
#endif
    // the step's own stores, after the tile copy (see ImPending)
    if (stepped && valid && leader) {
        im_flush_pending<M1>(P, pend, e);
        if (!POL || io.rew) {
            out_store(io.rew + oi, rew);
            out_store(io.term + oi, (uint8_t)0);
            out_store(io.trunc + oi, (uint8_t)(tr ? 1 : 0));
        }
        if (k == io.K - 1 && P.cm.info_demand) P.cm.info_demand[e] = dem;
    }
    TPROBE(4);
    wave_lds_sync();
}

template <int M1, bool BACKLOG, bool TU, bool ONE, bool POL, bool NPD, class G, bool RND = false, bool EXT = false,
          bool LVL = false>
__global__ void __launch_bounds__(WAVE)
im_run_kernel(ImParams P, int t_u, StepIO<int64_t, int64_t> io, PolicyIO pol) {
    extern __shared__ __attribute__((aligned(16))) int64_t im_tile[];
    const int lane = threadIdx.x;
    const int j = lane & (LPE - 1);
    const bool leader = j == 0;
    const int64_t e0 = (int64_t)blockIdx.x * EPW;
    const int64_t e = e0 + (lane / LPE);
    const int64_t N = P.cm.N;
    const bool valid = e < N;
    const int nvalid = (int)((N - e0) < EPW ? (N - e0) : EPW);
    const int O = M1 * (P.lt_max + 1);
    const int64_t S = P.cm.Npad;
    int64_t *trow = im_tile + (int64_t)(lane / LPE) * O;
    TPROBE(0);
    TPROBE_ID();
    if (ONE && TU && t_u >= P.periods) {
        // lock-step NEXT_STEP autoreset of the whole batch (the host refuses a
        // DISABLED overrun when the period is lock-step, and SAME_STEP resets in
        // the done step): no state to load, so a separate straight path
        if (valid) {
#pragma unroll
            for (int i = 0; i < M1; i++) P.I[i * S + e] = P.I0[i];
            if (BACKLOG) {
#pragma unroll
                for (int q = 0; q <= M1; q++) P.B[q * S + e] = 0;
            }
            out_store(io.rew + e, 0.0);
            out_store(io.term + e, (uint8_t)0);
            out_store(io.trunc + e, (uint8_t)0);
        }
        for (int q = 0; q < O; q++) trow[q] = (q < M1) ? P.I0[q] : 0;
        wave_lds_sync();
        store_tile(im_tile, io.obs + e0 * O, (int64_t)nvalid * O, lane);
        return;
    }
    // PTRS right-hand-side table -> LDS (after the obs tile), so the demand
    // draw's lookups do not queue behind the step's global loads (vmcnt is in order)
    // (fixed count of clamped loads issued first, written to LDS after the state
    // loads are in flight)
    // loads in the order their values are needed: period scalars, RHS table, PCG64, state
    const int t0 = TU ? t_u : (valid ? P.cm.period[e] : 0);   // padded lanes: any in-range period
    const int tc = t0 < P.periods ? t0 : 0;
    const double apow0 = P.alpha_pow[tc];
    const int64_t udem0 = P.user_D[tc];
    double *rhs_l = reinterpret_cast<double *>(im_tile + (int64_t)EPW * O);
    TableStage ts = im_stage_table(P, rhs_l, lane, P.pc.nk > 0);

    // state rows are Npad wide, so every lane loads unconditionally (straight-line
    // loads keep the compiler's vmcnt waits exact); lanes past N take the last
    // env's PCG64 stream (an all-zero stream would never leave the PTRS loop)
    std::conditional_t<RND, ImStateRnd<M1, BACKLOG, G>, ImState<M1, BACKLOG, G>> st;
    P.cm.rng.load(valid ? e : N - 1, st.g);
    st.g.set_step(P.cm.ph_step);
    st.u32 = (NPD && !G::kCounter) ? P.cm.u32buf[valid ? e : N - 1] : 0;
#pragma unroll
    for (int i = 0; i < M1; i++) st.I[i] = P.I[i * S + e];
#pragma unroll
    for (int q = 0; q <= M1; q++) st.B[q] = BACKLOG ? P.B[q * S + e] : 0;
    int t = t0;
    bool fault = false;
    if constexpr (RND) st.ag.load(pol, S, valid ? e : N - 1);
    constexpr int MD = 6;                       // metrics (invsim.h INVSIM_METRICS_*)
    double met[MD];
#pragma unroll
    for (int q = 0; q < MD; q++) met[q] = (POL && pol.metrics) ? pol.metrics[(valid ? e : N - 1) * MD + q] : 0.0;
    if (ONE) {
        im_launch_step<M1, BACKLOG, TU, false, NPD, RND, EXT, LVL>(P, io, 0, e, e0, lane, valid, nvalid, st, t, fault,
                                                                   im_tile, trow, rhs_l, &ts, &apow0, &udem0, pol, met);
    } else {
        ts.flush(lane);
        for (int k = 0; k < io.K; k++) {
            st.g.set_step(P.cm.ph_step + (uint64_t)k);
            im_launch_step<M1, BACKLOG, false, POL, NPD, RND, EXT, LVL>(P, io, k, e, e0, lane, valid, nvalid, st, t, fault,
                                                                        im_tile, trow, rhs_l, nullptr, nullptr, nullptr,
                                                                        pol, met);
        }
    }
    if (valid && leader) {
        P.cm.rng.store_state(e, st.g);
        if (NPD && !G::kCounter) P.cm.u32buf[e] = st.u32;
#pragma unroll
        for (int i = 0; i < M1; i++) st_store(P.I + i * S + e, st.I[i]);
        if (BACKLOG) {
#pragma unroll
            for (int q = 0; q <= M1; q++) st_store(P.B + q * S + e, st.B[q]);
        }
        if (!TU) P.cm.period[e] = t;
        if (fault) atomicOr(P.cm.status, 1u);
        if (POL && pol.metrics) {
#pragma unroll
            for (int q = 0; q < MD; q++) pol.metrics[e * MD + q] = met[q];
        }
        if constexpr (RND) st.ag.store(pol, S, e);
    }
    TWAIT();
    TPROBE(5);
}

template <int M1, bool BACKLOG>
__global__ void __launch_bounds__(256)
im_reset_kernel(ImParams P, const uint8_t *__restrict__ mask, int64_t *__restrict__ obs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.cm.N) return;
    if (mask && !mask[e]) return;
    const int64_t S = P.cm.Npad;
    const int O = M1 * (P.lt_max + 1);
#pragma unroll
    for (int i = 0; i < M1; i++) P.I[i * S + e] = P.I0[i];
    if (BACKLOG) {
#pragma unroll
        for (int q = 0; q <= M1; q++) P.B[q * S + e] = 0;
    }
    P.cm.period[e] = 0;
    if (obs) {
        int64_t *orow = obs + e * O;
        for (int q = 0; q < O; q++) orow[q] = (q < M1) ? P.I0[q] : 0;
    }
}

// Cross-wave LDS handoff inside a workgroup: orders LDS traffic only (an
// __syncthreads() would also drain each wave's outstanding global loads and
// stores, s_waitcnt vmcnt(0), before the s_barrier)
__device__ __forceinline__ void wg_lds_sync() {
    TBAR_T0();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    TBAR_ADD();
}

// Single lock-step step (invsim_step, K = 1, t_u < periods, no SAME_STEP reset
// in this step) with the work of 64 envs split over two waves of one
// workgroup:
//   wave 0 (window)   the observation window rows t+1-n .. t-1 of the action_log
//                     ring into the LDS tile, and this step's demand d
//   wave 1 (dynamics) actions, arrivals, I, B; the demand-independent part of
//                     the dynamics, then (after the handoff of d through LDS)
//                     sales, backlog, reward, the tile's inventory and newest
//                     action row, and the state / output stores
// Both waves then store half of the observation tile.
// With the lookahead (AHEAD) the dynamics wave loads d from the cache itself,
// so it computes as soon as its own loads land, and the waves meet only once,
// when the tile is complete (the window wave leaves the newest row's words to
// the dynamics wave).
//
// Demand lookahead (P.ahead: two slots of [state hi, state lo, demand, 32-bit
// buffer] x Npad, alternating per launch).  The demand is a function of the
// env's generator stream only, so each launch also draws the NEXT step's
// demand.  AHEAD (slot `cur` holds every env's state one draw past the
// committed one, and that draw): wave 0 just loads d, and `gla` extra
// workgroups at the front of the grid (128 envs each, no barriers) draw the
// next demand from slot cur's state and write it to slot cur ^ 1 -- so the
// Poisson chain (~2.5 us) runs beside the step instead of before it.
// !AHEAD (first step after a seed / set_state / other kernel): wave 0 draws d
// inline from cm.rng, stores that state to slot cur, then draws the lookahead
// into slot cur ^ 1.  Either way every stream is consumed in the reference's
// order.  The committed state (after this step's draw) is left in slot cur,
// which the host flips to `cur ^ 1` of the new current slot; cm.rng is brought
// up to date from it (im_commit_kernel) only before something reads it: another
// kernel, get_state, a masked seed.
// RG = PhiloxGen (the fast stream, invmgmt_ph.hip): the same lookahead, but a
// draw is a function of (key, launch step) only, so the cache holds just the
// next step's demand (row 2 of a slot) and no generator state is read or written.
//
// Arguments.  The first eight (14 dwords: IM_HOT_DWORDS, the Makefile's
// -amdgpu-kernarg-preload-count) are what a wave needs to pick its role and to
// form the addresses of its up-front loads; as leading scalar parameters they
// are in SGPRs when the wave starts (kernarg preload), so its first vector
// loads wait for no scalar load.  A struct parameter is never preloaded, hence
// no struct here.  In front of those loads the source uses no P field on the
// packed path, no value behind a pointer and no blockDim / gridDim (the hidden
// argument block).  The generated code still has one scalar-memory wait
// there: `hot ? f(hw) : g(P, t, n, nw)` below is compiled to selects, so every
// wave issues the s_loads of P.lt_max, t and n / nw at entry and waits for
// them (s_waitcnt lgkmcnt(0)) before the first select.  Writing the two
// derivations as two branches was measured and not kept: the loads of t and
// n / nw stay at entry (later code needs them), the register allocator puts a
// packed-path value into the unused fourth dword of their destination, and
// the wait moves into the packed arm; headline +0.1 % alone, -0.6 % on top of
// the streamed state stores, both inside the spread
// (profiles/state_writeback/table.md).
//   act, Ip, Bp, Rr, a32   io.act, P.I, P.B, P.Rring, P.alog32
//   Acur                   the current lookahead slot (P.ahead + cur * 4 * Npad), or null
//   n32                    N (the row stride follows: pad_n); the lookahead
//                          workgroups are the first ceil(N / 128) of an AHEAD grid
//   hw                     ImHot: the window's first ring slot, last logged row and
//                          depth, and the three arrival ring rows, packed by the
//                          host (im_split_args); 0 = not packable, derive from P
// Behind P, by value, what the host knows at launch: alpha ** t (apow), the
// window's rows and logged entries (n, nw), the truncation flag (t + 1 >= periods).
//
// im_split_waves: the waves per SIMD the register allocator must keep (1 = no
// request, as without the attribute).  With the leading arguments held in
// SGPRs one shape fell an occupancy step below what it had with all arguments
// loaded late (2 stages, dist 2-4, lookahead hit, PCG64: 97 VGPRs for 96);
// asking for that step keeps it, with no scratch (91 VGPRs).  The same request
// for the 6-stage backlog inline-draw variants or the Philox 2-stage ones
// only moved registers into scratch, so they carry none.
constexpr int im_split_waves(int m1, bool npd, bool ahead, bool counter) {
    return (m1 == 2 && npd && ahead && !counter) ? 5 : 1;
}
// EARLY (im_split_kernel): the dynamics wave issues its state stores in front
// of the tile barrier and computes the reward behind the tile copy.  The host
// picks that instantiation for lookahead steps of more than this many envs.
// With more than two step workgroups per CU (256 CUs x 2 x 64 envs) the launch
// ends at the plain-store rate and the dynamics wave idles at the barrier, so
// stores issued there are free; with two or fewer the step is one wave's
// load -> compute -> store chain, nothing waits at the barrier, and stores in
// front of it only delay the window wave's tile half (+6 % at 32 768 envs when
// tried).  !EARLY is the order the kernel always had.  The inline-draw step
// (!AHEAD, once after a seed or a set_state) keeps it at every size.
// profiles/early_stores/table.md
// The EARLY instantiations also stream the state they store early (wt_store:
// the dynamics wave's ring rows, action_log row, I and B, and the lookahead
// workgroups' rows of the next slot), which are issued around the middle of
// the wave's span and so can leave L2 before the kernel ends; 7.6 MB less to
// write back at the end of the headline's launch, +3.7 % on the step.
// Nothing in the launch reads these rows after they are written, and the
// next launch reads them from memory whichever XCD it runs on.
// profiles/state_writeback/table.md
constexpr int IM_EARLY_STORES_MIN_N = 32768;
template <int M1, bool BACKLOG, bool NPD, bool AHEAD, class RG = Pcg, bool EARLY = false>
__global__ void __launch_bounds__(2 * WAVE)
    __attribute__((amdgpu_waves_per_eu(im_split_waves(M1, NPD, AHEAD, RG::kCounter))))
im_split_kernel(const int64_t *act, int64_t *Ip, int64_t *Bp, const int64_t *Rr, const uint32_t *a32, uint64_t *Acur,
                int32_t n32, uint32_t hw, ImParams P, int t, StepIO<int64_t, int64_t> io, int cur, double apow,
                int n, int nw, int trunc) {
    extern __shared__ __attribute__((aligned(16))) int64_t im_tile[];
    const int64_t N = n32;
    const int64_t S = pad_n(N);
    const int la0 = 0;                                   // the lookahead workgroups lead the grid
    const int gla = AHEAD ? (int)((n32 + 2 * WAVE - 1) / (2 * WAVE)) : 0;
    // what the load addresses need, from the packed word (ImHot, M1 = 3) or,
    // where the host could not pack it, derived as the host does (im_split_args):
    //   D      window depth (P.lt_max)
    //   slot0  ring slot of the window's first row, (t + 1 - n) mod D
    //   rmax   last window row that holds a logged order
    //   arrival_row(i)  R-ring row of stage i's arrival, ring_off[i] + t mod L[i],
    //                   or -1: nothing arrives (L[i] = 0, or t < L[i])
    const bool hot = M1 == ImHot::M1 && __builtin_expect(ImHot::packed(hw), 1);
    const int D = hot ? ImHot::depth(hw) : P.lt_max;
    const int slot0 = hot ? ImHot::slot0(hw) : D > 0 ? (int)((uint32_t)(t + 1 - n) % (uint32_t)D) : 0;
    const int rmax = hot ? ImHot::rmax(hw) : nw > 0 ? nw / M1 - 1 : 0;
    auto arrival_row = [&](int i) -> int {
        if (hot) return ImHot::row(hw, i) == ImHot::NOARR ? -1 : ImHot::row(hw, i);
        const int L = P.L[i];
        return (L > 0 && t >= L) ? P.ring_off[i] + (int)((uint32_t)t % (uint32_t)L) : -1;
    };
    double *rhs_l = reinterpret_cast<double *>(im_tile + (int64_t)WAVE * M1 * (D + 1));
    // the other lookahead slot (a P field and an argument behind P: formed where it is stored to)
    auto anxt = [&]() -> uint64_t * { return P.ahead ? P.ahead + (int64_t)(cur ^ 1) * 4 * S : nullptr; };
    auto stage_table = [&](int lane) { return im_stage_table(P, rhs_l, lane, P.pc.nk > 0 && P.dist == 1); };
    auto draw = [&](auto &g, uint64_t &u32) -> int64_t {
#ifdef INVSIM_ABL_NO_POISSON  // profiling ablation build only (wrong results)
        int64_t x = 20 + (int64_t)(g.lo & 3);
        g.next64();
#else
        int64_t x = NPD ? np_demand(g, u32, P.nd) : (P.dist == 5) ? P.user_D[t] : env_poisson(g, P.pc, rhs_l);
#endif
        return x < 0 ? 0 : x;
    };
    // the lookahead workgroups' stores into the next slot: streamed in the EARLY
    // instantiations (kernels.hpp wt_store: 8 bytes per lane, whole lines per wave)
    auto la_store = [](uint64_t *p, uint64_t v) {
        if constexpr (EARLY) wt_store(p, v);
        else st_store(p, v);
    };
    // DEC: with the lookahead the dynamics wave loads d itself and the waves
    // meet once (tile complete); otherwise d is handed over at a first barrier
    constexpr bool DEC = AHEAD;
    const int bid = (int)blockIdx.x;
    TPROBE(0);
    TPROBE_ID();
    if (AHEAD && bid >= la0 && bid < la0 + gla) {   // ---- lookahead workgroup: 128 envs, one per lane
        TPROBE_ARGS(0, 0, (int)N + gla);
        const int64_t e = (int64_t)(bid - la0) * (2 * WAVE) + threadIdx.x;
        const bool valid = e < N;
        const int64_t ee = valid ? e : N - 1;
        TableStage ts;
        if constexpr (RG::kCounter) {   // the fast stream: the draw of launch step ph_step + 1
            ts = stage_table((int)(threadIdx.x & (WAVE - 1)));
            RG g;
            P.cm.rng.load(ee, g);
            g.set_step(P.cm.ph_step + 1);
            g.sub(0);
            uint64_t u32 = 0;
            ts.flush((int)(threadIdx.x & (WAVE - 1)));
            const int64_t dn = draw(g, u32);
            if (valid) la_store(anxt() + 2 * S + e, (uint64_t)dn);
            return;
        }
        // the slot's rows first: their addresses come from the leading arguments
        // alone; the increments' pointers and the table's are P fields (they
        // do not fit into the 14 dwords)
        Pcg g;
        g.hi = Acur[ee];
        g.lo = Acur[S + ee];
        uint64_t u32 = NPD ? Acur[3 * S + ee] : 0;
        ts = stage_table((int)(threadIdx.x & (WAVE - 1)));
        g.inc_hi = P.cm.rng.inc_hi[ee];
        g.inc_lo = P.cm.rng.inc_lo[ee];
        PtrsJumpLane jt;
        jt.load((int)(threadIdx.x & (WAVE - 1)));
        ts.flush((int)(threadIdx.x & (WAVE - 1)));   // each wave writes the whole (identical) table
        TPROBE(1);
        // slot cur keeps this state: the committed one once the slots flip
        int64_t dn;
#ifndef INVSIM_ABL_NO_POISSON
        if (!NPD && P.dist == 1 && P.pc.lam >= 10)   // PTRS with a compacted second round
            dn = np_poisson_ptrs_compact(
                g, P.pc, RhsTab{rhs_l}, true, jt,
                [](const PtrsConst &c, int) { return c; });
        else
#endif
            dn = draw(g, u32);
        TPROBE(2);
        if (valid) {
            uint64_t *const Anxt = anxt();
            la_store(Anxt + e, g.hi);
            la_store(Anxt + S + e, g.lo);
            la_store(Anxt + 2 * S + e, (uint64_t)dn);
            if (NPD) la_store(Anxt + 3 * S + e, u32);
        }
        TWAIT();
        TPROBE(5);
        return;
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const bool demand_wave = threadIdx.x < WAVE;
    const int64_t e0 = (int64_t)(AHEAD && bid >= la0 ? bid - gla : bid) * WAVE;
    const int64_t e = e0 + lane;
    const bool valid = e < N;
    const int nvalid = (int)((N - e0) < WAVE ? (N - e0) : WAVE);
    const int O = M1 * (D + 1);
    int64_t *trow = im_tile + (int64_t)lane * O;
    int64_t *w = trow + M1;
    int64_t *dsh = reinterpret_cast<int64_t *>(rhs_l + RHS_LDS_MAX);
    // the tile halves each wave stores (16-byte aligned: an even int64 count)
    const int64_t tcount = (int64_t)nvalid * O;
    const int64_t thalf = ((tcount / 2) + 1) & ~(int64_t)1;
    constexpr int WL = im_wlane(M1);
    const bool wreg = (D - 1) * M1 <= WL;   // launch-uniform
    // window rows t+1-n .. t-1 (:380), loaded whole (see im_step_regs)
    auto wrow = [&](int r) -> int64_t {
        int slot = slot0 + r;
        slot = slot >= D ? slot - D : slot;
        return ((int64_t)slot * S + e) * M1;
    };
    // DEC with a register window: the dynamics wave, whose own loads land
    // ~1.4 us before the window wave's (profiles/r06/split_dec), loads the
    // window rows RW .. RWN-1 and writes their tile words; the window wave the
    // rest.  RW = 6 of 9 measured fastest (Backlog 65 536 8.13 -> 7.81 us,
    // LostSales 32 768 6.19 -> 5.99 us; RW = 4, 5, 7 in between).  rmax: the last row that holds a logged order (earlier periods
    // re-read it: straight-line loads, entries past nw unused)
#ifndef INVSIM_IM_SPLIT_RW
#define INVSIM_IM_SPLIT_RW 6
#endif
    constexpr int RWN = WL / M1;
    constexpr int RW = INVSIM_IM_SPLIT_RW < RWN ? INVSIM_IM_SPLIT_RW : RWN;
    constexpr int WD = (RWN - RW) * M1 > 0 ? (RWN - RW) * M1 : 1;
    const bool wsplit = DEC && wreg && RW < RWN;
    const int u_dyn = wsplit ? RW * M1 : WL;   // log entries u_dyn <= u < nw: the dynamics wave's
    if (demand_wave) {
        TPROBE_ARGS(0, 0, (int)N + gla);
        const int64_t ee = valid ? e : N - 1;        // padded lanes: the last env's stream
        TableStage ts;
        RG g;
        uint64_t u32 = 0;
        int64_t d = 0;
        if (AHEAD) {
            if (!DEC) d = (int64_t)Acur[2 * S + ee];   // (DEC: the dynamics wave loads it)
        } else {
            ts = stage_table(lane);
            P.cm.rng.load(ee, g);
            g.set_step(P.cm.ph_step);
            g.sub(0);
            if (NPD && !RG::kCounter) u32 = P.cm.u32buf[ee];
        }
        uint32_t wv[WL];
        {
#pragma unroll
            for (int r = 0; r < RWN; r++) {
#ifdef INVSIM_ABL_NO_WINDOW   // profiling ablation build only (wrong results): no window read
#pragma unroll
                for (int i = 0; i < M1; i++) wv[r * M1 + i] = (uint32_t)(r + i);
#else
                if (r < RW || !wsplit) {
                    const uint32_t *src = a32 + wrow(r < rmax ? r : rmax);
#pragma unroll
                    for (int i = 0; i < M1; i++) wv[r * M1 + i] = src[i];
                } else {
#pragma unroll
                    for (int i = 0; i < M1; i++) wv[r * M1 + i] = 0;   // (the dynamics wave's rows)
                }
#endif
            }
        }
        if (!AHEAD) {
            ts.flush(lane);
            d = draw(g, u32);
        }
        if (!DEC) dsh[lane] = d;
        if (D > 0) {   // the window part of the obs rows; the newest row is the dynamics wave's
            if (wreg) {
                bool wide = false;
#pragma unroll
                for (int u = 0; u < WL; u++) {
                    // (not the newest row, nw .. nw + M1 - 1: the dynamics wave
                    // writes it, with no barrier in between under DEC)
                    // (nor the log entries u_dyn .. nw - 1: the dynamics wave's under wsplit)
                    if (u < (D - 1) * M1 && !(u >= nw && u < nw + M1) && !(u >= u_dyn && u < nw))
                        w[u] = (u < nw) ? (int64_t)wv[u] : 0;
                    wide |= (u < nw) && (u < u_dyn) && wv[u] == IM_WIDE;
                }
                if (wide) {
#pragma unroll
                    for (int u = 0; u < WL; u++)
                        if (u < nw && u < u_dyn && wv[u] == IM_WIDE) w[u] = P.alog[wrow(u / M1) + u % M1];
                }
                if (n < D)
                    for (int q = (D - 1) * M1; q < D * M1; q++) w[q] = 0;
            } else {
                for (int q = 0; q < nw; q++) w[q] = alog_get(P, wrow(q / M1) + q % M1);
                for (int q = n * M1; q < D * M1; q++) w[q] = 0;
            }
        }
        if (!DEC) wg_lds_sync();   // d -> dynamics wave
        if (DEC) TWAIT();  // (TIMING build: probe 6 after the window rows land)
        TPROBE(6);       // the window wave past its first barrier (DEC: window rows in)
        if constexpr (!RG::kCounter) {
            if (!AHEAD && valid) {   // committed generator state: after this step's draw
                if (Acur) {          // into slot cur (the committed slot once the slots flip)
                    st_store(Acur + e, g.hi);
                    st_store(Acur + S + e, g.lo);
                    if (NPD) st_store(Acur + 3 * S + e, u32);
                } else {
                    P.cm.rng.store_state(e, g);
                    if (NPD) P.cm.u32buf[e] = u32;
                }
            }
        }
        wg_lds_sync();   // tile complete
        store_tile<(M1 * 11 * WAVE * 8 / 2 + 16 * WAVE - 1) / (16 * WAVE)>(im_tile, io.obs + e0 * O,
                                                                          thalf < tcount ? thalf : tcount, lane);
        uint64_t *const Anxt = AHEAD ? nullptr : anxt();
        if (!AHEAD && Anxt) {    // lookahead after an inline draw (first step after invalidation)
            if constexpr (RG::kCounter) {
                g.set_step(P.cm.ph_step + 1);
                g.sub(0);
                u32 = 0;
            }
            const int64_t dn = draw(g, u32);
            if (valid) {
                if constexpr (!RG::kCounter) {
                    st_store(Anxt + e, g.hi);
                    st_store(Anxt + S + e, g.lo);
                    if (NPD) st_store(Anxt + 3 * S + e, u32);
                }
                st_store(Anxt + 2 * S + e, (uint64_t)dn);
            }
        }
        TWAIT();
        TPROBE(5);   // the window wave's exit
        return;
    }
    // ---- dynamics wave
    TPROBE_AT(3, WAVE);
    TPROBE_ARGS(1, WAVE, (int)N + gla);
    const int64_t *arow = act + (valid ? e : N - 1) * M1;
    int64_t req[M1], arr[M1], I[M1], B[M1 + 1];
    // DEC: this step's demand straight from the lookahead slot, so the dynamics
    // wave does not wait for the window wave's loads before its arithmetic
    const int64_t d_ahead = DEC ? (int64_t)Acur[2 * S + (valid ? e : N - 1)] : 0;
    uint32_t wd[WD];   // wsplit: window rows RW .. RWN-1
    if (wsplit) {
#pragma unroll
        for (int r = RW; r < RWN; r++) {
#ifdef INVSIM_ABL_NO_WINDOW
#pragma unroll
            for (int i = 0; i < M1; i++) wd[(r - RW) * M1 + i] = (uint32_t)(r + i);
#else
            const uint32_t *src = a32 + wrow(r < rmax ? r : rmax);
#pragma unroll
            for (int i = 0; i < M1; i++) wd[(r - RW) * M1 + i] = src[i];
#endif
        }
    }
#pragma unroll
    for (int i = 0; i < M1; i++) req[i] = arow[i];
#pragma unroll
    for (int i = 0; i < M1; i++) {                                  // arrivals R[t-L_i] (:271-277)
        const int row = arrival_row(i);
        const bool none = row < 0;                                  // (then any valid row, unused)
        arr[i] = Rr[(int64_t)(none ? 0 : row) * S + e];
        if (none) arr[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < M1; i++) I[i] = Ip[i * S + e];
#pragma unroll
    for (int q = 0; q <= M1; q++) B[q] = BACKLOG ? Bp[q * S + e] : 0;
    // episode sink (kernels.hpp EpSink): the running return and the group's
    // partials are loaded with the step's other loads (behind them: the sink's
    // pointers are P fields)
    double *const ep_part = P.cm.ep_ret ? P.cm.ep_part + 4 * (e0 / WAVE) : nullptr;
    EpPart epp;
    double ep_r = 0.0;
    if (ep_part) {
        epp.load(ep_part);
        ep_r = P.cm.ep_ret[valid ? e : N - 1];
    }
    // EARLY: where this step's ring and action_log stores go (im_store_rows),
    // worked out while the loads are in flight so that no division stands
    // between the dynamics and the stores: stage i's R[t] goes to ring slot
    // t mod L_i, the row its arrival was read from (t < L_i: slot t, nothing
    // arrived yet; L_i = 0: no ring store), and action_log[t] to slot t mod D,
    // the one after the window's n - 1 logged rows
    int srow[M1];
    int wslot = 0;
    int64_t *alogw = nullptr;
    if constexpr (EARLY) {
#pragma unroll
        for (int i = 0; i < M1; i++) {
            const int row = arrival_row(i);
            srow[i] = row >= 0 ? row : P.L[i] > 0 ? P.ring_off[i] + t : -1;
        }
        wslot = slot0 + n - 1;
        wslot = wslot >= D ? wslot - D : wslot;
        alogw = P.alog;
    }
    int64_t R[M1], Icur[M1], Sv[M1 + 1], U[M1 + 1];
    im_orders<M1>(P, req, I, B, [&](int i) { return arr[i]; }, [&](int i) { return P.L[i] == 0; }, R, Icur, Sv, U);
    if (!DEC) wg_lds_sync();   // d from the demand wave
    if (DEC) TWAIT();     // (TIMING build: probe 1 after the loads land)
    TPROBE_AT(1, WAVE);   // the dynamics wave: loads in, d handed over
    const int64_t d = DEC ? d_ahead : dsh[lane];
    im_sales(d, B[0], Icur[0], Sv[0], U[0]);
    // the reward (:315-322); nothing in the obs tile needs it
    double profit = 0.0, reward = 0.0;
    auto reward_chain = [&]() {
        profit = im_profit<M1>(P, Sv, U, Icur);
        reward = apow * profit;                                     // :322
    };
    auto info_record = [&]() {
        if (P.cm.info_rec) im_info_record<M1>(P, (int64_t *)P.cm.info_rec + e * (2 * (M1 + 1) + 5), Sv, U, Icur, profit);
    };
    auto tile_half = [&]() {
        const int64_t h = thalf < tcount ? thalf : tcount;
        if (tcount > h)
            store_tile<(M1 * 11 * WAVE * 8 / 2 + 16 * WAVE - 1) / (16 * WAVE)>(im_tile + h, io.obs + e0 * O + h,
                                                                              tcount - h, lane);
    };
    if constexpr (EARLY) {
        // The state stores in front of the tile barrier (see ImPending): each is
        // whole 128-byte lines from one wave instruction (streamed: wt_store),
        // and the wave would otherwise idle here until the window wave's rows
        // have landed.
        // Nothing between here and the tile copy writes a register they read.
        if (valid) {
            im_store_rows<M1>(const_cast<int64_t *>(Rr), const_cast<uint32_t *>(a32), alogw, S, D, srow, wslot, R, req,
                              e);   // Rr, a32: P.Rring, P.alog32
#pragma unroll
            for (int i = 0; i < M1; i++) wt_store(Ip + i * S + e, Icur[i]);   // :326
            if (BACKLOG) {
#pragma unroll
                for (int q = 0; q <= M1; q++) wt_store(Bp + q * S + e, U[q]);   // :307-312
            }
            out_store(io.term + e, (uint8_t)0);
            out_store(io.trunc + e, (uint8_t)(trunc ? 1 : 0));   // :350
        }
        TPROBE_STORES(WAVE);   // the dynamics wave: state stores issued
#pragma unroll
        for (int i = 0; i < M1; i++) trow[i] = Icur[i];                 // obs (:354-391)
        if (D > 0) {
#pragma unroll
            for (int i = 0; i < M1; i++) w[(n - 1) * M1 + i] = req[i];  // newest row last (:380)
        }
        if (wsplit) {   // its window rows
            bool wide = false;
#pragma unroll
            for (int j = 0; j < (RWN - RW) * M1; j++) {
                const int u = RW * M1 + j;
                if (u < nw) w[u] = (int64_t)wd[j];
                wide |= (u < nw) && wd[j] == IM_WIDE;
            }
            // an entry >= 2^32 - 1 from the int64 side ring: in a branch of its
            // own, as in the window wave, so that the wait for these loads (a
            // vmcnt wait, which would cover the state stores above) is only
            // reached by a wave that holds such an entry
            if (wide) {
#pragma unroll
                for (int j = 0; j < (RWN - RW) * M1; j++) {
                    const int u = RW * M1 + j;
                    if (u < nw && wd[j] == IM_WIDE) w[u] = alogw[wrow(u / M1) + u % M1];
                }
            }
        }
        wg_lds_sync();   // tile complete
        TPROBE_AT(2, WAVE);   // the dynamics wave: past the tile barrier, its tile half next
        tile_half();
        // the reward behind the tile copy: in front of the barrier the f64 chain
        // would hold up the window wave's tile half as well (the dynamics wave is
        // the later of the two there once it issues its state stores first)
        reward_chain();
        if (valid) {
            out_store(io.rew + e, reward);
            info_record();
            if (P.cm.info_demand) P.cm.info_demand[e] = d;
        }
    } else {
        // launches of at most IM_EARLY_STORES_MIN_N envs: the state stores after
        // the tile store (see ImPending)
        reward_chain();
        TPROBE_STORES(WAVE);   // (the reward computed)
#pragma unroll
        for (int i = 0; i < M1; i++) trow[i] = Icur[i];                 // obs (:354-391)
        if (D > 0) {
#pragma unroll
            for (int i = 0; i < M1; i++) w[(n - 1) * M1 + i] = req[i];  // newest row last (:380)
        }
        if (wsplit) {   // its window rows (an entry >= 2^32 - 1 from the int64 side ring)
#pragma unroll
            for (int j = 0; j < (RWN - RW) * M1; j++) {
                const int u = RW * M1 + j;
                if (u < nw) w[u] = wd[j] == IM_WIDE ? P.alog[wrow(u / M1) + u % M1] : (int64_t)wd[j];
            }
        }
        wg_lds_sync();   // tile complete
        TPROBE_AT(2, WAVE);   // the dynamics wave: step computed, stores next
        tile_half();
        if (valid) {
            info_record();
            ImPending<M1> pend;
#pragma unroll
            for (int i = 0; i < M1; i++) {
                pend.R[i] = R[i];                                           // ring slot t mod L <- R[t] (:267)
                pend.req[i] = req[i];                                       // action_log[t] (:268)
            }
            pend.t = t;
            im_flush_pending<M1>(P, pend, e);
            out_store(io.rew + e, reward);
            out_store(io.term + e, (uint8_t)0);
            out_store(io.trunc + e, (uint8_t)(trunc ? 1 : 0));   // :350
            if (P.cm.info_demand) P.cm.info_demand[e] = d;
#pragma unroll
            for (int i = 0; i < M1; i++) st_store(Ip + i * S + e, Icur[i]);   // :326
            if (BACKLOG) {
#pragma unroll
                for (int q = 0; q <= M1; q++) st_store(Bp + q * S + e, U[q]);   // :307-312
            }
        }
    }
    if (ep_part) {   // after the stores: the butterfly runs while they drain
        EpLane a;
        if (valid) {
            a.r = ep_r;
            a.add(reward, trunc != 0);                    // terminated is always False (:350)
            P.cm.ep_ret[e] = a.r;
        }
        epp.flush(ep_part, a, trunc != 0, lane);
    }
    TWAIT();
    TPROBE_AT(4, WAVE);   // the dynamics wave's exit (probe 3: its entry)
}

// K-step lock-step rollout (invsim_rollout, NEXT_STEP or DISABLED autoreset,
// Poisson demand) for 3 stages with compile-time lead times L0..L2 (the
// reference default [1, 5, 10]), one 128-thread workgroup per 64 envs:
//   wave 0 (demand)   draws the demands into an LDS ring of RD chunks of CH
//                     launch steps, ahead of the dynamics wave, as a flat
//                     per-lane loop (stream_flat_loop); a demand is a function
//                     of the env's stream only, and a NEXT_STEP reset step
//                     draws nothing (reset(), :186-222)
//   wave 1 (dynamics) the step (:224-352) with every window in registers,
//                     aligned by age: the fulfilled-order history of stage i
//                     (rw_i[a] = R[t - L_i + a], so the arrival is rw_i[0]) and
//                     the requested-order rows of the observation window
//                     (wv[a] = action_log[t - (D - 1) + a]).  A step reads only
//                     its actions (prefetched a step ahead) and writes the obs
//                     tile, reward, flags and the new ring slots (so the rings
//                     stay exact for every other kernel).
// Chunk handoff (c = 0, 1, ...): the demand wave fills buffer c & 1, then
// barrier c; the dynamics wave consumes chunk c after barrier c, so the
// demand wave's refill of a buffer follows the dynamics wave's use of it.
// The demand wave of the rollout kernels (stream_flat_loop): Poisson demand
// (:280) of each launch step into the ring dbuf [RD * CH][WAVE], nb barriers
template <int CH, int RD, class RG>
__device__ __forceinline__ void im_stream_loop(const ImParams &P, RG &g, const double *rhs_l, int64_t *dbuf,
                                               int lane, int K, int nb, int t_start) {
    StreamPos<RG> pos(P.cm.ph_step);
    stream_flat_loop<CH, RD, 1>(
        K, nb, t_start, P.periods,
        [&](int j, int, int64_t &d) {
#ifdef INVSIM_ABL_ROLL_NO_DRAW
            d = 20;
            return true;
#else
            pos.at(g, j, 0);
            return np_poisson_try(g, P.pc, rhs_l, d);
#endif
        },
        [&](int slot, int, int64_t d) { dbuf[slot * WAVE + lane] = d < 0 ? 0 : d; });
}

constexpr int IM_AP_LDS = 256;   // alpha**t LDS table of the 3-role rollout (periods <= this)

// demand chunk of im_roll3_kernel: 4 launch steps (round 5; 65 536 envs, K = 30:
// 108.0-109.0 us against 112.1-113.0 with 8, equal at 262 144 envs,
// profiles/r05/roll3_ring/ab.txt; a smaller first chunk starts the dynamics
// wave sooner)
#ifndef IM_ROLL3_CH
#define IM_ROLL3_CH 4
#endif
#ifndef IM_ROLL3_RD
#define IM_ROLL3_RD 4
#endif
template <int L0, int L1, int L2>
struct ImLt3 {
    static constexpr int M1 = 3;
    static constexpr int D = (L0 > L1 ? (L0 > L2 ? L0 : L2) : (L1 > L2 ? L1 : L2));
    static constexpr int O = M1 * (D + 1);
    static constexpr int CH = IM_ROLL3_CH;                               // demand chunk (launch steps)
    static constexpr int RD = IM_ROLL3_RD;                               // demand ring depth (chunks)
    static constexpr int lt(int i) { return i == 0 ? L0 : i == 1 ? L1 : L2; }
    static constexpr int W(int i) { return lt(i) > 0 ? lt(i) : 1; }      // register window length
    static constexpr size_t lds() {   // + the episode sink's [3][WAVE] sums (EpLaneLds)
        return (size_t)WAVE * O * 8 + RHS_LDS_MAX * 8 + (size_t)RD * CH * WAVE * 8 + 3 * WAVE * 8;
    }
};

// POL (invsim_rollout_policy with BASE_STOCK or CONSTANT): the dynamics wave
// computes each step's order from its registers instead of loading it --
// BaseStockAgent.get_action (benchmark_InvManagementBacklogEnv.py:152-198) needs
// I[t] and the requested orders of the last L_i periods, ages 1 .. L_i of the
// window it already holds (plus the age-D row, wold) -- every output is
// optional, and the evaluate_agent sums accumulate in registers (as
// im_launch_step / im_step_regs, same order).
// waves_per_eu(2): at most 256 registers in all, so two dynamics waves share a
// SIMD (the policy variant sits at 256 VGPRs, and the compiler would otherwise
// take AGPRs beyond them: one wave per SIMD, measured 104 -> 166 us)
// RND, LVL: the policy variants (the top of this file).
template <int L0, int L1, int L2, bool BACKLOG, bool POL, class RG = Pcg, bool RND = false, bool LVL = false>
__global__ void __launch_bounds__(2 * WAVE) __attribute__((amdgpu_waves_per_eu(2)))
im_roll3_kernel(ImParams P, int t_start, StepIO<int64_t, int64_t> io, PolicyIO pol, int g0) {
    using G = ImLt3<L0, L1, L2>;
    constexpr int M1 = G::M1, D = G::D, O = G::O, CH = G::CH;
    extern __shared__ __attribute__((aligned(16))) int64_t im_tile[];
    double *rhs_l = reinterpret_cast<double *>(im_tile + WAVE * O);
    int64_t *dbuf = reinterpret_cast<int64_t *>(rhs_l + RHS_LDS_MAX);   // [RD * CH][WAVE]
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t N = P.cm.N;
    const int64_t S = P.cm.Npad;
    const int64_t e0 = ((int64_t)blockIdx.x + g0) * WAVE;   // g0: the launch's first group
    const int64_t e = e0 + lane;
    const bool valid = e < N;
    const int64_t el = valid ? e : N - 1;          // padded lanes: the last env's data, never stored
    const int nvalid = (int)((N - e0) < WAVE ? (N - e0) : WAVE);
    const int K = io.K;
    const int nch = (K + CH - 1) / CH;
    if (threadIdx.x < WAVE) {   // ---- demand wave
        TableStage ts = im_stage_table(P, rhs_l, lane, P.pc.nk > 0);
        RG g;
        P.cm.rng.load(el, g);
        ts.flush(lane);
        im_stream_loop<CH, G::RD>(P, g, rhs_l, dbuf, lane, K, nch, t_start);   // barriers 0 .. nch - 1
        if (valid) P.cm.rng.store_state(e, g);
        return;
    }
    // ---- dynamics wave
    int64_t *trow = im_tile + (int64_t)lane * O;
    int t = t_start;
    int64_t I[M1], B[M1 + 1];
#pragma unroll
    for (int i = 0; i < M1; i++) I[i] = P.I[i * S + el];
#pragma unroll
    for (int q = 0; q <= M1; q++) B[q] = BACKLOG ? P.B[q * S + el] : 0;
    // fulfilled-order windows: rw_i[a] = R[t - L_i + a] from ring slot (t + a) mod L_i
    // (rows older than the episode are masked at use by t >= L_i)
    int64_t rw[M1][D > 0 ? D : 1];                 // stage i uses rw[i][0 .. W(i))
#pragma unroll
    for (int i = 0; i < M1; i++) {
#pragma unroll
        for (int a = 0; a < G::W(i); a++) {
            const int L = G::lt(i);
            rw[i][a] = L > 0 ? P.Rring[(int64_t)(P.ring_off[i] + (int)((uint32_t)(t + a) % (uint32_t)L)) * S + el] : 0;
        }
    }
    // requested-order rows: wv[a] = action_log[t - (D - 1) + a], slot (t + 1 + a) mod D
    int64_t wv[D > 1 ? D - 1 : 1][M1];
#pragma unroll
    for (int a = 0; a + 1 < D; a++) {
        const int64_t base = ((int64_t)((uint32_t)(t + 1 + a) % (uint32_t)D) * S + el) * M1;
#pragma unroll
        for (int i = 0; i < M1; i++) {
            const uint32_t v = P.alog32[base + i];
            wv[a][i] = (int64_t)v;
            if (v == IM_WIDE) wv[a][i] = P.alog[base + i];
        }
    }
    int64_t nact[M1];
#pragma unroll
    for (int i = 0; i < M1; i++) nact[i] = POL ? 0 : io.act[el * M1 + i];
    // POL: the age-D requested-order row (slot t mod D, before step t overwrites it)
    int64_t wold[M1];
#pragma unroll
    for (int i = 0; i < M1; i++) {
        wold[i] = 0;
        if (POL && G::lt(i) == D) wold[i] = alog_get(P, ((int64_t)((uint32_t)t % (uint32_t)D) * S + el) * M1 + i);
    }
    constexpr int MD = 6;                                 // metrics (invsim.h INVSIM_METRICS_*)
    double met[MD];
#pragma unroll
    for (int q = 0; q < MD; q++) met[q] = (POL && pol.metrics) ? pol.metrics[el * MD + q] : 0.0;
    double napow = P.alpha_pow[t < P.periods ? t : 0];   // alpha**t of the next step, prefetched
    int64_t dlast = 0;
    bool last_real = false;
    ActGen ag;
    if constexpr (RND) ag.load(pol, S, el);
    // episode sink (kernels.hpp EpSink), accumulated in registers over the launch;
    // the group's partials are read only after the loop (they would hold 8
    // VGPRs through it: the policy kernel then needs AGPRs, one wave per SIMD)
    double *const ep_part = P.cm.ep_ret ? P.cm.ep_part + 4 * (e0 / WAVE) : nullptr;
    EpLaneLds ep;
    bool ep_done = false;
    if (ep_part) ep.init(reinterpret_cast<double *>(dbuf + G::RD * CH * WAVE), lane, valid ? P.cm.ep_ret[e] : 0.0);
    wg_lds_sync();   // barrier 0: chunk 0 ready
    for (int c = 0; c < nch; c++) {
        const int64_t *db = dbuf + (c % G::RD) * CH * WAVE;
        for (int kk = 0; kk < CH && c * CH + kk < K; kk++) {
            const int k = c * CH + kk;
            const int64_t oi = (int64_t)k * N + e;
            int64_t req[M1];
#pragma unroll
            for (int i = 0; i < M1; i++) req[i] = nact[i];
            if constexpr (RND) {
#pragma unroll
                for (int i = 0; i < M1; i++) req[i] = act_draw(ag.g, pol.ci[i]);
                if (valid && pol.act_out) {
#pragma unroll
                    for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, req[i]);
                }
            }
            const double apow = napow;
            {
                const int tn = (t >= P.periods) ? 0 : t + 1;     // the next launch step's period
                napow = P.alpha_pow[tn < P.periods ? tn : 0];
            }
            ImLevels<M1> lvl;                      // LVL: read again every step (see ImLevels)
            if constexpr (LVL) lvl.load(pol, el);
            if (!POL && k + 1 < K) {               // prefetch the next step's actions
#pragma unroll
                for (int i = 0; i < M1; i++) nact[i] = io.act[((int64_t)(k + 1) * N + el) * M1 + i];
            }
            if (t >= P.periods) {                  // NEXT_STEP autoreset (:197-220)
#pragma unroll
                for (int i = 0; i < M1; i++) I[i] = P.I0[i];
#pragma unroll
                for (int q = 0; q <= M1; q++) B[q] = 0;
#pragma unroll
                for (int q = 0; q < O; q++) trow[q] = (q < M1) ? P.I0[q] : 0;
                if (valid && (!POL || io.rew)) {
                    out_store(io.rew + oi, 0.0);
                    out_store(io.term + oi, (uint8_t)0);
                    out_store(io.trunc + oi, (uint8_t)0);
                }
                if (ep_part) ep.add(0.0, false);   // the reset step's row: reward 0, no flag
                t = 0;
            } else {
                const int64_t d = db[kk * WAVE + lane];
                if (POL && !RND) {
                    if (LVL || pol.kind == POL_BASE_STOCK) {   // im_base_stock from the register windows
#pragma unroll
                        for (int i = 0; i < M1; i++) {
                            constexpr int DD = D;
                            int64_t pos = I[i];                                 // observation[:M1] = I[t]
                            int64_t pipe = 0;
#pragma unroll
                            for (int a = 1; a <= G::lt(i); a++) {               // action_log[max(0, t - L_i) : t, i]
                                const int64_t v = (a <= DD - 1) ? wv[(DD - 1 - a) >= 0 ? DD - 1 - a : 0][i] : wold[i];
                                if (t - a >= 0) pipe = wrap_add(pipe, v);
                            }
                            if (G::lt(i) > 0) pos = wrap_add(pos, pipe);
                            if constexpr (LVL) req[i] = im_levels_order(lvl.lv[i], lvl.ro[i], pos, P.c[i]);
                            else req[i] = im_base_stock_order(pol, G::lt(i), pos, P.c[i]);
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < M1; i++) req[i] = pol.ci[i];
                    }
                    if (valid && pol.act_out) {
#pragma unroll
                        for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, req[i]);
                    }
                }
                int64_t R[M1], Icur[M1], Sv[M1 + 1], U[M1 + 1];
                im_orders<M1>(
                    P, req, I, B, [&](int i) { return (G::lt(i) > 0 && t >= G::lt(i)) ? rw[i][0] : (int64_t)0; },
                    [](int i) { return G::lt(i) == 0; }, R, Icur, Sv, U);
                im_sales(d, B[0], Icur[0], Sv[0], U[0]);
                const double reward = apow * im_profit<M1>(P, Sv, U, Icur);     // :322
                if (POL) {
                    im_metric_sums<M1>(met, d, Sv[0], U[0], Icur);
                    met[0] += reward;                                           // episode_reward += reward
                    met[1] += 1.0;                                              // episode_steps
                }
                // observation (:354-391): I, then the window rows t+1-n .. t, zeros after
                const int n = (t + 1 < D) ? t + 1 : D;
#pragma unroll
                for (int i = 0; i < M1; i++) trow[i] = Icur[i];
#pragma unroll
                for (int a = 0; a + 1 < D; a++) {
                    const int r = a - D + n;                                    // obs row of wv[a]
                    if (r >= 0) {
#pragma unroll
                        for (int i = 0; i < M1; i++) trow[M1 + r * M1 + i] = wv[a][i];
                    }
                }
#pragma unroll
                for (int i = 0; i < M1; i++) trow[M1 + (n - 1) * M1 + i] = req[i];
                for (int q = M1 + n * M1; q < O; q++) trow[q] = 0;
                // the new ring slots: R[t] (:267), action_log[t] (:268)
                if (valid) {
#pragma unroll
                    for (int i = 0; i < M1; i++) {
                        const int L = G::lt(i);
                        if (L > 0) st_store(P.Rring + (int64_t)(P.ring_off[i] + (int)((uint32_t)t % (uint32_t)L)) * S + e, R[i]);
                    }
                    const int64_t wb = ((int64_t)((uint32_t)t % (uint32_t)D) * S + e) * M1;
#pragma unroll
                    for (int i = 0; i < M1; i++) {
                        const bool wide = req[i] >= (int64_t)IM_WIDE;
                        st_store(P.alog32 + wb + i, wide ? IM_WIDE : (uint32_t)req[i]);
                        if (wide) st_store(P.alog + wb + i, req[i]);
                    }
                    if (!POL || io.rew) {
                        out_store(io.rew + oi, reward);
                        out_store(io.term + oi, (uint8_t)0);
                        out_store(io.trunc + oi, (uint8_t)(t + 1 >= P.periods ? 1 : 0));   // :350
                    }
                }
                if (ep_part) {
                    const bool done = valid && t + 1 >= P.periods;
                    ep.add(valid ? reward : 0.0, done);
                    ep_done |= done;
                }
                // age the windows by one period
#pragma unroll
                for (int i = 0; i < M1; i++) {
                    const int L = G::lt(i);
                    if (L > 0) {
#pragma unroll
                        for (int a = 0; a + 1 < G::W(i); a++) rw[i][a] = rw[i][a + 1];
                        rw[i][G::W(i) - 1] = R[i];
                    }
                }
                if (POL && D > 1) {
#pragma unroll
                    for (int i = 0; i < M1; i++) wold[i] = wv[0][i];             // age D - 1 -> age D
                }
#pragma unroll
                for (int a = 0; a + 2 < D; a++) {
#pragma unroll
                    for (int i = 0; i < M1; i++) wv[a][i] = wv[a + 1][i];
                }
                if (D > 1) {
#pragma unroll
                    for (int i = 0; i < M1; i++) wv[D - 2][i] = req[i];
                }
#pragma unroll
                for (int i = 0; i < M1; i++) I[i] = Icur[i];                    // :326
#pragma unroll
                for (int q = 0; q <= M1; q++) B[q] = BACKLOG ? U[q] : 0;        // :307-312
                dlast = d;
                last_real = k == K - 1;
                t += 1;
            }
            wave_lds_sync();
#ifndef INVSIM_ABL_ROLL_NO_STORE
            if (!POL || io.obs)
                store_tile<(O * WAVE * 8 + 16 * WAVE - 1) / (16 * WAVE)>(im_tile, io.obs + ((int64_t)k * N + e0) * O,
                                                                        (int64_t)nvalid * O, lane);
#endif
            wave_lds_sync();
        }
        if (c + 1 < nch) wg_lds_sync();   // barrier c + 1
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < M1; i++) st_store(P.I + i * S + e, I[i]);
        if (BACKLOG) {
#pragma unroll
            for (int q = 0; q <= M1; q++) st_store(P.B + q * S + e, B[q]);
        }
        if (P.cm.info_demand && last_real) P.cm.info_demand[e] = dlast;
        if (POL && pol.metrics) {
#pragma unroll
            for (int q = 0; q < MD; q++) pol.metrics[e * MD + q] = met[q];
        }
        if (ep_part) P.cm.ep_ret[e] = ep.r;
        if constexpr (RND) ag.store(pol, S, e);
    }
    if (ep_part) {
        EpPart epp;
        epp.load(ep_part);
        epp.flush(ep_part, ep.get(), __ballot(ep_done) != 0, lane);
    }
}

// im_roll3_kernel with the observation work moved to a third wave (for small
// batches, where a dynamics wave has a SIMD to itself and its instruction
// chain is the step time): one 192-thread workgroup per 64 envs, three roles
// pipelined over chunks of CH launch steps:
//   wave 0 (demand)   draws the demands up to RD chunks ahead into an LDS
//                     ring (stream_flat_loop); a demand is a function of the
//                     env's stream only, and a NEXT_STEP reset step draws
//                     nothing (:186-222)
//   wave 1 (dynamics) consumes chunk c: the step (:224-352) with the
//                     fulfilled-order history in registers aligned by age
//                     (rw_i[a] = R[t - L_i + a], so the arrival is rw_i[0]);
//                     stores reward, flags, the new R ring slots, and hands the
//                     end-of-step inventory of every step to wave 2 in LDS
//   wave 2 (obs)      builds the observations of chunk c - 1: the inventory
//                     from wave 1, the requested-order rows from its own copy
//                     of the actions (wv[a] = action_log[t - (D - 1) + a], in
//                     registers), the obs tile store, and the action_log ring
// Each role's next step's actions / alpha**t are loaded a step ahead, before
// the previous step's stores (vmcnt is in order).  One barrier per chunk: the
// demand wave fills dbuf[c & 1] before barrier c, the dynamics wave consumes it
// between barriers c and c + 1 and fills ibuf[c & 1], which the obs wave
// consumes between barriers c + 1 and c + 2.
#ifndef IM_ROLL3O_CH
#define IM_ROLL3O_CH 2   // swept on MI355X (LostSales 32768 envs): (CH, RD) = (2, 8) 65.6 us, (4, 4) 67.0, (4, 8) 66.5, (8, 4) 74.6
#endif
#ifndef IM_ROLL3O_RD
#define IM_ROLL3O_RD 8
#endif
template <int L0, int L1, int L2>
struct ImLt3o : ImLt3<L0, L1, L2> {
    static constexpr int CH = IM_ROLL3O_CH;                              // chunk (launch steps)
    static constexpr int RD = IM_ROLL3O_RD;                              // demand ring depth (chunks)
    static constexpr int M1 = 3, O = ImLt3<L0, L1, L2>::O;
    // tile, RHS table, demand ring, ibuf [2][CH][M1][WAVE] (inventory, dynamics ->
    // obs wave), abuf [2][CH][M1][WAVE] (requested orders, dynamics -> obs wave;
    // only with POL), alpha**t.  Open-loop actions are loaded by the dynamics and
    // obs waves themselves (staging them through LDS on the demand wave measured
    // slower: 64.9-65.5 against 63.1-64.1 us, profiles/r04/stage_ab)
    static constexpr size_t abuf_n(bool pol) { return pol ? (size_t)2 * CH * M1 * WAVE : 0; }
    static constexpr size_t lds(bool pol) {
        return (size_t)WAVE * O * 8 + RHS_LDS_MAX * 8 + (size_t)RD * CH * WAVE * 8 + (size_t)2 * CH * M1 * WAVE * 8 +
               abuf_n(pol) * 8 + IM_AP_LDS * 8 + 3 * WAVE * 8;   // + EpLaneLds sums
    }
};

// POL (invsim_rollout_policy, BASE_STOCK / CONSTANT): the dynamics wave
// computes each step's order from I and its own register history of the last
// L_i orders per stage (hv), and hands the orders to the obs wave in LDS (abuf)
// beside the inventory; outputs optional, metrics in registers (as im_roll3_kernel).
// G2 = 2 (INVSIM_IM_ROLL3O_G2=1, A/B): two 64-env groups per 6-wave
// workgroup.  The dispatcher puts waves w and w + 4 of a 6-wave workgroup on
// one SIMD and waves 2 and 3 on a SIMD each (tools/wave_placement,
// profiles/r03/launch/placement.txt), so the two dynamics waves take waves 2
// and 3 and every demand wave shares its SIMD with the other group's obs wave.
// RND, LVL: the policy variants (the top of this file), in the dynamics wave.
template <int L0, int L1, int L2, bool BACKLOG, bool POL, class RG = Pcg, int G2 = 1, bool RND = false, bool LVL = false>
__global__ void __launch_bounds__(3 * WAVE * G2)
im_roll3o_kernel(ImParams P, int t_start, StepIO<int64_t, int64_t> io, PolicyIO pol) {
    using G = ImLt3o<L0, L1, L2>;
    constexpr int M1 = G::M1, D = G::D, O = G::O, CH = G::CH;
    extern __shared__ __attribute__((aligned(16))) int64_t im_lds3o[];
    const int w = threadIdx.x / WAVE;
    // G2 = 2: wave -> (role, group) = 0 (0,0) 1 (0,1) 2 (1,0) 3 (1,1) 4 (2,1) 5 (2,0)
    const int role = G2 == 1 ? w : (w >> 1);
    const int grp = G2 == 1 ? 0 : (w < 4 ? (w & 1) : ((w & 1) ^ 1));
    int64_t *im_tile = im_lds3o + (int64_t)grp * (int64_t)(G::lds(POL) / sizeof(int64_t));
    double *rhs_l = reinterpret_cast<double *>(im_tile + WAVE * O);
    int64_t *dbuf = reinterpret_cast<int64_t *>(rhs_l + RHS_LDS_MAX);   // [RD * CH][WAVE]
    int64_t *ibuf = dbuf + G::RD * CH * WAVE;                             // [2][CH][M1][WAVE]
    int64_t *abuf = ibuf + 2 * CH * M1 * WAVE;                            // [2][CH][M1][WAVE] (POL)
    double *ap_l = reinterpret_cast<double *>(abuf + G::abuf_n(POL));     // alpha**t, t < periods
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t N = P.cm.N;
    const int64_t S = P.cm.Npad;
    const int64_t e0 = ((int64_t)blockIdx.x * G2 + grp) * WAVE;
    const int64_t e = e0 + lane;
    const bool valid = e < N;
    const int64_t el = valid ? e : N - 1;          // padded lanes: the last env's data, never stored
    const int nvalid = (int)((N - e0) < WAVE ? (N - e0) : WAVE);
    const int K = io.K;
    const int nch = (K + CH - 1) / CH;
    TPROBE_W(0);
    TPROBE_W_ID();
    if (role == 0) {   // ---- demand wave
        TableStage ts = im_stage_table(P, rhs_l, lane, P.pc.nk > 0);
        RG g;
        P.cm.rng.load(el, g);
        for (int q = lane; q < P.periods; q += WAVE) ap_l[q] = P.alpha_pow[q];   // before barrier 0
        ts.flush(lane);
        // barriers 0 .. nch - 1 (demand chunk c ready), nch (the obs wave's last chunk)
        im_stream_loop<CH, G::RD>(P, g, rhs_l, dbuf, lane, K, nch + 1, t_start);
        if (valid) P.cm.rng.store_state(e, g);
        TWAIT();
        TPROBE_W(6);
        return;
    }
    if (role == 2) {   // ---- obs wave
        int64_t *trow = im_tile + (int64_t)lane * O;
        int t = t_start;
        // requested-order rows: wv[a] = action_log[t - (D - 1) + a], slot (t + 1 + a) mod D
        int64_t wv[D > 1 ? D - 1 : 1][M1];
#pragma unroll
        for (int a = 0; a + 1 < D; a++) {
            const int64_t base = ((int64_t)((uint32_t)(t + 1 + a) % (uint32_t)D) * S + el) * M1;
#pragma unroll
            for (int i = 0; i < M1; i++) {
                const uint32_t v = P.alog32[base + i];
                wv[a][i] = (int64_t)v;
                if (v == IM_WIDE) wv[a][i] = P.alog[base + i];
            }
        }
        constexpr bool HANDED = POL;   // requested orders from the dynamics wave
        int64_t nact[M1];
#pragma unroll
        for (int i = 0; i < M1; i++) nact[i] = HANDED ? 0 : io.act[el * M1 + i];
        wg_lds_sync();   // barrier 0
        for (int c = 0; c < nch; c++) {
            wg_lds_sync();   // barrier c + 1: inventory chunk c ready
            const int64_t *ib = ibuf + (c & 1) * CH * M1 * WAVE;
            const int64_t *ab = abuf + (c & 1) * CH * M1 * WAVE;
            for (int kk = 0; kk < CH && c * CH + kk < K; kk++) {
                const int k = c * CH + kk;
                int64_t req[M1];
#pragma unroll
                for (int i = 0; i < M1; i++) req[i] = HANDED ? ab[(kk * M1 + i) * WAVE + lane] : nact[i];
                if (!HANDED && k + 1 < K) {            // the next step's actions
#pragma unroll
                    for (int i = 0; i < M1; i++) nact[i] = io.act[((int64_t)(k + 1) * N + el) * M1 + i];
                }
                if (t >= P.periods) {                  // NEXT_STEP autoreset: [I0, 0...] (:220)
#pragma unroll
                    for (int q = 0; q < O; q++) trow[q] = (q < M1) ? ib[(kk * M1 + q) * WAVE + lane] : 0;
                    t = 0;
                } else {
#pragma unroll
                    for (int i = 0; i < M1; i++) req[i] = req[i] > 0 ? req[i] : 0;   // :250
                    // observation (:354-391): I, then the window rows t+1-n .. t, zeros after
                    const int n = (t + 1 < D) ? t + 1 : D;
#pragma unroll
                    for (int i = 0; i < M1; i++) trow[i] = ib[(kk * M1 + i) * WAVE + lane];
#pragma unroll
                    for (int a = 0; a + 1 < D; a++) {
                        const int r = a - D + n;                                // obs row of wv[a]
                        if (r >= 0) {
#pragma unroll
                            for (int i = 0; i < M1; i++) trow[M1 + r * M1 + i] = wv[a][i];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < M1; i++) trow[M1 + (n - 1) * M1 + i] = req[i];
                    for (int q = M1 + n * M1; q < O; q++) trow[q] = 0;
                    if (valid) {                                                // action_log[t] (:268)
                        const int64_t wb = ((int64_t)((uint32_t)t % (uint32_t)D) * S + e) * M1;
#pragma unroll
                        for (int i = 0; i < M1; i++) {
                            const bool wide = req[i] >= (int64_t)IM_WIDE;
                            st_store(P.alog32 + wb + i, wide ? IM_WIDE : (uint32_t)req[i]);
                            if (wide) st_store(P.alog + wb + i, req[i]);
                        }
                    }
#pragma unroll
                    for (int a = 0; a + 2 < D; a++) {
#pragma unroll
                        for (int i = 0; i < M1; i++) wv[a][i] = wv[a + 1][i];
                    }
                    if (D > 1) {
#pragma unroll
                        for (int i = 0; i < M1; i++) wv[D - 2][i] = req[i];
                    }
                    t += 1;
                }
                wave_lds_sync();
#ifndef INVSIM_ABL_ROLL_NO_STORE
                if (!POL || io.obs)
                    store_tile<(O * WAVE * 8 + 16 * WAVE - 1) / (16 * WAVE)>(im_tile, io.obs + ((int64_t)k * N + e0) * O,
                                                                            (int64_t)nvalid * O, lane);
#endif
                wave_lds_sync();
            }
        }
        TWAIT();
        TPROBE_W(6);
        return;
    }
    // ---- dynamics wave
    int t = t_start;
    int64_t I[M1], B[M1 + 1];
#pragma unroll
    for (int i = 0; i < M1; i++) I[i] = P.I[i * S + el];
#pragma unroll
    for (int q = 0; q <= M1; q++) B[q] = BACKLOG ? P.B[q * S + el] : 0;
    // fulfilled-order windows: rw_i[a] = R[t - L_i + a] from ring slot (t + a) mod L_i
    // (rows older than the episode are masked at use by t >= L_i)
    int64_t rw[M1][D > 0 ? D : 1];                 // stage i uses rw[i][0 .. W(i))
#pragma unroll
    for (int i = 0; i < M1; i++) {
#pragma unroll
        for (int a = 0; a < G::W(i); a++) {
            const int L = G::lt(i);
            rw[i][a] = L > 0 ? P.Rring[(int64_t)(P.ring_off[i] + (int)((uint32_t)(t + a) % (uint32_t)L)) * S + el] : 0;
        }
    }
    // POL: hv[i][a] = action_log[t - 1 - a, i], the last W(i) requested orders of stage i
    int64_t hv[M1][D > 0 ? D : 1];
#pragma unroll
    for (int i = 0; i < M1; i++) {
#pragma unroll
        for (int a = 0; a < G::W(i); a++)
            hv[i][a] = POL ? alog_get(P, ((int64_t)((uint32_t)(t - 1 - a + 256 * D) % (uint32_t)D) * S + el) * M1 + i) : 0;
    }
    constexpr int MD = 6;                                 // metrics (invsim.h INVSIM_METRICS_*)
    double met[MD];
#pragma unroll
    for (int q = 0; q < MD; q++) met[q] = (POL && pol.metrics) ? pol.metrics[el * MD + q] : 0.0;
    int64_t nact[M1];
#pragma unroll
    for (int i = 0; i < M1; i++) nact[i] = POL ? 0 : io.act[el * M1 + i];
    int64_t dlast = 0;
    bool last_real = false;
    ActGen ag;
    if constexpr (RND) ag.load(pol, S, el);
    ImLevels<M1> lvl;                              // LVL: held over the K steps (see ImLevels)
    if constexpr (LVL) lvl.load(pol, el);
    // episode sink (kernels.hpp EpSink), accumulated in registers over the launch;
    // the group's partials are read only after the loop (they would hold 8
    // VGPRs through it: the policy kernel then needs AGPRs, one wave per SIMD)
    double *const ep_part = P.cm.ep_ret ? P.cm.ep_part + 4 * (e0 / WAVE) : nullptr;
    EpLaneLds ep;
    bool ep_done = false;
    if (ep_part) ep.init(reinterpret_cast<double *>(ap_l + IM_AP_LDS), lane, valid ? P.cm.ep_ret[e] : 0.0);
    wg_lds_sync();   // barrier 0: demand chunk 0 (and alpha**t) ready
    for (int c = 0; c < nch; c++) {
        const int64_t *db = dbuf + (c % G::RD) * CH * WAVE;
        int64_t *ib = ibuf + (c & 1) * CH * M1 * WAVE;
        int64_t *ab = abuf + (c & 1) * CH * M1 * WAVE;
        for (int kk = 0; kk < CH && c * CH + kk < K; kk++) {
            const int k = c * CH + kk;
            const int64_t oi = (int64_t)k * N + e;
            int64_t req[M1];
#pragma unroll
            for (int i = 0; i < M1; i++) req[i] = nact[i];
            if constexpr (RND) {
#pragma unroll
                for (int i = 0; i < M1; i++) req[i] = act_draw(ag.g, pol.ci[i]);
                if (valid && pol.act_out) {
#pragma unroll
                    for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, req[i]);
                }
            }
            if (!POL && k + 1 < K) {    // prefetch the next step's actions
#pragma unroll
                for (int i = 0; i < M1; i++) nact[i] = io.act[((int64_t)(k + 1) * N + el) * M1 + i];
            }
            const double apow = ap_l[t < P.periods ? t : 0];
            if (t >= P.periods) {                  // NEXT_STEP autoreset (:197-220)
#pragma unroll
                for (int i = 0; i < M1; i++) I[i] = P.I0[i];
#pragma unroll
                for (int q = 0; q <= M1; q++) B[q] = 0;
#pragma unroll
                for (int i = 0; i < M1; i++) ib[(kk * M1 + i) * WAVE + lane] = I[i];
                if (valid && (!POL || io.rew)) {
                    out_store(io.rew + oi, 0.0);
                    out_store(io.term + oi, (uint8_t)0);
                    out_store(io.trunc + oi, (uint8_t)0);
                }
                if (ep_part) ep.add(0.0, false);   // the reset step's row: reward 0, no flag
                t = 0;
            } else {
                const int64_t d = db[kk * WAVE + lane];
                if (POL && !RND) {
                    if (LVL || pol.kind == POL_BASE_STOCK) {   // im_base_stock from the register history
#pragma unroll
                        for (int i = 0; i < M1; i++) {
                            int64_t pos = I[i];                                 // observation[:M1] = I[t]
                            int64_t pipe = 0;
#pragma unroll
                            for (int a = 0; a < G::lt(i); a++)                  // action_log[max(0, t - L_i) : t, i]
                                if (t - 1 - a >= 0) pipe = wrap_add(pipe, hv[i][a]);
                            if (G::lt(i) > 0) pos = wrap_add(pos, pipe);
                            if constexpr (LVL) req[i] = im_levels_order(lvl.lv[i], lvl.ro[i], pos, P.c[i]);
                            else req[i] = im_base_stock_order(pol, G::lt(i), pos, P.c[i]);
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < M1; i++) req[i] = pol.ci[i];
                    }
                    if (valid && pol.act_out) {
#pragma unroll
                        for (int i = 0; i < M1; i++) out_store((int64_t *)pol.act_out + oi * M1 + i, req[i]);
                    }
                }
                int64_t R[M1], Icur[M1], Sv[M1 + 1], U[M1 + 1];
                im_orders<M1>(
                    P, req, I, B, [&](int i) { return (G::lt(i) > 0 && t >= G::lt(i)) ? rw[i][0] : (int64_t)0; },
                    [](int i) { return G::lt(i) == 0; }, R, Icur, Sv, U);
                im_sales(d, B[0], Icur[0], Sv[0], U[0]);
                const double reward = apow * im_profit<M1>(P, Sv, U, Icur);     // :322
                if (POL) {
                    im_metric_sums<M1>(met, d, Sv[0], U[0], Icur);
                    met[0] += reward;                                           // episode_reward += reward
                    met[1] += 1.0;                                              // episode_steps
#pragma unroll
                    for (int i = 0; i < M1; i++) {
#pragma unroll
                        for (int a = G::W(i) - 1; a >= 1; a--) hv[i][a] = hv[i][a - 1];
                        hv[i][0] = req[i];
                    }
                }
                if (POL) {
#pragma unroll
                    for (int i = 0; i < M1; i++) ab[(kk * M1 + i) * WAVE + lane] = req[i];   // the order -> obs wave
                }
#pragma unroll
                for (int i = 0; i < M1; i++) ib[(kk * M1 + i) * WAVE + lane] = Icur[i];   // obs I (:366)
                // the new fulfilled-order ring slots R[t] (:267)
                if (valid) {
#pragma unroll
                    for (int i = 0; i < M1; i++) {
                        const int L = G::lt(i);
                        if (L > 0) st_store(P.Rring + (int64_t)(P.ring_off[i] + (int)((uint32_t)t % (uint32_t)L)) * S + e, R[i]);
                    }
                    if (!POL || io.rew) {
                        out_store(io.rew + oi, reward);
                        out_store(io.term + oi, (uint8_t)0);
                        out_store(io.trunc + oi, (uint8_t)(t + 1 >= P.periods ? 1 : 0));   // :350
                    }
                }
                if (ep_part) {
                    const bool done = valid && t + 1 >= P.periods;
                    ep.add(valid ? reward : 0.0, done);
                    ep_done |= done;
                }
                // age the windows by one period
#pragma unroll
                for (int i = 0; i < M1; i++) {
                    const int L = G::lt(i);
                    if (L > 0) {
#pragma unroll
                        for (int a = 0; a + 1 < G::W(i); a++) rw[i][a] = rw[i][a + 1];
                        rw[i][G::W(i) - 1] = R[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < M1; i++) I[i] = Icur[i];                    // :326
#pragma unroll
                for (int q = 0; q <= M1; q++) B[q] = BACKLOG ? U[q] : 0;        // :307-312
                dlast = d;
                last_real = k == K - 1;
                t += 1;
            }
        }
        wg_lds_sync();   // barrier c + 1: inventory chunk c ready, demand chunk c + 1 ready
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < M1; i++) st_store(P.I + i * S + e, I[i]);
        if (BACKLOG) {
#pragma unroll
            for (int q = 0; q <= M1; q++) st_store(P.B + q * S + e, B[q]);
        }
        if (P.cm.info_demand && last_real) P.cm.info_demand[e] = dlast;
        if (POL && pol.metrics) {
#pragma unroll
            for (int q = 0; q < MD; q++) pol.metrics[e * MD + q] = met[q];
        }
        if (ep_part) P.cm.ep_ret[e] = ep.r;
        if constexpr (RND) ag.store(pol, S, e);
    }
    if (ep_part) {
        EpPart epp;
        epp.load(ep_part);
        epp.flush(ep_part, ep.get(), __ballot(ep_done) != 0, lane);
    }
    TWAIT();
    TPROBE_W(6);
}

// the lock-step split step kernel applies (both streams)
inline bool im_split_applies(const ImParams &p, int t_u, const PolicyIO *pol, const StepIO<int64_t, int64_t> &io) {
    return !pol && io.K == 1 && t_u >= 0 && t_u < p.periods && io.obs &&
           !(p.cm.autoreset == AR_SAME_STEP && t_u + 1 >= p.periods) && p.cm.kn.im_split;
}

// The lock-step NEXT_STEP reset step (one step at t_u >= periods): its output row
// is reward 0 with no flag, whose fold changes nothing (EpLane adds +0.0 to
// returns restarted at +0.0), so the episode sink needs no work for it
inline bool im_sink_noop(const ImParams &p, int t_u, const PolicyIO *pol, const StepIO<int64_t, int64_t> &io) {
    return lockstep_reset_launch(pol, io, t_u, p.periods) && p.cm.autoreset == AR_NEXT_STEP;
}

// the 2-/3-role rollout kernels of the reference's default lead times apply
// (open loop, or the in-kernel BaseStock / ConstantOrder agents)
inline bool im_roll_applies(const ImParams &p, int M1, int t_u, const PolicyIO *pol,
                            const StepIO<int64_t, int64_t> &io) {
    const bool pol_roll = pol && (pol->kind == POL_BASE_STOCK || pol->kind == POL_CONSTANT || pol->kind == POL_RANDOM ||
                                  pol->kind == POL_LEVELS) &&
                          p.cm.kn.im_pol_roll;
    return (!pol || pol_roll) && io.K > 1 && t_u >= 0 && p.cm.autoreset != AR_SAME_STEP && p.dist == 1 &&
           !p.cm.info_rec && M1 == 3 && p.L[0] == 1 && p.L[1] == 5 && p.L[2] == 10 && p.lt_max == 10 &&
           p.cm.kn.im_roll;
}

// Modes: the Run modes whose instantiations the calling unit holds (the end of
// this file)
template <class RG, class Modes>
hipError_t im_roll_launch(const ImParams &p, bool backlog, int t_u, const PolicyIO *pol,
                          const StepIO<int64_t, int64_t> &io, hipStream_t s) {
    const PolicyIO &pv = pol_or_none(pol);
    using G = ImLt3<1, 5, 10>;
    using G3 = ImLt3o<1, 5, 10>;
    const dim3 g3(grid_for(p.cm.N, WAVE));
    // up to one 2-role workgroup per SIMD pair (N <= 32768): the dynamics
    // wave's chain is the step time, so split it (measured on MI355X:
    // LostSales 32768 envs 87.5 -> 77.7 us per K = 30; at 65536 the
    // 2-role kernel is faster, 118 vs 152 us)
    const bool three = p.cm.N <= p.cm.kn.im_roll3o_max_n && p.periods <= IM_AP_LDS;   // alpha**t table in LDS
    // two groups per workgroup when the group count is even (every workgroup full)
    // two 64-env groups per 6-wave workgroup: the default for policy rollouts
    // (BaseStock at 32 768 envs: 63.1-64.8 against 66.5-67.7 us per 30 steps),
    // equal open loop (profiles/r03/launch/g2_stage.txt)
    const bool g2 = p.cm.kn.im_roll3o_g2 < 0 ? pol != nullptr : p.cm.kn.im_roll3o_g2 == 1;
    const bool two = three && g2 && (g3.x % 2) == 0;
    // INVSIM_IM_ROLL_SUB (default 65 536): the 2-role rollout as back-to-back
    // launches of at most that many envs (whole 64-env groups), each over its
    // own groups: one round of 1 024 workgroups (four per CU) per launch.
    // Measured at K = 30 (profiles/r06/roll_sub): 262 144 envs 618 -> 564 us,
    // 1 048 576 envs 2 433 -> 2 300 us; sub-launches of 131 072 envs (two
    // rounds each) are slower than one launch, of 16 384 far slower
    const int sub = p.cm.kn.im_roll_sub >= WAVE ? (int)std::min<int64_t>(p.cm.kn.im_roll_sub / WAVE, g3.x) : (int)g3.x;
    auto launch = [&](auto B_, auto R_) {
        constexpr bool B = decltype(B_)::value;
        using MD = RunMode<decltype(R_)::value>;
        constexpr bool POL = MD::POL, RND = MD::RND, LVL = MD::LVL;
        if (two)
            hipLaunchKernelGGL((im_roll3o_kernel<1, 5, 10, B, POL, RG, 2, RND, LVL>), dim3(g3.x / 2), dim3(6 * WAVE),
                               2 * G3::lds(POL), s, p, t_u, io, pv);
        else if (three)
            hipLaunchKernelGGL((im_roll3o_kernel<1, 5, 10, B, POL, RG, 1, RND, LVL>), g3, dim3(3 * WAVE), G3::lds(POL), s, p,
                               t_u, io, pv);
        else
            for (int g0 = 0; g0 < (int)g3.x; g0 += sub)
                hipLaunchKernelGGL((im_roll3_kernel<1, 5, 10, B, POL, RG, RND, LVL>), dim3(min(sub, (int)g3.x - g0)),
                                   dim3(2 * WAVE), G::lds(), s, p, t_u, io, pv, g0);
        return hipGetLastError();
    };
    const Run mode = run_mode_variant(pol, io.K, POL_LEVELS);
    return dispatch_bool(backlog, [&](auto B) {
        return dispatch(Modes{}, mode, [&](auto R) { return launch(B, R); }, invalid_value);
    });
}

// im_split_kernel's launch-time values (see the kernel's argument list): the
// host knows t, so every wave need not derive them
struct ImSplitArgs {
    int32_t n32;
    uint32_t hw;     // ImHot word, or 0
    uint64_t *acur;  // the current lookahead slot, or null
    double apow;     // alpha ** t, the very double of the device table
    int n, nw, trunc;
};
inline ImSplitArgs im_split_args(const ImParams &q, const double *ap_host, int M1, int t, int cur) {
    ImSplitArgs a{};
    a.n32 = (int32_t)q.cm.N;
    a.acur = q.ahead ? q.ahead + (int64_t)cur * 4 * pad_n(q.cm.N) : nullptr;
    a.apow = ap_host[t];
    const int D = q.lt_max, t1 = t + 1;
    a.n = D > 0 ? (t1 < D ? t1 : D) : 0;                      // window rows incl. the newest
    a.nw = a.n > 0 ? (a.n - 1) * M1 : 0;
    a.trunc = t1 >= q.periods ? 1 : 0;                        // :350
    int sumL = 0;
    for (int i = 0; i < M1; i++) sumL += q.L[i];
    if (M1 == ImHot::M1 && D <= 15 && sumL <= ImHot::NOARR) {
        const uint32_t slot0 = D > 0 ? (uint32_t)(t1 - a.n) % (uint32_t)D : 0;
        const uint32_t rmax = a.nw > 0 ? (uint32_t)(a.nw / M1 - 1) : 0;
        uint32_t w = (1u << 31) | slot0 | (rmax << 4) | ((uint32_t)D << 8);
        for (int i = 0; i < M1; i++) {
            const int L = q.L[i];
            const uint32_t row = (L > 0 && t >= L) ? (uint32_t)(q.ring_off[i] + t % L) : (uint32_t)ImHot::NOARR;
            w |= row << (12 + 6 * i);
        }
        a.hw = w;
    }
    return a;
}

// Stage count (M1 stages and the market) and backlog mode -> template arguments:
// f(Const<M1>, std::bool_constant<backlog>)
using ImStageCounts = Values<1, 2, 3, 4, 5, 6, 7, 8>;
template <class F>
hipError_t im_dispatch_shape(int M1, bool backlog, F &&f) {
    return dispatch(ImStageCounts{}, M1, [&](auto M) {
        return dispatch_bool(backlog, [&](auto B) { return f(M, B); });
    }, invalid_value);
}

// The one-wave run kernel, in every translation unit.  Modes: the Run modes
// whose instantiations the calling unit holds (the end of this file); a launch
// of any other mode is refused.
template <class RG, class Modes>
hipError_t im_run_kernel_launch(const ImParams &p, int M1, bool backlog, int t_u, const PolicyIO *pol,
                                const StepIO<int64_t, int64_t> &io, hipStream_t s) {
    const size_t lds = im_run_lds_bytes(M1, p.lt_max);
    const dim3 grid(grid_for(p.cm.N, EPW)), block(WAVE);
    const PolicyIO &pv = pol_or_none(pol);
    const bool npd = p.dist >= 2 && p.dist <= 4;
    const Run mode = run_mode_variant(pol, io.K, POL_LEVELS);
    return im_dispatch_shape(M1, backlog, [&](auto M_, auto B_) {
        constexpr int M = decltype(M_)::value;
        constexpr bool B = decltype(B_)::value;
        return dispatch_bool(t_u >= 0, [&](auto TU_) {
            constexpr bool TU = decltype(TU_)::value;
            return dispatch_bool(npd, [&](auto NPD_) {
                constexpr bool NPD = decltype(NPD_)::value;
                return dispatch(Modes{}, mode, [&](auto R) {
                    using MD = RunMode<decltype(R)::value>;
                    hipLaunchKernelGGL((im_run_kernel<M, B, TU, MD::ONE, MD::POL, NPD, RG, MD::RND, MD::EXT, MD::LVL>), grid,
                                       block, lds, s, p, t_u, io, pv);
                    return hipGetLastError();
                }, invalid_value);
            });
        });
    });
}

// im_split_kernel's instantiations: AHEAD = the cache holds this step's demand
// (else it is drawn inline), EARLY only for a lookahead step
enum class ImSplit { MISS, HIT, HIT_EARLY };

// The split / rollout / run dispatch of one demand stream: RG = Pcg (numpy's
// PCG64, parity) or PhiloxGen (the fast stream; instantiated in
// invmgmt_ph.hip).  The parity stream's lookahead cache holds generator state,
// which is committed to cm.rng (im_commit_launch) before a kernel that reads
// cm.rng; the fast stream's holds demands only: it is never committed, and any
// other launch leaves it stale (the launch-step counter moves past it).
template <class RG>
hipError_t im_launch_rg(const ImParams &p, const double *ap_host, int M1, bool backlog, int t_u, const PolicyIO *pol,
                        const StepIO<int64_t, int64_t> &io, Lookahead &la, bool &sunk, hipStream_t s) {
    constexpr bool ph = RG::kCounter;
    sunk = im_sink_noop(p, t_u, pol, io);
    if (p.cm.N == 0 || io.K <= 0) return hipSuccess;
    // the parity stream's commit rule: before a kernel that reads cm.rng
    auto commit = [&] {
        const hipError_t ce = im_commit_launch(p, la.slot, s);
        la.valid = false;
        return ce;
    };
    if (im_split_applies(p, t_u, pol, io)) {
        const size_t lds2 = im_split_lds_bytes(M1, p.lt_max);
        ImParams q = p;
        if (!p.cm.kn.im_ahead) q.ahead = nullptr;
        if (!ph && la.valid && !q.ahead) {      // lookahead switched off: commit, then draw inline
            const hipError_t ce = commit();
            if (ce != hipSuccess) return ce;
        }
        const bool hit = la.valid && q.ahead;
        const int gla = hit ? (int)grid_for(p.cm.N, 2 * WAVE) : 0;   // lookahead workgroups
        const dim3 grid2(grid_for(p.cm.N, EPW) + gla), block2(2 * WAVE);
        const int cur = la.slot;
        // (the lookahead workgroups are the first gla of the grid: the kernel derives gla from N)
        if (p.cm.N > INT32_MAX - 2 * WAVE) return hipErrorInvalidValue;   // N travels as one dword
        if (!ImStageCounts::has(M1)) return hipErrorInvalidValue;
        const ImSplitArgs ha = im_split_args(q, ap_host, M1, t_u, cur);
        const bool early = p.cm.N > IM_EARLY_STORES_MIN_N;   // the EARLY instantiation (lookahead steps only)
        const ImSplit mode = !hit ? ImSplit::MISS : early ? ImSplit::HIT_EARLY : ImSplit::HIT;
        const bool npd = p.dist >= 2 && p.dist <= 4;
        sunk = true;                  // the split kernel folds into the episode sink (if one is set)
        la.valid = q.ahead != nullptr;   // every env drew its next demand into slot cur ^ 1
        if (la.valid) la.slot ^= 1;
        return im_dispatch_shape(M1, backlog, [&](auto M_, auto B_) {
            constexpr int M = decltype(M_)::value;
            constexpr bool B = decltype(B_)::value;
            return dispatch_bool(npd, [&](auto NPD_) {
                constexpr bool NPD = decltype(NPD_)::value;
                return dispatch(Values<ImSplit::MISS, ImSplit::HIT, ImSplit::HIT_EARLY>{}, mode, [&](auto S_) {
                    constexpr bool HIT = decltype(S_)::value != ImSplit::MISS, EARLY = decltype(S_)::value == ImSplit::HIT_EARLY;
                    // the kernel's argument list: its ImParams is q, the launch-time values ha
                    hipLaunchKernelGGL((im_split_kernel<M, B, NPD, HIT, RG, EARLY>), grid2, block2, lds2, s, io.act, q.I, q.B,
                                       q.Rring, q.alog32, ha.acur, ha.n32, ha.hw, q, t_u, io, cur, ha.apow, ha.n, ha.nw, ha.trunc);
                    return hipGetLastError();
                }, invalid_value);
            });
        });
    }
    // every other kernel draws from the committed state (brought into cm.rng
    // first): the cache is stale after it, unless this launch is the lock-step
    // autoreset (no draw).  The fast stream's cache just ends.
    if (ph) {
        la.valid = false;
    } else if (la.valid && !lockstep_reset_launch(pol, io, t_u, p.periods)) {
        const hipError_t ce = commit();
        if (ce != hipSuccess) return ce;
    }
    // the policy variants: the same rows from the translation units that hold
    // them (RANDOM: invmgmt_rnd.hip, LEVELS: invmgmt_lvl.hip, and EXTERNAL, the
    // caller's actions on the run kernel for any K: invmgmt_ext.hip)
    if (pol && pol->kind == POL_RANDOM) return im_rnd_launch(p, M1, backlog, t_u, *pol, io, ph, sunk, s);
    if (pol && pol->kind == POL_LEVELS) return im_lvl_launch(p, M1, backlog, t_u, *pol, io, ph, sunk, s);
    if (pol && pol->kind == POL_EXTERNAL) return im_ext_launch(p, M1, backlog, t_u, *pol, io, ph, s);
    // lock-step rollout of the reference's default lead times: register windows
    // and a demand wave (im_roll3_kernel / im_roll3o_kernel), open loop or with
    // the in-kernel BaseStock / ConstantOrder agents
    if (im_roll_applies(p, M1, t_u, pol, io)) {
        sunk = true;                  // so do the rollout kernels
        return im_roll_launch<RG, Values<Run::STEPS, Run::POLICY>>(p, backlog, t_u, pol, io, s);
    }
    return im_run_kernel_launch<RG, Values<Run::STEP, Run::STEPS, Run::POLICY>>(p, M1, backlog, t_u, pol, io, s);
}

// A variant unit's launch (R = Run::RANDOM or Run::LEVELS), both demand
// streams: the variant's instantiations of im_roll3o_kernel / im_roll3_kernel
// where im_roll_applies (the rows of BaseStock / ConstantOrder), of
// im_run_kernel otherwise.
template <Run R>
hipError_t im_variant_launch(const ImParams &p, int M1, bool backlog, int t_u, const PolicyIO &pol,
                             const StepIO<int64_t, int64_t> &io, bool philox, bool &sunk, hipStream_t s) {
    return dispatch_bool(philox, [&](auto PH) {
        using RG = std::conditional_t<decltype(PH)::value, PhiloxGen, Pcg>;
        if (im_roll_applies(p, M1, t_u, &pol, io)) {
            sunk = true;
            return im_roll_launch<RG, Values<R>>(p, backlog, t_u, &pol, io, s);
        }
        return im_run_kernel_launch<RG, Values<R>>(p, M1, backlog, t_u, &pol, io, s);
    });
}

}  // namespace

// The translation units.  This file is compiled five times (invmgmt.hip and
// the four files that include it under a macro) into five objects, and the
// macro decides one thing: which exported launchers the object defines.  A
// launcher names the demand stream and the Run modes it dispatches over, and an
// object holds the kernel instantiations its launchers name and no other:
//   invmgmt.o      numpy's PCG64 stream: STEP, STEPS, POLICY; reset and commit
//   invmgmt_ph.o   the fast stream: STEP, STEPS, POLICY
//   invmgmt_rnd.o  RANDOM, invmgmt_lvl.o LEVELS, invmgmt_ext.o EXTERNAL: both streams
// The variants stay out of the first two objects: with the RANDOM kernels in
// invmgmt.o the lock-step step ran 1.0-1.5 % slower, its own code unchanged
// (DESIGN, RandomAgent); and the objects compile in parallel.
#if defined(INVSIM_IM_RND_TU)
hipError_t im_rnd_launch(const ImParams &p, int M1, bool backlog, int t_u, const PolicyIO &pol,
                         const StepIO<int64_t, int64_t> &io, bool philox, bool &sunk, hipStream_t s) {
    return im_variant_launch<Run::RANDOM>(p, M1, backlog, t_u, pol, io, philox, sunk, s);
}
#elif defined(INVSIM_IM_LVL_TU)
hipError_t im_lvl_launch(const ImParams &p, int M1, bool backlog, int t_u, const PolicyIO &pol,
                         const StepIO<int64_t, int64_t> &io, bool philox, bool &sunk, hipStream_t s) {
    return im_variant_launch<Run::LEVELS>(p, M1, backlog, t_u, pol, io, philox, sunk, s);
}
#elif defined(INVSIM_IM_EXT_TU)
// im_run_kernel only, one step or K: invsim_rollout_metrics has no fused
// rollout.  The caller (im_launch_rg) has committed the lookahead cache; the
// kernel does not fold into the episode sink, so the host folds the output rows.
hipError_t im_ext_launch(const ImParams &p, int M1, bool backlog, int t_u, const PolicyIO &pol,
                         const StepIO<int64_t, int64_t> &io, bool philox, hipStream_t s) {
    if (philox) return im_run_kernel_launch<PhiloxGen, Values<Run::EXTERNAL>>(p, M1, backlog, t_u, &pol, io, s);
    return im_run_kernel_launch<Pcg, Values<Run::EXTERNAL>>(p, M1, backlog, t_u, &pol, io, s);
}
#elif defined(INVSIM_IM_FAST_TU)
hipError_t im_run_launch_ph(const ImParams &p, const double *ap_host, int M1, bool backlog, int t_u, const PolicyIO *pol,
                            const StepIO<int64_t, int64_t> &io, Lookahead &la, bool &sunk, hipStream_t s) {
    return im_launch_rg<PhiloxGen>(p, ap_host, M1, backlog, t_u, pol, io, la, sunk, s);
}

INVSIM_PTRS_STATS_TU(im_ph)
#else
hipError_t im_run_launch(const ImParams &p, const double *ap_host, int M1, bool backlog, int t_u, const PolicyIO *pol,
                         const StepIO<int64_t, int64_t> &io, Lookahead &la, bool &sunk, hipStream_t s) {
    if (p.cm.philox) return im_run_launch_ph(p, ap_host, M1, backlog, t_u, pol, io, la, sunk, s);   // invmgmt_ph.hip
    return im_launch_rg<Pcg>(p, ap_host, M1, backlog, t_u, pol, io, la, sunk, s);
}

namespace {
// cm.rng <- the committed slot of the lookahead cache (see im_split_kernel)
__global__ void __launch_bounds__(256) im_commit_kernel(ImParams P, int slot) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.cm.N) return;
    const int64_t S = P.cm.Npad;
    const uint64_t *A = P.ahead + (int64_t)slot * 4 * S;
    P.cm.rng.hi[e] = A[e];
    P.cm.rng.lo[e] = A[S + e];
    if (P.cm.u32buf) P.cm.u32buf[e] = A[3 * S + e];
}
}  // namespace

hipError_t im_commit_launch(const ImParams &p, int slot, hipStream_t s) {
    if (p.cm.N == 0 || !p.ahead) return hipSuccess;
    hipLaunchKernelGGL(im_commit_kernel, dim3(grid_for(p.cm.N, 256)), dim3(256), 0, s, p, slot ^ 1);
    return hipGetLastError();
}

hipError_t im_reset_launch(const ImParams &p, int M1, bool backlog, const uint8_t *mask,
                           int64_t *obs, hipStream_t s) {
    if (p.cm.N == 0) return hipSuccess;
    return im_dispatch_shape(M1, backlog, [&](auto M, auto B) {
        hipLaunchKernelGGL((im_reset_kernel<decltype(M)::value, decltype(B)::value>), dim3(grid_for(p.cm.N, 256)), dim3(256), 0, s,
                           p, mask, obs);
        return hipGetLastError();
    });
}

INVSIM_PTRS_STATS_TU(im)

#ifdef INVSIM_TIMING   // the profiling build's probe buffers (this object's only)
extern "C" int invsim_debug_timing(void *dst, int64_t bytes) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(invsim::g_tbuf), (size_t)bytes, 0, hipMemcpyDeviceToHost);
}
extern "C" int invsim_debug_timing_args(void *dst, int64_t bytes) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(invsim::g_targ), (size_t)bytes, 0, hipMemcpyDeviceToHost);
}
extern "C" int invsim_debug_timing_bar(void *dst, int64_t bytes) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(invsim::g_tbar), (size_t)bytes, 0, hipMemcpyDeviceToHost);
}
#endif
#endif

}  // namespace invsim
