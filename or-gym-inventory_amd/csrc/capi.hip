// C ABI of libinvsim (include/invsim.h): handle lifetime, HBM state arena,
// spec validation (the reference's assert checks), and kernel launches.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/invsim.h"
#include "kernels.hpp"
#include "launch.hpp"
#include "gae.hpp"
#include "mlp_policy.hpp"
#include "norm.hpp"
#include "ppo_grad.hpp"

using namespace invsim;

namespace {

thread_local std::string g_last_error;

struct Field {
    std::string name;
    int64_t offset;   // bytes from arena start
    int32_t elem;     // element bytes
    int32_t rows;     // rows, or record width
    int32_t kind;     // 0: [rows][Npad]; 1: record [Npad][rows]; 2: other (opaque)
};

}  // namespace

namespace invsim {
int net_spec_match(const invsim_netinvmgmt_spec &h);   // netspec.hip
#ifdef INVSIM_PTRS_STATS
hipError_t ptrs_stats_nv(unsigned long long *out, bool clear);
hipError_t ptrs_stats_nv_ph(unsigned long long *out, bool clear);
hipError_t ptrs_stats_im(unsigned long long *out, bool clear);
hipError_t ptrs_stats_im_ph(unsigned long long *out, bool clear);
hipError_t ptrs_stats_netspec(unsigned long long *out, bool clear);
hipError_t ptrs_stats_net(unsigned long long *out, bool clear);
#endif
}

struct invsim_handle {
    int32_t family = 0;
    int32_t device = 0;
    int64_t N = 0, Npad = 0;
    int32_t obs_dim = 0, act_dim = 0, demand_dim = 1;
    char *arena = nullptr;      // state (get/set_state blob)
    int64_t arena_bytes = 0;
    char *tables = nullptr;     // read-only tables (not part of the state blob)
    void *scratch = nullptr;    // caches derived from the state (not part of the blob)
    Lookahead la;               // demand lookahead cache (Nv/Im/NetParams::ahead): valid, and its current slot
    std::vector<Field> fields;
    Common cm{};
    NvParams nv{};
    ImParams im{};
    std::vector<double> im_ap;  // host copy of im.alpha_pow (the split step takes alpha ** t by value)
    NetParams net{};
    int32_t im_m1 = 0;
    bool im_backlog = false;
    int32_t net_spec = 0;     // NET_SPEC_*: compile-time specialised kernel for this graph
    // lock-step period tracking (see kernels.hpp next_period)
    bool t_known = true;
    int32_t t_cur = 0;
    int32_t horizon = 0;
    bool past_ok = false;     // Newsvendor keeps stepping past step_limit with autoreset off
    // demand stream (invsim_set_demand_stream): numpy PCG64 (parity) or the fast
    // counter-based Philox stream, whose launch-step counter lives here and in
    // the state blob ("philox_step")
    int32_t demand_stream = INVSIM_DEMAND_NUMPY;
    uint64_t ph_step = 0;
    int64_t o_phstep = 0;
    bool ph_from_blob = false;  // set_state loaded the blob: its philox_step is the counter
    // graph capture (invsim_capture_begin / _end): the host-side position at
    // begin, put back at end, and the env steps the captured calls enqueue
    bool capturing = false;
    bool cap_t_known = true;
    int32_t cap_t_cur = 0;
    Lookahead cap_la;
    int64_t cap_steps = 0;
    // RandomAgent's action generators (invsim_set_action_rng): caller-owned u64 [4][Npad], or null
    uint64_t *arng = nullptr;
    // the LEVELS policy's per-env parameters (invsim_set_policy_levels; on a NetInvMgmt handle NET_LEVELS',
    // invsim_set_policy_net_levels): caller-owned f64 [N][action_dim], or null
    const double *levels = nullptr, *reorder = nullptr;
    std::string err;
};

// An MLP actor of one handle (invsim_mlp_create): the kernel's argument block,
// the device blob it points into, and the closed loop's scratch rows.
struct invsim_mlp {
    invsim_handle *owner = nullptr;
    MlpDev dev{};               // host copy (launch geometry); the kernel reads dev_copy
    const MlpDev *dev_copy = nullptr;
    float *blob = nullptr;
    void *obs_row = nullptr;    // [N][O], obs dtype
    void *act_row = nullptr;    // [N][A], action dtype
    // the Gaussian around the output (invsim_mlp_set_gaussian): two [A] rows of the blob
    float *g_std = nullptr, *g_log_std = nullptr;
    bool gauss = false;
    float logp0 = 0.0f;         // (float)(-0.5 * log(2 pi) * A)
    bool value = false;         // a value network (invsim_mlp_create_value): one output, no conversion, no scratch rows
};

namespace {

// roctx range around an ABI call (SURVEY §5 tracing: step / rollout / reset
// show up as named ranges under `rocprofv3 --marker-trace`; a no-op call when
// no profiler is attached).  roctx is opened with dlopen at the first call, so
// libinvsim.so has no load-time dependency on it; without it ranges are no-ops.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        void *so = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!so) so = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!so) return;
        push = reinterpret_cast<int (*)(const char *)>(dlsym(so, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(so, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};

const Roctx &roctx() {
    static const Roctx r;
    return r;
}

struct TraceRange {
    explicit TraceRange(const char *name) {
        if (roctx().push) roctx().push(name);
    }
    ~TraceRange() {
        if (roctx().pop) roctx().pop();
    }
};

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

int fail(invsim_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    g_last_error = msg;
    return code;
}

void mlp_free(invsim_mlp *m) {
    if (m->blob) (void)hipFree(m->blob);
    if (m->obs_row) (void)hipFree(m->obs_row);
    if (m->act_row) (void)hipFree(m->act_row);
    delete m;
}

int hip_fail(invsim_handle *h, hipError_t e, const char *what) {
    return fail(h, INVSIM_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Calls that synchronise with the host cannot be recorded into a graph.
int refuse_in_capture(invsim_handle *h, const char *what) {
    if (!h->capturing) return INVSIM_OK;
    return fail(h, INVSIM_EINVAL, std::string(what) + " synchronises with the host and cannot be captured "
                                                      "(between invsim_capture_begin and invsim_capture_end)");
}

// A launching call on a stream that is being captured must be inside the
// capture bracket: otherwise the host-side position advances while the device
// state does not (nothing runs until the graph is replayed).
int capture_check(invsim_handle *h, hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();   // e.g. the legacy stream while another one captures: not ours to record
        st = hipStreamCaptureStatusNone;
    }
    if (st == hipStreamCaptureStatusActive && !h->capturing)
        return fail(h, INVSIM_EINVAL, "this stream is being captured into a graph: bracket the capture with "
                                      "invsim_capture_begin / invsim_capture_end");
    return INVSIM_OK;
}

// Lay out named SoA fields (rows x Npad elements each, 256-byte aligned).
struct Layout {
    std::vector<Field> f;
    int64_t bytes = 0;
    int64_t add(const char *name, int32_t elem, int32_t rows, int64_t npad, int32_t kind = 0) {
        bytes = (bytes + 255) / 256 * 256;
        Field x{name, bytes, elem, rows, kind};
        f.push_back(x);
        bytes += (int64_t)elem * rows * npad;
        return x.offset;
    }
};

template <typename T>
T *at(invsim_handle *h, int64_t off) {
    return reinterpret_cast<T *>(h->arena + off);
}

int alloc_arena(invsim_handle *h, const Layout &lay) {
    h->fields = lay.f;
    h->arena_bytes = std::max<int64_t>(lay.bytes, 256);
    hipError_t e = hipMalloc(&h->arena, (size_t)h->arena_bytes);
    if (e != hipSuccess) return fail(h, INVSIM_ENOMEM, std::string("hipMalloc(state): ") + hipGetErrorString(e));
    e = hipMemset(h->arena, 0, (size_t)h->arena_bytes);
    if (e != hipSuccess) return hip_fail(h, e, "hipMemset(state)");
    return INVSIM_OK;
}

int common_fields(invsim_handle *h, Layout &lay, int64_t &o_rng, int64_t &o_period, int64_t &o_status) {
    o_rng = lay.add("rng", 8, 4, h->Npad);   // rows: state_hi, state_lo, inc_hi, inc_lo
    o_period = lay.add("period", 4, 1, h->Npad);
    o_status = lay.add("status", 4, 1, 1);
    h->o_phstep = lay.add("philox_step", 8, 1, 1);
    return 0;
}

// The A/B launch switches (kernels.hpp Knobs), read from the environment once,
// here, when a handle is created: the only environment reads of the library.
// A flag is "0" or "1" exactly; anything else (unset, empty, "false", "on")
// keeps the default.
bool env_flag(const char *name, bool dflt) {
    const char *v = std::getenv(name);
    if (!v || (v[0] != '0' && v[0] != '1') || v[1]) return dflt;
    return v[0] == '1';
}

// A tri-state starts with '0' or '1' (off / on), else the default (-1).
int8_t env_tri(const char *name, int8_t dflt) {
    const char *v = std::getenv(name);
    return v && (v[0] == '0' || v[0] == '1') ? (int8_t)(v[0] - '0') : dflt;
}

// A count is a full non-negative decimal, else the default.
int64_t env_count(const char *name, int64_t dflt) {
    const char *v = std::getenv(name);
    if (!v || !v[0]) return dflt;
    char *end = nullptr;
    const long long x = std::strtoll(v, &end, 10);
    return end && !*end && x >= 0 ? (int64_t)x : dflt;
}

// One row per switch: the kind (flag, tri-state, count) is the member's type.
struct KnobRow {
    const char *env;
    enum { FLAG, TRI, COUNT } kind;
    union {
        bool Knobs::*flag;
        int8_t Knobs::*tri;
        int64_t Knobs::*count;
    };
    constexpr KnobRow(const char *e, bool Knobs::*m) : env(e), kind(FLAG), flag(m) {}
    constexpr KnobRow(const char *e, int8_t Knobs::*m) : env(e), kind(TRI), tri(m) {}
    constexpr KnobRow(const char *e, int64_t Knobs::*m) : env(e), kind(COUNT), count(m) {}
};

// The list of switches.  Defaults are the Knobs member initialisers.
const KnobRow KNOBS[] = {
    {"INVSIM_IM_SPLIT", &Knobs::im_split},                // =0: single steps on the one-wave kernel
    {"INVSIM_IM_ROLL", &Knobs::im_roll},                  // =0: rollouts on the one-wave kernel
    {"INVSIM_IM_POL_ROLL", &Knobs::im_pol_roll},          // =0: policy rollouts on im_run_kernel
    {"INVSIM_IM_AHEAD", &Knobs::im_ahead},                // =0: no demand lookahead
    {"INVSIM_IM_ROLL3O_G2", &Knobs::im_roll3o_g2},        // =1 / =0: two groups per workgroup on / off (default: policy rollouts only)
    {"INVSIM_IM_ROLL3O_MAX_N", &Knobs::im_roll3o_max_n},  // largest batch for the 3-role rollout
    {"INVSIM_IM_ROLL_SUB", &Knobs::im_roll_sub},          // 2-role rollouts as back-to-back launches of at most this many envs (0: one launch)
    {"INVSIM_NV_ROLL", &Knobs::nv_roll},                  // =0: rollouts on nv_run_kernel
    {"INVSIM_NV_POL_ROLL", &Knobs::nv_pol_roll},          // =0: policy rollouts on nv_run_kernel
    {"INVSIM_NV_AHEAD", &Knobs::nv_ahead},                // =0: no demand lookahead
    {"INVSIM_NET_ROLL", &Knobs::net_roll},                // =0: rollouts on net_spec_kernel
    {"INVSIM_NET_ROLL3", &Knobs::net_roll3},              // =0: net_roll_kernel instead of net_roll3o_kernel
    {"INVSIM_NET_SPLIT", &Knobs::net_split},              // =0: the step on the one-wave net_step1_kernel
    {"INVSIM_NET_POL_ROLL", &Knobs::net_pol_roll},        // =0: ConstantOrder rollouts on net_spec_kernel
    {"INVSIM_NET_AHEAD", &Knobs::net_ahead},              // =0: no demand lookahead
    {"INVSIM_NET_GENERIC", &Knobs::net_generic},          // =1: the generic kernel for the built-in graphs
    {"INVSIM_NET_ROLL4_MAX_N", &Knobs::net_roll4_max_n},  // largest batch for the 4-role Net rollout (0: never)
};

Knobs read_knobs() {
    Knobs k;
    for (const KnobRow &r : KNOBS) {
        switch (r.kind) {
            case KnobRow::FLAG: k.*r.flag = env_flag(r.env, k.*r.flag); break;
            case KnobRow::TRI: k.*r.tri = env_tri(r.env, k.*r.tri); break;
            case KnobRow::COUNT: k.*r.count = env_count(r.env, k.*r.count); break;
        }
    }
    return k;
}

void bind_common(invsim_handle *h, int64_t o_rng, int64_t o_period, int64_t o_status, int32_t ar) {
    Common &c = h->cm;
    c.kn = read_knobs();
    c.N = h->N;
    c.Npad = h->Npad;
    c.autoreset = ar;
    uint64_t *r = at<uint64_t>(h, o_rng);
    c.rng.hi = r;
    c.rng.lo = r + h->Npad;
    c.rng.inc_hi = r + 2 * h->Npad;
    c.rng.inc_lo = r + 3 * h->Npad;
    c.period = at<int32_t>(h, o_period);
    c.status = at<uint32_t>(h, o_status);
    c.info_demand = nullptr;
    c.u32buf = nullptr;
    c.info_rec = nullptr;
}

// "done" marker: period = horizon, so NEXT_STEP autoreset resets on first step
int init_period(invsim_handle *h, int32_t horizon) {
    h->horizon = horizon;
    h->t_known = true;
    h->t_cur = horizon;  // "done": the first NEXT_STEP step resets
    std::vector<int32_t> v((size_t)h->Npad, horizon);
    hipError_t e = hipMemcpy(h->cm.period, v.data(), sizeof(int32_t) * h->Npad, hipMemcpyHostToDevice);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "hipMemcpy(period)");
}

int upload_tables(invsim_handle *h, const std::vector<char> &blob) {
    if (blob.empty()) return INVSIM_OK;
    hipError_t e = hipMalloc(&h->tables, blob.size());
    if (e != hipSuccess) return fail(h, INVSIM_ENOMEM, "hipMalloc(tables)");
    e = hipMemcpy(h->tables, blob.data(), blob.size(), hipMemcpyHostToDevice);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "hipMemcpy(tables)");
}

// host-side packer for read-only tables
struct Blob {
    std::vector<char> b;
    template <typename T>
    int64_t put(const T *p, size_t n) {
        size_t off = (b.size() + 15) / 16 * 16;
        b.resize(off + std::max<size_t>(n, 1) * sizeof(T), 0);
        if (p && n) std::memcpy(b.data() + off, p, n * sizeof(T));
        return (int64_t)off;
    }
};

template <typename T>
const T *tab(invsim_handle *h, int64_t off) {
    return reinterpret_cast<const T *>(h->tables + off);
}

bool valid_autoreset(int32_t m) { return m >= 0 && m <= 2; }

int finish_create(invsim_handle *h, invsim_handle **out, int rc) {
    if (rc != INVSIM_OK) {
        g_last_error = h->err;
        invsim_destroy(h);
        *out = nullptr;
        return rc;
    }
    *out = h;
    return INVSIM_OK;
}

// (rhs_table, the host table of PTRS's right-hand side: ptrs_table.hpp)

}  // namespace

extern "C" {

int invsim_abi_version(void) { return INVSIM_ABI_VERSION; }

const char *invsim_last_error(const invsim_handle *h) {
    return h ? h->err.c_str() : g_last_error.c_str();
}

void invsim_destroy(invsim_handle *h) {
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->arena) (void)hipFree(h->arena);
    if (h->tables) (void)hipFree(h->tables);
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
}

// ------------------------------------------------------------------ Newsvendor
int invsim_create_newsvendor(const invsim_newsvendor_spec *spec, int64_t n, int32_t device,
                             int32_t ar, invsim_handle **out) {
    if (!spec || !out) return fail(nullptr, INVSIM_EINVAL, "null argument");
    if (n < 0 || n > (int64_t)1 << 31) return fail(nullptr, INVSIM_EINVAL, "n_envs out of range");
    if (!valid_autoreset(ar)) return fail(nullptr, INVSIM_EINVAL, "bad autoreset mode");
    const int L = std::max(0, spec->lead_time);  // newsvendor.py:65
    if (L > 128) return fail(nullptr, INVSIM_ERANGE, "lead_time > 128 not supported");
    if (!(spec->mu_max >= 0) || spec->mu_max > 1e18)
        return fail(nullptr, INVSIM_EINVAL, "mu_max must be in [0, 1e18] (numpy poisson lam range)");
    DeviceGuard g(device);
    if (!g.ok) return fail(nullptr, INVSIM_EDEVICE, "hipSetDevice failed");
    auto *h = new invsim_handle();
    h->family = INVSIM_NEWSVENDOR;
    h->device = device;
    h->N = n;
    h->Npad = pad_n(n);
    h->obs_dim = L + 5;
    h->act_dim = 1;
    Layout lay;
    int64_t o_rng, o_per, o_st;
    common_fields(h, lay, o_rng, o_per, o_st);
    int64_t o_par = lay.add("params", 8, 5, h->Npad);
    int64_t o_pipe = lay.add("pipeline", 4, std::max(L, 1), h->Npad);
    // loggam(k + 1) for the per-env PTRS right-hand side (numpy's formula, host libm)
    Blob tb;
    std::vector<double> lg(RHS_LDS_MAX);
    for (int k = 0; k < RHS_LDS_MAX; k++) lg[k] = np_loggam((double)(k + 1));
    const int64_t t_lg = tb.put(lg.data(), lg.size());
    int rc = alloc_arena(h, lay);
    if (rc == INVSIM_OK) rc = upload_tables(h, tb.b);
    if (rc == INVSIM_OK) {
        bind_common(h, o_rng, o_per, o_st, ar);
        NvParams &p = h->nv;
        p.lgtab = tab<double>(h, t_lg);
        p.cm = h->cm;
        p.L = L;
        p.step_limit = spec->step_limit;
        p.max_inventory = spec->max_inventory;
        p.max_order = spec->max_order_quantity;
        p.p_max = spec->p_max;
        p.h_max = spec->h_max;
        p.k_max = spec->k_max;
        p.mu_max = spec->mu_max;
        p.par = at<double>(h, o_par);
        p.pipe = at<float>(h, o_pipe);
        p.ahead = nullptr;
        p.pcon = nullptr;
        {   // demand lookahead cache: 2 slots x 3 rows x Npad u64, then 6 rows of Poisson constants
            hipError_t e = hipMalloc(&h->scratch, (size_t)((2 * 3 + 6) * h->Npad * sizeof(uint64_t)));
            if (e != hipSuccess) {
                rc = fail(h, INVSIM_ENOMEM, "hipMalloc(lookahead cache)");
            } else {
                p.ahead = static_cast<uint64_t *>(h->scratch);
                p.pcon = reinterpret_cast<double *>(p.ahead + 2 * 3 * h->Npad);
            }
        }
        h->past_ok = true;
        if (rc == INVSIM_OK) rc = init_period(h, std::max(spec->step_limit, 0));
    }
    return finish_create(h, out, rc);
}

// ------------------------------------------------------------------ InvMgmt
int invsim_create_invmgmt(const invsim_invmgmt_spec *s, int64_t n, int32_t device, int32_t ar,
                          invsim_handle **out) {
    if (!s || !out) return fail(nullptr, INVSIM_EINVAL, "null argument");
    if (n < 0 || n > (int64_t)1 << 31) return fail(nullptr, INVSIM_EINVAL, "n_envs out of range");
    if (!valid_autoreset(ar)) return fail(nullptr, INVSIM_EINVAL, "bad autoreset mode");
    const int m = s->num_stages, m1 = m - 1;
    // inventory_management.py:144-167 validation
    if (m < 2) return fail(nullptr, INVSIM_EINVAL, "Minimum number of stages is 2");
    if (m1 > IM_MAX_M1) return fail(nullptr, INVSIM_ERANGE, "at most 9 stages supported");
    if (s->periods <= 0) return fail(nullptr, INVSIM_EINVAL, "Number of periods must be positive");
    if (!s->I0 || !s->unit_price || !s->unit_cost || !s->demand_cost || !s->holding_cost ||
        !s->supply_capacity || !s->lead_time)
        return fail(nullptr, INVSIM_EINVAL, "null parameter array");
    for (int i = 0; i < m1; i++) {
        if (s->I0[i] < 0) return fail(nullptr, INVSIM_EINVAL, "Initial inventory cannot be negative");
        if (s->supply_capacity[i] <= 0) return fail(nullptr, INVSIM_EINVAL, "Supply capacities must be positive");
        if (s->lead_time[i] < 0) return fail(nullptr, INVSIM_EINVAL, "Lead times cannot be negative");
        if (s->lead_time[i] > 255) return fail(nullptr, INVSIM_ERANGE, "lead time > 255 not supported");
    }
    for (int j = 0; j < m; j++) {
        if (!(s->unit_price[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Sales prices cannot be negative");
        if (!(s->unit_cost[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Procurement costs cannot be negative");
        if (!(s->demand_cost[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Unfulfilled demand costs cannot be negative");
        if (!(s->holding_cost[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Holding costs cannot be negative");
    }
    if (!(s->alpha > 0 && s->alpha <= 1)) return fail(nullptr, INVSIM_EINVAL, "alpha must be in the range (0, 1]");
    if (s->dist == 1) {
        if (!(s->mu >= 0) || s->mu > 1e18) return fail(nullptr, INVSIM_EINVAL, "poisson mu out of range");
    } else if (s->dist == 5) {
        if (!s->user_D) return fail(nullptr, INVSIM_EINVAL, "User specified demand length != num periods");
    } else if (s->dist == 2) {   // numpy Generator.binomial argument checks
        if (s->dist_n < 0) return fail(nullptr, INVSIM_EINVAL, "n < 0");
        if (!(s->dist_p >= 0 && s->dist_p <= 1)) return fail(nullptr, INVSIM_EINVAL, "p < 0, p > 1 or p is NaN");
    } else if (s->dist == 3) {   // Generator.integers(low, high + 1)
        if (s->dist_high == INT64_MAX) return fail(nullptr, INVSIM_EINVAL, "high is out of bounds for int64");
        if (s->dist_low > s->dist_high) return fail(nullptr, INVSIM_EINVAL, "low >= high");
    } else if (s->dist == 4) {   // Generator.geometric
        if (!(s->dist_p > 0 && s->dist_p <= 1)) return fail(nullptr, INVSIM_EINVAL, "p <= 0, p > 1 or p contains NaNs");
    } else {
        return fail(nullptr, INVSIM_EINVAL, "dist must be one of 1, 2, 3, 4, 5");
    }
    int D = 0, sumL = 0;
    for (int i = 0; i < m1; i++) {
        D = std::max<int>(D, (int)s->lead_time[i]);
        sumL += (int)s->lead_time[i];
    }
    // the largest dynamic LDS a launch of this handle asks (the split step's: a
    // wave's obs window tile, the PTRS table, one int64 per lane): with 160 KiB
    // that is an observation length (m-1)*(max(L)+1) of at most 311
    if (im_split_lds_bytes(m1, D) > LDS_LIMIT_BYTES)
        return fail(nullptr, INVSIM_ERANGE, "observation length (m-1)*(max(L)+1) too large for the LDS window tile (at most 311)");
    DeviceGuard g(device);
    if (!g.ok) return fail(nullptr, INVSIM_EDEVICE, "hipSetDevice failed");
    auto *h = new invsim_handle();
    h->family = INVSIM_INVMGMT;
    h->device = device;
    h->N = n;
    h->Npad = pad_n(n);
    h->obs_dim = m1 * (D + 1);
    h->act_dim = m1;
    h->im_m1 = m1;
    h->im_backlog = s->backlog != 0;
    Layout lay;
    int64_t o_rng, o_per, o_st;
    common_fields(h, lay, o_rng, o_per, o_st);
    int64_t o_I = lay.add("I", 8, m1, h->Npad);
    int64_t o_B = lay.add("B", 8, h->im_backlog ? m : 1, h->Npad);
    int64_t o_R = lay.add("Rring", 8, std::max(sumL, 1), h->Npad);
    int64_t o_A = lay.add("alog", 8, std::max(D * m1, 1), h->Npad, 2);      // [D][Npad][m1]
    int64_t o_A32 = lay.add("alog32", 4, std::max(D * m1, 1), h->Npad, 2);  // [D][Npad][m1]
    // Generator.integers draws 32-bit halves: the bit generator's buffered half is
    // state (the dist 2-4 kernel variant carries the row; only dist 3 uses it)
    const int64_t o_U32 = (s->dist >= 2 && s->dist <= 4) ? lay.add("u32buf", 8, 1, h->Npad) : -1;
    // read-only tables: alpha**t (Python float pow == C pow), user_D
    Blob tb;
    std::vector<double> ap((size_t)s->periods);
    for (int t = 0; t < s->periods; t++) ap[t] = std::pow(s->alpha, (double)t);
    int64_t o_ap = tb.put(ap.data(), ap.size());
    std::vector<int64_t> ud((size_t)s->periods, 0);
    if (s->dist == 5) std::memcpy(ud.data(), s->user_D, sizeof(int64_t) * s->periods);
    int64_t o_ud = tb.put(ud.data(), ud.size());
    PtrsConst pc = ptrs_const(s->dist == 1 ? s->mu : 0.0);  // host libm, as numpy
    std::vector<double> rhs;
    rhs_table(pc, rhs);
    const int64_t o_rhs = tb.put(rhs.data(), rhs.size());
    int rc = alloc_arena(h, lay);
    if (rc == INVSIM_OK) rc = upload_tables(h, tb.b);
    if (rc == INVSIM_OK) {
        bind_common(h, o_rng, o_per, o_st, ar);
        if (o_U32 >= 0) h->cm.u32buf = at<uint64_t>(h, o_U32);
        ImParams &p = h->im;
        p.rhs = pc.nk > 0 ? tab<double>(h, o_rhs) : nullptr;
        p.cm = h->cm;
        if (s->dist == 2) p.nd = np_dist_binomial(s->dist_n, s->dist_p);
        if (s->dist == 3) p.nd = np_dist_integers(s->dist_low, s->dist_high);
        if (s->dist == 4) p.nd = np_dist_geometric(s->dist_p);
        p.periods = s->periods;
        p.lt_max = D;
        p.dist = s->dist;
        int off = 0;
        for (int i = 0; i < m1; i++) {
            p.L[i] = (int32_t)s->lead_time[i];
            p.ring_off[i] = off;
            off += p.L[i];
            p.c[i] = s->supply_capacity[i];
            p.I0[i] = s->I0[i];
        }
        for (int j = 0; j < m; j++) {
            p.up[j] = (double)s->unit_price[j];
            p.uc[j] = (double)s->unit_cost[j];
            p.hc[j] = (double)s->holding_cost[j];
            p.kc[j] = (double)s->demand_cost[j];
        }
        p.pc = pc;
        p.alpha_pow = tab<double>(h, o_ap);
        h->im_ap = ap;
        p.user_D = tab<int64_t>(h, o_ud);
        p.I = at<int64_t>(h, o_I);
        p.B = at<int64_t>(h, o_B);
        p.Rring = at<int64_t>(h, o_R);
        p.alog = at<int64_t>(h, o_A);
        p.alog32 = at<uint32_t>(h, o_A32);
        p.ahead = nullptr;
        if (s->dist >= 1 && s->dist <= 4) {   // demand lookahead cache: 2 slots x 4 rows x Npad u64
            hipError_t e = hipMalloc(&h->scratch, (size_t)(2 * 4 * h->Npad * sizeof(uint64_t)));
            if (e != hipSuccess) rc = fail(h, INVSIM_ENOMEM, "hipMalloc(lookahead cache)");
            else p.ahead = static_cast<uint64_t *>(h->scratch);
        }
        if (rc == INVSIM_OK) rc = init_period(h, s->periods);
    }
    return finish_create(h, out, rc);
}

// ------------------------------------------------------------------ NetInvMgmt
int invsim_create_netinvmgmt(const invsim_netinvmgmt_spec *s, int64_t n, int32_t device, int32_t ar,
                             invsim_handle **out) {
    if (!s || !out) return fail(nullptr, INVSIM_EINVAL, "null argument");
    if (n < 0 || n > (int64_t)1 << 31) return fail(nullptr, INVSIM_EINVAL, "n_envs out of range");
    if (!valid_autoreset(ar)) return fail(nullptr, INVSIM_EINVAL, "bad autoreset mode");
    const int J = s->n_main, E = s->n_reorder, RL = s->n_retail;
    if (J < 1 || E < 0 || RL < 0 || J > 64 || E > 256 || RL > 64)
        return fail(nullptr, INVSIM_ERANGE, "topology size out of supported range");
    if (s->num_periods <= 0) return fail(nullptr, INVSIM_EINVAL, "num_periods must be positive");
    if (!(s->alpha > 0 && s->alpha <= 1)) return fail(nullptr, INVSIM_EINVAL, "alpha must be in (0, 1]");
    if (!s->I0 || !s->h || !s->C || !s->o || !s->v || !s->is_factory || !s->is_retail ||
        (E && (!s->sup || !s->pur || !s->sup_is_factory || !s->L || !s->lp || !s->lg)) ||
        (RL && (!s->rl_node || !s->rl_p || !s->rl_b || !s->rl_lam || !s->rl_user)) ||
        !s->succ_ptr || !s->pred_ptr)
        return fail(nullptr, INVSIM_EINVAL, "null topology table");
    // network_management.py:197-238 validation
    for (int j = 0; j < J; j++) {
        if (!(s->I0[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing I0>=0");
        if (!(s->h[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing h>=0");
        if (s->is_factory[j]) {
            if (!(s->C[j] > 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing C>0");
            if (!(s->o[j] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing o>=0");
            if (!(s->v[j] > 0 && s->v[j] <= 1)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing v in (0, 1]");
        }
        if (!(s->v[j] > 0)) return fail(nullptr, INVSIM_EINVAL, "yield v must be > 0");
    }
    int sumL = 0;
    for (int k = 0; k < E; k++) {
        if (s->L[k] < 0 || s->L[k] > 255) return fail(nullptr, INVSIM_ERANGE, "Invalid or missing L>=0 (max 255)");
        if (!(s->lp[k] >= 0) || !(s->lg[k] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing p/g>=0");
        if (s->sup[k] < -1 || s->sup[k] >= J || s->pur[k] < 0 || s->pur[k] >= J)
            return fail(nullptr, INVSIM_EINVAL, "reorder link endpoint out of range");
        sumL += s->L[k];
    }
    for (int r = 0; r < RL; r++) {
        if (s->rl_node[r] < 0 || s->rl_node[r] >= J) return fail(nullptr, INVSIM_EINVAL, "retail link node out of range");
        if (!(s->rl_p[r] >= 0) || !(s->rl_b[r] >= 0)) return fail(nullptr, INVSIM_EINVAL, "Invalid or missing p/b>=0");
        const int dk = s->rl_dist ? s->rl_dist[r] : 1;
        if (!s->rl_user[r]) {
            if (dk < 1 || dk > 4) return fail(nullptr, INVSIM_EINVAL, "market sampler must be 1..4");
            if (dk == 1 && (!(s->rl_lam[r] >= 0) || s->rl_lam[r] > 1e18))
                return fail(nullptr, INVSIM_EINVAL, "poisson lam out of range");
            if (dk > 1 && (!s->rl_n || !s->rl_high || !s->rl_dp)) return fail(nullptr, INVSIM_EINVAL, "null market sampler table");
            if (dk == 2 && (s->rl_n[r] < 0 || !(s->rl_dp[r] >= 0 && s->rl_dp[r] <= 1)))
                return fail(nullptr, INVSIM_EINVAL, "binomial market needs n >= 0 and 0 <= p <= 1");
            if (dk == 3 && !(s->rl_high[r] > s->rl_n[r]))
                return fail(nullptr, INVSIM_EINVAL, "integers market: low >= high");
            if (dk == 4 && !(s->rl_dp[r] > 0 && s->rl_dp[r] <= 1))
                return fail(nullptr, INVSIM_EINVAL, "geometric market needs 0 < p <= 1");
        }
        if (s->rl_user[r] && !s->user_D) return fail(nullptr, INVSIM_EINVAL, "user_D table missing");
    }
    const int nsucc = s->succ_ptr[J], npred = s->pred_ptr[J];
    if (nsucc < 0 || npred < 0 || (nsucc && (!s->succ_kind || !s->succ_idx)) || (npred && !s->pred_idx))
        return fail(nullptr, INVSIM_EINVAL, "bad adjacency tables");
    for (int q = 0; q < nsucc; q++) {
        if (s->succ_kind[q] == 0 ? (s->succ_idx[q] < 0 || s->succ_idx[q] >= E)
                                 : (s->succ_idx[q] < 0 || s->succ_idx[q] >= RL))
            return fail(nullptr, INVSIM_EINVAL, "successor index out of range");
    }
    for (int q = 0; q < npred; q++)
        if (s->pred_idx[q] < 0 || s->pred_idx[q] >= E) return fail(nullptr, INVSIM_EINVAL, "predecessor index out of range");
    DeviceGuard g(device);
    if (!g.ok) return fail(nullptr, INVSIM_EDEVICE, "hipSetDevice failed");
    auto *h = new invsim_handle();
    h->family = INVSIM_NETINVMGMT;
    h->device = device;
    h->N = n;
    h->Npad = pad_n(n);
    h->obs_dim = RL + J + sumL;
    h->act_dim = E;
    h->demand_dim = std::max(RL, 1);
    Layout lay;
    int64_t o_rng, o_per, o_st;
    common_fields(h, lay, o_rng, o_per, o_st);
    int64_t o_X = lay.add("X", 8, J, h->Npad);
    int64_t o_U = lay.add("U", 8, std::max(RL, 1), h->Npad);
    int64_t o_Y = lay.add("Y", 8, std::max(E, 1), h->Npad);
    int64_t o_R = lay.add("Rring", 8, std::max(sumL, 1), h->Npad);
    bool any_int = false, any_npd = false;
    std::vector<int32_t> rdist((size_t)std::max(RL, 1), 1);
    std::vector<NpDist> rnd((size_t)std::max(RL, 1));
    for (int r = 0; r < RL; r++) {
        rdist[r] = (s->rl_dist && !s->rl_user[r]) ? s->rl_dist[r] : 1;
        if (rdist[r] == 2) rnd[r] = np_dist_binomial(s->rl_n[r], s->rl_dp[r]);
        if (rdist[r] == 3) rnd[r] = np_dist_integers(s->rl_n[r], s->rl_high[r] - 1);
        if (rdist[r] == 4) rnd[r] = np_dist_geometric(s->rl_dp[r]);
        any_int = any_int || rdist[r] == 3;
        any_npd = any_npd || rdist[r] > 1;
    }
    // numpy's buffered 32-bit half of the bit generator (integers markets only)
    const int64_t o_U32 = any_int ? lay.add("u32buf", 8, 1, h->Npad) : -1;
    Blob tb;
    int64_t t_I0 = tb.put(s->I0, J), t_h = tb.put(s->h, J), t_C = tb.put(s->C, J),
            t_o = tb.put(s->o, J), t_v = tb.put(s->v, J);
    int64_t t_if = tb.put(s->is_factory, J), t_ir = tb.put(s->is_retail, J);
    int64_t t_sup = tb.put(s->sup, E), t_pur = tb.put(s->pur, E), t_sf = tb.put(s->sup_is_factory, E),
            t_L = tb.put(s->L, E), t_lp = tb.put(s->lp, E), t_lg = tb.put(s->lg, E);
    std::vector<int32_t> roff((size_t)std::max(E, 1), 0);
    for (int k = 0, off = 0; k < E; k++) {
        roff[k] = off;
        off += s->L[k];
    }
    int64_t t_ro = tb.put(roff.data(), roff.size());
    std::vector<int32_t> woff((size_t)std::max(E, 1), 0);  // obs offset of each link's order window
    for (int k = 0, off = RL + J; k < E; k++) {
        woff[k] = off;
        off += s->L[k];
    }
    int64_t t_wo = tb.put(woff.data(), woff.size());
    int64_t t_rn = tb.put(s->rl_node, RL), t_ru = tb.put(s->rl_user, RL), t_rp = tb.put(s->rl_p, RL),
            t_rb = tb.put(s->rl_b, RL);
    std::vector<PtrsConst> pcs((size_t)std::max(RL, 1));
    std::vector<double> rhs;
    for (int r = 0; r < RL; r++) {
        pcs[r] = ptrs_const(s->rl_user[r] ? 0.0 : s->rl_lam[r]);
        rhs_table(pcs[r], rhs);
    }
    int64_t t_pc = tb.put(pcs.data(), pcs.size());
    int64_t t_rhs = tb.put(rhs.data(), rhs.size());
    int64_t t_rd = tb.put(rdist.data(), rdist.size()), t_rnd = tb.put(rnd.data(), rnd.size());
    std::vector<double> ud((size_t)std::max(RL, 1) * s->num_periods, 0.0);
    if (s->user_D) std::memcpy(ud.data(), s->user_D, sizeof(double) * RL * s->num_periods);
    int64_t t_ud = tb.put(ud.data(), ud.size());
    int64_t t_sp = tb.put(s->succ_ptr, J + 1), t_sk = tb.put(s->succ_kind, nsucc),
            t_sx = tb.put(s->succ_idx, nsucc), t_pp = tb.put(s->pred_ptr, J + 1),
            t_px = tb.put(s->pred_idx, npred);
    std::vector<double> ap((size_t)s->num_periods);
    for (int t = 0; t < s->num_periods; t++) ap[t] = std::pow(s->alpha, (double)t);
    int64_t t_ap = tb.put(ap.data(), ap.size());
    int rc = alloc_arena(h, lay);
    if (rc == INVSIM_OK) rc = upload_tables(h, tb.b);
    if (rc == INVSIM_OK) {
        bind_common(h, o_rng, o_per, o_st, ar);
        NetParams &p = h->net;
        p.J = J;
        p.E = E;
        p.RL = RL;
        p.sumL = sumL;
        if (net_lds_bytes(p) > LDS_LIMIT_BYTES) rc = fail(h, INVSIM_ERANGE, "topology too large for the LDS scratch");
    }
    if (rc == INVSIM_OK) {
        NetParams &p = h->net;
        p.cm = h->cm;
        p.J = J;
        p.E = E;
        p.RL = RL;
        p.T = s->num_periods;
        p.backlog = s->backlog != 0;
        p.sumL = sumL;
        p.I0 = tab<double>(h, t_I0);
        p.h = tab<double>(h, t_h);
        p.C = tab<double>(h, t_C);
        p.o = tab<double>(h, t_o);
        p.v = tab<double>(h, t_v);
        p.is_factory = tab<int32_t>(h, t_if);
        p.is_retail = tab<int32_t>(h, t_ir);
        p.sup = tab<int32_t>(h, t_sup);
        p.pur = tab<int32_t>(h, t_pur);
        p.sup_is_factory = tab<int32_t>(h, t_sf);
        p.L = tab<int32_t>(h, t_L);
        p.ring_off = tab<int32_t>(h, t_ro);
        p.lp = tab<double>(h, t_lp);
        p.lg = tab<double>(h, t_lg);
        p.rl_node = tab<int32_t>(h, t_rn);
        p.rl_user = tab<int32_t>(h, t_ru);
        p.rl_p = tab<double>(h, t_rp);
        p.rl_b = tab<double>(h, t_rb);
        p.rl_pc = tab<PtrsConst>(h, t_pc);
        p.rl_dist = any_npd ? tab<int32_t>(h, t_rd) : nullptr;
        p.rl_nd = tab<NpDist>(h, t_rnd);
        if (o_U32 >= 0) h->cm.u32buf = at<uint64_t>(h, o_U32);
        p.cm = h->cm;
        p.rhs = rhs.empty() ? nullptr : tab<double>(h, t_rhs);
        p.win_off = tab<int32_t>(h, t_wo);
        p.user_D = tab<double>(h, t_ud);
        p.succ_ptr = tab<int32_t>(h, t_sp);
        p.succ_kind = tab<int32_t>(h, t_sk);
        p.succ_idx = tab<int32_t>(h, t_sx);
        p.pred_ptr = tab<int32_t>(h, t_pp);
        p.pred_idx = tab<int32_t>(h, t_px);
        p.alpha_pow = tab<double>(h, t_ap);
        p.X = at<double>(h, o_X);
        p.U = at<double>(h, o_U);
        p.Y = at<double>(h, o_Y);
        p.Rring = at<double>(h, o_R);
        rc = init_period(h, s->num_periods);
        // the reference's own graphs run the compile-time specialised kernel
        // (INVSIM_NET_GENERIC=1 forces the generic one, for cross-checks)
        h->net_spec = h->cm.kn.net_generic ? NET_SPEC_NONE : net_spec_match(*s);
        p.ahead = nullptr;
        if (rc == INVSIM_OK && h->net_spec != NET_SPEC_NONE) {   // lookahead cache: 2 slots x (2 + RL) rows
            hipError_t e = hipMalloc(&h->scratch, (size_t)(2 * (2 + p.RL) * h->Npad * sizeof(uint64_t)));
            if (e != hipSuccess) rc = fail(h, INVSIM_ENOMEM, "hipMalloc(lookahead cache)");
            else p.ahead = static_cast<uint64_t *>(h->scratch);
        }
    }
    return finish_create(h, out, rc);
}

// ------------------------------------------------------------------ common entry points
int invsim_dims(const invsim_handle *h, int32_t *obs_dim, int32_t *action_dim, int32_t *demand_dim,
                int32_t *family) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (obs_dim) *obs_dim = h->obs_dim;
    if (action_dim) *action_dim = h->act_dim;
    if (demand_dim) *demand_dim = h->demand_dim;
    if (family) *family = h->family;
    return INVSIM_OK;
}

static void sync_common(invsim_handle *h) {
    h->nv.cm = h->cm;
    h->im.cm = h->cm;
    h->net.cm = h->cm;
}

// the fast stream's counter into the kernel parameters (after set_state: from
// the blob first, which is the one synchronising read of that stream)
static int ph_counter_sync(invsim_handle *h, hipStream_t s) {
    if (h->ph_from_blob) {
        hipError_t e = hipMemcpyAsync(&h->ph_step, h->arena + h->o_phstep, sizeof(uint64_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(h, e, "philox_step read");
        h->ph_from_blob = false;
    }
    h->cm.ph_step = h->ph_step;
    sync_common(h);
    return INVSIM_OK;
}


int invsim_set_autoreset(invsim_handle *h, int32_t mode) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_autoreset")) return rc;
    if (!valid_autoreset(mode)) return fail(h, INVSIM_EINVAL, "bad autoreset mode");
    h->cm.autoreset = mode;
    sync_common(h);
    return INVSIM_OK;
}

static int info_record_dim(const invsim_handle *h) {
    if (h->family == INVSIM_INVMGMT) return 2 * (h->im_m1 + 1) + 5;
    if (h->family == INVSIM_NETINVMGMT) return 2 * h->net.RL + 2 * h->net.J + 2 * h->net.E;
    if (h->family == INVSIM_NEWSVENDOR) return 5;
    return 0;
}

int invsim_info_record_dim(const invsim_handle *h, int32_t *dim) {
    if (!h || !dim) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *dim = info_record_dim(h);
    return INVSIM_OK;
}

int invsim_set_info_record(invsim_handle *h, void *record) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_info_record")) return rc;
    if (record && info_record_dim(h) == 0) return fail(h, INVSIM_EINVAL, "this env family has no step record");
    h->cm.info_rec = record;
    sync_common(h);
    return INVSIM_OK;
}

int invsim_set_info_demand(invsim_handle *h, int64_t *demand) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_info_demand")) return rc;
    h->cm.info_demand = demand;
    sync_common(h);
    return INVSIM_OK;
}

// bring cm.rng up to date from the demand lookahead cache (the cache stays valid)
static int commit_rng(invsim_handle *h, hipStream_t s) {
    // a fast-stream cache holds demands only (set_demand_stream drops the other kind)
    if (!h->la.valid || h->demand_stream == INVSIM_DEMAND_PHILOX) return INVSIM_OK;
    hipError_t e = hipSuccess;
    if (h->family == INVSIM_INVMGMT) e = im_commit_launch(h->im, h->la.slot, s);
    else if (h->family == INVSIM_NEWSVENDOR) e = nv_commit_launch(h->nv, h->la.slot, s);
    else if (h->family == INVSIM_NETINVMGMT) e = net_commit_launch(h->net, h->la.slot, s);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "rng commit");
}

// An unmasked seed restarts the fast stream's launch-step counter, so the same
// seeds give the same demands again (gymnasium's reset(seed=s) contract); a
// masked one keeps it, since the other envs' streams continue.
static void ph_counter_restart(invsim_handle *h) {
    h->ph_step = 0;
    h->ph_from_blob = false;
    h->cm.ph_step = 0;
    sync_common(h);
}

int invsim_seed_range(invsim_handle *h, uint64_t base_lo, uint64_t base_hi, int64_t first,
                      const uint8_t *mask, void *stream) {
    TraceRange tr_("invsim_seed_range");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (first < 0) return fail(h, INVSIM_EINVAL, "first_index must be >= 0");
    if (int rc = capture_check(h, (hipStream_t)stream)) return rc;
    DeviceGuard g(h->device);
    int rc = commit_rng(h, (hipStream_t)stream);   // a masked seed keeps the other streams
    if (rc != INVSIM_OK) return rc;
    h->la.valid = false;   // the lookahead cache follows the old streams
    if (!mask) ph_counter_restart(h);
    hipError_t e = seed_range_launch(h->cm, base_lo, base_hi, first, mask, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "seed_range launch");
}

int invsim_seed_words(invsim_handle *h, const uint32_t *words, const int32_t *nwords,
                      const uint8_t *mask, void *stream) {
    TraceRange tr_("invsim_seed_words");
    if (!h || (!words && h->N) || (!nwords && h->N)) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = capture_check(h, (hipStream_t)stream)) return rc;
    DeviceGuard g(h->device);
    int rc = commit_rng(h, (hipStream_t)stream);
    if (rc != INVSIM_OK) return rc;
    h->la.valid = false;
    if (!mask) ph_counter_restart(h);
    hipError_t e = seed_words_launch(h->cm, words, nwords, mask, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "seed_words launch");
}

// materialise the lock-step period into the per-env row before it stops being uniform
static int materialize_period(invsim_handle *h, hipStream_t s) {
    if (!h->t_known) return INVSIM_OK;
    hipError_t e = period_fill_launch(h->cm, h->t_cur, s);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "period fill");
}

int invsim_reset(invsim_handle *h, const uint8_t *mask, void *obs, void *stream) {
    TraceRange tr_("invsim_reset");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = capture_check(h, (hipStream_t)stream)) return rc;
    if (h->capturing && h->demand_stream == INVSIM_DEMAND_PHILOX)
        return fail(h, INVSIM_EINVAL, "graph capture needs the numpy demand stream");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (mask) {
        int rc = materialize_period(h, s);
        if (rc != INVSIM_OK) return rc;
    }
    if (h->family == INVSIM_NEWSVENDOR) {   // its reset draws from cm.rng (or the fast stream)
        int rc = commit_rng(h, s);
        if (rc != INVSIM_OK) return rc;
        h->la.valid = false;
        if (h->demand_stream == INVSIM_DEMAND_PHILOX) {
            rc = ph_counter_sync(h, s);
            if (rc != INVSIM_OK) return rc;
            h->ph_step += 1;                  // the reset's uniforms own a counter value
        }
    }
    hipError_t e = hipSuccess;
    switch (h->family) {
        case INVSIM_NEWSVENDOR: e = nv_reset_launch(h->nv, mask, (float *)obs, s); break;
        case INVSIM_INVMGMT: e = im_reset_launch(h->im, h->im_m1, h->im_backlog, mask, (int64_t *)obs, s); break;
        case INVSIM_NETINVMGMT: e = net_reset_launch(h->net, mask, (float *)obs, s); break;
        default: return fail(h, INVSIM_EINVAL, "bad handle family");
    }
    if (e != hipSuccess) return hip_fail(h, e, "reset launch");
    // episode sink: the reset envs abandon their episode, so their running
    // return restarts (the harness zeroes episode_reward at every reset,
    // benchmark_InvManagementBacklogEnv.py:368-371); nothing finished, part stays
    if (h->cm.ep_ret) {
        e = episode_ret_reset_launch(h->cm.ep_ret, mask, h->N, s);
        if (e != hipSuccess) return hip_fail(h, e, "episode sink reset");
    }
    if (mask) {
        h->t_known = false;
    } else {
        h->t_known = true;
        h->t_cur = 0;
    }
    return INVSIM_OK;
}

// A call that steps every env K times is steps_begin (every refusal that needs
// no device work, for all K steps, before the first launch), one or more
// steps_launch whose step counts add up to K, and steps_end.  run_steps is the
// three in a row; invsim_rollout_mlp puts K one-step launches between them.
static int steps_begin(invsim_handle *h, int K, const double *reward, hipStream_t s) {
    if (int rc = capture_check(h, s)) return rc;
    if (h->capturing) {
        if (h->demand_stream == INVSIM_DEMAND_PHILOX)
            return fail(h, INVSIM_EINVAL, "graph capture needs the numpy demand stream: the fast stream's launch-step "
                                          "counter is a launch parameter and would repeat on every replay");
        if (!h->t_known && h->cm.autoreset == AR_DISABLED && !h->past_ok)
            return fail(h, INVSIM_EINVAL, "graph capture of steps with autoreset DISABLED after a masked reset: "
                                          "the horizon check reads the device status word (a host synchronisation)");
        h->cap_steps += K;
    }
    if (h->t_known) {
        // DISABLED autoreset: refuse to step InvMgmt/NetInvMgmt past the horizon
        // (the reference raises IndexError, inventory_management.py:267)
        int t = h->t_cur;
        for (int k = 0; k < K; k++) {
            if (t >= h->horizon && h->cm.autoreset == AR_DISABLED && !h->past_ok)
                return fail(h, INVSIM_ERANGE, "step past the episode horizon with autoreset disabled; reset first");
            t = next_period(t, h->horizon, h->cm.autoreset, h->past_ok);
        }
    }
    // episode sink: a kernel that does not fold in-kernel leaves it to the
    // group fold of its output rows (the same arithmetic, kernels.hpp EpSink)
    if (h->cm.ep_ret && h->N && !reward)
        return fail(h, INVSIM_EINVAL, "the episode sink folds the reward outputs: pass reward / terminated / truncated");
    return INVSIM_OK;
}

static int steps_launch(invsim_handle *h, int K, const void *actions, void *obs, double *reward,
                        uint8_t *terminated, uint8_t *truncated, void *final_obs, hipStream_t s, const PolicyIO *pol) {
    const int t_u = h->t_known ? h->t_cur : -1;
    if (h->demand_stream == INVSIM_DEMAND_PHILOX) {
        int rc = ph_counter_sync(h, s);
        if (rc != INVSIM_OK) return rc;
    }
    bool sunk = false;
    hipError_t e = hipSuccess;
    switch (h->family) {
        case INVSIM_NEWSVENDOR: {
            StepIO<float, float> io{K, (const float *)actions, (float *)obs, reward, terminated, truncated, (float *)final_obs};
            e = nv_run_launch(h->nv, t_u, pol, io, h->la, s);
            break;
        }
        case INVSIM_INVMGMT: {
            StepIO<int64_t, int64_t> io{K, (const int64_t *)actions, (int64_t *)obs, reward, terminated, truncated,
                                        (int64_t *)final_obs};
            e = im_run_launch(h->im, h->im_ap.data(), h->im_m1, h->im_backlog, t_u, pol, io, h->la, sunk, s);
            break;
        }
        case INVSIM_NETINVMGMT: {
            StepIO<float, float> io{K, (const float *)actions, (float *)obs, reward, terminated, truncated, (float *)final_obs};
            e = h->net_spec ? net_spec_launch(h->net_spec, h->net, t_u, pol, io, h->la, s)
                            : net_run_launch(h->net, t_u, pol, io, s);
            break;
        }
        default: return fail(h, INVSIM_EINVAL, "bad handle family");
    }
    if (e != hipSuccess) {
        h->la.valid = false;
        return hip_fail(h, e, "step launch");
    }
    if (h->cm.ep_ret && !sunk) {
        if (!reward) return fail(h, INVSIM_EINVAL, "the episode sink needs this launch's reward outputs");
        e = episode_fold_groups_launch(reward, terminated, truncated, K, h->N, h->cm.ep_ret, h->cm.ep_part, s);
        if (e != hipSuccess) return hip_fail(h, e, "episode sink fold");
    }
    if (h->demand_stream == INVSIM_DEMAND_PHILOX) h->ph_step += (uint64_t)K;   // one counter value per launch step
    if (h->t_known)
        for (int k = 0; k < K; k++) h->t_cur = next_period(h->t_cur, h->horizon, h->cm.autoreset, h->past_ok);
    return INVSIM_OK;
}

static int steps_end(invsim_handle *h, hipStream_t s) {
    if (!h->t_known && h->cm.autoreset == AR_DISABLED && !h->past_ok) {
        // per-env periods (after a masked reset): the kernels skip an env stepped
        // past its horizon and flag it; surface that now, as the reference's
        // IndexError (inventory_management.py:267), at the cost of one sync
        uint32_t flags = 0;
        hipError_t e = hipMemcpyAsync(&flags, h->cm.status, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(h, e, "status read");
        if (flags & 1u) {
            e = hipMemsetAsync(h->cm.status, 0, sizeof(uint32_t), s);
            if (e != hipSuccess) return hip_fail(h, e, "status clear");
            return fail(h, INVSIM_ERANGE,
                        "an env was stepped past its episode horizon with autoreset disabled (that env's step was "
                        "not applied; its outputs are undefined); reset it first");
        }
    }
    return INVSIM_OK;
}

static int run_steps(invsim_handle *h, int K, const void *actions, void *obs, double *reward,
                     uint8_t *terminated, uint8_t *truncated, void *final_obs, hipStream_t s,
                     const PolicyIO *pol = nullptr) {
    if (int rc = steps_begin(h, K, reward, s)) return rc;
    if (int rc = steps_launch(h, K, actions, obs, reward, terminated, truncated, final_obs, s, pol)) return rc;
    return steps_end(h, s);
}

int invsim_step(invsim_handle *h, const void *actions, void *obs, double *reward, uint8_t *terminated,
                uint8_t *truncated, void *final_obs, void *stream) {
    TraceRange tr_("invsim_step");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (h->N && (!actions || !obs || !reward || !terminated || !truncated))
        return fail(h, INVSIM_EINVAL, "null output/input buffer");
    DeviceGuard g(h->device);
    return run_steps(h, 1, actions, obs, reward, terminated, truncated,
                     h->cm.autoreset == AR_SAME_STEP ? final_obs : nullptr, (hipStream_t)stream);
}

int invsim_rollout(invsim_handle *h, int32_t K, const void *actions, void *obs, double *reward,
                   uint8_t *terminated, uint8_t *truncated, void *stream) {
    TraceRange tr_("invsim_rollout");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (K < 0) return fail(h, INVSIM_EINVAL, "K must be >= 0");
    if (K == 0) return INVSIM_OK;
    if (h->N && (!actions || !obs || !reward || !terminated || !truncated))
        return fail(h, INVSIM_EINVAL, "null output/input buffer");
    if (h->cm.autoreset == AR_SAME_STEP)
        return fail(h, INVSIM_EINVAL, "rollout does not return final_obs: use NEXT_STEP or DISABLED autoreset");
    DeviceGuard g(h->device);
    return run_steps(h, K, actions, obs, reward, terminated, truncated, nullptr, (hipStream_t)stream);
}

static int metrics_dim(const invsim_handle *h) {
    switch (h->family) {
        case INVSIM_NEWSVENDOR: return 2;
        case INVSIM_INVMGMT: return 6;
        case INVSIM_NETINVMGMT: return 5 + h->net.J;
        default: return 0;
    }
}

int invsim_metrics_dim(const invsim_handle *h, int32_t *dim) {
    if (!h || !dim) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *dim = metrics_dim(h);
    return INVSIM_OK;
}

// what invsim_rollout_metrics and invsim_rollout_mlp refuse alike
static int metric_rollout_checks(invsim_handle *h, const double *reward, const uint8_t *terminated,
                                 const uint8_t *truncated) {
    if (h->cm.autoreset == AR_SAME_STEP)
        return fail(h, INVSIM_EINVAL, "metric rollouts do not return final_obs: use NEXT_STEP or DISABLED autoreset");
    if ((reward == nullptr) != (terminated == nullptr) || (reward == nullptr) != (truncated == nullptr))
        return fail(h, INVSIM_EINVAL, "reward, terminated and truncated are given together or not at all");
    return INVSIM_OK;
}

// the EXT run kernels: the policy bookkeeping, the actions of StepIO::act
static PolicyIO external_policy(const invsim_handle *h, double *metrics) {
    PolicyIO p{};
    p.kind = POL_EXTERNAL;
    p.metrics = metrics;
    p.mdim = metrics_dim(h);
    return p;
}

// the RANDOM kind's PolicyIO fields: the upper bounds `high` (host, [action_dim]
// in the action dtype) and the attached action generators
static int random_policy(invsim_handle *h, const void *high, PolicyIO &p, bool rollout) {
    if (!high) return fail(h, INVSIM_EINVAL, "RANDOM policy needs the action space's upper bounds");
    if (h->act_dim > POL_MAX_A) return fail(h, INVSIM_ERANGE, "action_dim too large for a RANDOM policy");
    if (rollout && h->family == INVSIM_NETINVMGMT && !h->net_spec && net_random_lds_bytes(h->net) > LDS_LIMIT_BYTES)
        return fail(h, INVSIM_ERANGE, "topology too large for the LDS scratch of a RANDOM policy rollout "
                                      "(the generic kernel keeps the drawn actions of 64 envs in LDS)");
    if (!h->arng)
        return fail(h, INVSIM_EINVAL, "no action generators attached: seed a buffer with invsim_seed_action_rng and "
                                      "attach it with invsim_set_action_rng");
    p.kind = POL_RANDOM;
    p.arng = h->arng;
    for (int a = 0; a < h->act_dim; a++) {
        if (h->family == INVSIM_INVMGMT) p.ci[a] = ((const int64_t *)high)[a];
        else p.cf[a] = ((const float *)high)[a];
    }
    return INVSIM_OK;
}

int invsim_rollout_policy(invsim_handle *h, int32_t K, const invsim_policy *policy, void *obs, double *reward,
                          uint8_t *terminated, uint8_t *truncated, void *actions, double *metrics, void *stream) {
    TraceRange tr_("invsim_rollout_policy");
    if (!h || !policy) return fail(h, INVSIM_EINVAL, "null argument");
    if (K < 0) return fail(h, INVSIM_EINVAL, "K must be >= 0");
    if (K == 0) return INVSIM_OK;
    if (h->cm.autoreset == AR_SAME_STEP)
        return fail(h, INVSIM_EINVAL, "policy rollouts do not return final_obs: use NEXT_STEP or DISABLED autoreset");
    if ((reward == nullptr) != (terminated == nullptr) || (reward == nullptr) != (truncated == nullptr))
        return fail(h, INVSIM_EINVAL, "reward, terminated and truncated are given together or not at all");
    PolicyIO p{};
    p.kind = policy->kind;
    p.variant = policy->variant;
    p.sf = policy->safety_factor;
    p.mu = policy->mu;
    p.act_out = actions;
    p.metrics = metrics;
    p.mdim = metrics_dim(h);
    switch (policy->kind) {
        case INVSIM_POLICY_CONSTANT:
            if (!policy->constant) return fail(h, INVSIM_EINVAL, "CONSTANT policy needs its action vector");
            if (h->act_dim > POL_MAX_A) return fail(h, INVSIM_ERANGE, "action_dim too large for a CONSTANT policy");
            for (int a = 0; a < h->act_dim; a++) {
                if (h->family == INVSIM_INVMGMT) p.ci[a] = ((const int64_t *)policy->constant)[a];
                else p.cf[a] = ((const float *)policy->constant)[a];
            }
            break;
        case INVSIM_POLICY_BASE_STOCK:
            if (h->family != INVSIM_INVMGMT) return fail(h, INVSIM_EINVAL, "BASE_STOCK is an InvMgmt policy");
            break;
        case INVSIM_POLICY_ORDER_UP_TO:
            if (h->family != INVSIM_NEWSVENDOR) return fail(h, INVSIM_EINVAL, "ORDER_UP_TO is a Newsvendor policy");
            break;
        case INVSIM_POLICY_CLASSIC_NV:
        case INVSIM_POLICY_SS: {
            if (h->family != INVSIM_NEWSVENDOR)
                return fail(h, INVSIM_EINVAL, "CLASSIC_NV / SS are Newsvendor policies");
            if (policy->kind == INVSIM_POLICY_CLASSIC_NV && (policy->variant < 0 || policy->variant > 1))
                return fail(h, INVSIM_EINVAL, "CLASSIC_NV variant: 0 'k_vs_h' or 1 'profit_margin'");
            // the device ppf walks the Poisson CDF: bounded work per env
            const double sf = policy->kind == INVSIM_POLICY_CLASSIC_NV ? policy->safety_factor : 1.0;
            const double lam = (double)(float)h->nv.mu_max * (h->nv.L + 1) * (sf > 1 ? sf : 1.0);
            if (!(lam <= 1e6))
                return fail(h, INVSIM_ERANGE, "critical-ratio policies need mu_max * (lead_time + 1) * safety_factor <= 1e6");
            break;
        }
        case INVSIM_POLICY_RANDOM:
            if (int rc = random_policy(h, policy->constant, p, true)) return rc;
            break;
        case INVSIM_POLICY_LEVELS:
            if (h->family != INVSIM_INVMGMT) return fail(h, INVSIM_EINVAL, "LEVELS is an InvMgmt policy");
            if (!h->levels)
                return fail(h, INVSIM_EINVAL, "no levels attached: attach a device f64 [N][action_dim] array with "
                                              "invsim_set_policy_levels");
            p.kind = POL_LEVELS;        // (the public 7 is POL_EXTERNAL inside)
            p.levels = h->levels;       // safety_factor / mu are ignored: their slots hold the two pointers
            p.reorder = h->reorder;
            break;
        case INVSIM_POLICY_NET_LEVELS:
            if (h->family != INVSIM_NETINVMGMT) return fail(h, INVSIM_EINVAL, "NET_LEVELS is a NetInvMgmt policy");
            if (!policy->constant) return fail(h, INVSIM_EINVAL, "NET_LEVELS policy needs the action space's upper bounds");
            if (h->act_dim > POL_MAX_A) return fail(h, INVSIM_ERANGE, "action_dim too large for a NET_LEVELS policy");
            if (!h->net_spec && net_random_lds_bytes(h->net) > LDS_LIMIT_BYTES)
                return fail(h, INVSIM_ERANGE, "topology too large for the LDS scratch of a NET_LEVELS policy rollout "
                                              "(the generic kernel keeps the orders of 64 envs in LDS)");
            if (!h->levels)
                return fail(h, INVSIM_EINVAL, "no levels attached: attach a device f64 [N][action_dim] array with "
                                              "invsim_set_policy_net_levels");
            p.kind = POL_NET_LEVELS;
            p.levels = h->levels;       // safety_factor / mu are ignored: their slots hold the two pointers
            p.reorder = h->reorder;
            for (int a = 0; a < h->act_dim; a++) p.cf[a] = ((const float *)policy->constant)[a];
            break;
        default: return fail(h, INVSIM_EINVAL, "unknown policy kind");
    }
    DeviceGuard g(h->device);
    return run_steps(h, K, nullptr, obs, reward, terminated, truncated, nullptr, (hipStream_t)stream, &p);
}

int invsim_rollout_metrics(invsim_handle *h, int32_t K, const void *actions, void *obs, double *reward,
                           uint8_t *terminated, uint8_t *truncated, double *metrics, void *stream) {
    TraceRange tr_("invsim_rollout_metrics");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (K < 0) return fail(h, INVSIM_EINVAL, "K must be >= 0");
    if (K == 0) return INVSIM_OK;
    if (h->N && !actions) return fail(h, INVSIM_EINVAL, "null actions");
    if (int rc = metric_rollout_checks(h, reward, terminated, truncated)) return rc;
    const PolicyIO p = external_policy(h, metrics);
    DeviceGuard g(h->device);
    return run_steps(h, K, actions, obs, reward, terminated, truncated, nullptr, (hipStream_t)stream, &p);
}

// ------------------------------------------------------------------ MLP actor
// invsim_mlp_create, and with `value` invsim_mlp_create_value: the same blob
// with one output unit in place of the handle's action_dim
static int mlp_create(invsim_handle *h, const invsim_mlp_spec *sp, invsim_mlp **out, bool value) {
    if (!h || !sp || !out) return fail(h, INVSIM_EINVAL, "null argument");
    *out = nullptr;
    if (int rc = refuse_in_capture(h, "mlp_create")) return rc;
    const int out_dim = value ? 1 : h->act_dim;
    const int n = sp->n_layers;
    if (n < 1 || n > INVSIM_MLP_MAX_LAYERS)
        return fail(h, INVSIM_ERANGE, "n_layers must be 1.." + std::to_string(INVSIM_MLP_MAX_LAYERS));
    if (!sp->dims || !sp->weight) return fail(h, INVSIM_EINVAL, "null dims / weight");
    if (sp->dims[0] != h->obs_dim || sp->dims[n] != out_dim)
        return fail(h, INVSIM_ERANGE, "dims[0] / dims[n_layers] must be the handle's obs_dim " + std::to_string(h->obs_dim) +
                                          (value ? " / 1 (a value network)" : " / action_dim " + std::to_string(out_dim)));
    if (h->obs_dim > INVSIM_MLP_MAX_WIDTH) return fail(h, INVSIM_ERANGE, "obs_dim too large for an MLP actor");
    if (out_dim > INVSIM_POLICY_MAX_ACTION) return fail(h, INVSIM_ERANGE, "action_dim too large for an MLP actor");
    for (int l = 1; l < n; l++)
        if (sp->dims[l] < 1 || sp->dims[l] > INVSIM_MLP_MAX_WIDTH)
            return fail(h, INVSIM_ERANGE, "hidden widths must be 1.." + std::to_string(INVSIM_MLP_MAX_WIDTH));
    if (n > 1 && sp->activation != INVSIM_MLP_RELU && sp->activation != INVSIM_MLP_TANH)
        return fail(h, INVSIM_EINVAL, "hidden activation must be INVSIM_MLP_RELU or INVSIM_MLP_TANH");
    if (sp->out_activation != INVSIM_MLP_NONE && sp->out_activation != INVSIM_MLP_TANH)
        return fail(h, INVSIM_EINVAL, "out_activation must be INVSIM_MLP_NONE or INVSIM_MLP_TANH");
    if ((sp->in_scale == nullptr) != (sp->in_shift == nullptr) || (sp->out_scale == nullptr) != (sp->out_shift == nullptr))
        return fail(h, INVSIM_EINVAL, "scale and shift are given in pairs");
    if (value && sp->clip) return fail(h, INVSIM_EINVAL, "a value network has no action bounds: clip must be 0");
    if (sp->clip && (!sp->low || !sp->high)) return fail(h, INVSIM_EINVAL, "clip needs the action bounds low / high");
    for (int l = 0; l < n; l++)
        if (!sp->weight[l]) return fail(h, INVSIM_EINVAL, "null weight matrix");

    // one blob of 8-byte slots: per layer the transposed weights [in][opad] and the
    // bias [opad], then the scales and the bounds
    const bool i64 = h->family == INVSIM_INVMGMT;
    const int O = h->obs_dim, A = out_dim;
    auto m = new invsim_mlp();
    m->owner = h;
    m->value = value;
    MlpDev &d = m->dev;
    d.n_layers = n;
    d.act = n > 1 ? sp->activation : INVSIM_MLP_NONE;
    d.out_act = sp->out_activation;
    d.clip = sp->clip ? 1 : 0;
    std::vector<float> blob;
    auto reserve = [&blob](size_t floats) {          // returns the offset; keeps 8-byte alignment
        const size_t off = blob.size();
        blob.resize(off + (floats + 1) / 2 * 2, 0.0f);
        return off;
    };
    size_t o_wt[MLP_LAYERS], o_b[MLP_LAYERS], o_is = 0, o_ih = 0, o_os = 0, o_oh = 0, o_lo = 0, o_hi = 0;
    d.rows = 0;
    for (int l = 0; l <= n; l++) {
        d.dims[l] = sp->dims[l];
        d.rows = std::max(d.rows, sp->dims[l]);
    }
    for (int l = 0; l < n; l++) {
        const int in = d.dims[l], outn = d.dims[l + 1], opad = (outn + 3) / 4 * 4;
        d.opad[l] = opad;
        o_wt[l] = reserve((size_t)in * opad);
        for (int j = 0; j < outn; j++)
            for (int i = 0; i < in; i++) blob[o_wt[l] + (size_t)i * opad + j] = sp->weight[l][(size_t)j * in + i];
        o_b[l] = reserve(opad);
        if (sp->bias && sp->bias[l]) std::copy(sp->bias[l], sp->bias[l] + outn, blob.begin() + o_b[l]);
    }
    const int apad = d.opad[n - 1];
    if (sp->in_scale) {
        o_is = reserve(O), o_ih = reserve(O);
        std::copy(sp->in_scale, sp->in_scale + O, blob.begin() + o_is);
        std::copy(sp->in_shift, sp->in_shift + O, blob.begin() + o_ih);
    }
    if (sp->out_scale) {
        o_os = reserve(apad), o_oh = reserve(apad);
        std::copy(sp->out_scale, sp->out_scale + A, blob.begin() + o_os);
        std::copy(sp->out_shift, sp->out_shift + A, blob.begin() + o_oh);
    }
    if (sp->clip) {      // f32 spaces: the bounds; int64 spaces: the bounds as f64 (the clamp runs in f64)
        o_lo = reserve(2 * (size_t)A), o_hi = reserve(2 * (size_t)A);
        for (int a = 0; a < A; a++) {
            if (i64) {
                const double lo = (double)((const int64_t *)sp->low)[a], hi = (double)((const int64_t *)sp->high)[a];
                std::memcpy(&blob[o_lo + 2 * a], &lo, 8);
                std::memcpy(&blob[o_hi + 2 * a], &hi, 8);
            } else {
                blob[o_lo + a] = ((const float *)sp->low)[a];
                blob[o_hi + a] = ((const float *)sp->high)[a];
            }
        }
    }
    const size_t o_dev = reserve((sizeof(MlpDev) + 3) / 4);
    const size_t o_gs = reserve(A), o_gl = reserve(A);     // invsim_mlp_set_gaussian's std and log_std
    m->logp0 = (float)(-0.91893853320467274178 * (double)A);
    DeviceGuard g(h->device);
    const size_t esz = i64 ? 8 : 4;
    const size_t n_el = (size_t)std::max<int64_t>(h->N, 1);
    hipError_t e = mlp_prepare();
    if (e == hipSuccess) e = ppo_prepare();
    if (e == hipSuccess) e = hipMalloc(&m->blob, blob.size() * sizeof(float));
    if (!value) {        // the closed loop's scratch rows: a value network is never in that loop
        if (e == hipSuccess) e = hipMalloc(&m->obs_row, n_el * O * esz);
        if (e == hipSuccess) e = hipMalloc(&m->act_row, n_el * A * esz);
    }
    if (e == hipSuccess) {
        const float *base = m->blob;
        for (int l = 0; l < n; l++) {
            d.wt[l] = base + o_wt[l];
            d.bias[l] = base + o_b[l];
        }
        if (sp->in_scale) d.in_scale = base + o_is, d.in_shift = base + o_ih;
        if (sp->out_scale) d.out_scale = base + o_os, d.out_shift = base + o_oh;
        if (sp->clip) {
            d.lo_f = base + o_lo, d.hi_f = base + o_hi;
            d.lo_d = (const double *)(base + o_lo), d.hi_d = (const double *)(base + o_hi);
        }
        std::memcpy(&blob[o_dev], &d, sizeof(MlpDev));
        m->dev_copy = (const MlpDev *)(base + o_dev);
        m->g_std = m->blob + o_gs, m->g_log_std = m->blob + o_gl;
        e = hipMemcpy(m->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        mlp_free(m);
        return fail(h, e == hipErrorOutOfMemory ? INVSIM_ENOMEM : INVSIM_EDEVICE,
                    std::string("mlp_create: ") + hipGetErrorString(e));
    }
    *out = m;
    return INVSIM_OK;
}

int invsim_mlp_create(invsim_handle *h, const invsim_mlp_spec *sp, invsim_mlp **out) {
    return mlp_create(h, sp, out, false);
}

int invsim_mlp_create_value(invsim_handle *h, const invsim_mlp_spec *sp, invsim_mlp **out) {
    return mlp_create(h, sp, out, true);
}

// what every call that takes an actor checks of its object
static int mlp_actor_check(invsim_handle *h, const invsim_mlp *m) {
    if (m->owner != h) return fail(h, INVSIM_EINVAL, "this invsim_mlp was created for another handle");
    if (m->value)
        return fail(h, INVSIM_EINVAL, "this invsim_mlp is a value network (invsim_mlp_create_value): it produces no "
                                      "actions; evaluate it with invsim_mlp_values");
    return INVSIM_OK;
}

void invsim_mlp_destroy(invsim_mlp *m) {
    if (!m) return;
    if (m->owner->capturing) {     // hipFree synchronises: the object stays valid
        (void)refuse_in_capture(m->owner, "mlp_destroy");
        return;
    }
    DeviceGuard g(m->owner->device);
    mlp_free(m);
}

int invsim_mlp_actions(invsim_handle *h, const invsim_mlp *m, const void *obs, void *actions, float *raw,
                       void *stream) {
    TraceRange tr_("invsim_mlp_actions");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = mlp_actor_check(h, m)) return rc;
    if (h->N && !obs) return fail(h, INVSIM_EINVAL, "null obs");
    DeviceGuard g(h->device);
    hipError_t e = mlp_launch(m->dev, m->dev_copy, h->family == INVSIM_INVMGMT, obs, actions, raw, h->N, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "mlp launch");
}

int invsim_mlp_values(invsim_handle *h, const invsim_mlp *m, const void *obs, int64_t rows, float *values,
                      void *stream) {
    TraceRange tr_("invsim_mlp_values");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (m->owner != h) return fail(h, INVSIM_EINVAL, "this invsim_mlp was created for another handle");
    if (!m->value)
        return fail(h, INVSIM_EINVAL, "this invsim_mlp is an actor: a value network comes from invsim_mlp_create_value");
    if (rows < 0) return fail(h, INVSIM_EINVAL, "rows must be >= 0");
    if (rows == 0) return INVSIM_OK;
    // the launch's grid is rows / 64 workgroups in one dimension; every index in the kernel is 64-bit
    if (rows > (int64_t)INT32_MAX * MLP_ENVS) return fail(h, INVSIM_ERANGE, "too many rows for one launch");
    if (!obs || !values) return fail(h, INVSIM_EINVAL, "null obs / values");
    DeviceGuard g(h->device);
    // the network kernel through its raw output: one unit per row, no conversion
    hipError_t e = mlp_launch(m->dev, m->dev_copy, h->family == INVSIM_INVMGMT, obs, nullptr, values, rows, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "mlp values launch");
}

int invsim_mlp_update(invsim_handle *h, invsim_mlp *m, const float *const *weight, const float *const *bias,
                      const float *std, const float *log_std, void *stream) {
    TraceRange tr_("invsim_mlp_update");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (m->owner != h) return fail(h, INVSIM_EINVAL, "this invsim_mlp was created for another handle");
    if ((std == nullptr) != (log_std == nullptr)) return fail(h, INVSIM_EINVAL, "std and log_std are given together");
    if (std && m->value) return fail(h, INVSIM_EINVAL, "a value network has no Gaussian: std must be NULL");
    const MlpDev &d = m->dev;
    MlpUpdate u{};
    u.n_layers = d.n_layers;
    u.A = d.dims[d.n_layers];
    for (int l = 0; l < d.n_layers; l++) {
        u.in[l] = d.dims[l], u.out[l] = d.dims[l + 1], u.opad[l] = d.opad[l];
        u.w_src[l] = weight ? weight[l] : nullptr;
        u.b_src[l] = bias ? bias[l] : nullptr;
        u.wt[l] = const_cast<float *>(d.wt[l]);         // into m->blob, which is ours to write
        u.bias[l] = const_cast<float *>(d.bias[l]);
    }
    u.std_src = std, u.log_std_src = log_std;
    u.std = m->g_std, u.log_std = m->g_log_std;
    DeviceGuard g(h->device);
    hipError_t e = mlp_update_launch(u, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, "mlp update launch");
    if (std) m->gauss = true;
    return INVSIM_OK;
}

// what the sampling launch needs beyond the network: a Gaussian on m and the
// action generators on h; fills the launch's arguments but mean and logp
static int mlp_sample_args(invsim_handle *h, const invsim_mlp *m, MlpSample &sm) {
    if (!m->gauss)
        return fail(h, INVSIM_EINVAL, "no Gaussian set on this invsim_mlp: give std and log_std with "
                                      "invsim_mlp_set_gaussian");
    if (!h->arng)
        return fail(h, INVSIM_EINVAL, "no action generators attached: seed a buffer with invsim_seed_action_rng and "
                                      "attach it with invsim_set_action_rng");
    sm = MlpSample{nullptr, nullptr, h->arng, h->Npad, m->g_std, m->g_log_std, m->logp0};
    return INVSIM_OK;
}

int invsim_mlp_set_gaussian(invsim_handle *h, invsim_mlp *m, const float *std, const float *log_std) {
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = mlp_actor_check(h, m)) return rc;
    if (int rc = refuse_in_capture(h, "mlp_set_gaussian")) return rc;
    if (!std) {
        m->gauss = false;
        return INVSIM_OK;
    }
    if (!log_std) return fail(h, INVSIM_EINVAL, "std without log_std");
    const int A = h->act_dim;
    for (int a = 0; a < A; a++) {
        if (!std::isfinite(std[a]) || !(std[a] >= 0.0f)) return fail(h, INVSIM_EINVAL, "std must be finite and >= 0");
        if (!std::isfinite(log_std[a])) return fail(h, INVSIM_EINVAL, "log_std must be finite");
    }
    // the blob's rows are overwritten: wait for every launch that may still read them
    DeviceGuard g(h->device);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(m->g_std, std, A * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->g_log_std, log_std, A * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        m->gauss = false;
        return hip_fail(h, e, "mlp_set_gaussian");
    }
    m->gauss = true;
    return INVSIM_OK;
}

int invsim_mlp_sample(invsim_handle *h, const invsim_mlp *m, const void *obs, void *actions, float *raw, float *mean,
                      float *logp, void *stream) {
    TraceRange tr_("invsim_mlp_sample");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = mlp_actor_check(h, m)) return rc;
    if (h->N && !obs) return fail(h, INVSIM_EINVAL, "null obs");
    if (!actions && !raw && !mean && !logp) return fail(h, INVSIM_EINVAL, "no output: every output pointer is null");
    MlpSample sm{};
    if (int rc = mlp_sample_args(h, m, sm)) return rc;
    sm.mean = mean, sm.logp = logp;
    DeviceGuard g(h->device);
    hipError_t e = mlp_sample_launch(m->dev, m->dev_copy, h->family == INVSIM_INVMGMT, obs, actions, raw, sm, h->N,
                                     (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "mlp sample launch");
}

// invsim_rollout_mlp, and with `sample` invsim_rollout_mlp_sample: the same loop
// with the sampling launch (raw [K][N][A], logp [K][N], either may be null)
static int rollout_mlp(invsim_handle *h, int32_t K, const invsim_mlp *m, const void *obs0, void *obs, double *reward,
                       uint8_t *terminated, uint8_t *truncated, void *actions, float *raw, float *logp, double *metrics,
                       void *stream, bool sample) {
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (K < 0) return fail(h, INVSIM_EINVAL, "K must be >= 0");
    if (K == 0) return INVSIM_OK;
    if (int rc = mlp_actor_check(h, m)) return rc;
    if (h->N && !obs0) return fail(h, INVSIM_EINVAL, "null obs0: the network's first input is the observation the env "
                                                     "last returned");
    if (int rc = metric_rollout_checks(h, reward, terminated, truncated)) return rc;
    MlpSample sm{};
    if (sample)
        if (int rc = mlp_sample_args(h, m, sm)) return rc;
    const PolicyIO p = external_policy(h, metrics);
    const bool i64 = h->family == INVSIM_INVMGMT;
    const size_t o_row = (size_t)h->N * h->obs_dim * (i64 ? 8 : 4), a_row = (size_t)h->N * h->act_dim * (i64 ? 8 : 4);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g(h->device);
    if (int rc = steps_begin(h, K, reward, s)) return rc;
    // episode sink: the call's K output rows are folded once, after the loop, as
    // one invsim_rollout_metrics launch of K steps folds them (K folds of one row
    // each add to part in another order); the one-step launches run without it
    struct SinkOff {
        invsim_handle *h;
        double *ret, *part;
        explicit SinkOff(invsim_handle *h_) : h(h_), ret(h_->cm.ep_ret), part(h_->cm.ep_part) { set(nullptr, nullptr); }
        ~SinkOff() { set(ret, part); }
        void set(double *r, double *p) {
            if (!ret) return;
            h->cm.ep_ret = r, h->cm.ep_part = p;
            sync_common(h);
        }
    } sink(h);
    const void *in = obs0;
    for (int k = 0; k < K; k++) {
        void *a_k = actions ? (char *)actions + k * a_row : m->act_row;
        void *o_k = obs ? (char *)obs + k * o_row : m->obs_row;   // in == o_k then: read before it is overwritten (stream order)
        const size_t r = (size_t)k * h->N;
        hipError_t e;
        if (sample) {
            sm.logp = logp ? logp + r : nullptr;
            e = mlp_sample_launch(m->dev, m->dev_copy, i64, in, a_k, raw ? raw + r * h->act_dim : nullptr, sm, h->N, s);
        } else {
            e = mlp_launch(m->dev, m->dev_copy, i64, in, a_k, nullptr, h->N, s);
        }
        if (e != hipSuccess) return hip_fail(h, e, "mlp launch");
        if (int rc = steps_launch(h, 1, a_k, o_k, reward ? reward + r : nullptr, terminated ? terminated + r : nullptr,
                                  truncated ? truncated + r : nullptr, nullptr, s, &p))
            return rc;
        in = o_k;
    }
    if (sink.ret && h->N) {      // (steps_begin made sure of the reward triple)
        hipError_t e = episode_fold_groups_launch(reward, terminated, truncated, K, h->N, sink.ret, sink.part, s);
        if (e != hipSuccess) return hip_fail(h, e, "episode sink fold");
    }
    return steps_end(h, s);
}

int invsim_rollout_mlp(invsim_handle *h, int32_t K, const invsim_mlp *m, const void *obs0, void *obs, double *reward,
                       uint8_t *terminated, uint8_t *truncated, void *actions, double *metrics, void *stream) {
    TraceRange tr_("invsim_rollout_mlp");
    return rollout_mlp(h, K, m, obs0, obs, reward, terminated, truncated, actions, nullptr, nullptr, metrics, stream, false);
}

int invsim_rollout_mlp_sample(invsim_handle *h, int32_t K, const invsim_mlp *m, const void *obs0, void *obs,
                              double *reward, uint8_t *terminated, uint8_t *truncated, void *actions, float *raw,
                              float *logp, double *metrics, void *stream) {
    TraceRange tr_("invsim_rollout_mlp_sample");
    return rollout_mlp(h, K, m, obs0, obs, reward, terminated, truncated, actions, raw, logp, metrics, stream, true);
}

int invsim_action_rng_bytes(const invsim_handle *h, int64_t *bytes) {
    if (!h || !bytes) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *bytes = 4 * h->Npad * (int64_t)sizeof(uint64_t);
    return INVSIM_OK;
}

int invsim_seed_action_rng(invsim_handle *h, uint64_t *arng, uint64_t base_lo, uint64_t base_hi, int64_t first,
                           void *stream) {
    TraceRange tr_("invsim_seed_action_rng");
    if (!h || !arng) return fail(h, INVSIM_EINVAL, "null argument");
    if (first < 0) return fail(h, INVSIM_EINVAL, "first_index must be >= 0");
    if (int rc = capture_check(h, (hipStream_t)stream)) return rc;
    DeviceGuard g(h->device);
    // seed_range_kernel over the caller's rows: the demand generators, their
    // lookahead cache and the fast stream's counter are not touched
    Common c = h->cm;
    c.rng = act_rng_rows(arng, h->Npad);
    c.u32buf = nullptr;
    hipError_t e = seed_range_launch(c, base_lo, base_hi, first, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "seed_action_rng launch");
}

int invsim_set_action_rng(invsim_handle *h, uint64_t *arng) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_action_rng")) return rc;
    h->arng = arng;
    return INVSIM_OK;
}

int invsim_set_policy_levels(invsim_handle *h, const double *levels, const double *reorder) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_policy_levels")) return rc;
    if (h->family != INVSIM_INVMGMT) return fail(h, INVSIM_EINVAL, "LEVELS is an InvMgmt policy");
    h->levels = levels;
    h->reorder = levels ? reorder : nullptr;
    return INVSIM_OK;
}

int invsim_set_policy_net_levels(invsim_handle *h, const double *levels, const double *reorder) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_policy_net_levels")) return rc;
    if (h->family != INVSIM_NETINVMGMT) return fail(h, INVSIM_EINVAL, "NET_LEVELS is a NetInvMgmt policy");
    h->levels = levels;
    h->reorder = levels ? reorder : nullptr;
    return INVSIM_OK;
}

int invsim_sample_actions(invsim_handle *h, int32_t K, const void *high, void *actions, void *stream) {
    TraceRange tr_("invsim_sample_actions");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (K < 0) return fail(h, INVSIM_EINVAL, "K must be >= 0");
    if (K == 0) return INVSIM_OK;
    if (h->N && !actions) return fail(h, INVSIM_EINVAL, "null output/input buffer");
    PolicyIO p{};
    if (int rc = random_policy(h, high, p, false)) return rc;   // (no LDS check: sample_actions_kernel uses none)
    if (int rc = capture_check(h, (hipStream_t)stream)) return rc;
    p.act_out = actions;
    DeviceGuard g(h->device);
    hipError_t e = sample_actions_launch(p, h->family == INVSIM_INVMGMT, K, h->N, h->Npad, h->act_dim, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "sample_actions launch");
}

int invsim_episode_fold(const double *reward, const uint8_t *terminated, const uint8_t *truncated, int32_t K,
                        int64_t n_envs, double *ret, double *acc, void *stream) {
    TraceRange tr_("invsim_episode_fold");
    if (!reward || !ret || !acc || K < 0 || n_envs < 0)
        return fail(nullptr, INVSIM_EINVAL, "episode_fold: null buffer or negative size");
    hipError_t e = episode_fold_launch(reward, terminated, truncated, K, n_envs, ret, acc, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "episode_fold launch");
}

int invsim_episode_fold_groups(const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                               int32_t K, int64_t n_envs, double *ret, double *part, void *stream) {
    TraceRange tr_("invsim_episode_fold_groups");
    if ((!reward && K > 0 && n_envs > 0) || !ret || !part || K < 0 || n_envs < 0)
        return fail(nullptr, INVSIM_EINVAL, "episode_fold_groups: null buffer or negative size");
    hipError_t e = episode_fold_groups_launch(reward, terminated, truncated, K, n_envs, ret, part, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "episode_fold_groups launch");
}

int invsim_gae(const double *reward, const uint8_t *terminated, const uint8_t *truncated, const uint8_t *done0,
               const float *value0, const float *values, int32_t K, int64_t n_envs, double gamma, double lambda,
               float *advantages, float *returns, uint8_t *valid, void *stream) {
    TraceRange tr_("invsim_gae");
    if (K < 0 || n_envs < 0) return fail(nullptr, INVSIM_EINVAL, "gae: negative size");
    if (K == 0 || n_envs == 0) return INVSIM_OK;
    if (!reward || !value0 || !values || !advantages || !returns)
        return fail(nullptr, INVSIM_EINVAL, "gae: null reward / value0 / values / advantages / returns");
    hipError_t e = gae_launch(reward, terminated, truncated, done0, value0, values, K, n_envs, gamma, lambda, advantages,
                              returns, valid, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "gae launch");
}

// ------------------------------------------------------------------ running normalisation
static int moments_shape_check(int64_t rows, int32_t cols) {
    if (rows < 0 || cols < 1) return fail(nullptr, INVSIM_EINVAL, "moments: rows must be >= 0 and cols >= 1");
    if (cols > 1024) return fail(nullptr, INVSIM_ERANGE, "moments: at most 1024 columns");
    return INVSIM_OK;
}

int invsim_moments_scratch_bytes(int64_t rows, int32_t cols, int64_t *bytes) {
    if (!bytes) return fail(nullptr, INVSIM_EINVAL, "null argument");
    if (int rc = moments_shape_check(rows, cols)) return rc;
    *bytes = moments_scratch_bytes(rows, cols);
    return INVSIM_OK;
}

int invsim_moments(const void *x, int32_t dtype, int64_t rows, int32_t cols, const uint8_t *mask, double *stats,
                   void *scratch, int64_t scratch_bytes, void *stream) {
    TraceRange tr_("invsim_moments");
    if (int rc = moments_shape_check(rows, cols)) return rc;
    if (dtype != INVSIM_DTYPE_I64 && dtype != INVSIM_DTYPE_F32 && dtype != INVSIM_DTYPE_F64)
        return fail(nullptr, INVSIM_EINVAL, "moments: dtype must be INVSIM_DTYPE_I64, _F32 or _F64");
    if (rows == 0) return INVSIM_OK;
    if (!x || !stats || !scratch) return fail(nullptr, INVSIM_EINVAL, "moments: null x / stats / scratch");
    if (scratch_bytes < moments_scratch_bytes(rows, cols))
        return fail(nullptr, INVSIM_ERANGE, "moments: scratch is smaller than invsim_moments_scratch_bytes");
    hipError_t e = moments_launch(x, dtype, rows, cols, mask, stats, static_cast<double *>(scratch), (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "moments launch");
}

int invsim_discounted_returns(const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                              const uint8_t *done0, int32_t K, int64_t n_envs, double gamma, double *ret, double *out,
                              uint8_t *valid, void *stream) {
    TraceRange tr_("invsim_discounted_returns");
    if (K < 0 || n_envs < 0) return fail(nullptr, INVSIM_EINVAL, "discounted_returns: negative size");
    if (K == 0 || n_envs == 0) return INVSIM_OK;
    if (!reward || !ret || !out) return fail(nullptr, INVSIM_EINVAL, "discounted_returns: null reward / ret / out");
    hipError_t e = discounted_returns_launch(reward, terminated, truncated, done0, K, n_envs, gamma, ret, out, valid,
                                             (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "discounted_returns launch");
}

int invsim_normalize_rewards(const double *reward, int64_t count, const double *stats, double epsilon, double clip,
                             double *out, void *stream) {
    TraceRange tr_("invsim_normalize_rewards");
    if (!(clip > 0.0)) return fail(nullptr, INVSIM_EINVAL, "normalize_rewards: clip must be > 0");
    if (count < 0) return fail(nullptr, INVSIM_EINVAL, "normalize_rewards: negative count");
    if (count == 0) return INVSIM_OK;
    if (!reward || !stats || !out) return fail(nullptr, INVSIM_EINVAL, "normalize_rewards: null reward / stats / out");
    hipError_t e = normalize_rewards_launch(reward, count, stats, epsilon, clip, out, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "normalize_rewards launch");
}

int invsim_norm_params(const double *stats, int32_t cols, double epsilon, float *scale, float *shift, void *stream) {
    TraceRange tr_("invsim_norm_params");
    if (cols < 1) return fail(nullptr, INVSIM_EINVAL, "norm_params: cols must be >= 1");
    if (cols > 1024) return fail(nullptr, INVSIM_ERANGE, "norm_params: at most 1024 columns");
    if (!stats || !scale) return fail(nullptr, INVSIM_EINVAL, "norm_params: null stats / scale");
    hipError_t e = norm_params_launch(stats, cols, epsilon, scale, shift, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(nullptr, e, "norm_params launch");
}

int invsim_mlp_set_input_norm(invsim_handle *h, invsim_mlp *m, const float *scale, const float *shift, void *stream) {
    TraceRange tr_("invsim_mlp_set_input_norm");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (m->owner != h) return fail(h, INVSIM_EINVAL, "this invsim_mlp was created for another handle");
    if (!m->dev.in_scale)
        return fail(h, INVSIM_EINVAL, "this invsim_mlp was created without in_scale / in_shift: it has no input rows to write");
    if (!scale || !shift) return fail(h, INVSIM_EINVAL, "null scale / shift");
    DeviceGuard g(h->device);
    // into m->blob, which is ours to write
    hipError_t e = mlp_set_rows_launch(const_cast<float *>(m->dev.in_scale), const_cast<float *>(m->dev.in_shift), scale,
                                       shift, m->dev.dims[0], (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "mlp set_input_norm launch");
}

// ------------------------------------------------------------------ PPO gradients
static int ppo_dims_check(invsim_handle *h, const int32_t *dims, int32_t n_layers) {
    if (!dims || n_layers < 1 || n_layers > INVSIM_MLP_MAX_LAYERS)
        return fail(h, INVSIM_EINVAL, "ppo: dims must hold n_layers + 1 widths, n_layers in 1.." + std::to_string(INVSIM_MLP_MAX_LAYERS));
    for (int l = 0; l <= n_layers; l++)
        if (dims[l] < 1 || dims[l] > (l == n_layers ? INVSIM_POLICY_MAX_ACTION : INVSIM_MLP_MAX_WIDTH))
            return fail(h, INVSIM_EINVAL, "ppo: a width outside what invsim_mlp_create accepts");
    if (ppo_lds_bytes(dims, n_layers) > PPO_LDS_MAX)
        return fail(h, INVSIM_ERANGE, "ppo: the activations of one 64-sample tile, (sum of dims + dims[n_layers]) * 260 B, "
                                      "exceed the 160 KiB of LDS");
    return INVSIM_OK;
}

int invsim_ppo_scratch_bytes(const int32_t *dims, int32_t n_layers, int64_t rows, int64_t *bytes) {
    if (!bytes) return fail(nullptr, INVSIM_EINVAL, "null argument");
    if (rows < 0) return fail(nullptr, INVSIM_EINVAL, "ppo: rows must be >= 0");
    if (int rc = ppo_dims_check(nullptr, dims, n_layers)) return rc;
    *bytes = ppo_scratch_bytes(dims, n_layers, rows);
    return INVSIM_OK;
}

// what the two gradient calls share: the object's shapes, the scratch layout and the output pointers
static int ppo_common(invsim_handle *h, const invsim_mlp *m, const void *obs0, int64_t n0, const void *obs, const int64_t *idx,
                      int64_t rows, const uint8_t *valid, float *const *gw, float *const *gb, double *stats, void *scratch,
                      int64_t scratch_bytes, PpoArgs &a) {
    const MlpDev &d = m->dev;
    if (rows < 0 || n0 < 0) return fail(h, INVSIM_EINVAL, "ppo: rows and n0 must be >= 0");
    if (int rc = ppo_dims_check(h, d.dims, d.n_layers)) return rc;
    if (rows == 0) return INVSIM_OK;
    if ((n0 > 0 && !obs0) || !obs) return fail(h, INVSIM_EINVAL, "ppo: null obs0 / obs");
    if (!scratch) return fail(h, INVSIM_EINVAL, "ppo: null scratch");
    if (scratch_bytes < ppo_scratch_bytes(d.dims, d.n_layers, rows))
        return fail(h, INVSIM_ERANGE, "ppo: scratch is smaller than invsim_ppo_scratch_bytes");
    a.dev = m->dev_copy;
    a.obs0 = obs0, a.obs = obs, a.n0 = n0, a.rows = rows, a.idx = idx, a.valid = valid;
    a.groups = ppo_groups(rows);
    a.pfloats = ppo_partial_floats(d.dims, d.n_layers);
    a.stat_part = static_cast<double *>(scratch);
    a.part = reinterpret_cast<float *>(a.stat_part + (int64_t)a.groups * PPO_STATS);
    a.n_layers = d.n_layers, a.A = d.dims[d.n_layers];
    int64_t off = 0;
    for (int l = 0; l < d.n_layers; l++) {
        a.in[l] = d.dims[l], a.out[l] = d.dims[l + 1];
        a.off[l] = off;
        off += ((int64_t)d.dims[l] + 1) * d.dims[l + 1];
        a.gw[l] = gw ? gw[l] : nullptr;
        a.gb[l] = gb ? gb[l] : nullptr;
    }
    a.off[d.n_layers] = off;
    a.stats = stats;
    return INVSIM_OK;
}

int invsim_ppo_actor_grad(invsim_handle *h, const invsim_mlp *m, const void *obs0, int64_t n0, const void *obs,
                          const int64_t *idx, int64_t rows, const uint8_t *valid, const float *raw_actions,
                          const float *old_logp, const float *advantages, const double *adv_stats, double clip_range,
                          double ent_coef, float *const *grad_weight, float *const *grad_bias, float *grad_log_std,
                          double *stats, void *scratch, int64_t scratch_bytes, void *stream) {
    TraceRange tr_("invsim_ppo_actor_grad");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = mlp_actor_check(h, m)) return rc;
    if (!m->gauss)
        return fail(h, INVSIM_EINVAL, "no Gaussian set on this invsim_mlp: give std and log_std with "
                                      "invsim_mlp_set_gaussian or invsim_mlp_update");
    if (!(clip_range > 0.0)) return fail(h, INVSIM_EINVAL, "ppo: clip_range must be > 0");
    PpoArgs a{};
    if (int rc = ppo_common(h, m, obs0, n0, obs, idx, rows, valid, grad_weight, grad_bias, stats, scratch, scratch_bytes, a))
        return rc;
    if (rows == 0) return INVSIM_OK;
    if (!raw_actions || !old_logp || !advantages) return fail(h, INVSIM_EINVAL, "ppo: null raw_actions / old_logp / advantages");
    a.raw = raw_actions, a.old_logp = old_logp, a.adv = advantages, a.adv_stats = adv_stats;
    a.std = m->g_std, a.log_std = m->g_log_std, a.logp0 = m->logp0;
    a.clip_lo = (float)(1.0 - clip_range), a.clip_hi = (float)(1.0 + clip_range);
    a.gls = grad_log_std;
    a.scale = 1.0, a.ent_coef = ent_coef;
    DeviceGuard g(h->device);
    hipError_t e = ppo_grad_launch(m->dev, a, h->family == INVSIM_INVMGMT, false, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "ppo actor gradient launch");
}

int invsim_value_grad(invsim_handle *h, const invsim_mlp *m, const void *obs0, int64_t n0, const void *obs,
                      const int64_t *idx, int64_t rows, const uint8_t *valid, const float *returns, double vf_coef,
                      float *const *grad_weight, float *const *grad_bias, double *stats, void *scratch,
                      int64_t scratch_bytes, void *stream) {
    TraceRange tr_("invsim_value_grad");
    if (!h || !m) return fail(h, INVSIM_EINVAL, "null argument");
    if (m->owner != h) return fail(h, INVSIM_EINVAL, "this invsim_mlp was created for another handle");
    if (!m->value)
        return fail(h, INVSIM_EINVAL, "this invsim_mlp is an actor: its gradient comes from invsim_ppo_actor_grad");
    PpoArgs a{};
    if (int rc = ppo_common(h, m, obs0, n0, obs, idx, rows, valid, grad_weight, grad_bias, stats, scratch, scratch_bytes, a))
        return rc;
    if (rows == 0) return INVSIM_OK;
    if (!returns) return fail(h, INVSIM_EINVAL, "ppo: null returns");
    a.returns = returns;
    a.log_std = nullptr;
    a.scale = vf_coef, a.ent_coef = 0.0;
    DeviceGuard g(h->device);
    hipError_t e = ppo_grad_launch(m->dev, a, h->family == INVSIM_INVMGMT, true, (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "value gradient launch");
}

int invsim_set_episode_sink(invsim_handle *h, double *ret, double *part) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_episode_sink")) return rc;
    if ((ret == nullptr) != (part == nullptr)) return fail(h, INVSIM_EINVAL, "episode sink: ret and part together");
    h->cm.ep_ret = ret;
    h->cm.ep_part = part;
    sync_common(h);
    return INVSIM_OK;
}

int invsim_debug_ptrs_stats(uint64_t *out, int32_t clear) {
    if (!out) return fail(nullptr, INVSIM_EINVAL, "null argument");
#ifdef INVSIM_PTRS_STATS
    hipError_t (*tus[6])(unsigned long long *, bool) = {ptrs_stats_nv, ptrs_stats_nv_ph, ptrs_stats_im,
                                                        ptrs_stats_im_ph, ptrs_stats_netspec, ptrs_stats_net};
    out[0] = out[1] = out[3] = out[4] = 0;
    out[2] = 0x7ff0000000000000ull;
    for (auto f : tus) {
        unsigned long long v[5];
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = f(v, clear != 0);
        if (e != hipSuccess) return hip_fail(nullptr, e, "ptrs stats");
        out[0] += v[0];
        out[1] += v[1];
        out[3] += v[3];
        out[4] += v[4];
        out[2] = std::min<uint64_t>(out[2], v[2]);
    }
    return INVSIM_OK;
#else
    (void)clear;
    return fail(nullptr, INVSIM_EINVAL, "not a PTRS-statistics build (make -C csrc ptrs_stats)");
#endif
}

int invsim_set_demand_stream(invsim_handle *h, int32_t mode) {
    TraceRange tr_("invsim_set_demand_stream");
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (int rc = refuse_in_capture(h, "set_demand_stream")) return rc;
    if (mode != INVSIM_DEMAND_NUMPY && mode != INVSIM_DEMAND_PHILOX)
        return fail(h, INVSIM_EINVAL, "demand stream must be INVSIM_DEMAND_NUMPY or INVSIM_DEMAND_PHILOX");
    if (mode == h->demand_stream) return INVSIM_OK;
    DeviceGuard g(h->device);
    // steps may still be queued on a caller's non-blocking stream, which the
    // legacy stream does not wait for: drain the device before the commit reads
    // the lookahead slot those steps write
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(h, e, "demand stream switch");
    int rc = commit_rng(h, nullptr);   // the parity stream's lookahead cache ends (legacy stream)
    if (rc != INVSIM_OK) return rc;
    e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return hip_fail(h, e, "demand stream switch");
    h->la.valid = false;
    h->demand_stream = mode;
    h->cm.philox = mode == INVSIM_DEMAND_PHILOX ? 1 : 0;
    sync_common(h);
    return INVSIM_OK;
}

int invsim_demand_stream(const invsim_handle *h, int32_t *mode) {
    if (!h || !mode) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *mode = h->demand_stream;
    return INVSIM_OK;
}

int invsim_kernel_variant(const invsim_handle *h, int32_t *variant) {
    if (!h || !variant) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *variant = h->family == INVSIM_NETINVMGMT ? h->net_spec : 0;
    return INVSIM_OK;
}

int invsim_status(invsim_handle *h, uint32_t *flags, int32_t clear) {
    if (!h || !flags) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = refuse_in_capture(h, "status")) return rc;
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpy(flags, h->cm.status, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(h, e, "status read");
    if (clear && *flags) {
        e = hipMemset(h->cm.status, 0, sizeof(uint32_t));
        if (e != hipSuccess) return hip_fail(h, e, "status clear");
    }
    return INVSIM_OK;
}

int invsim_state_bytes(const invsim_handle *h, int64_t *bytes) {
    if (!h || !bytes) return fail(nullptr, INVSIM_EINVAL, "null argument");
    *bytes = h->arena_bytes;
    return INVSIM_OK;
}

int invsim_state_field(const invsim_handle *h, int32_t idx, char name[32], int64_t *offset,
                       int32_t *elem_bytes, int32_t *rows, int64_t *row_stride) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (idx < 0 || idx >= (int32_t)h->fields.size()) return INVSIM_ERANGE;
    const Field &f = h->fields[idx];
    if (name) {
        std::memset(name, 0, 32);
        std::strncpy(name, f.name.c_str(), 31);
    }
    if (offset) *offset = f.offset;
    if (elem_bytes) *elem_bytes = f.elem;
    if (rows) *rows = f.rows;
    // > 0: [rows][row_stride]; < 0: record layout [-row_stride][rows]; 0: other layout
    if (row_stride) *row_stride = (f.name == "status" || f.name == "philox_step") ? 1 : f.kind == 1 ? -h->Npad : f.kind == 2 ? 0 : h->Npad;
    return INVSIM_OK;
}

int invsim_get_state(invsim_handle *h, void *dst, void *stream) {
    TraceRange tr_("invsim_get_state");
    if (!h || !dst) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = refuse_in_capture(h, "get_state")) return rc;
    DeviceGuard g(h->device);
    int rc = materialize_period(h, (hipStream_t)stream);  // the blob carries per-env periods
    if (rc == INVSIM_OK) rc = commit_rng(h, (hipStream_t)stream);   // and the committed PCG64 states
    if (rc != INVSIM_OK) return rc;
    if (!h->ph_from_blob) {                                // and the fast stream's counter
        hipError_t e0 = hipMemcpyAsync(h->arena + h->o_phstep, &h->ph_step, sizeof(uint64_t),
                                       hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e0 == hipSuccess) e0 = hipStreamSynchronize((hipStream_t)stream);   // the host word may change next
        if (e0 != hipSuccess) return hip_fail(h, e0, "philox_step write");
    }
    hipError_t e = hipMemcpyAsync(dst, h->arena, (size_t)h->arena_bytes, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    return e == hipSuccess ? INVSIM_OK : hip_fail(h, e, "get_state");
}

int invsim_set_state(invsim_handle *h, const void *src, void *stream) {
    TraceRange tr_("invsim_set_state");
    if (!h || !src) return fail(h, INVSIM_EINVAL, "null argument");
    if (int rc = refuse_in_capture(h, "set_state")) return rc;
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpyAsync(h->arena, src, (size_t)h->arena_bytes, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(h, e, "set_state");
    h->t_known = false;  // periods now come from the blob
    h->la.valid = false;
    h->ph_from_blob = true;   // and the fast stream's counter (read when next needed)
    return INVSIM_OK;
}

// ------------------------------------------------------------------ graph capture
int invsim_capture_begin(invsim_handle *h) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (h->capturing) return fail(h, INVSIM_EINVAL, "capture_begin: this handle is already capturing");
    if (h->demand_stream == INVSIM_DEMAND_PHILOX)
        return fail(h, INVSIM_EINVAL, "graph capture needs the numpy demand stream: the fast stream's launch-step "
                                      "counter is a launch parameter and would repeat on every replay");
    h->capturing = true;
    h->cap_t_known = h->t_known;
    h->cap_t_cur = h->t_cur;
    h->cap_la = h->la;
    h->cap_steps = 0;
    return INVSIM_OK;
}

int invsim_capture_end(invsim_handle *h, int64_t *steps) {
    if (!h) return fail(nullptr, INVSIM_EINVAL, "null handle");
    if (!h->capturing) return fail(h, INVSIM_EINVAL, "capture_end without capture_begin");
    if (steps) *steps = h->cap_steps;
    const bool closed = h->t_known == h->cap_t_known && (!h->t_known || h->t_cur == h->cap_t_cur) &&
                        h->la.valid == h->cap_la.valid && (!h->la.valid || h->la.slot == h->cap_la.slot);
    const int32_t t_end = h->t_known ? h->t_cur : -1;
    const bool la_end = h->la.valid;
    // nothing ran: the device is still where capture_begin found it
    h->capturing = false;
    h->t_known = h->cap_t_known;
    h->t_cur = h->cap_t_cur;
    h->la = h->cap_la;
    if (closed) return INVSIM_OK;
    std::string msg = "the captured calls (" + std::to_string(h->cap_steps) + " env steps) move the handle from period " +
                      std::to_string(h->t_known ? h->t_cur : -1) + " to " + std::to_string(t_end);
    if (la_end != h->la.valid) msg += " and change the demand lookahead state";
    msg += ": a replay would not start where the graph was recorded; capture a whole number of episode cycles (" +
           std::to_string(h->horizon + (h->cm.autoreset == AR_NEXT_STEP ? 1 : 0)) +
           " steps) from a handle that has already stepped once";
    return fail(h, INVSIM_ERANGE, msg);
}

int invsim_position(const invsim_handle *h, int64_t *pos) {
    if (!h || !pos) return fail(nullptr, INVSIM_EINVAL, "null argument");
    const uint64_t t = h->t_known ? (uint32_t)h->t_cur : 0xFFFFFFFFu;
    const uint64_t la = h->la.valid ? 2u + (uint64_t)(h->la.slot & 1) : 0u;
    *pos = (int64_t)(t | (la << 32) | ((uint64_t)(h->demand_stream & 1) << 34));
    return INVSIM_OK;
}

}  // extern "C"
