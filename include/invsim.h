/* invsim — MI355X-native vectorised inventory-simulation engine: C ABI.
 *
 * This is the drop-in boundary for the reference's hot path, the Gymnasium
 * `Env.reset()` / `Env.step()` pair of the five environment classes of
 * jacklu2016/or-gym-inventory.  One handle = one batch of N independent env
 * instances of one class, resident in HBM (SoA state), bound to one GPU.
 *
 *   reference interface                                  replaced by
 *   ---------------------------------------------------  ----------------------------------
 *   NewsvendorEnv.__init__            newsvendor.py:52-97   invsim_create_newsvendor
 *   InvManagementMasterEnv.__init__   inventory_management.py:48-141
 *     (+ Backlog/LostSales subclasses :429-451)            invsim_create_invmgmt
 *   NetInvMgmtMasterEnv.__init__      network_management.py:55-106,146-195
 *     (+ Backlog/LostSales subclasses :747-770)            invsim_create_netinvmgmt
 *   gym.Env.reset(seed=s) -> seeding.np_random(s)
 *     (newsvendor.py:102, inventory_management.py:197,
 *      network_management.py:303)                          invsim_seed_range / invsim_seed_words
 *   Env.reset()  newsvendor.py:100-123,
 *                inventory_management.py:186-222,
 *                network_management.py:301-332              invsim_reset
 *   Env.step()   newsvendor.py:125-204,
 *                inventory_management.py:224-352,
 *                network_management.py:436-635              invsim_step
 *   K x Env.step() with pre-computed actions                invsim_rollout
 *   (no reference equivalent: env state is never
 *    checkpointed there)                                   invsim_state_* / invsim_get_state / invsim_set_state
 *
 * Conventions
 *  - Every buffer argument of reset/step/rollout/seed/state calls is a DEVICE
 *    pointer on the handle's GPU, owned by the caller.  Spec structs passed to
 *    invsim_create_* are HOST memory and are copied.
 *  - `stream` is a hipStream_t (NULL = default stream).  Calls are
 *    asynchronous on that stream; the library never synchronises.
 *  - Dtypes follow the reference spaces: Newsvendor obs/action f32;
 *    InvMgmt obs/action int64; NetInvMgmt obs/action f32.  Rewards f64.
 *    terminated/truncated are uint8 (0/1).
 *  - Return 0 on success, a negative errno-style code on failure;
 *    invsim_last_error(h) (or invsim_last_error(NULL) after a failed create)
 *    gives the message.  No exceptions cross the ABI.
 *  - A handle is not thread-safe.  One handle per GPU per process.
 */
#ifndef INVSIM_H
#define INVSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INVSIM_ABI_VERSION 4   /* 2: market samplers appended to invsim_netinvmgmt_spec
                                  3: graph capture (invsim_capture_begin / _end, invsim_position)
                                  4: episode sink (invsim_set_episode_sink, invsim_episode_fold_groups) */

#define INVSIM_OK 0
#define INVSIM_EINVAL (-22)
#define INVSIM_ENOMEM (-12)
#define INVSIM_EDEVICE (-5)
#define INVSIM_ERANGE (-34)

/* Env families */
#define INVSIM_NEWSVENDOR 1
#define INVSIM_INVMGMT 2
#define INVSIM_NETINVMGMT 3

/* Vector autoreset modes (gymnasium.vector.AutoresetMode) */
#define INVSIM_AUTORESET_NEXT_STEP 0 /* gymnasium >= 1.0 default: reset on the step after done   */
#define INVSIM_AUTORESET_SAME_STEP 1 /* SB3 VecEnv: reset in the done step, final obs separately */
#define INVSIM_AUTORESET_DISABLED 2  /* caller resets explicitly                                   */

typedef struct invsim_handle invsim_handle;

/* newsvendor.py:52-61 constructor arguments */
typedef struct {
    int32_t lead_time;         /* <0 is clamped to 0 (:65); at most 128 */
    int32_t step_limit;
    double max_inventory;
    double max_order_quantity;
    double p_max, h_max, k_max, mu_max;
    double gamma;              /* accepted, unused by the dynamics (as in the reference) */
} invsim_newsvendor_spec;

/* inventory_management.py:48-101 after parameter processing.  Coefficient
 * arrays are the reference's float32 arrays (:89-92). */
typedef struct {
    int32_t num_stages;              /* m = len(I0) + 1, 2..9 */
    int32_t periods;
    int32_t backlog;                 /* 1 = InvManagementBacklogEnv, 0 = LostSales */
    int32_t dist;                    /* 1 Poisson(mu), 2 binomial(n, p), 3 integers(low, high + 1),
                                        4 geometric(p), 5 user_D  (inventory_management.py:169-184) */
    double mu;                       /* dist_param['mu'] */
    double alpha;                    /* discount; reward *= alpha**t */
    const int64_t *I0;               /* [m-1] */
    const float *unit_price;         /* [m] = append(p, r[:-1]) */
    const float *unit_cost;          /* [m] = r */
    const float *demand_cost;        /* [m] = k */
    const float *holding_cost;       /* [m] = append(h, 0) */
    const int64_t *supply_capacity;  /* [m-1] = c */
    const int64_t *lead_time;        /* [m-1] = L, each 0..255, and the observation length
                                        (m-1) * (max(L) + 1) <= 311: a wave's window tile
                                        (512 B per entry), the 4 KiB PTRS table and the split
                                        step's 512 B must fit the 160 KiB LDS of a workgroup
                                        (else INVSIM_ERANGE, before any device call) */
    const int64_t *user_D;           /* [periods], dist == 5 only (else NULL) */
    int64_t dist_n;                  /* dist 2: dist_param['n'] */
    double dist_p;                   /* dist 2, 4: dist_param['p'] */
    int64_t dist_low, dist_high;     /* dist 3: dist_param['low'], ['high'] (inclusive) */
} invsim_invmgmt_spec;

/* network_management.py:146-195 classification, compiled to index tables by
 * the host (main nodes sorted; reorder links sorted; retail links in graph
 * edge order; adjacency lists in graph adjacency order). */
typedef struct {
    int32_t n_main;      /* J */
    int32_t n_reorder;   /* E  (= action dim) */
    int32_t n_retail;    /* RL */
    int32_t num_periods;
    int32_t backlog;     /* EFFECTIVE flag (the reference LostSales class runs backlog=True) */
    double alpha;
    /* main nodes [J] */
    const double *I0, *h, *C, *o, *v;
    const int32_t *is_factory, *is_retail;
    /* reorder links [E] */
    const int32_t *sup;             /* supplier main-node index, -1 = raw material */
    const int32_t *pur;             /* purchaser main-node index */
    const int32_t *sup_is_factory;
    const int32_t *L;               /* lead time, 0..255 */
    const double *lp, *lg;          /* price p, pipeline holding g */
    /* retail links [RL] */
    const int32_t *rl_node;         /* retailer main-node index */
    const double *rl_p, *rl_b, *rl_lam;
    const int32_t *rl_user;         /* 1: demand = user_D row (network_management.py:250-255) */
    const double *user_D;           /* [RL][num_periods] or NULL */
    /* CSR adjacency.  succ: successors of each main node (kind 0 = reorder link idx,
     * kind 1 = retail link idx); pred: reorder links into each main node. */
    const int32_t *succ_ptr;        /* [J+1] */
    const int32_t *succ_kind;       /* [succ_ptr[J]] */
    const int32_t *succ_idx;        /* [succ_ptr[J]] */
    const int32_t *pred_ptr;        /* [J+1] */
    const int32_t *pred_idx;        /* [pred_ptr[J]] */
    /* market demand samplers per retail link, the numpy Generator method the
     * edge's demand_dist_func calls with dist_param (network_management.py:
     * 125-127, 257-263; demand = max(0, int(round(draw)))).  rl_dist NULL = all
     * Poisson(rl_lam).  1 poisson(rl_lam), 2 binomial(rl_n, rl_dp),
     * 3 integers(rl_n, rl_high) (high exclusive), 4 geometric(rl_dp).  Graphs
     * with a non-Poisson market run the generic kernel. */
    const int32_t *rl_dist;
    const int64_t *rl_n, *rl_high;
    const double *rl_dp;
} invsim_netinvmgmt_spec;

int invsim_abi_version(void);
const char *invsim_last_error(const invsim_handle *h);

int invsim_create_newsvendor(const invsim_newsvendor_spec *spec, int64_t n_envs, int32_t device,
                             int32_t autoreset_mode, invsim_handle **out);
int invsim_create_invmgmt(const invsim_invmgmt_spec *spec, int64_t n_envs, int32_t device,
                          int32_t autoreset_mode, invsim_handle **out);
int invsim_create_netinvmgmt(const invsim_netinvmgmt_spec *spec, int64_t n_envs, int32_t device,
                             int32_t autoreset_mode, invsim_handle **out);
void invsim_destroy(invsim_handle *h);

/* obs_dim, action_dim, number of demand draws per step (info_demand width), env family */
int invsim_dims(const invsim_handle *h, int32_t *obs_dim, int32_t *action_dim, int32_t *demand_dim,
                int32_t *family);
int invsim_set_autoreset(invsim_handle *h, int32_t mode);

/* Seeding = gymnasium seeding.np_random(seed): numpy SeedSequence(seed) -> PCG64.
 * seed_range: env i (mask[i] != 0, or all when mask == NULL) gets the 128-bit
 * integer seed  base + first_index + i  (gymnasium SyncVectorEnv: seed + i).
 * seed_words: env i gets the little-endian uint32 entropy words[i][0..nwords[i]).
 * An unmasked seed (mask == NULL) also restarts the fast demand stream's
 * launch-step counter (INVSIM_DEMAND_PHILOX below), so reseeding every env with
 * the same seeds replays the same demands; a masked seed keeps the counter. */
int invsim_seed_range(invsim_handle *h, uint64_t base_lo, uint64_t base_hi, int64_t first_index,
                      const uint8_t *mask, void *stream);
int invsim_seed_words(invsim_handle *h, const uint32_t *words /*[N][4]*/,
                      const int32_t *nwords /*[N]*/, const uint8_t *mask, void *stream);

/* Env.reset() on every env (mask NULL) or on mask[i] != 0; writes obs rows of
 * the reset envs (obs may be NULL).  RNG streams continue (reset without seed). */
int invsim_reset(invsim_handle *h, const uint8_t *mask, void *obs, void *stream);

/* One Env.step() on all N envs.  actions [N][A]; obs [N][O]; reward [N];
 * terminated/truncated [N]; final_obs [N][O] (SAME_STEP mode only, may be NULL). */
int invsim_step(invsim_handle *h, const void *actions, void *obs, double *reward,
                uint8_t *terminated, uint8_t *truncated, void *final_obs, void *stream);

/* K consecutive steps in one launch (state held in registers between steps):
 * identical results to K invsim_step calls.  actions [K][N][A]; obs [K][N][O];
 * reward/terminated/truncated [K][N]. */
int invsim_rollout(invsim_handle *h, int32_t K, const void *actions, void *obs, double *reward,
                   uint8_t *terminated, uint8_t *truncated, void *stream);

/* Sticky device status word (bit 0: an env was stepped past its horizon with
 * autoreset disabled while the period was not lock-step; such steps are not
 * applied).  Synchronous.  clear != 0 resets it.  invsim_step / invsim_rollout /
 * invsim_rollout_policy of an InvMgmt or NetInvMgmt handle in that state read it
 * themselves (one stream sync) and return INVSIM_ERANGE ("...horizon...") after
 * clearing it: the reference's IndexError (inventory_management.py:267). */
int invsim_status(invsim_handle *h, uint32_t *flags, int32_t clear);

/* ---- Closed-loop rollouts with an in-kernel heuristic agent.
 * The reference's benchmark agents, restated on device:
 *   INVSIM_POLICY_CONSTANT     ConstantOrderAgent  benchmark_NetInvMgmtBacklogEnv.py:119-135
 *                              (any family: the same action every step)
 *   INVSIM_POLICY_BASE_STOCK   BaseStockAgent      benchmark_InvManagementBacklogEnv.py:142-198
 *                              (InvMgmt; also benchmark_InvManagementLostSalesEnv.py:137-165)
 *   INVSIM_POLICY_ORDER_UP_TO  OrderUpToHeuristicAgent  benchmark_newsvendor.py:97-111 (Newsvendor)
 *   INVSIM_POLICY_CLASSIC_NV   ClassicNewsvendorAgent   benchmark_newsvendor.py:113-161 (Newsvendor;
 *                              variant 0 = cr_method 'k_vs_h', 1 = 'profit_margin'; scipy
 *                              poisson.ppf restated on device, newsvendor.hip nv_poisson_ppf)
 *   INVSIM_POLICY_SS           sSPolicyAgent  benchmark_newsvendor_sb3_rllib.py:363-371 (Newsvendor;
 *                              safety_factor carries S_buffer_factor)
 *   INVSIM_POLICY_RANDOM       RandomAgent (env.action_space.sample() every step; the first
 *                              agent of every benchmark_*.py list), any family and any graph:
 *                              see "RandomAgent" below
 *   INVSIM_POLICY_LEVELS       BaseStockAgent's rule with per-env, per-stage order-up-to levels
 *                              (and optional reorder points) from attached device arrays
 *                              (InvMgmt): see "Per-env base-stock levels" below
 *   INVSIM_POLICY_NET_LEVELS   installation base-stock on a supply network: every reorder link
 *                              orders up to its own per-env level against its purchaser's
 *                              inventory position (NetInvMgmt, any graph): see "Per-env
 *                              order-up-to levels on a supply network" below
 * CLASSIC_NV / SS need mu_max * (lead_time + 1) * max(1, safety_factor) <= 1e6 (INVSIM_ERANGE).
 * Per-env metrics (f64, accumulated with += so a caller may chain launches),
 * the sums evaluate_agent keeps (benchmark_InvManagementBacklogEnv.py:346-440,
 * benchmark_NetInvMgmtLostSalesEnv.py:241-312, benchmark_newsvendor.py:219-250):
 *   [0] sum of rewards (TotalReward)   [1] steps
 *   InvMgmt:    [2] demand_realized  [3] sales[0]  [4] unfulfilled[0]
 *               [5] sum over stages of max(0, ending_inventory)
 *   NetInvMgmt: [2] retail demand D  [3] retail sales S  [4] retail U[t+1]
 *               [5 + j] X[t+1] of main node j (j < n_main)
 *   Newsvendor: [0], [1] only
 * Unavailable with SAME_STEP autoreset.  On NetInvMgmt graphs other than the
 * reference's default / custom ones (invsim_kernel_variant == 0) the agents
 * are CONSTANT, RANDOM and NET_LEVELS. */
#define INVSIM_POLICY_CONSTANT 1
#define INVSIM_POLICY_BASE_STOCK 2
#define INVSIM_POLICY_ORDER_UP_TO 3
#define INVSIM_POLICY_CLASSIC_NV 4
#define INVSIM_POLICY_SS 5
#define INVSIM_POLICY_RANDOM 6
#define INVSIM_POLICY_MAX_ACTION 32

typedef struct {
    int32_t kind;            /* INVSIM_POLICY_* */
    int32_t variant;         /* CLASSIC_NV: 0 'k_vs_h', 1 'profit_margin'; else 0 */
    double safety_factor;    /* BASE_STOCK / ORDER_UP_TO / CLASSIC_NV; SS: S_buffer_factor */
    double mu;               /* BASE_STOCK: env.dist_param.get('mu', 10) as the agent reads it */
    const void *constant;    /* CONSTANT: host array [action_dim] in the action dtype: the action.
                              * RANDOM: host array [action_dim] in the action dtype: the action
                              * space's upper bounds `high` (the field's second use).
                              * NET_LEVELS: the same f32 upper bounds `high`.
                              * All: action_dim <= INVSIM_POLICY_MAX_ACTION (INVSIM_ERANGE) */
} invsim_policy;

int invsim_metrics_dim(const invsim_handle *h, int32_t *dim);

/* K steps of every env under `policy`.  All outputs may be NULL: obs [K][N][O],
 * reward / terminated / truncated [K][N], actions [K][N][A] (the actions the
 * agent took), metrics [N][invsim_metrics_dim] (+=).  Autoreset as set. */
int invsim_rollout_policy(invsim_handle *h, int32_t K, const invsim_policy *policy, void *obs, double *reward,
                          uint8_t *terminated, uint8_t *truncated, void *actions, double *metrics, void *stream);

/* K steps with caller-supplied actions, as invsim_rollout, that also keep
 * evaluate_agent's per-env sums, as invsim_rollout_policy does for its agents:
 * the entry point for policies that run outside the kernels (a torch network
 * between K = 1 launches on the same stream, or open-loop [K][N][A] plans
 * scored by their per-env return).
 *   outputs    `actions` is required (INVSIM_EINVAL).  obs may be NULL; reward /
 *              terminated / truncated are given together or not at all; metrics
 *              may be NULL.
 *   dynamics   identical to invsim_rollout with the same actions: where given,
 *              obs, rewards and flags have the same bits, and so do the state
 *              blob, info_demand and the info record afterwards.
 *   metrics    accumulated exactly where and how invsim_rollout_policy
 *              accumulates them: the same columns, += per applied step in step
 *              order.  A NEXT_STEP reset step adds nothing; a step refused past
 *              the horizon adds nothing.  A call with the actions an in-kernel
 *              agent recorded leaves the metric bits of that agent's rollout.
 *   shared     unavailable with SAME_STEP autoreset (INVSIM_EINVAL); the episode
 *              sink (which then needs the reward triple), the capture bracket
 *              and the horizon refusal (INVSIM_ERANGE, before any launch when
 *              the period is lock-step) behave as for invsim_rollout_policy.
 *              Both demand streams, every NetInvMgmt graph, per-env periods.
 * Every K runs the one-wave run kernels (there is no fused variant). */
int invsim_rollout_metrics(invsim_handle *h, int32_t K, const void *actions /* [K][N][A], action dtype */,
                           void *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                           double *metrics /* [N][invsim_metrics_dim], += */, void *stream);

/* ---- MLP actor: a trained feed-forward policy evaluated by the library, one
 * kernel per step (the actors the reference's scripts wrap in SB3AgentWrapper,
 * benchmark_InvManagementBacklogEnv.py:332-342; SB3's mlp_extractor +
 * action_net).  The network is a kernel of its own, observations in, actions
 * out; invsim_rollout_mlp issues the closed loop in C: per step that kernel and
 * then the one-step run kernel of invsim_rollout_metrics, on one stream, with
 * no host round trip.
 *
 * Arithmetic contract.  Results here are defined bit for bit, so the network is
 * defined op by op; a CPU restatement reproduces it exactly.
 *   numbers    everything is IEEE binary32, round to nearest, subnormals kept.
 *              Every multiply-add is one fused fmaf(a, b, c) (one rounding);
 *              there is no unfused a * b + c anywhere.
 *   input      x[i] = (float)obs[i]: int64 observations are cast round to
 *              nearest (numpy's astype(float32)), f32 ones are taken as they
 *              are.  With in_scale: x[i] = fmaf(x[i], in_scale[i], in_shift[i]).
 *   linear     layer l, output unit j: acc = bias[l][j] (+0.0f without a bias);
 *              then for i = 0 .. in - 1 in ascending order
 *              acc = fmaf(W[l][j][i], x[i], acc).  The order within one unit is
 *              the contract; how units are spread over lanes and waves is not.
 *   hidden     one activation kind per network, after every layer but the last:
 *              INVSIM_MLP_RELU  acc > 0 ? acc : +0.0f (a NaN gives +0.0f);
 *              INVSIM_MLP_TANH  the device's tanhf(acc).
 *   output     out_activation NONE or TANH on the last layer's units; then, with
 *              out_scale, raw[a] = fmaf(raw[a], out_scale[a], out_shift[a]) (the
 *              rescaling of a squashed actor: low + 0.5 (tanh + 1) (high - low)
 *              is out_scale = 0.5 (high - low), out_shift = low + out_scale).
 *   conversion raw -> action is invsim.policies.convert_actions.  int64 spaces:
 *              promote to f64; with clip, x < low ? low : x, then x > high ?
 *              high : x, on the bounds as f64; NaN -> 0; truncate toward zero
 *              (without clip the caller answers for the int64 range).  f32
 *              spaces: with clip, (r > low || r is NaN) ? r : low, then (x < high
 *              || NaN) ? x : high: a NaN passes, an infinite bound leaves the
 *              value alone, a value equal to a bound becomes the bound (-0.0 at
 *              a bound of 0 gives +0.0).
 * A RELU or purely linear network without a TANH output activation is therefore
 * reproducible bit for bit on a CPU.  TANH networks are defined up to the
 * device's tanhf: its last-ulp results are the ROCm device library's, not
 * glibc's; everything around it is still exact (actions == the conversion of
 * the raw outputs the kernel reports).  No matrix-core instructions are used:
 * their accumulation order could not be restated.
 *
 * invsim_mlp_create validates on the host before any device call: n_layers
 * outside 1..INVSIM_MLP_MAX_LAYERS, dims[0] != obs_dim, dims[n_layers] !=
 * action_dim, a hidden width outside 1..INVSIM_MLP_MAX_WIDTH, obs_dim >
 * INVSIM_MLP_MAX_WIDTH or action_dim > INVSIM_POLICY_MAX_ACTION return
 * INVSIM_ERANGE; unknown activation kinds, a scale without its shift, clip
 * without bounds and null arguments return INVSIM_EINVAL.  It copies the
 * parameters to the handle's GPU, allocates the closed loop's scratch (one
 * [N][O] obs row, one [N][A] action row), and may synchronise: not during
 * capture.  The object belongs to the handle it was created for (another
 * handle: INVSIM_EINVAL) and must be destroyed before it.  invsim_mlp_destroy
 * frees device memory, which synchronises: inside a capture bracket it does
 * nothing but set the handle's error message, and the object stays valid.
 *
 * invsim_mlp_actions is one launch, obs rows -> raw outputs and / or actions;
 * it does not touch env state and is legal inside a capture bracket.
 *
 * invsim_rollout_mlp: for k = 0 .. K - 1 the network reads obs0 (k = 0) or obs
 * row k - 1 and one env step with those actions writes obs row k.  obs0 is
 * required (INVSIM_EINVAL); when `obs` is given its rows are both the output
 * and the next step's input, otherwise (and for `actions`) the object's
 * scratch rows are used.  In everything else it is invsim_rollout_metrics
 * with the actions the network produced: SAME_STEP refused, the reward triple
 * together or not at all, metrics += per applied step (a NEXT_STEP reset step
 * still runs the network and records its action, and adds nothing), episode
 * sink (the call's K output rows are folded once, after the loop, as
 * invsim_episode_fold_groups over those K rows would), capture bracket, both
 * demand streams, every NetInvMgmt graph, per-env periods.  The lock-step horizon refusal (INVSIM_ERANGE) covers all K steps
 * and comes before the first launch; with per-env periods and DISABLED
 * autoreset the status word is read once, after the loop. */
#define INVSIM_MLP_NONE 0
#define INVSIM_MLP_RELU 1
#define INVSIM_MLP_TANH 2
#define INVSIM_MLP_MAX_LAYERS 5     /* linear layers: up to 4 hidden */
#define INVSIM_MLP_MAX_WIDTH 256    /* hidden units per layer */

typedef struct {
    int32_t n_layers;               /* linear layers, 1..INVSIM_MLP_MAX_LAYERS */
    int32_t activation;             /* hidden: RELU or TANH (ignored when n_layers == 1) */
    int32_t out_activation;         /* NONE or TANH */
    int32_t clip;                   /* 1: clamp to the bounds below */
    const int32_t *dims;            /* host [n_layers + 1]; dims[0] = obs_dim, dims[n_layers] = action_dim */
    const float *const *weight;     /* host [n_layers] -> row-major [dims[l+1]][dims[l]] (torch Linear.weight) */
    const float *const *bias;       /* host [n_layers] -> [dims[l+1]]; the array or an entry may be NULL */
    const float *in_scale, *in_shift;    /* host [obs_dim], both or neither */
    const float *out_scale, *out_shift;  /* host [action_dim], both or neither */
    const void *low, *high;         /* host [action_dim], action dtype; needed when clip */
} invsim_mlp_spec;
typedef struct invsim_mlp invsim_mlp;

int invsim_mlp_create(invsim_handle *h, const invsim_mlp_spec *spec, invsim_mlp **out);
void invsim_mlp_destroy(invsim_mlp *m);
int invsim_mlp_actions(invsim_handle *h, const invsim_mlp *m, const void *obs /* [N][O], obs dtype */,
                       void *actions /* [N][A], action dtype, may be NULL */,
                       float *raw /* [N][A], may be NULL */, void *stream);
int invsim_rollout_mlp(invsim_handle *h, int32_t K, const invsim_mlp *m, const void *obs0 /* [N][O] */,
                       void *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                       void *actions, double *metrics, void *stream);

/* ---- Gaussian MLP actor: rollout collection for on-policy learners (the
 * reference's benchmark_*_sb3_rllib.py train SB3 PPO / A2C and RLlib PPO, whose
 * rollouts come from a diagonal Gaussian around the network's output).  The
 * sampling launch is the MLP actor's kernel with one more stage: after the last
 * layer every env draws action_dim standard normals from its action generator
 * (the RandomAgent section's PCG64 streams: seeding, checkpointing and sharding
 * are theirs), and the launch reports the sample, its log-probability and the
 * converted action.  The critic is not part of this: values do not feed back
 * into the closed loop, a caller evaluates them over the returned obs rows.
 *
 * Contract (on top of "MLP actor"; A = action_dim):
 *   draws      every launch step of every env < N consumes exactly A standard
 *              normals z from the env's action generator, in ascending action
 *              index, whether or not the step is applied (a NEXT_STEP reset step
 *              draws too, as RANDOM does).  z is numpy 2.2.6's
 *              Generator.standard_normal (random_standard_normal: the 256-level
 *              ziggurat over ki / wi / fi, unfused f64 arithmetic), bit for bit
 *              up to the device library's log1p / exp on the 1.4 % of draws
 *              that leave the fast path.  The demand `rng` rows and philox_step
 *              are never touched.
 *   sample     zf = (float)z;  raw[a] = fmaf(std[a], zf, mean[a]), where mean is
 *              what invsim_mlp_actions reports as raw.
 *   log-prob   acc = (float)(-0.91893853320467274178 * (double)A), computed on
 *              the host; for a ascending: acc = fmaf(-0.5f * zf, zf, acc), then
 *              acc = acc - log_std[a].  The density of the unclipped sample,
 *              which is what SB3 stores.
 *   conversion exactly the MLP actor's, applied to raw.
 *
 * invsim_mlp_set_gaussian copies std and log_std (host [A] arrays) into the
 * object's parameter blob; it waits for the device first and is refused during
 * capture.  std must be finite and >= 0 and log_std finite (INVSIM_EINVAL).
 * The library calls no transcendental: the caller supplies both arrays and
 * answers for their agreement.  NULL std clears the Gaussian.
 *
 * invsim_mlp_sample is one launch.  Each output may be NULL, but not all of
 * them; whatever is requested, the generators advance by A normals.  Without a
 * Gaussian on m or without action generators on h (invsim_set_action_rng) it
 * returns INVSIM_EINVAL.  It does not touch env state and is legal inside a
 * capture bracket: the generators are device-resident, so a replay continues
 * the stream.
 *
 * invsim_rollout_mlp_sample is invsim_rollout_mlp with the sampling launch in
 * place of the deterministic one; raw [K][N][A] and logp [K][N] may be NULL.
 * Everything else is unchanged: every refusal comes before the first launch,
 * SAME_STEP refused, the sink folded once, capture, both demand streams, every
 * graph, per-env periods. */
int invsim_mlp_set_gaussian(invsim_handle *h, invsim_mlp *m, const float *std /* host [A], NULL clears */,
                            const float *log_std /* host [A] */);
int invsim_mlp_sample(invsim_handle *h, const invsim_mlp *m, const void *obs /* [N][O], obs dtype */,
                      void *actions /* [N][A], action dtype */, float *raw /* [N][A] */, float *mean /* [N][A] */,
                      float *logp /* [N] */, void *stream);
int invsim_rollout_mlp_sample(invsim_handle *h, int32_t K, const invsim_mlp *m, const void *obs0 /* [N][O] */,
                              void *obs, double *reward, uint8_t *terminated, uint8_t *truncated, void *actions,
                              float *raw /* [K][N][A] */, float *logp /* [K][N] */, double *metrics, void *stream);

/* ---- Critic, GAE and parameter updates: what an on-policy iteration (PPO /
 * A2C, the reference's benchmark_*_sb3_rllib.py) needs around the collected
 * rollout, with no host synchronisation: values under the MLP actor's
 * arithmetic, advantages as one backward scan, and new weights written into an
 * existing object on the stream.
 *
 * Value networks.  invsim_mlp_create_value is invsim_mlp_create (same spec,
 * same host-side validation, same blob) with these differences: dims[n_layers]
 * must be 1 (INVSIM_ERANGE); clip must be 0 (INVSIM_EINVAL), low / high are
 * ignored; out_scale / out_shift are [1] and de-normalise the value; no scratch
 * rows are allocated.  invsim_mlp_destroy frees it.  invsim_mlp_values is the
 * MLP actor's kernel through its raw output: values[r] is the "MLP actor"
 * contract up to `output` on obs row r, and no conversion is applied.  `rows`
 * is independent of the handle's N (one launch covers [K][N][O]); rows == 0
 * is a no-op, rows < 0 INVSIM_EINVAL.  It does not touch env state and is legal
 * inside a capture bracket.  A value object is refused (INVSIM_EINVAL) by
 * invsim_mlp_actions, invsim_mlp_sample, invsim_mlp_set_gaussian,
 * invsim_rollout_mlp and invsim_rollout_mlp_sample; an actor is refused by
 * invsim_mlp_values; another handle's object is refused everywhere.
 *
 * GAE.  invsim_gae is handle-free, like invsim_episode_fold, and runs on the
 * current device.  value0[n] is V of the observation the first step's network
 * saw (obs0), values[k][n] V of obs row k, done0 terminated | truncated of the
 * row just before this block (the previous call's last row; NULL: no env had
 * just finished).  Per env n, for k = K - 1 down to 0, in f64 with every
 * operation rounded separately (no fused multiply-add), carry = +0.0 at first:
 *   done_k = terminated[k][n] | truncated[k][n]           (a NULL array reads 0)
 *   prev   = k > 0 ? done_{k-1} : (done0 ? done0[n] != 0 : 0)
 *   vp = (double)(k > 0 ? values[k-1][n] : value0[n]);   vn = (double)values[k][n]
 *   if prev:      the row after a finished episode: NEXT_STEP's reset row, no transition
 *       advantages[k][n] = +0.0f;  returns[k][n] = (float)vp;  valid = 0;  carry = +0.0
 *   else:
 *       b     = terminated[k][n] ? +0.0 : gamma * vn        truncation bootstraps from the final obs
 *       delta = (reward[k][n] + b) - vp
 *       adv   = done_k ? delta : delta + gl * carry         gl = gamma * lambda, one product on the host
 *       carry = adv;  advantages[k][n] = (float)adv;  returns[k][n] = (float)(adv + vp);  valid = 1
 * Under NEXT_STEP autoreset obs row k of a truncated step is the episode's
 * final observation, so gamma * V(that row) is the truncation bootstrap; row
 * k + 1 is the reset row (reward 0, action ignored by the env), which `valid`
 * masks out of a loss.  K < 0 or n_envs < 0 is INVSIM_EINVAL; K == 0 or n_envs
 * == 0 returns INVSIM_OK without a launch; otherwise a NULL reward, value0,
 * values, advantages or returns is INVSIM_EINVAL.  NaN and infinite inputs
 * propagate by the formulas; gamma and lambda are not range-checked.  One
 * launch, no atomics: the result is deterministic.  Capturable.
 *
 * Parameter updates.  invsim_mlp_update enqueues one small launch on `stream`
 * that rewrites the object's parameter blob from the caller's device arrays, in
 * the layout invsim_mlp_create builds (transposed, zero padded: the padding
 * stays zero); a NULL weight / bias entry, or a NULL array, keeps what the
 * object has.  With std / log_std (device [A], both or neither: INVSIM_EINVAL)
 * it also writes the Gaussian rows and sets the object's Gaussian, as
 * invsim_mlp_set_gaussian does; on a value object std is INVSIM_EINVAL.  No
 * allocation, no host copy, no synchronisation: launches on `stream` after it
 * see the new parameters, and the caller orders it against launches on other
 * streams.  Legal inside a capture bracket; a replay re-reads the caller's
 * arrays as they are then.  The layer shapes are the object's: there is nothing
 * to validate on the device, and the caller answers for finite std >= 0. */
int invsim_mlp_create_value(invsim_handle *h, const invsim_mlp_spec *spec, invsim_mlp **out);
int invsim_mlp_values(invsim_handle *h, const invsim_mlp *m, const void *obs /* [rows][O], obs dtype */,
                      int64_t rows, float *values /* [rows] */, void *stream);
int invsim_gae(const double *reward /* [K][n] */, const uint8_t *terminated, const uint8_t *truncated /* [K][n], either may be NULL */,
               const uint8_t *done0 /* [n] or NULL */, const float *value0 /* [n] */, const float *values /* [K][n] */,
               int32_t K, int64_t n_envs, double gamma, double lambda,
               float *advantages /* [K][n] */, float *returns /* [K][n] */, uint8_t *valid /* [K][n], may be NULL */,
               void *stream);
int invsim_mlp_update(invsim_handle *h, invsim_mlp *m,
                      const float *const *weight /* host array of n_layers DEVICE pointers, row-major [dims[l+1]][dims[l]] */,
                      const float *const *bias /* likewise, [dims[l+1]] */, const float *std,
                      const float *log_std /* DEVICE [A], both or neither */, void *stream);

/* ---- Running normalisation: what SB3's VecNormalize keeps around a PPO / A2C
 * learner on these envs (observations are raw inventory counts, rewards are in
 * the hundreds): running moments of the observations, the running variance of
 * the discounted return, rewards scaled by it, and the network's in_scale /
 * in_shift rows rewritten from the moments, all on the stream.
 *
 * Shared rules.  The entry points without a handle run on the current device,
 * like invsim_gae; invsim_mlp_set_input_norm runs on its handle's device.  None
 * allocates or synchronises, all are legal inside a capture bracket, none uses
 * atomics (the results are deterministic), and every refusal happens on the
 * host before any launch.  All arithmetic is f64 with one rounding per
 * operation (no fused multiply-add); division and square root are the IEEE
 * correctly rounded ones, so a numpy restatement gives the same bits.  NaN and
 * infinity propagate by the formulas.
 *
 * invsim_moments folds the rows of x [rows][cols] (row-major, `dtype` one of
 * INVSIM_DTYPE_*) into stats, device f64 [3][cols], in/out: row 0 the count,
 * row 1 the mean, row 2 M2, the sum of squared deviations.  mask [rows] u8 or
 * NULL: a row counts where its byte is non-zero (NULL: every row).
 *   leaves  rows are cut into blocks of INVSIM_MOMENTS_BLOCK consecutive rows
 *           (the last may be short).  Per block and column c:
 *             n = the number of unmasked rows, as a double
 *             s = +0.0;  for unmasked r ascending: s = s + (double)x[r][c]
 *             mean = s / n
 *             q = +0.0;  for unmasked r ascending: d = (double)x[r][c] - mean;  q = q + d * d
 *           the leaf is (n, mean, q); a block with no unmasked row is (0, +0.0, +0.0).
 *   merge   Merge(a, b): if n_b == 0 the result is a; else if n_a == 0 it is b; else
 *             n = n_a + n_b;  d = mean_b - mean_a;  w = n_b / n
 *             mean = mean_a + d * w;  M2 = (M2_a + M2_b) + (d * d) * (n_a * w)
 *   tree    level 0 is the leaves in block order; node i of level l + 1 is
 *           Merge(node 2i, node 2i + 1) of level l, an unpaired last node passes
 *           up unchanged; this repeats until one node is left, the batch.  Then
 *           stats = Merge(stats, batch), the running statistics on the left.
 * How blocks map to lanes, workgroups and launches is not part of the contract
 * (any aligned power-of-two group of nodes reduced in one place reproduces the
 * tree).  scratch is device memory of at least invsim_moments_scratch_bytes
 * bytes, 8-byte aligned; the call may overwrite all of it.  rows < 0, cols < 1
 * or an unknown dtype is INVSIM_EINVAL, cols > 1024 INVSIM_ERANGE; then rows == 0
 * returns INVSIM_OK without a launch; then a NULL x / stats / scratch is
 * INVSIM_EINVAL and a scratch_bytes below the requirement INVSIM_ERANGE.
 *
 * invsim_discounted_returns is VecNormalize's `returns` over K rows.  ret [n]
 * f64, in/out, is the running discounted return; out [K][n] f64; valid [K][n]
 * u8 may be NULL.  done_k and prev are invsim_gae's, with its done0 and
 * NULL-flag rules.  Per env, for k ascending:
 *   if prev:   the NEXT_STEP reset row:  out[k][n] = +0.0;  valid = 0;  ret = +0.0
 *   else:      t = ret * gamma;  ret = t + reward[k][n];  out[k][n] = ret;  valid = 1;
 *              if done_k: ret = +0.0 after the store
 * K < 0 or n_envs < 0 is INVSIM_EINVAL; K == 0 or n_envs == 0 returns INVSIM_OK
 * without a launch; otherwise a NULL reward, ret or out is INVSIM_EINVAL.
 *
 * invsim_normalize_rewards: stats is the [3][1] statistics of the returns;
 *   var = cnt == 0 ? 1.0 : M2 / cnt;  sd = sqrt(var + epsilon);  v = reward[i] / sd
 *   out[i] = v < -clip ? -clip : (v > clip ? clip : v)          a NaN passes
 * i.e. np.clip(reward / np.sqrt(var + eps), -clip, clip).  out may alias reward.
 * clip <= 0 or NaN and count < 0 are INVSIM_EINVAL; count == 0 is a no-op;
 * otherwise a NULL reward / stats / out is INVSIM_EINVAL.
 *
 * invsim_norm_params: var as above per column; inv = 1.0 / sqrt(var + epsilon);
 * scale[c] = (float)inv;  shift[c] = (float)(-(mean * inv)): device f32 [cols],
 * shift may be NULL.  fmaf(x, scale, shift) is then the "MLP actor" input stage.
 * cols < 1 or a NULL stats / scale is INVSIM_EINVAL, cols > 1024 INVSIM_ERANGE.
 *
 * invsim_mlp_set_input_norm writes the object's in_scale / in_shift rows from
 * device f32 [obs_dim] arrays: one small launch on `stream`, with
 * invsim_mlp_update's ordering and capture rules (launches on `stream` after it
 * see the new rows; a replay re-reads the arrays).  Actors and value objects
 * alike.  INVSIM_EINVAL: an object created without in_scale (it has no such
 * rows), another handle's object, a NULL array. */
#define INVSIM_DTYPE_I64 0
#define INVSIM_DTYPE_F32 1
#define INVSIM_DTYPE_F64 2
#define INVSIM_MOMENTS_BLOCK 64     /* rows per leaf of invsim_moments' tree */
int invsim_moments_scratch_bytes(int64_t rows, int32_t cols, int64_t *bytes);
int invsim_moments(const void *x /* [rows][cols] */, int32_t dtype, int64_t rows, int32_t cols,
                   const uint8_t *mask /* [rows] or NULL */, double *stats /* [3][cols], in/out */,
                   void *scratch, int64_t scratch_bytes, void *stream);
int invsim_discounted_returns(const double *reward /* [K][n] */, const uint8_t *terminated, const uint8_t *truncated /* [K][n], either may be NULL */,
                              const uint8_t *done0 /* [n] or NULL */, int32_t K, int64_t n_envs, double gamma,
                              double *ret /* [n], in/out */, double *out /* [K][n] */, uint8_t *valid /* [K][n], may be NULL */,
                              void *stream);
int invsim_normalize_rewards(const double *reward /* [count] */, int64_t count, const double *stats /* [3][1] */,
                             double epsilon, double clip, double *out /* [count], may alias reward */, void *stream);
int invsim_norm_params(const double *stats /* [3][cols] */, int32_t cols, double epsilon, float *scale /* [cols] */,
                       float *shift /* [cols], may be NULL */, void *stream);
int invsim_mlp_set_input_norm(invsim_handle *h, invsim_mlp *m, const float *scale, const float *shift /* DEVICE [obs_dim] */,
                              void *stream);

/* ---- PPO gradients: the learner's half of an on-policy iteration for the
 * in-library actor and critic (separate networks, a state-independent log_std):
 * SB3's PPO.train loss and its gradient with respect to every weight, bias and
 * log_std, over one minibatch of a collected rollout.  The optimiser stays with
 * the caller: the gradients land in device arrays of torch's layouts, and
 * invsim_mlp_update hands the new weights back.
 *
 * Sample space.  A call addresses samples s = 0 .. S - 1.  Sample s reads
 * observation row s of the virtual concatenation of obs0 [n0][O] and obs [.][O]
 * (obs dtype): row s is s < n0 ? obs0[s] : obs[s - n0].  With n0 = N, obs0 the
 * rollout's first input and obs its [K][N][O] block, sample k * N + n gets the
 * observation the network saw at step k; no copy and no cast is made.  The
 * kernel casts as the "MLP actor" `input` stage does, in_scale / in_shift as
 * they are in the object's blob when the launch runs.  raw_actions [S][A],
 * old_logp [S], advantages [S], returns [S] and valid [S] (u8, or NULL: every
 * sample counts) are indexed by s.  idx (device int64 [rows], or NULL: 0 ..
 * rows - 1) names the minibatch's samples; repeats are allowed.  The caller
 * answers for 0 <= idx[r] < S: nothing is written through idx.
 *
 * Loss, over the minibatch's valid samples (valid[s] != 0), n their count,
 * every mean a sum divided by n; a minibatch with n = 0 writes all-zero
 * gradients and stats:
 *   forward    mean [A] (actor) and v (critic) are the "MLP actor" contract
 *              through `output`, out_activation and out_scale / out_shift included
 *   sample     z_a = (raw_a - mean_a) / std_a
 *   log-prob   logp = logp0 - sum_a (0.5 z_a^2 + log_std_a), logp0 the
 *              "Gaussian MLP actor" constant
 *   ratio      ratio = exp(logp - old_logp)
 *   advantage  with adv_stats (device f64 [3]: count, mean, M2, the layout of
 *              invsim_moments with one column): adv = (advantages[s] - mean) /
 *              (sqrt(M2 / (count - 1)) + 1e-8); a count below 2 leaves the
 *              advantage as it is.  Without: adv = advantages[s]
 *   policy     policy_loss = -mean(min(adv * ratio, adv * clamp(ratio, 1 -
 *              clip_range, 1 + clip_range)))
 *   entropy    entropy = sum_a (0.5 + 0.5 log(2 pi) + log_std_a)
 *   actor      policy_loss - ent_coef * entropy
 *   critic     vf_coef * mean((returns - v)^2)
 * The outputs are the gradients of the actor loss (invsim_ppo_actor_grad) and
 * of the critic loss (invsim_value_grad) with respect to every weight, bias
 * and log_std.  std = exp(log_std) is treated as tied: d logp / d log_std_a =
 * z_a^2 - 1.  tanh' is 1 - y^2 on the stored activation, relu' is y > 0; the
 * derivative of a TANH output activation and the factor out_scale are
 * included.  The clipped branch, where it is the smaller, has no gradient.
 * A2C is the same call with clip_range = +inf and old_logp the current
 * log-density.
 *   actor stats   f64 [6]: n, policy_loss, entropy, approx_kl = mean((ratio - 1)
 *                 - log ratio), clip fraction = mean(ratio outside [1 -
 *                 clip_range, 1 + clip_range]), mean ratio
 *   critic stats  f64 [2]: n, the unscaled mean((returns - v)^2)
 *
 * Rules.  A sample with valid[s] == 0 is selected out, not multiplied by zero:
 * NaN or garbage in its rows reaches no output.  No atomics: the same call on
 * the same inputs gives the same bits.  The forward half keeps the "MLP actor"
 * contract op by op; how the backward half's partial sums are grouped (64
 * samples in sequence per tile, tiles per workgroup, then at most
 * INVSIM_PPO_MAX_GROUPS partials per parameter in f64) is the implementation's,
 * so gradients are defined to a tolerance, not op by op.  Outputs are
 * overwritten, not accumulated.  grad_weight / grad_bias are host arrays of
 * n_layers DEVICE pointers in torch's layouts ([dims[l+1]][dims[l]] /
 * [dims[l+1]]); the arrays or an entry may be NULL (that gradient is not
 * written), as may grad_log_std [A] and stats.  The calls make no allocation
 * and no synchronisation and are legal inside a capture bracket; they read the
 * object's blob when they run, so a replay after invsim_mlp_update follows the
 * new weights.  scratch is caller-owned device memory of at least
 * invsim_ppo_scratch_bytes bytes, 8-byte aligned; the call may overwrite all of
 * it.  Two launches per call: min(ceil(rows / 64), INVSIM_PPO_MAX_GROUPS)
 * workgroups, then the reduction of their partial sums.
 *
 * Refusals are decided on the host before any launch.  INVSIM_EINVAL: a value
 * object given to invsim_ppo_actor_grad or an actor to invsim_value_grad; an
 * actor without a Gaussian; another handle's object; rows < 0 or n0 < 0;
 * clip_range <= 0 or NaN; then, unless rows == 0 (a no-op returning INVSIM_OK):
 * a NULL obs, a NULL obs0 with n0 > 0, NULL raw_actions / old_logp / advantages
 * / returns, a NULL scratch.  INVSIM_ERANGE: scratch_bytes below the
 * requirement, and a network whose activations of one tile do not fit the LDS:
 *   (dims[0] + ... + dims[n_layers] + dims[n_layers]) * 260 > 163840
 * (every layer's 64 activations at a row stride of 65 floats, and the rescaled
 * output beside the last layer's).  33-256-256-3 and 68-256-256-11 fit; not
 * every legal invsim_mlp does.  invsim_ppo_scratch_bytes is handle-free and
 * host only: INVSIM_EINVAL for NULL dims, n_layers outside
 * 1..INVSIM_MLP_MAX_LAYERS, a width outside what invsim_mlp_create accepts or
 * rows < 0, INVSIM_ERANGE by the same inequality; its value is monotone in
 * rows. */
#define INVSIM_PPO_MAX_GROUPS 256   /* workgroups of one gradient launch: the number of partial sums */
int invsim_ppo_scratch_bytes(const int32_t *dims /* host [n_layers + 1] */, int32_t n_layers, int64_t rows, int64_t *bytes);
int invsim_ppo_actor_grad(invsim_handle *h, const invsim_mlp *m, const void *obs0 /* [n0][O] */, int64_t n0,
                          const void *obs /* [.][O] */, const int64_t *idx /* [rows] or NULL */, int64_t rows,
                          const uint8_t *valid /* [S] or NULL */, const float *raw_actions /* [S][A] */,
                          const float *old_logp /* [S] */, const float *advantages /* [S] */,
                          const double *adv_stats /* [3] or NULL */, double clip_range, double ent_coef,
                          float *const *grad_weight, float *const *grad_bias, float *grad_log_std /* [A] or NULL */,
                          double *stats /* [6] or NULL */, void *scratch, int64_t scratch_bytes, void *stream);
int invsim_value_grad(invsim_handle *h, const invsim_mlp *m, const void *obs0 /* [n0][O] */, int64_t n0,
                      const void *obs /* [.][O] */, const int64_t *idx /* [rows] or NULL */, int64_t rows,
                      const uint8_t *valid /* [S] or NULL */, const float *returns /* [S] */, double vf_coef,
                      float *const *grad_weight, float *const *grad_bias, double *stats /* [2] or NULL */,
                      void *scratch, int64_t scratch_bytes, void *stream);

/* ---- RandomAgent (INVSIM_POLICY_RANDOM).  The reference never seeds
 * action_space, so its RandomAgent has no trajectory to match; the contract is
 * numpy's Generator on a stream of the env's own:
 *   generator  one PCG64 per env, separate from the demand generator, in a
 *              caller-owned device buffer u64 [4][Npad] (invsim_action_rng_bytes;
 *              rows state hi / state lo / inc hi / inc lo, as the `rng` state
 *              field).  invsim_seed_action_rng gives env i
 *              SeedSequence(base + first_index + i); invsim's Python layer uses
 *              base = 2**64 + seed (base_hi = 1), so the actions of seed s do not
 *              replay the demand uniforms of reset(seed=s).  Checkpointing the
 *              stream is cloning the buffer; the handle's arena and state blob
 *              do not hold it.
 *   draws      one launch step of one env consumes exactly action_dim doubles
 *              u = (next_uint64 >> 11) * 2**-53 in action-index order, whether
 *              or not the step is applied (a NEXT_STEP reset step and a step
 *              refused past the horizon draw too): K launch steps advance
 *              every generator by K * action_dim doubles.
 *   actions    f32 spaces (Newsvendor, NetInvMgmt): (float)((double)high[a] * u)
 *              int64 spaces (InvMgmt): (int64)floor((double)(high[a] + 1) * u)
 *              i.e. Generator.uniform(0, high) / uniform(0, high + 1) floored.
 *   recorded   `actions` of invsim_rollout_policy holds the drawn action of
 *              every step, reset steps included (the other agents leave those
 *              rows unwritten), and equals what invsim_sample_actions writes.
 * The action stream is PCG64 under both demand streams and never touches the
 * `rng` rows or philox_step.  The generators are device-resident, so a captured
 * launch continues the stream at every replay.
 * invsim_set_action_rng attaches the buffer to h (NULL detaches; not during
 * capture); a RANDOM rollout or invsim_sample_actions without one returns
 * INVSIM_EINVAL.  invsim_sample_actions draws K steps of actions [K][N][A]
 * (action dtype) from the attached generators and advances them: random
 * actions for callers who feed invsim_step / invsim_rollout themselves. */
int invsim_action_rng_bytes(const invsim_handle *h, int64_t *bytes);
int invsim_seed_action_rng(invsim_handle *h, uint64_t *arng, uint64_t base_lo, uint64_t base_hi,
                           int64_t first_index, void *stream);
int invsim_set_action_rng(invsim_handle *h, uint64_t *arng);
int invsim_sample_actions(invsim_handle *h, int32_t K, const void *high, void *actions /* [K][N][A] */,
                          void *stream);

/* ---- Per-env base-stock levels (INVSIM_POLICY_LEVELS; InvMgmt handles only).
 * The reference's BaseStockAgent orders up to (L_i + 1) * mu * safety_factor,
 * one scalar for every stage and env, and calls that "a HUGE simplification"
 * (benchmark_InvManagementBacklogEnv.py:145-148).  LEVELS is the same rule with
 * the order-up-to level of every env and stage read from a device array, so
 * one launch scores N candidate level vectors (under common random numbers
 * when the envs are seeded alike).
 *
 * invsim_set_policy_levels attaches `levels`, and optionally `reorder`, to h:
 * device f64 [N][action_dim], caller-owned, not copied, read by every LEVELS
 * launch at the time it runs: the caller may rewrite them on the same stream
 * between launches, and a captured graph reads the current values at every
 * replay.  NULL levels detaches both.  Not during capture, and not on another
 * family's handle (INVSIM_EINVAL).
 *
 * invsim_rollout_policy with kind = INVSIM_POLICY_LEVELS (safety_factor, mu,
 * variant and constant are ignored; INVSIM_EINVAL on another family's handle or
 * with nothing attached).  For env n, stage i, at an applied step of period t,
 * bit for bit:
 *   pos = I[t][i] + sum(action_log[max(0, t - L_i) : t, i])   int64, wrapping,
 *                                                  as BASE_STOCK sums it
 *   x = levels[n][i] - (double)pos
 *   with reorder: if not ((double)pos < reorder[n][i]) then x = 0   (the strict <
 *                 of the reference's sSPolicyAgent; a NaN reorder point never orders)
 *   x = x > 0 ? x : 0                              (a NaN level orders 0)
 *   x = x > (double)c_i ? (double)c_i : x
 *   action = (int64_t)x
 * With reorder == NULL and levels[n][i] the f64 value of ((double)(L_i + 1) * mu)
 * * sf, the launch is bit-identical to INVSIM_POLICY_BASE_STOCK with that mu and
 * sf: actions, obs, rewards, flags, metrics, the state blob and the RNG state.
 * Everything else is BASE_STOCK's: `actions` records the order of every stepped
 * env, a NEXT_STEP reset step leaves its row unwritten and adds nothing to the
 * metrics (same columns, same += order), SAME_STEP is refused, and the horizon
 * refusal, the episode sink, the capture bracket, both demand streams, every
 * `dist`, lock-step and per-env periods are unchanged.  It runs on the launch
 * paths BASE_STOCK has (the fused rollout kernels of the default lead times,
 * the one-wave run kernel otherwise). */
#define INVSIM_POLICY_LEVELS 7
int invsim_set_policy_levels(invsim_handle *h, const double *levels, const double *reorder);

/* ---- Per-env order-up-to levels on a supply network (INVSIM_POLICY_NET_LEVELS;
 * NetInvMgmt handles only, any graph).  The reference's NetInvMgmt scripts ship
 * RandomAgent and ConstantOrderAgent only; the classical baseline on a network is
 * an installation base-stock policy: every reorder link orders up to a level of
 * its own against the inventory position of the node that buys over it.  The
 * levels (and optional reorder points) of every env and link are read from a
 * device array, so one launch scores N candidate vectors.
 *
 * invsim_set_policy_net_levels attaches `levels`, and optionally `reorder`, to h:
 * device f64 [N][action_dim] (link k in the handle's reorder-link order),
 * caller-owned, not copied, read by every NET_LEVELS launch at the time it runs
 * (rewritable on the same stream between launches and between replays of a
 * captured graph).  NULL levels detaches both.  Not during capture, and not on
 * another family's handle (INVSIM_EINVAL).  INVSIM_POLICY_LEVELS and
 * invsim_set_policy_levels stay InvMgmt's and refuse a NetInvMgmt handle.
 *
 * invsim_rollout_policy with kind = INVSIM_POLICY_NET_LEVELS: `constant` carries
 * the host f32 [action_dim] upper bounds `high` of the action space (its use
 * under RANDOM); safety_factor, mu and variant are ignored.  action_dim >
 * INVSIM_POLICY_MAX_ACTION returns INVSIM_ERANGE; another family's handle, a NULL
 * `constant` or nothing attached INVSIM_EINVAL.  For env n and reorder link k
 * with purchaser p = pur[k], an applied step of period t computes, from the
 * state at the start of the period (no order of this step placed yet; all links
 * from the same state), bit for bit:
 *   pos = X[t][p]                                                     f64
 *   for k' = 0 .. E-1 ascending, if pur[k'] == p:   pos = pos + Y[t][k']
 *   for r  = 0 .. RL-1 ascending, if rl_node[r] == p: pos = pos - U[t][r]
 *   x = levels[n][k] - pos
 *   with reorder: if not (pos < reorder[n][k]) then x = 0   (strict <; a NaN
 *                 reorder point never orders)
 *   x = x > 0 ? x : 0                               (a NaN level orders 0)
 *   x = x > (double)high[k] ? (double)high[k] : x
 *   action[k] = (float)x                            (f64 -> f32, round to nearest even)
 * Plain f64 adds and subtracts in exactly that order (factory yields below 1
 * make X fractional, so the order of the sum shows in the bits).  The step then
 * treats `action` as any caller's action (rint, max(0, .)).  Everything else is
 * CONSTANT's on NetInvMgmt: `actions` records the order of every stepped env, a
 * NEXT_STEP reset step leaves its row unwritten and adds nothing to the metrics
 * (same columns, same += order), SAME_STEP is refused, and the horizon refusal,
 * the episode sink, the capture bracket, both demand streams, every market
 * `dist` and user_D, lock-step and per-env periods and every graph are
 * unchanged.  It runs on the launch paths CONSTANT has: the fused 3-role rollout
 * and the one-wave specialised kernel on the reference's two graphs, the
 * table-walking kernel on any other. */
#define INVSIM_POLICY_NET_LEVELS 8
int invsim_set_policy_net_levels(invsim_handle *h, const double *levels, const double *reorder);

/* Episodic-return statistics of K steps of outputs, the reduction the
 * reference's evaluation harness keeps per episode (episode_rewards ->
 * mean/std, benchmark_InvManagementBacklogEnv.py:389-440).  Handle-free:
 * reward [K][n_envs] f64; terminated / truncated [K][n_envs] u8 (either may be
 * NULL); ret [n_envs] f64 running per-env return (in/out); acc [4] f64 (+=):
 * sum of finished-episode returns, sum of their squares, finished episodes,
 * sum of every reward folded.  Device pointers; the stream's device runs it.
 * invsim.distributed.EpisodeStats all-reduces acc over RCCL. */
int invsim_episode_fold(const double *reward, const uint8_t *terminated, const uint8_t *truncated, int32_t K,
                        int64_t n_envs, double *ret, double *acc, void *stream);

/* The same fold into per-group partials, deterministic (no atomics): part
 * [ceil(n_envs / 64)][4] f64 (+=), row g = [sum of finished-episode returns,
 * sum of their squares, finished episodes, sum of every reward folded] of envs
 * 64 g .. 64 g + 63.  Per env, in row order: ret += reward; at terminated |
 * truncated the return is folded and restarts at 0; each group's per-lane sums
 * over the K rows are then reduced in a fixed order and added to part[g].
 * The statistics are the column sums of part. */
int invsim_episode_fold_groups(const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                               int32_t K, int64_t n_envs, double *ret, double *part, void *stream);

/* Episode sink: the evaluation harness's `episode_reward += reward` per step
 * and its per-episode bookkeeping at done (benchmark_InvManagementBacklogEnv.py:
 * 371, 386, 434), kept on the device inside the step.  With a sink set, every
 * invsim_step / invsim_rollout / invsim_rollout_policy on h folds the rows it
 * produces into ret [N] and part [ceil(N / 64)][4] exactly as
 * invsim_episode_fold_groups over those rows would (same ret and part bits):
 * the lock-step InvMgmt step and rollout kernels in-kernel, other launches by
 * that fold of their outputs on the same stream (reward / terminated /
 * truncated must then be given).  invsim_reset abandons the episodes of the
 * envs it resets, as the harness's `episode_reward = 0.0` at every reset does
 * (:368-371): on the reset's stream their ret restarts at +0.0 (every env, or
 * the masked ones); part is left alone, since nothing finished.  A caller who
 * folds output rows itself with invsim_episode_fold_groups zeroes ret likewise.
 * NULL, NULL detaches.  Not during capture. */
int invsim_set_episode_sink(invsim_handle *h, double *ret, double *part);

/* Debug builds only (make -C csrc ptrs_stats -> invsim/_lib/debug/): PTRS
 * log-acceptance statistics since the last clear, summed over kernels:
 * out[0] log tests, out[1] tests ptrs_log_accept's f32 pre-test left to f64,
 * out[2] bit pattern of the smallest relative margin |lhs - rhs| / (sum of
 * |terms|) (f64), out[3] f32-decided tests that disagree with the f64 test,
 * out[4] log tests the decide path's own f32 test (ptrs_decide_d) left to
 * the exact branch (0 in a branchy build).  out has 5 words.  Synchronises the
 * device.  The product build returns INVSIM_EINVAL.  (No reference
 * equivalent: evidence for the numpy random_poisson_ptrs restatement,
 * distributions.c, SURVEY App. B.) */
int invsim_debug_ptrs_stats(uint64_t *out, int32_t clear);

/* Demand stream of a handle.  INVSIM_DEMAND_NUMPY (default): numpy's PCG64
 * Generator stream and samplers, bit-exact with the reference on the same
 * seeds (newsvendor.py:146, inventory_management.py:172,
 * network_management.py:540).  INVSIM_DEMAND_PHILOX: an opt-in, NON-parity
 * fast stream: rocRAND's Philox4x32-10 used counter-based,
 * key = the env's seeded PCG64 increment (high word), counter = (block, draw
 * stream, handle launch step); the same PTRS / multiplication / binomial /
 * integers / geometric transforms.  No per-env generator state is read or
 * written per step.  Every step / rollout step (and a Newsvendor reset)
 * advances the handle's launch-step counter, which get_state / set_state carry
 * ("philox_step"; the first fast-stream call after set_state reads it back,
 * synchronously).  Switching streams synchronises the device (work queued on
 * any stream finishes first); the PCG64 states are untouched by fast-stream
 * steps.
 *
 * The fast stream, exactly (the CPU oracle restates this text, oracle/oracle.c,
 * and tests/test_gpu_philox_oracle.py holds every kernel to it bit for bit):
 *   block      x = Philox4x32-10(counter (j, r, s_lo, s_hi), key): j the block
 *              index of the draw, r its draw stream, s the 64-bit launch step
 *              (low word counter word 2, high word counter word 3).
 *   key        the env's `rng` row 2 (PCG64 increment, high word) as seeded:
 *              low 32 bits key word 0, high 32 bits key word 1.  A reseed of an
 *              env re-keys it; nothing else does.
 *   outputs    a block gives two 64-bit outputs, (x.y:x.x) then (x.w:x.z); a
 *              uniform double is (output >> 11) * 2**-53.  A draw starts at
 *              block j = 0 of its (s, r) with no output held over, and a
 *              sampler that needs more (a PTRS rejection, a longer product)
 *              continues with the held second output, then j = 1, 2, ...  A
 *              second output left unused by a draw is dropped, never given to
 *              another draw.  The 32-bit half that numpy's integers() buffers
 *              is empty at the start of every launch step (within a Net step
 *              it passes from one integers market to the next, as numpy's
 *              does), and the `u32buf` state field is neither read nor written.
 *   streams    r = 0: the demand of InvMgmt and Newsvendor.  Net: market r of
 *              the step draws from stream r, r its index in retail-link order,
 *              counting the markets that draw nothing (user_D replays and
 *              markets without a demand source) too.  r = 0xffffffff (RESET):
 *              the five uniforms of a Newsvendor reset, in the reference's
 *              order (price, cost, h, k, mu).  dist 5 (user_D) draws nothing.
 *   counter    one per handle, 0 at create and after an unmasked seed
 *              (invsim_seed_range / invsim_seed_words with mask == NULL); a
 *              masked seed keeps it.  Launch step k of a step / rollout /
 *              policy-rollout call of K steps uses s + k for every env, whatever
 *              the env's own period; the call then adds K.  Switching streams
 *              keeps it; steps on the numpy stream do not advance it.
 *   resets     A NEXT_STEP reset step is a launch step like any other: it
 *              consumes its counter value; InvMgmt and Net draw nothing in it,
 *              Newsvendor draws the reset's uniforms from stream RESET at that
 *              value.  A SAME_STEP autoreset happens inside the done step and
 *              has no value of its own: Newsvendor draws the new episode's
 *              uniforms from stream RESET at the done step's value (its demand
 *              came from stream 0 of the same value).  invsim_reset, masked or
 *              not: InvMgmt and Net leave the counter alone; on Newsvendor the
 *              reset envs draw from stream RESET at the current value s and the
 *              handle's counter becomes s + 1 (for every env, also under a mask).
 *   lookahead  a kernel may draw launch step s + 1 while it applies step s;
 *              the draw is the one of (key, s + 1, r) and is discarded when
 *              the counter or a key moves (seed, set_state, reset, a switch).
 *   capture    no two draws of one env ever share a block: (s, r) differs
 *              between any two draws, because every call that draws consumes
 *              the values it uses.  A captured launch would break this (s is a
 *              launch parameter and would repeat on replay), so capture on the
 *              fast stream is refused (INVSIM_EINVAL). */
#define INVSIM_DEMAND_NUMPY 0
#define INVSIM_DEMAND_PHILOX 1
int invsim_set_demand_stream(invsim_handle *h, int32_t mode);
int invsim_demand_stream(const invsim_handle *h, int32_t *mode);

/* Which kernel a handle runs: 0 = the generic kernel of its family, 1 / 2 =
 * NetInvMgmt specialised at compile time for the reference's default /
 * custom supply network (chosen at create when the graph equals one of them). */
int invsim_kernel_variant(const invsim_handle *h, int32_t *variant);

/* Optional per-step demand record (info['demand'] / D): int64 [N][demand_dim],
 * written by every subsequent step/rollout(last step) when non-NULL. */
int invsim_set_info_demand(invsim_handle *h, int64_t *demand);

/* Optional per-step record of the reference's step info (for a single-env
 * view that keeps the reference's history arrays), written by every
 * subsequent step/rollout (last step) when non-NULL:
 *   InvMgmt    int64 [N][2m + 5]:    sales S[t] (m), unfulfilled U[t] (m), then the
 *                                    float64 bit patterns of period_profit, revenue,
 *                                    procurement, holding and penalty cost sums
 *                                    (inventory_management.py:314-345)
 *   NetInvMgmt f64 [N][2 RL + 2 J + 2 E]: S[t, retail links], U[t+1, retail links],
 *                                    X[t+1, main nodes], R[t, reorder links], Y[t+1, reorder
 *                                    links], P[t, main nodes]  (network_management.py:436-619)
 *   Newsvendor f64 [N][5]:          revenue, purchase_cost, holding_cost,
 *                                    lost_sales_penalty (newsvendor.py:149-170, 195-199)
 *                                    and their NumPy-2 kinds packed as
 *                                    k_rev + 4 k_pur + 16 k_hold + 64 k_pen
 *                                    (0 Python float, 1 np.float32, 2 np.float64,
 *                                    3 Python int) */
int invsim_info_record_dim(const invsim_handle *h, int32_t *dim);
int invsim_set_info_record(invsim_handle *h, void *record);

/* Checkpoint / debug: the full device state as one opaque blob of state_bytes,
 * plus a field directory for tests: name, byte offset, element size, rows and
 * row_stride: > 0 rows of row_stride elements ([rows][row_stride]); < 0 a
 * record per env ([-row_stride][rows]); 0 another layout (opaque). */
int invsim_state_bytes(const invsim_handle *h, int64_t *bytes);
int invsim_state_field(const invsim_handle *h, int32_t idx, char name[32], int64_t *offset,
                       int32_t *elem_bytes, int32_t *rows, int64_t *row_stride);
int invsim_get_state(invsim_handle *h, void *dst, void *stream);
int invsim_set_state(invsim_handle *h, const void *src, void *stream);

/* HIP-graph capture of a step loop (SURVEY §7 layer 5; the reference's
 * per-step loop is the caller's `for t: a = agent(obs); env.step(a)`,
 * benchmark_InvManagementBacklogEnv.py:389-440).  The caller records its own
 * stream capture (hipStreamBeginCapture ... hipStreamEndCapture, or
 * torch.cuda.graph) of any mix of its policy launches and invsim_reset /
 * invsim_step / invsim_rollout / invsim_rollout_policy calls on one handle,
 * bracketed by invsim_capture_begin / invsim_capture_end.  Inside the bracket
 * those calls enqueue kernels only; a call that would need a host
 * synchronisation (autoreset DISABLED after a masked reset, get/set_state,
 * status, set_demand_stream) or the fast demand stream (its launch-step
 * counter is a launch parameter and would repeat on replay) fails with
 * INVSIM_EINVAL.  A step call on a capturing stream outside the bracket fails
 * too (the handle's host-side position would drift from the device).
 *
 * The host side of a handle keeps a position (lock-step period, demand
 * lookahead slot) that picks each launch's kernel and parameters.  Nothing
 * runs during capture, so capture_end puts the position back to where
 * capture_begin found it and returns INVSIM_OK only if the captured calls
 * bring it back there (a whole number of episode cycles: periods + 1 steps
 * with NEXT_STEP autoreset, periods with SAME_STEP), so that every replay
 * starts where the graph was recorded; otherwise INVSIM_ERANGE (the graph
 * must not be replayed).  *steps receives the env steps captured.
 * invsim_position returns an opaque token of that position: a graph replays
 * correctly whenever the token equals its value at capture_begin (it does
 * after any number of replays, and after eager calls that close a cycle). */
int invsim_capture_begin(invsim_handle *h);
int invsim_capture_end(invsim_handle *h, int64_t *steps);
int invsim_position(const invsim_handle *h, int64_t *pos);

#ifdef __cplusplus
}
#endif
#endif /* INVSIM_H */
