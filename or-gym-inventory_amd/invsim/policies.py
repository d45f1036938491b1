"""Device-side heuristic agents and batched ``evaluate_agent``.

The reference's benchmark scripts drive one env per episode from Python:
``agent.get_action(obs, env)`` then ``env.step``, accumulating per-episode sums
(``evaluate_agent``).  Here the agent runs inside the step kernel
(``invsim_rollout_policy``): N episodes advance together with no host round
trip, and the per-env sums come back as one array.

Agents (restated from the reference, same names and constructor arguments):

* ``BaseStockAgent(safety_factor)``        benchmark_InvManagementBacklogEnv.py:142-198
  (and benchmark_InvManagementLostSalesEnv.py:137-165), InvMgmt envs
* ``ConstantOrderAgent(order_fraction)``   benchmark_NetInvMgmtBacklogEnv.py:119-135
  (and benchmark_NetInvMgmtLostSalesEnv.py:131-142), any env
* ``OrderUpToHeuristicAgent(safety_factor)`` benchmark_newsvendor.py:97-111, Newsvendor
* ``ClassicNewsvendorAgent(cr_method, safety_factor)`` benchmark_newsvendor.py:113-161,
  Newsvendor (scipy ``poisson.ppf`` restated on device, float32 loops included)
* ``sSPolicyAgent(s_quantile, S_buffer_factor)`` benchmark_newsvendor_sb3_rllib.py:363-371,
  Newsvendor (the module's last definition; ``s_quantile`` is unused there too)
* ``RandomAgent(seed)`` the ``RandomAgent`` every benchmark script's agent list
  starts with (``env.action_space.sample()`` every step), any env and any graph.
  The reference never seeds ``action_space``, so there is no trajectory to
  match: the actions are numpy's ``Generator.uniform`` on a per-env PCG64
  stream of their own (``include/invsim.h``, "RandomAgent")

* ``LevelsAgent(levels, reorder)`` BaseStock's rule with the order-up-to level
  (and optionally the reorder point) of every env and stage read from a device
  tensor, InvMgmt envs: one launch scores ``num_envs`` level vectors.
  ``evaluate_levels`` scores ``[C, A]`` candidates on common seeds in one
  launch and ``tune_levels`` searches them (``include/invsim.h``, "Per-env
  base-stock levels")
* ``NetLevelsAgent(levels, reorder)`` the same on a supply network: every
  reorder link orders up to its own per-env level against its purchaser's
  inventory position, NetInvMgmt envs and any graph; ``from_mean_demand``
  derives levels from the topology, and ``evaluate_levels`` / ``tune_levels``
  take NetInvMgmt env classes too (``include/invsim.h``, "Per-env order-up-to
  levels on a supply network")

Policies computed outside the kernels (a trained ``torch.nn.Module`` actor, the
scripts' ``SB3AgentWrapper``: benchmark_InvManagementBacklogEnv.py:332-342) go
through ``TorchPolicyAgent(fn)``: the network runs in torch on the env's device
and stream between one-step ``invsim_rollout_metrics`` launches, which keep the
same per-env sums for the actions they are handed, so ``rollout_policy`` and
``evaluate_agent`` take the agent like any other; ``convert_actions`` is the
wrapper's post-processing of the network's output.  A plain feed-forward actor
(Linear / ReLU / Tanh, at most 5 layers of at most 256 units) can instead be
handed to the library as an ``MLPPolicyAgent``: the network is then a HIP
kernel of its own and the closed loop is issued in C (``invsim_rollout_mlp``),
two launches per step with no Python between them.  A
``GaussianMLPPolicyAgent`` is that actor with a diagonal Gaussian around it,
sampled in the same kernel: ``collect_rollout`` returns what an on-policy
learner (the scripts' SB3 ``PPO`` / ``A2C``) stores per step, log-probabilities
included.  With ``critic=ValueMLP(...)`` it also evaluates the value network in
the same kernel's arithmetic and computes the advantages in one launch (``gae``;
truncation bootstraps from the final observation, NEXT_STEP reset rows are
masked), and ``update_from_module`` writes the optimiser's new weights into the
device copies on the stream (``include/invsim.h``, "Critic, GAE and parameter
updates").

``evaluate_agent(agent, env_cls, env_config, n_episodes, seed_offset)`` returns
the reference's summary columns (benchmark_InvManagementBacklogEnv.py:346-440,
benchmark_NetInvMgmtLostSalesEnv.py:241-312, benchmark_newsvendor.py:219-262):
episode i is env i seeded ``seed_offset + i``.
"""
import ctypes as C
import os
import time
import weakref

import numpy as np
import torch

from . import _capi


class _Agent:
    kind = None
    name = "agent"

    def device_spec(self, env):
        """(PolicySpec, keep-alive) for invsim_rollout_policy."""
        raise NotImplementedError


class BaseStockAgent(_Agent):
    """Independent base-stock level (L_i + 1) * mu * safety_factor per stage."""

    def __init__(self, safety_factor=1.0):
        self.name = f"BaseStock_SF={safety_factor:.1f}"
        self.safety_factor = safety_factor

    def device_spec(self, env):
        if env.family != _capi.INVSIM_INVMGMT:
            raise TypeError("BaseStockAgent needs an InvManagement env")
        mu = env.dist_param.get("mu", 10)       # the agent's own default (:156)
        return _capi.PolicySpec(_capi.POLICY_KINDS["base_stock"], 0, float(self.safety_factor), float(mu), None), None


class ConstantOrderAgent(_Agent):
    """order_fraction * action_space.high every step (inf bounds -> 1000)."""

    def __init__(self, order_fraction=0.1):
        self.name = f"ConstantOrder_{order_fraction * 100:.0f}%"
        self.order_fraction = order_fraction

    def action(self, env):
        sp = env.single_action_space
        high = np.array(sp.high, copy=True)
        high[high == np.inf] = 1000
        return (high * self.order_fraction).astype(sp.dtype)

    def device_spec(self, env):
        a = np.ascontiguousarray(self.action(env))
        return _capi.PolicySpec(_capi.POLICY_KINDS["constant"], 0, 0.0, 0.0, a.ctypes.data), a


class OrderUpToHeuristicAgent(_Agent):
    """Order up to mu * (lead_time + 1) * safety_factor over the pipeline."""

    def __init__(self, safety_factor=1.0):
        self.name = f"OrderUpTo_SF={safety_factor:.1f}"
        self.safety_factor = safety_factor

    def device_spec(self, env):
        if env.family != _capi.INVSIM_NEWSVENDOR:
            raise TypeError("OrderUpToHeuristicAgent needs a Newsvendor env")
        return _capi.PolicySpec(_capi.POLICY_KINDS["order_up_to"], 0, float(self.safety_factor), 0.0, None), None


class ClassicNewsvendorAgent(_Agent):
    """Order up to poisson.ppf(critical ratio, mu * (lead_time + 1) * sf) over
    the pipeline; cr_method 'k_vs_h' (k / (h + k), also any unknown method) or
    'profit_margin' ((p - c + k) / (p - c + k + h)), falling back to OrderUpTo
    without the safety factor when the ratio is undefined."""

    def __init__(self, cr_method="k_vs_h", safety_factor=1.0):
        self.name = f"ClassicNV_SF={safety_factor:.1f}_{cr_method}"
        self.cr_method = cr_method
        self.safety_factor = safety_factor

    def device_spec(self, env):
        if env.family != _capi.INVSIM_NEWSVENDOR:
            raise TypeError("ClassicNewsvendorAgent needs a Newsvendor env")
        variant = 1 if self.cr_method == "profit_margin" else 0
        return _capi.PolicySpec(_capi.POLICY_KINDS["classic_nv"], variant, float(self.safety_factor), 0.0,
                                None), None


class sSPolicyAgent(_Agent):
    """(s, S): s = poisson.ppf(clip(k / (h + k), 0.001, 0.999), mu * (lead_time + 1)),
    S = s * S_buffer_factor; order S - position when the position is below s."""

    def __init__(self, s_quantile=0.5, S_buffer_factor=1.2):
        self.name = f"sS_Policy(s={s_quantile:.2f},S={S_buffer_factor:.1f}s)"
        self.s_quantile = s_quantile
        self.S_buffer_factor = S_buffer_factor

    def device_spec(self, env):
        if env.family != _capi.INVSIM_NEWSVENDOR:
            raise TypeError("sSPolicyAgent needs a Newsvendor env")
        return _capi.PolicySpec(_capi.POLICY_KINDS["ss"], 0, float(self.S_buffer_factor), 0.0, None), None


def _require_agreed_seed(seed, world):
    """RandomAgent(seed=None) draws its base from OS entropy, which the ranks of
    a distributed job would each draw differently: refuse before any collective."""
    if seed is None and world > 1:
        raise ValueError("RandomAgent(seed=None) under torch.distributed with more than one rank: every rank "
                         "must use the same seed, pass one explicitly")


class RandomAgent(_Agent):
    """Uniform random actions over the env's action space, drawn in the step
    kernel: env with global index g draws from
    ``Generator(PCG64(SeedSequence(2**64 + seed + g)))``, ``action_dim`` doubles
    per step (``uniform(0, high)`` for float32 spaces, ``floor(uniform(0, high +
    1))`` for int64 ones).  The first time the agent meets an env it seeds the
    env's action generators (``env.seed_actions(seed)``) and remembers that
    buffer; later launches on that env continue it, so 5 steps then 7 equal 12.
    If something else has attached other generators to the env since (another
    agent, ``env.seed_actions``, ``env.set_action_rng_state``), the agent puts
    its own buffer back first, so its stream on an env is always its own; to
    continue from a restored checkpoint, sample with ``env.sample_actions``.
    The first meeting launches the seeding kernel: under ``env.capture`` let
    the agent meet the env (or call ``device_spec``) before the capture."""

    name = "Random"

    def __init__(self, seed=None):
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        _require_agreed_seed(seed, world)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little") >> 1      # 63 bits of OS entropy
        self.seed = int(seed)
        self._bufs = weakref.WeakKeyDictionary()       # env -> the generators this agent seeded for it

    def device_spec(self, env):
        buf = self._bufs.get(env)
        if buf is None:
            env.seed_actions(self.seed)
            self._bufs[env] = env._arng
        elif env._arng is not buf:
            env._attach_action_rng(buf)
        high = env._action_high()
        return _capi.PolicySpec(_capi.POLICY_KINDS["random"], 0, 0.0, 0.0, high.ctypes.data), high


class LevelsAgent(_Agent):
    """Order up to a level of the env's own, per stage: BaseStockAgent's rule
    (order ``level - inventory position``, clipped to ``[0, c]``) with ``levels``
    in place of ``(L + 1) * mu * safety_factor``, and with ``reorder`` only
    while the position is strictly below the reorder point (an (s, S) policy).
    ``levels`` / ``reorder``: array-likes or tensors ``[A]`` (every env alike) or
    ``[N, A]`` (env n's own row), held as contiguous float64 tensors on the
    env's device and attached to it for the launch
    (``invsim_set_policy_levels``).  A tensor is used in place exactly when it is
    float64, ``[N, A]``, contiguous and on the env's GPU: the kernels read it when
    they run, so in-place updates (also between replays of a captured graph) are
    seen by the next launch.  Anything else (another dtype, shape ``[A]``, a
    non-contiguous view, the host, another GPU) is copied once, when the agent
    first meets the env, and later changes to the original are not seen;
    ``agent.tensors(env)`` returns the pair the kernels read, whichever it is.
    Under ``env.capture`` let the agent meet the env (``device_spec``) before the
    capture: attaching is refused inside one.  A captured graph holds the
    addresses of the tensors attached when it was recorded; the ``StepGraph``
    keeps those tensors alive, and replaying it reads them whichever agent is
    attached by then."""

    def __init__(self, levels, reorder=None, name="Levels"):
        self.levels = levels
        self.reorder = reorder
        self.name = name
        self._bufs = weakref.WeakKeyDictionary()       # env -> (levels, reorder) on its device

    @classmethod
    def from_safety_factor(cls, env, sf, **kw):
        """The levels BaseStockAgent(sf) orders up to on ``env``, ``(lead_time +
        1) * mu * sf`` evaluated in numpy in that order with the agent's own
        ``mu`` default; ``sf`` a scalar, ``[N]`` or ``[N, A]``.  With a scalar the
        rollouts equal BaseStockAgent's bit for bit."""
        mu = env.dist_param.get("mu", 10)
        sf = np.asarray(sf, np.float64)
        if sf.ndim == 1:
            sf = sf[:, None]
        return cls((env.lead_time + 1) * mu * sf, **kw)

    def _on_device(self, env, a, what):
        N, A = env.num_envs, env.action_dim
        if (type(a) is torch.Tensor and a.dtype == torch.float64 and a.is_cuda
                and a.get_device() == env.device_index     # the resolved index: "cuda" without one is the current device
                and a.is_contiguous() and tuple(a.shape) == (N, A)):
            return a                                   # in place
        t = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64))
        if tuple(t.shape) == (A,):
            t = t.expand(N, A)
        if tuple(t.shape) != (N, A):
            raise ValueError(f"{what} must have shape {(A,)} or {(N, A)}, got {tuple(t.shape)}")
        return t.contiguous().to(env.device)

    def tensors(self, env):
        """(levels, reorder or None): the float64 ``[N, A]`` device tensors the
        kernels read for this agent on ``env`` (made at the first call)."""
        if env.family != _capi.INVSIM_INVMGMT:
            raise TypeError("LevelsAgent needs an InvManagement env")
        bufs = self._bufs.get(env)
        if bufs is None:
            bufs = (self._on_device(env, self.levels, "levels"),
                    None if self.reorder is None else self._on_device(env, self.reorder, "reorder"))
            self._bufs[env] = bufs
        return bufs

    def device_spec(self, env):
        bufs = self.tensors(env)
        env._attach_policy_levels(*bufs)               # (kept alive by the env while attached)
        return _capi.PolicySpec(_capi.POLICY_KINDS["levels"], 0, 0.0, 0.0, None), bufs


def _market_means(tp):
    """Mean demand per period of every market link of a compiled topology:
    poisson lam, binomial n p, integers the mean of numpy's half-open range,
    geometric 1 / p, a user_D replay the mean of max(0, round(x))."""
    t = tp.tables
    out = np.zeros(len(tp.retail_links), np.float64)
    for r in range(len(tp.retail_links)):
        if t["rl_user"][r]:
            out[r] = float(np.mean(np.maximum(0.0, np.rint(t["user_D"][r]))))
            continue
        kind = int(t["rl_dist"][r])
        if kind == 1:
            out[r] = float(t["rl_lam"][r])
        elif kind == 2:
            out[r] = float(t["rl_n"][r]) * float(t["rl_dp"][r])
        elif kind == 3:
            out[r] = (float(t["rl_n"][r]) + float(t["rl_high"][r]) - 1.0) / 2.0
        else:
            out[r] = 1.0 / float(t["rl_dp"][r])
    return out


class NetLevelsAgent(LevelsAgent):
    """Installation base-stock on a supply network (NetInvMgmt envs, any graph):
    every reorder link ``k`` orders up to ``levels[n][k]`` against the inventory
    position of the node that buys over it -- its on-hand ``X``, plus the
    pipelines ``Y`` of every link into it, minus the backlog ``U`` of its
    markets -- clipped to ``[0, action_space.high]``, and with ``reorder`` only
    while that position is strictly below the link's reorder point
    (``include/invsim.h``, "Per-env order-up-to levels on a supply network").
    The tensors, what is used in place, captures and keep-alive are
    ``LevelsAgent``'s; the kernels are the NetInvMgmt ones."""

    def __init__(self, levels, reorder=None, name="NetLevels"):
        super().__init__(levels, reorder, name)

    @classmethod
    def from_mean_demand(cls, env_or_topology, safety_factor=1.0, **kw):
        """Levels that cover the mean demand over each link's lead time plus the
        review period, ``safety_factor * (L_k + 1) * f[k]``, from the compiled
        topology alone (host only).  ``d[j]``, the demand rate at node ``j``, is
        the mean demand of its markets plus ``f[k] / v[j]`` over the links ``j``
        supplies; a node splits its rate evenly over the links into it, ``f[k] =
        d[pur[k]] / (links into pur[k])``; evaluated from the markets upstream."""
        tp = getattr(env_or_topology, "topology", env_or_topology)
        t = tp.tables
        E, J = len(tp.reorder_links), len(tp.main_nodes)
        pur, sup = t["pur"][:E], t["sup"][:E]
        mkt = _market_means(tp)
        n_in = np.bincount(pur, minlength=J)
        d, f = [None] * J, [None] * E
        busy = set()

        def rate(j):
            if d[j] is None:
                if j in busy:
                    raise ValueError("from_mean_demand needs an acyclic supply network")
                busy.add(j)
                x = 0.0
                for r in range(len(tp.retail_links)):
                    if t["rl_node"][r] == j:
                        x += mkt[r]
                for k in range(E):
                    if sup[k] == j:
                        x += flow(k) / float(t["v"][j])
                busy.discard(j)
                d[j] = x
            return d[j]

        def flow(k):
            if f[k] is None:
                f[k] = rate(int(pur[k])) / float(n_in[pur[k]])
            return f[k]

        lv = np.array([safety_factor * (float(t["L"][k]) + 1.0) * flow(k) for k in range(E)], np.float64)
        return cls(lv, **kw)

    def tensors(self, env):
        """(levels, reorder or None): the float64 ``[N, A]`` device tensors the
        kernels read for this agent on ``env`` (made at the first call)."""
        if env.family != _capi.INVSIM_NETINVMGMT:
            raise TypeError("NetLevelsAgent needs a NetInvMgmt env")
        bufs = self._bufs.get(env)
        if bufs is None:
            bufs = (self._on_device(env, self.levels, "levels"),
                    None if self.reorder is None else self._on_device(env, self.reorder, "reorder"))
            self._bufs[env] = bufs
        return bufs

    def device_spec(self, env):
        bufs = self.tensors(env)
        env._attach_policy_levels(*bufs)               # (kept alive by the env while attached)
        high = env._action_high()
        return _capi.PolicySpec(_capi.POLICY_KINDS["net_levels"], 0, 0.0, 0.0, high.ctypes.data), (bufs, high)


def convert_actions(raw, low, high, dtype):
    """What the reference's ``SB3AgentWrapper.get_action`` does to a network's
    output, on torch tensors: ``np.clip(raw, low, high)`` (SB3 ``predict`` clips
    the actions of unsquashed policies to the Box bounds; an infinite bound
    leaves the value alone) and then ``.astype(action_space.dtype)``, which for
    int64 spaces truncates toward zero.  ``raw`` [..., A] float tensor;
    ``low`` / ``high`` [A] (tensors or arrays, the space's bounds); ``dtype``
    torch.int64 or torch.float32.

    NaN: numpy leaves ``nan.astype(int64)`` undefined, so for int64 spaces a NaN
    maps to 0 (no order); for float spaces a NaN passes through unchanged, as
    ``np.clip`` passes it, and the env's dynamics see it.  Signed zero: a -0.0
    clipped at a bound of 0 gives +0.0, the bound."""
    lo = torch.as_tensor(low, device=raw.device)
    hi = torch.as_tensor(high, device=raw.device)
    if dtype == torch.int64:
        # numpy promotes float32 values with int64 bounds to float64: clip there
        x = torch.clamp(raw.to(torch.float64), lo.to(torch.float64), hi.to(torch.float64))
        x = torch.where(x != x, torch.zeros_like(x), x)
        return x.to(torch.int64)                    # truncation toward zero
    # promotes as np.clip does; NaN and a value at an infinite bound pass.  A value
    # equal to a bound becomes the bound, so -0.0 at a bound of 0 is +0.0 (numpy's
    # own result for that one input depends on the code path it takes)
    nan = raw != raw
    x = torch.where((raw > lo) | nan, raw, lo)
    return torch.where((x < hi) | nan, x, hi).to(dtype)


class TorchPolicyAgent(_Agent):
    """A policy computed in torch, outside the kernels: ``fn`` is any callable
    (an ``nn.Module`` actor, a lambda around one) on the env's device.  Every
    step it receives the observations as float32 ``[N, O]`` (the scripts'
    ``observation.astype(np.float32)``) and returns raw actions ``[N, A]``,
    which ``convert_actions`` clips to the action space and casts to its dtype
    (``clip=False``: cast only; the caller answers for the range).  It runs
    under ``torch.no_grad()`` on the env's current stream, so a rollout is one
    stream of launches with no host round trip.

    A squashed (tanh) actor, SAC's, is unscaled by the caller in ``fn``:
    ``lambda o: low + 0.5 * (actor(o) + 1.0) * (high - low)``."""

    def __init__(self, fn, name="TorchPolicy", clip=True):
        if not callable(fn):
            raise TypeError("TorchPolicyAgent needs a callable (obs [N, O] float32 -> actions [N, A])")
        self.fn = fn
        self.name = name
        self.clip = bool(clip)

    def device_spec(self, env):
        raise TypeError("TorchPolicyAgent runs outside the kernels: use rollout_policy / evaluate_agent")


def _rollout_torch(env, agent, K, obs, rewards, actions, metrics, obs0):
    """The closed loop of a TorchPolicyAgent: fn -> convert_actions -> one
    invsim_rollout_metrics step, K times on the env's stream, every step
    writing row k of the preallocated outputs."""
    if obs0 is None:
        raise ValueError("a TorchPolicyAgent rollout needs obs0, the observation the env last returned "
                         "(reset()'s, or the last row of the previous rollout's obs)")
    N, dev, A = env.num_envs, env.device, env.action_dim
    obs0 = torch.as_tensor(obs0, device=dev)
    if tuple(obs0.shape) != (N, env.obs_dim):
        raise ValueError(f"obs0 must have shape {(N, env.obs_dim)}, got {tuple(obs0.shape)}")
    metrics = env._metrics_arg(metrics)
    sp = env.single_action_space
    low = torch.as_tensor(np.asarray(sp.low).reshape(-1), device=dev)
    high = torch.as_tensor(np.asarray(sp.high).reshape(-1), device=dev)
    out = {}
    # without obs the loop keeps only the last row: fn has read it (stream order) when the step overwrites it
    o = torch.empty((K if obs else 1, N, env.obs_dim), dtype=env.obs_dtype, device=dev)
    if rewards:
        out["reward"] = torch.empty((K, N), dtype=torch.float64, device=dev)
        out["terminated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
        out["truncated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
    a_all = torch.empty((K, N, A), dtype=env.act_dtype, device=dev) if actions else None
    rew, term, trunc = out.get("reward"), out.get("terminated"), out.get("truncated")
    cur = obs0
    with torch.no_grad():
        for k in range(K):
            raw = agent.fn(cur.to(torch.float32))
            a = convert_actions(raw, low, high, env.act_dtype) if agent.clip else raw.to(env.act_dtype)
            if a.numel() != N * A:
                raise ValueError(f"the policy must return actions of shape {(N, A)}, got {tuple(raw.shape)}")
            a = a.reshape(N, A)
            if a_all is not None:
                a_all[k].copy_(a)
                a = a_all[k]
            elif not a.is_contiguous():
                a = a.contiguous()
            ok = o[k if obs else 0]
            env._rollout_metrics(1, a, ok, rew[k] if rewards else None, term[k] if rewards else None,
                                 trunc[k] if rewards else None, metrics)
            cur = ok
    if obs:
        out["obs"] = o
    if actions:
        out["actions"] = a_all
    return out


def _f32(a, shape, what):
    """a parameter as a contiguous float32 host array of the given shape"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {a.shape}")
    return a


class MLPPolicyAgent(_Agent):
    """A trained feed-forward actor evaluated by the library itself: one HIP
    kernel per step takes the observations to actions, and the closed loop
    (network, env step, network, ...) is issued in C on the env's stream
    (``invsim_rollout_mlp``), two launches per step with no Python in between.
    The arithmetic is defined op by op in ``include/invsim.h`` ("MLP actor"):
    float32 ``fmaf`` chains in ascending input order, so a ReLU or linear
    network is reproducible bit for bit on a CPU (``tests/mlp_model.py``); a
    tanh network is defined up to the device's ``tanhf``.

    ``layers``: a list of ``(weight, bias)`` pairs, ``weight`` ``[out, in]`` as
    ``torch.nn.Linear.weight``, ``bias`` ``[out]`` or ``None``; at most 5 linear
    layers, hidden widths at most 256 (wider actors: ``TorchPolicyAgent``).
    ``activation`` ("relu" / "tanh") follows every layer but the last,
    ``out_activation`` (``None`` / "tanh") the last.  ``in_scale`` / ``in_shift``
    ``[obs_dim]`` normalise the observations (``x * scale + shift``, fused);
    ``out_scale`` / ``out_shift`` ``[action_dim]`` rescale the outputs, e.g. a
    squashed actor's ``low + 0.5 * (tanh + 1) * (high - low)`` is ``out_scale =
    0.5 * (high - low)``, ``out_shift = low + out_scale``.  The result goes
    through ``convert_actions`` (``clip=False``: cast only).

    ``rollout_policy`` / ``evaluate_agent`` take it like a ``TorchPolicyAgent``
    (``obs0`` required, the same returned dict); ``env.mlp_actions(agent, obs)``
    is the single launch.  The device copy is built once per env and freed
    with it."""

    def __init__(self, layers, activation="tanh", out_activation=None, in_scale=None, in_shift=None,
                 out_scale=None, out_shift=None, clip=True, name="MLP"):
        layers = list(layers)
        if not 1 <= len(layers) <= _capi.MLP_MAX_LAYERS:
            raise ValueError(f"an MLPPolicyAgent has 1..{_capi.MLP_MAX_LAYERS} linear layers, got {len(layers)}")
        if activation not in ("relu", "tanh"):
            raise ValueError("activation must be 'relu' or 'tanh'")
        if out_activation not in (None, "none", "tanh"):
            raise ValueError("out_activation must be None or 'tanh'")
        if (in_scale is None) != (in_shift is None) or (out_scale is None) != (out_shift is None):
            raise ValueError("scale and shift are given in pairs")
        self.weights, self.biases = [], []
        for l, (w, b) in enumerate(layers):
            w = _f32(w, None, "weight")
            if w.ndim != 2 or 0 in w.shape:
                raise ValueError(f"layer {l}: weight must be [out, in], got {w.shape}")
            if self.weights and w.shape[1] != self.weights[-1].shape[0]:
                raise ValueError(f"layer {l}: weight {w.shape} does not take the {self.weights[-1].shape[0]} outputs "
                                 "of the layer before")
            self.weights.append(w)
            self.biases.append(None if b is None else _f32(b, (w.shape[0],), f"layer {l}: bias"))
        self.dims = [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]
        if any(d > _capi.MLP_MAX_WIDTH for d in self.dims[1:-1]):
            raise ValueError(f"hidden widths are at most {_capi.MLP_MAX_WIDTH}, got {self.dims[1:-1]} "
                             "(a wider actor runs through TorchPolicyAgent)")
        O, A = self.dims[0], self.dims[-1]
        self.in_scale = None if in_scale is None else _f32(in_scale, (O,), "in_scale")
        self.in_shift = None if in_shift is None else _f32(in_shift, (O,), "in_shift")
        self.out_scale = None if out_scale is None else _f32(out_scale, (A,), "out_scale")
        self.out_shift = None if out_shift is None else _f32(out_shift, (A,), "out_shift")
        self.activation = activation
        self.out_activation = None if out_activation in (None, "none") else out_activation
        self.clip = bool(clip)
        self.name = name
        self._objs = weakref.WeakKeyDictionary()      # env -> (its handle, the invsim_mlp built for it)
        self._live = None         # update_from_module: the device tensors the last update reads
        self._updated = False     # the device copies no longer hold this object's host arrays

    _value = False                # ValueMLP: one output unit, invsim_mlp_create_value

    @classmethod
    def _walk(cls, module):
        """(layers, hidden activation, output activation) of an ``nn.Sequential``
        of ``Linear`` / ``ReLU`` / ``Tanh``; TypeError for anything else."""
        nn = torch.nn
        if not isinstance(module, nn.Sequential):
            raise TypeError("from_module takes an nn.Sequential of Linear / ReLU / Tanh")
        layers, acts = [], []         # acts[i]: the activation after linear layer i, or None
        for m in module:
            if isinstance(m, nn.Linear):
                if len(acts) < len(layers):
                    raise TypeError("two Linear layers without an activation between them")
                layers.append((m.weight, m.bias))
            elif isinstance(m, (nn.ReLU, nn.Tanh)):
                if len(acts) >= len(layers):
                    raise TypeError("an activation must follow a Linear layer")
                acts.append("relu" if isinstance(m, nn.ReLU) else "tanh")
            else:
                raise TypeError(f"from_module: unsupported module {type(m).__name__} (Linear, ReLU and Tanh only)")
        if not layers:
            raise TypeError("from_module: no Linear layer")
        out_act = acts.pop() if len(acts) == len(layers) else None
        if out_act == "relu":
            raise TypeError("from_module: the output activation is none or Tanh")
        if len(set(acts)) > 1:
            raise TypeError("from_module: mixed hidden activations (one kind per network)")
        return layers, acts[0] if acts else "tanh", out_act

    @classmethod
    def from_module(cls, module, **kw):
        """From an ``nn.Sequential`` of ``Linear`` / ``ReLU`` / ``Tanh`` (SB3's
        ``mlp_extractor.policy_net`` followed by ``action_net``, flattened into
        one Sequential): a Linear, then activation and Linear alternating, an
        optional activation at the end (which must be Tanh).  The parameters are
        copied as float32.  Anything else, or two different hidden activations,
        is a TypeError.  Other arguments go to the constructor."""
        layers, act, out_act = cls._walk(module)
        if "activation" in kw or "out_activation" in kw:
            raise TypeError("from_module reads the activations from the module")
        return cls(layers, activation=act, out_activation=out_act, **kw)

    def device_spec(self, env):
        raise TypeError("MLPPolicyAgent runs in its own kernel: use rollout_policy / evaluate_agent / env.mlp_actions")

    def device_object(self, env):
        """The ``invsim_mlp`` of this network on ``env`` (built at the first call;
        synchronises then: under ``env.capture`` let the agent meet the env first)."""
        hit = self._objs.get(env)
        if hit is not None and hit[0] is env._h:
            return hit[1]
        if self._updated:
            raise RuntimeError(f"{self.name}: update_from_module / set_input_norm has replaced the parameters on the "
                               "env it was called with, and this object's host arrays are the old ones: build a new "
                               "agent from the module for another env")
        out_dim = 1 if self._value else env.action_dim
        if self.dims[0] != env.obs_dim or self.dims[-1] != out_dim:
            raise ValueError(f"the network maps {self.dims[0]} -> {self.dims[-1]}, the env needs "
                             f"{env.obs_dim} -> {out_dim}")
        n = len(self.weights)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        dims = np.asarray(self.dims, np.int32)
        W = (C.c_void_p * n)(*[w.ctypes.data for w in self.weights])
        B = (C.c_void_p * n)(*[ptr(b) for b in self.biases])
        sp = env.single_action_space
        low = np.ascontiguousarray(np.asarray(sp.low, dtype=sp.dtype).reshape(-1))
        high = np.ascontiguousarray(np.asarray(sp.high, dtype=sp.dtype).reshape(-1))
        spec = _capi.MLPSpec(n, _capi.MLP_ACTIVATIONS[self.activation], _capi.MLP_ACTIVATIONS[self.out_activation],
                             int(self.clip), dims.ctypes.data, C.cast(W, C.c_void_p), C.cast(B, C.c_void_p),
                             ptr(self.in_scale), ptr(self.in_shift), ptr(self.out_scale), ptr(self.out_shift),
                             low.ctypes.data, high.ctypes.data)
        obj = C.c_void_p()
        create = env._lib.invsim_mlp_create_value if self._value else env._lib.invsim_mlp_create
        _capi.check(create(env._h, C.byref(spec), C.byref(obj)), env._h, "mlp_create")
        env._mlps.append(obj)            # the env destroys it in close(), before its handle
        self._objs[env] = (env._h, obj)
        return obj

    def _module_params(self, module):
        """The (weight, bias) parameters of ``module``'s Linear layers, checked
        against this network's ``dims`` (ValueError) before anything else happens."""
        lin = [m for m in module.modules() if isinstance(m, torch.nn.Linear)]
        if len(lin) != len(self.dims) - 1:
            raise ValueError(f"{self.name}: the module has {len(lin)} Linear layers, the network {len(self.dims) - 1}")
        for l, m in enumerate(lin):
            if tuple(m.weight.shape) != (self.dims[l + 1], self.dims[l]):
                raise ValueError(f"{self.name}: layer {l} is {tuple(m.weight.shape)} in the module, "
                                 f"{(self.dims[l + 1], self.dims[l])} in the network")
        return [(m.weight, m.bias) for m in lin]

    def update_from_module(self, env, module, log_std=None):
        """Write ``module``'s current parameters into this network's device copy
        on ``env``: one small launch on the env's stream (``invsim_mlp_update``),
        no allocation by the library, no host copy, no synchronisation, legal
        under ``env.capture`` (a replay re-reads the tensors, so a captured
        iteration picks up the optimiser's weights).  The module's Linear layers
        must have this network's shapes (ValueError); float32 contiguous
        parameters on ``env.device`` are read in place, others are copied there
        first; a layer without a bias keeps the bias the object has.  A
        ``GaussianMLPPolicyAgent`` takes ``log_std`` too (``exp`` runs in torch,
        float32).  The tensors passed stay referenced until the next update.
        The host arrays of this object are NOT refreshed: afterwards it serves
        ``env`` only, and meeting another env raises."""
        params = self._module_params(module)
        if log_std is not None and (self._value or not hasattr(self, "log_std")):
            raise TypeError(f"{type(self).__name__} has no Gaussian: log_std goes with a GaussianMLPPolicyAgent")
        if log_std is not None and tuple(log_std.shape) != (self.dims[-1],):
            raise ValueError(f"log_std must have shape {(self.dims[-1],)}, got {tuple(log_std.shape)}")
        obj = self.device_object(env)

        def on_device(t):
            t = t.detach()
            if t.dtype == torch.float32 and t.is_contiguous() and t.device == env.device:
                return t
            return t.to(device=env.device, dtype=torch.float32).contiguous()
        ws = [on_device(w) for w, _ in params]
        bs = [None if b is None else on_device(b) for _, b in params]
        ls = None if log_std is None else on_device(log_std)
        sd = None if ls is None else ls.exp()
        n = len(ws)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        W = (C.c_void_p * n)(*[p(w) for w in ws])
        B = (C.c_void_p * n)(*[p(b) for b in bs])
        _capi.check(env._lib.invsim_mlp_update(env._h, obj, C.cast(W, C.c_void_p), C.cast(B, C.c_void_p), p(sd), p(ls),
                                               env._stream()), env._h, "mlp_update")
        self._live = (ws, bs, sd, ls)
        self._updated = True

    def set_input_norm(self, env, scale, shift):
        """Write new ``in_scale`` / ``in_shift`` rows into this network's device
        copy on ``env`` from device tensors (``invsim_mlp_set_input_norm``): one
        small launch on the env's stream, no allocation, no synchronisation,
        legal under ``env.capture``.  ``scale`` / ``shift``: float32 contiguous
        ``[obs_dim]`` tensors (``RunningMoments.scale_shift``'s); anything else is
        a TypeError / ValueError before any library call, as is a network built
        without ``in_scale`` (it has no such rows: give it any pair at
        construction, e.g. ones and zeros).  The tensors stay referenced until
        the next call.  As after ``update_from_module``, this object's host
        arrays are not refreshed: afterwards it serves ``env`` only."""
        if self.in_scale is None:
            raise ValueError(f"{self.name}: built without in_scale / in_shift, so its device copy has no input rows to "
                             "write; construct it with a pair (ones and zeros leave the input as it is)")
        O = self.dims[0]
        for t, what in ((scale, "scale"), (shift, "shift")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what} must be a torch tensor on the env's device, got {type(t).__name__}")
            if t.dtype != torch.float32:
                raise TypeError(f"{what} must be float32, got {t.dtype}")
            if tuple(t.shape) != (O,) or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {(O,)}, got {tuple(t.shape)}")
        if scale.device != env.device or shift.device != env.device:
            raise ValueError(f"scale / shift must be on {env.device}")
        obj = self.device_object(env)
        _capi.check(env._lib.invsim_mlp_set_input_norm(env._h, obj, scale.data_ptr(), shift.data_ptr(), env._stream()),
                    env._h, "mlp_set_input_norm")
        self._live_norm = (scale, shift)
        self._updated = True


class ValueMLP(MLPPolicyAgent):
    """A critic evaluated by the library: the ``MLPPolicyAgent`` network with
    one output unit and no action conversion, under the same arithmetic
    contract (``include/invsim.h``, "Critic, GAE and parameter updates").
    ``env.mlp_values(critic, obs)`` is the launch, over any number of obs rows;
    ``collect_rollout(..., critic=...)`` evaluates it over the collected rows
    and feeds ``gae``.  ``out_scale`` / ``out_shift`` ``[1]`` de-normalise the
    value.  A last width other than 1 is a ValueError."""

    _value = True

    def __init__(self, layers, activation="tanh", in_scale=None, in_shift=None, out_scale=None, out_shift=None,
                 name="Value"):
        super().__init__(layers, activation=activation, out_activation=None, in_scale=in_scale, in_shift=in_shift,
                         out_scale=out_scale, out_shift=out_shift, clip=False, name=name)
        if self.dims[-1] != 1:
            raise ValueError(f"a ValueMLP ends in one unit, got {self.dims[-1]}")

    @classmethod
    def from_module(cls, module, **kw):
        """``MLPPolicyAgent.from_module`` for a critic: no output activation."""
        layers, act, out_act = cls._walk(module)
        if out_act is not None:
            raise TypeError("ValueMLP.from_module: a critic has no output activation")
        if "activation" in kw:
            raise TypeError("from_module reads the activations from the module")
        return cls(layers, activation=act, **kw)

    def device_spec(self, env):
        raise TypeError("ValueMLP is a critic: use env.mlp_values / collect_rollout(critic=...)")

    def update_from_module(self, env, module):
        """``MLPPolicyAgent.update_from_module`` for the critic."""
        super().update_from_module(env, module)


class GaussianMLPPolicyAgent(MLPPolicyAgent):
    """An ``MLPPolicyAgent`` that samples: a diagonal Gaussian around the
    network's output, the stochastic actor an on-policy learner (SB3 ``PPO`` /
    ``A2C``) collects its rollouts from.  The network kernel draws the noise
    itself, ``action_dim`` of numpy's ``standard_normal`` per env and step from
    the env's action generator, and reports the sample, its log-probability and
    the converted action (``include/invsim.h``, "Gaussian MLP actor"):
    ``raw = fmaf(std, (float)z, mean)``, ``log_prob`` the density of the
    unclipped sample, as SB3 stores it.

    ``log_std`` ``[action_dim]`` is SB3's state-independent parameter;
    ``std = exp(log_std)`` is computed here in float64 and rounded to float32.
    ``seed`` and the action stream follow ``RandomAgent``'s rule: env with
    global index g draws from ``Generator(PCG64(SeedSequence(2**64 + seed +
    g)))``; the first meeting with an env seeds its action generators, and the
    agent re-attaches its own buffer if another has been attached since.  The
    other arguments are ``MLPPolicyAgent``'s.

    ``collect_rollout(env, agent, K, obs0)`` is the rollout buffer's content
    in one C call; ``env.mlp_sample(agent, obs)`` the single launch;
    ``rollout_policy`` / ``evaluate_agent`` take the agent with their usual
    keys (``actions`` then holds the sampled, converted actions)."""

    def __init__(self, layers, log_std, seed=None, name="GaussianMLP", **kw):
        super().__init__(layers, name=name, **kw)
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        _require_agreed_seed(seed, world)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little") >> 1      # 63 bits of OS entropy
        self.seed = int(seed)
        self.log_std = _f32(log_std, (self.dims[-1],), "log_std")
        if not np.all(np.isfinite(self.log_std)):
            raise ValueError("log_std must be finite")
        with np.errstate(over="ignore"):
            self.std = np.exp(self.log_std.astype(np.float64)).astype(np.float32)
        if not np.all(np.isfinite(self.std)):
            raise ValueError("exp(log_std) must be finite in float32")
        self._bufs = weakref.WeakKeyDictionary()       # env -> the generators this agent seeded for it

    @classmethod
    def from_module(cls, module, log_std=None, **kw):
        """``MLPPolicyAgent.from_module`` plus ``log_std`` (SB3's ``policy.log_std``)."""
        if log_std is None:
            raise TypeError("GaussianMLPPolicyAgent.from_module needs log_std")
        return super().from_module(module, log_std=log_std, **kw)

    def device_object(self, env):
        """The ``invsim_mlp`` of this network on ``env`` with its Gaussian set, and
        this agent's action generators attached to ``env``."""
        fresh = self._objs.get(env) is None or self._objs[env][0] is not env._h
        obj = super().device_object(env)
        if fresh:
            _capi.check(env._lib.invsim_mlp_set_gaussian(env._h, obj, self.std.ctypes.data, self.log_std.ctypes.data),
                        env._h, "mlp_set_gaussian")
        buf = self._bufs.get(env)
        if buf is None:
            env.seed_actions(self.seed)
            self._bufs[env] = env._arng
        elif env._arng is not buf:
            env._attach_action_rng(buf)
        return obj


def _rollout_mlp_sample(env, agent, K, obs, rewards, actions, metrics, obs0, raw=False, log_prob=False):
    """The closed loop of a GaussianMLPPolicyAgent: one invsim_rollout_mlp_sample call."""
    if obs0 is None:
        raise ValueError("a GaussianMLPPolicyAgent rollout needs obs0, the observation the env last returned "
                         "(reset()'s, or the last row of the previous rollout's obs)")
    N, dev, A = env.num_envs, env.device, env.action_dim
    obs0 = torch.as_tensor(obs0, device=dev)
    if tuple(obs0.shape) != (N, env.obs_dim):
        raise ValueError(f"obs0 must have shape {(N, env.obs_dim)}, got {tuple(obs0.shape)}")
    obs0 = obs0.to(env.obs_dtype).contiguous()
    metrics = env._metrics_arg(metrics)
    obj = agent.device_object(env)
    out = {}
    o = torch.empty((K, N, env.obs_dim), dtype=env.obs_dtype, device=dev) if obs else None
    if rewards:
        out["reward"] = torch.empty((K, N), dtype=torch.float64, device=dev)
        out["terminated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
        out["truncated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
    a = torch.empty((K, N, A), dtype=env.act_dtype, device=dev) if actions else None
    r = torch.empty((K, N, A), dtype=torch.float32, device=dev) if raw else None
    lp = torch.empty((K, N), dtype=torch.float32, device=dev) if log_prob else None
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _capi.check(env._lib.invsim_rollout_mlp_sample(
        env._h, int(K), obj, obs0.data_ptr(), p(o), p(out.get("reward")), p(out.get("terminated")),
        p(out.get("truncated")), p(a), p(r), p(lp), p(metrics), env._stream()), env._h, "rollout_mlp_sample")
    for key, t in (("obs", o), ("actions", a), ("raw_actions", r), ("log_prob", lp)):
        if t is not None:
            out[key] = t
    return out


def gae(reward, terminated, truncated, value0, values, gamma=0.99, gae_lambda=0.95, done0=None, stream=None):
    """Generalised advantage estimation over K rows of a rollout, one HIP launch
    (``invsim_gae``; the recurrence is stated op by op in ``include/invsim.h``,
    "Critic, GAE and parameter updates", float64 inside).  ``reward`` [K, n]
    float64; ``terminated`` / ``truncated`` [K, n] bool or uint8, either may be
    ``None``; ``value0`` [n] float32, V of the observation the first step's
    policy saw; ``values`` [K, n] float32, V of obs row k; ``done0`` [n], the
    done flag of the row before this block (the previous call's last row), or
    ``None``.  A truncated step bootstraps from ``gamma * values[k]``, the
    value of its final observation; the row after a finished episode (NEXT_STEP
    autoreset's reset row) is no transition: advantage 0, ``valid`` False.
    Returns a dict of device tensors ``advantages`` / ``returns`` float32 and
    ``valid`` bool, all [K, n].  ``stream``: a raw stream handle (default:
    torch's current stream on ``reward``'s device)."""
    dev = reward.device
    if reward.dim() != 2:
        raise ValueError(f"reward must be [K, n], got {tuple(reward.shape)}")
    K, n = reward.shape

    def flag(t, shape, what):
        if t is None:
            return None
        t = torch.as_tensor(t, device=dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
        return (t if t.dtype in (torch.bool, torch.uint8) else t != 0).contiguous()

    def f32(t, shape, what):
        t = torch.as_tensor(t, device=dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
        return t.to(torch.float32).contiguous()
    reward = reward.to(torch.float64).contiguous()
    te, tr = flag(terminated, (K, n), "terminated"), flag(truncated, (K, n), "truncated")
    d0 = flag(done0, (n,), "done0")
    v0, v = f32(value0, (n,), "value0"), f32(values, (K, n), "values")
    out = {"advantages": torch.empty((K, n), dtype=torch.float32, device=dev),
           "returns": torch.empty((K, n), dtype=torch.float32, device=dev),
           "valid": torch.empty((K, n), dtype=torch.bool, device=dev)}
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(_capi.lib().invsim_gae(p(reward), p(te), p(tr), p(d0), p(v0), p(v), int(K), int(n), float(gamma),
                                           float(gae_lambda), p(out["advantages"]), p(out["returns"]), p(out["valid"]),
                                           stream), None, "invsim_gae")
    return out


_NORM_DTYPES = {torch.int64: _capi.DTYPE_I64, torch.float32: _capi.DTYPE_F32, torch.float64: _capi.DTYPE_F64}


def _stream_or_current(dev, stream):
    return torch.cuda.current_stream(dev).cuda_stream if stream is None else stream


def _norm_flag(t, shape, what, dev):
    if t is None:
        return None
    t = torch.as_tensor(t, device=dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return (t if t.dtype in (torch.bool, torch.uint8) else t != 0).contiguous()


class RunningMoments:
    """Running per-column count, mean and M2 (sum of squared deviations) on the
    device, float64 ``[3, cols]`` in ``stats``, advanced by ``invsim_moments``:
    a fixed binary tree of Chan merges over leaves of 64 rows, stated op by op
    in ``include/invsim.h`` ("Running normalisation") and restated in
    ``tests/norm_model.py``, so the statistics are defined bit for bit and do
    not depend on scheduling.  It starts as SB3's ``RunningMeanStd``: count
    1e-4, mean 0, variance 1 (M2 = 1e-4).

    ``update(x, mask=None)`` folds the rows of ``x`` in: ``x`` is ``[..., cols]``
    (any shape when ``cols == 1``), int64 / float32 / float64, on the device;
    ``mask`` (bool / uint8, one entry per row) leaves rows out.  It reads ``x``
    once, allocates nothing once its scratch is large enough (the scratch grows
    on demand, which is refused during stream capture: run the largest shape
    once before capturing), and never synchronises."""

    def __init__(self, cols, device):
        cols = int(cols)
        if not 1 <= cols <= _capi.MOMENTS_MAX_COLS:
            raise ValueError(f"cols must be 1..{_capi.MOMENTS_MAX_COLS}, got {cols}")
        self.cols = cols
        self.device = torch.device(device)
        init = np.zeros((3, cols))
        init[0] = init[2] = 1e-4
        self.stats = torch.from_numpy(init).to(self.device)
        self._scratch = None

    def _rows(self, x, mask):
        """validate; (x contiguous, mask uint8 / bool contiguous or None, rows)"""
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"x must be a torch tensor, got {type(x).__name__}")
        if x.dtype not in _NORM_DTYPES:
            raise TypeError(f"x must be int64, float32 or float64, got {x.dtype}")
        if x.device != self.device:
            raise ValueError(f"x must be on {self.device}, got {x.device}")
        if self.cols > 1 and (x.dim() < 1 or x.shape[-1] != self.cols):
            raise ValueError(f"x must have shape [..., {self.cols}], got {tuple(x.shape)}")
        rows = x.numel() // self.cols
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device)
            if mask.numel() != rows:
                raise ValueError(f"mask must have one entry per row ({rows}), got shape {tuple(mask.shape)}")
            mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
        return x.contiguous(), mask, rows

    def update(self, x, mask=None, stream=None):
        x, mask, rows = self._rows(x, mask)
        if rows == 0:
            return self
        lib = _capi.lib()
        need = C.c_int64()
        _capi.check(lib.invsim_moments_scratch_bytes(rows, self.cols, C.byref(need)), None, "moments_scratch_bytes")
        if self._scratch is None or self._scratch.numel() < need.value:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RunningMoments: the scratch must grow, which allocates: update once with the "
                                   "largest shape before capturing")
            self._scratch = torch.empty(max(need.value, 8), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(lib.invsim_moments(x.data_ptr(), _NORM_DTYPES[x.dtype], rows, self.cols,
                                           None if mask is None else mask.data_ptr(), self.stats.data_ptr(),
                                           self._scratch.data_ptr(), self._scratch.numel(),
                                           _stream_or_current(self.device, stream)), None, "invsim_moments")
        return self

    @property
    def count(self):
        return self.stats[0]

    @property
    def mean(self):
        return self.stats[1]

    @property
    def var(self):
        """M2 / count (float64 ``[cols]``, a torch operation on the current stream)"""
        return self.stats[2] / self.stats[0]

    def scale_shift(self, epsilon=1e-8, stream=None):
        """``(scale, shift)``, new float32 ``[cols]`` device tensors with
        ``x * scale + shift = (x - mean) / sqrt(var + epsilon)`` (``invsim_norm_params``)"""
        scale = torch.empty(self.cols, dtype=torch.float32, device=self.device)
        shift = torch.empty_like(scale)
        with torch.cuda.device(self.device):
            _capi.check(_capi.lib().invsim_norm_params(self.stats.data_ptr(), self.cols, float(epsilon),
                                                       scale.data_ptr(), shift.data_ptr(),
                                                       _stream_or_current(self.device, stream)),
                        None, "invsim_norm_params")
        return scale, shift


def discounted_returns(reward, terminated, truncated, ret, gamma=0.99, done0=None, stream=None):
    """VecNormalize's running discounted return over K rows, one HIP launch
    (``invsim_discounted_returns``): ``ret`` ``[n]`` float64 is advanced in place
    (``ret = ret * gamma + reward``, reset to 0 after a done and on the NEXT_STEP
    reset row that follows it).  ``reward`` [K, n] float64; flags and ``done0`` as
    in ``gae``.  Returns ``(out, valid)``: the return after every row, float64
    [K, n], and bool [K, n], False on reset rows."""
    if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
        raise ValueError("reward must be a [K, n] tensor")
    if reward.dtype != torch.float64:
        raise TypeError(f"reward must be float64, got {reward.dtype}")
    dev = reward.device
    K, n = reward.shape
    if (not isinstance(ret, torch.Tensor) or ret.dtype != torch.float64 or tuple(ret.shape) != (n,)
            or not ret.is_contiguous()):
        raise ValueError(f"ret must be a contiguous float64 tensor of shape {(n,)}: it is advanced in place")
    te, tr = _norm_flag(terminated, (K, n), "terminated", dev), _norm_flag(truncated, (K, n), "truncated", dev)
    d0 = _norm_flag(done0, (n,), "done0", dev)
    reward = reward.contiguous()
    out = torch.empty((K, n), dtype=torch.float64, device=dev)
    valid = torch.empty((K, n), dtype=torch.bool, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().invsim_discounted_returns(p(reward), p(te), p(tr), p(d0), int(K), int(n), float(gamma),
                                                          p(ret), p(out), p(valid), _stream_or_current(dev, stream)),
                    None, "invsim_discounted_returns")
    return out, valid


def normalize_rewards(reward, stats, epsilon=1e-8, clip=10.0, out=None, stream=None):
    """``clip(reward / sqrt(var + epsilon), -clip, clip)`` with ``var`` from the
    ``[3, 1]`` statistics of the discounted returns (``invsim_normalize_rewards``);
    float64 in and out, ``out`` may be ``reward`` itself."""
    if not isinstance(reward, torch.Tensor) or reward.dtype != torch.float64:
        raise TypeError("reward must be a float64 tensor")
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or tuple(stats.shape) != (3, 1):
        raise ValueError("stats must be the float64 [3, 1] statistics of a RunningMoments(1, ...)")
    if not float(clip) > 0:
        raise ValueError(f"clip must be > 0, got {clip}")
    reward = reward.contiguous()
    if out is None:
        out = torch.empty_like(reward)
    elif out.dtype != torch.float64 or out.shape != reward.shape or not out.is_contiguous():
        raise ValueError("out must be float64, contiguous and of reward's shape")
    with torch.cuda.device(reward.device):
        s = _stream_or_current(reward.device, stream)
        _capi.check(_capi.lib().invsim_normalize_rewards(reward.data_ptr(), reward.numel(), stats.data_ptr(),
                                                         float(epsilon), float(clip), out.data_ptr(), s),
                    None, "invsim_normalize_rewards")
    return out


class Normalizer:
    """What SB3's ``VecNormalize`` keeps for a PPO / A2C learner, on the device:
    ``obs_rms`` (``RunningMoments`` of the observations), ``ret_rms`` (of the
    discounted return), the running return ``ret`` ``[N]``, and the current
    ``obs_scale`` / ``obs_shift`` (float32 ``[obs_dim]``: ``obs * scale + shift``
    is the normalised observation, for the learner's torch forward pass).
    ``collect_rollout(..., normalize=norm)`` advances it; ``observe(obs)`` folds
    further rows in (the first reset's ``obs0``).

    Differences from ``VecNormalize``: the statistics advance once per K-step
    ``collect_rollout`` call, not once per step (a rollout runs under the rows
    the call began with); there is no ``clip_obs`` (the network's fused input
    stage has no clamp); advantage normalisation stays with the learner (SB3
    does it per minibatch); reset rows (``valid`` False) do not enter the
    return statistics."""

    def __init__(self, env, gamma=0.99, epsilon=1e-8, clip_reward=10.0, norm_obs=True, norm_reward=True):
        if not float(clip_reward) > 0:
            raise ValueError(f"clip_reward must be > 0, got {clip_reward}")
        self.gamma, self.epsilon, self.clip_reward = float(gamma), float(epsilon), float(clip_reward)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.device = env.device
        self.obs_rms = RunningMoments(env.obs_dim, env.device)
        self.ret_rms = RunningMoments(1, env.device)
        self.ret = torch.zeros(env.num_envs, dtype=torch.float64, device=env.device)
        self.obs_scale, self.obs_shift = self.obs_rms.scale_shift(self.epsilon)

    def observe(self, obs, stream=None):
        """fold observation rows ``[..., obs_dim]`` (the env's obs dtype) into ``obs_rms`` and refresh the rows"""
        self.obs_rms.update(obs, stream=stream)
        self.obs_scale, self.obs_shift = self.obs_rms.scale_shift(self.epsilon, stream=stream)
        return self

    def normalize_obs(self, obs):
        """``obs`` as the network's input stage sees it: float32 ``fma(obs, scale, shift)`` in torch"""
        return torch.addcmul(self.obs_shift, obs.to(torch.float32), self.obs_scale)


def collect_rollout(env, agent, K, obs0, metrics=None, critic=None, gamma=0.99, gae_lambda=0.95, done0=None,
                    normalize=None):
    """K steps of every env under a ``GaussianMLPPolicyAgent``, everything an
    on-policy rollout buffer stores, from one C call (two launches per step,
    no Python in the loop).  Returns device tensors: ``obs`` [K, N, O] (row k is
    the observation after step k; the network's input at step k is ``obs0`` /
    row k - 1), ``actions`` [K, N, A] (action dtype, what the env was stepped
    with), ``raw_actions`` [K, N, A] and ``log_prob`` [K, N] float32 (the
    unclipped sample and its log-density), ``reward`` [K, N] float64,
    ``terminated`` / ``truncated`` [K, N] bool.  ``metrics`` as in
    ``rollout_policy``.

    With ``critic`` (a ``ValueMLP``, or any callable taking the float32
    observations ``[K + 1, N, O]`` of ``obs0`` and the K rows) the values and
    advantages come with it, three more launches and no host synchronisation:
    ``values`` [K, N] float32, V of each step's input observation,
    ``last_value`` [N], V of the last row; ``advantages`` / ``returns`` /
    ``valid`` [K, N] from ``gae`` with ``gamma`` / ``gae_lambda``; ``done`` [N]
    bool, the last row's terminated | truncated, which is the next call's
    ``done0`` (``None``: no env finished just before ``obs0``).  Rows with
    ``valid`` False are NEXT_STEP reset rows: mask them out of the loss.
    Without a critic the call and its result are what they were.

    With ``normalize`` (a ``Normalizer``) the running statistics advance inside
    the call, a handful of further launches and still no synchronisation, in
    this order: the rollout runs under the actor's current input rows; the K obs
    rows are folded into ``normalize.obs_rms``; the new scale / shift are
    written into the actor and into a ``ValueMLP`` critic (both must have been
    built with ``in_scale`` / ``in_shift``); the critic's values are computed
    under the new rows (a callable critic gets the observations already
    normalised); the running discounted return advances over the K rows and its
    valid rows are folded into ``normalize.ret_rms``; ``reward_norm`` is the
    clipped reward over the return's standard deviation; GAE runs on
    ``reward_norm``.  New keys: ``reward_norm`` [K, N] float64 (``reward`` stays
    raw), ``obs_scale`` / ``obs_shift`` [O] float32 (the rows just written), and
    ``done`` also without a critic.  Unlike SB3's ``VecNormalize`` the
    statistics advance once per call, not per step; there is no ``clip_obs``;
    advantages are not normalised (SB3 does that per minibatch, in the
    learner).  Without ``normalize`` the call, its launches and its result are
    what they were."""
    if not isinstance(agent, GaussianMLPPolicyAgent):
        raise TypeError("collect_rollout needs a GaussianMLPPolicyAgent")
    K = int(K)
    if normalize is not None and not isinstance(normalize, Normalizer):
        raise TypeError("normalize must be a Normalizer")
    if critic is None and normalize is None:
        return _rollout_mlp_sample(env, agent, K, True, True, True, metrics, obs0, raw=True, log_prob=True)
    if critic is not None and not isinstance(critic, ValueMLP) and not callable(critic):
        raise TypeError("critic must be a ValueMLP or a callable on the observations")
    norm = normalize
    if norm is not None and norm.norm_obs:
        for net in (agent, critic) if isinstance(critic, ValueMLP) else (agent,):
            if net.in_scale is None:
                raise ValueError(f"{net.name}: normalize needs a network built with in_scale / in_shift")
    if obs0 is not None:
        obs0 = torch.as_tensor(obs0, device=env.device).to(env.obs_dtype).contiguous()
    out = _rollout_mlp_sample(env, agent, K, True, True, True, metrics, obs0, raw=True, log_prob=True)
    N, s = env.num_envs, env._stream()
    if norm is not None and norm.norm_obs:
        norm.obs_rms.update(out["obs"], stream=s)
        norm.obs_scale, norm.obs_shift = norm.obs_rms.scale_shift(norm.epsilon, stream=s)
        agent.set_input_norm(env, norm.obs_scale, norm.obs_shift)
        if isinstance(critic, ValueMLP):
            critic.set_input_norm(env, norm.obs_scale, norm.obs_shift)
    if isinstance(critic, ValueMLP):
        v = torch.empty((K + 1, N), dtype=torch.float32, device=env.device)
        env._mlp_values_into(critic, obs0, N, v[0])
        env._mlp_values_into(critic, out["obs"], K * N, v[1:])
    elif critic is not None:
        allobs = torch.cat([obs0[None], out["obs"]])
        v = critic(norm.normalize_obs(allobs) if norm is not None and norm.norm_obs else allobs.float())
        v = v.detach().reshape(K + 1, N).to(torch.float32).contiguous()
    reward = out["reward"]
    if norm is not None:
        if norm.norm_reward:
            dr, dr_valid = discounted_returns(reward, out["terminated"], out["truncated"], norm.ret, norm.gamma, done0,
                                              stream=s)
            norm.ret_rms.update(dr, mask=dr_valid, stream=s)
            reward = normalize_rewards(reward, norm.ret_rms.stats, norm.epsilon, norm.clip_reward, stream=s)
        out["reward_norm"] = reward
        out["obs_scale"], out["obs_shift"] = norm.obs_scale, norm.obs_shift
    if critic is not None:
        out.update(gae(reward, out["terminated"], out["truncated"], v[0], v[1:], gamma, gae_lambda, done0, stream=s))
        out["values"], out["last_value"] = v[:K], v[K]
    out["done"] = (out["terminated"][K - 1] | out["truncated"][K - 1]) if K else torch.zeros(N, dtype=torch.bool,
                                                                                          device=env.device)
    return out


def ppo_scratch_bytes(dims, rows):
    """``invsim_ppo_scratch_bytes``: the scratch one gradient call over ``rows``
    samples needs for a network of widths ``dims`` (host only, no GPU)."""
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.int32))
    need = C.c_int64()
    _capi.check(_capi.lib().invsim_ppo_scratch_bytes(d.ctypes.data, len(d) - 1, int(rows), C.byref(need)), None,
                "ppo_scratch_bytes")
    return need.value


def _ppo_tensor(t, what, dtypes, numel, dev):
    """a device array of a gradient call: checked, never converted (no hidden copy of a rollout)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{what} must be on {dev}, got {t.device}")
    if not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise ValueError(f"{what} must be contiguous" + (f" with {numel} elements" if numel is not None else "")
                         + f", got shape {tuple(t.shape)}")
    return t


def _ppo_samples(env, net, buf, obs0, idx, keys):
    """What the two gradient wrappers check before any library call.  Returns
    (obs0 or None, n0, obs, idx or None, rows, valid or None, [buf[k] for k in keys])."""
    if not isinstance(buf, dict):
        raise TypeError("buf must be the dict collect_rollout(critic=...) returns")
    for k in ("obs",) + tuple(keys):
        if k not in buf:
            raise ValueError(f"buf has no {k!r}: collect the rollout with critic=...")
    dev, O = env.device, env.obs_dim
    if net.dims[0] != O:
        raise ValueError(f"{net.name} takes {net.dims[0]} inputs, the env's observations have {O}")
    obs = _ppo_tensor(buf["obs"], "buf['obs']", (env.obs_dtype,), None, dev)
    if obs.dim() < 2 or obs.shape[-1] != O:
        raise ValueError(f"buf['obs'] must have shape [..., {O}], got {tuple(obs.shape)}")
    n0 = 0
    if obs0 is not None:
        obs0 = _ppo_tensor(obs0, "obs0", (env.obs_dtype,), None, dev)
        if obs0.dim() != 2 or obs0.shape[1] != O:
            raise ValueError(f"obs0 must have shape [n0, {O}], got {tuple(obs0.shape)}")
        n0 = obs0.shape[0]
    S = obs.numel() // O          # samples: the first S rows of cat([obs0, obs])
    per = [_ppo_tensor(buf[k], f"buf[{k!r}]", (torch.float32,), S * (net.dims[-1] if k == "raw_actions" else 1), dev)
           for k in keys]
    valid = buf.get("valid")
    if valid is not None:
        valid = _ppo_tensor(valid, "buf['valid']", (torch.bool, torch.uint8), S, dev)
    rows = S
    if idx is not None:
        idx = _ppo_tensor(idx, "idx", (torch.int64,), None, dev)
        if idx.dim() != 1:
            raise ValueError(f"idx must be one-dimensional, got shape {tuple(idx.shape)}")
        rows = idx.shape[0]
    return obs0, n0, obs, idx, rows, valid, per


class _PPOGrads:
    """Gradient tensors of one network in torch's layouts, the pointer arrays a
    gradient call takes, and a scratch that grows on demand (not during capture)."""

    def __init__(self, net, dev, log_std=False):
        self.dims = list(net.dims)
        self.weight = [torch.zeros(w.shape, dtype=torch.float32, device=dev) for w in net.weights]
        self.bias = [torch.zeros(w.shape[0], dtype=torch.float32, device=dev) for w in net.weights]
        self.log_std = torch.zeros(net.dims[-1], dtype=torch.float32, device=dev) if log_std else None
        self.stats = torch.zeros(6 if log_std else 2, dtype=torch.float64, device=dev)
        n = len(self.weight)
        self.W = (C.c_void_p * n)(*[t.data_ptr() for t in self.weight])
        self.B = (C.c_void_p * n)(*[t.data_ptr() for t in self.bias])
        self.scratch = None

    def scratch_for(self, rows, dev):
        need = ppo_scratch_bytes(self.dims, rows)
        if self.scratch is None or self.scratch.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the gradient scratch must grow, which allocates: call once with the largest "
                                   "minibatch before capturing")
            self.scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        return self.scratch

    def result(self):
        out = {"weight": self.weight, "bias": self.bias, "stats": self.stats}
        if self.log_std is not None:
            out["log_std"] = self.log_std
        return out


def ppo_actor_grad(env, pi, buf, obs0, idx=None, clip_range=0.2, ent_coef=0.0, adv_stats=None, out=None):
    """The gradient of SB3's PPO actor loss over one minibatch of a collected
    rollout, two HIP launches (``invsim_ppo_actor_grad``; ``include/invsim.h``
    "PPO gradients" states the loss).  ``pi``: the ``GaussianMLPPolicyAgent`` the
    rollout was collected with; ``buf``: ``collect_rollout(critic=...)``'s dict
    (``obs``, ``raw_actions``, ``log_prob``, ``advantages`` and, if present,
    ``valid`` are read in place, never copied or cast); ``obs0``: the rollout's
    first input ``[N, O]``, so that sample ``k * N + n`` reads the observation
    the network saw at step k (``None``: sample s reads ``obs`` row s).  ``idx``:
    int64 device tensor of sample numbers, the minibatch (``None``: every
    sample; the caller answers for its range).  ``adv_stats``: float64 ``[3]``
    or ``[3, 1]`` (``RunningMoments(1).stats``) to normalise the advantages
    with, or ``None``.  A2C: ``clip_range=float('inf')``.  Returns ``{"weight":
    [...], "bias": [...], "log_std": t, "stats": t}``, float32 device tensors in
    ``torch.nn.Linear``'s layouts and float64 ``[6]`` (n, policy loss, entropy,
    approx_kl, clip fraction, mean ratio).  ``out``: an earlier result's holder
    (``PPOLearner`` keeps one), else new tensors.  No synchronisation; legal
    under ``env.capture`` once the scratch has its size."""
    if not isinstance(pi, GaussianMLPPolicyAgent):
        raise TypeError("ppo_actor_grad needs the GaussianMLPPolicyAgent the rollout was collected with")
    if not float(clip_range) > 0:
        raise ValueError(f"clip_range must be > 0, got {clip_range}")
    obs0, n0, obs, idx, rows, valid, (raw, logp, adv) = _ppo_samples(env, pi, buf, obs0, idx,
                                                                    ("raw_actions", "log_prob", "advantages"))
    if adv_stats is not None:
        if (not isinstance(adv_stats, torch.Tensor) or adv_stats.dtype != torch.float64 or adv_stats.numel() != 3
                or not adv_stats.is_contiguous() or adv_stats.device != env.device):
            raise ValueError("adv_stats must be a contiguous float64 device tensor of 3 entries (count, mean, M2)")
    g = out if out is not None else _PPOGrads(pi, env.device, log_std=True)
    obj = pi.device_object(env)
    if rows == 0:
        return g.result()
    scratch = g.scratch_for(rows, env.device)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _capi.check(env._lib.invsim_ppo_actor_grad(
        env._h, obj, p(obs0), n0, p(obs), p(idx), rows, p(valid), p(raw), p(logp), p(adv), p(adv_stats),
        float(clip_range), float(ent_coef), C.cast(g.W, C.c_void_p), C.cast(g.B, C.c_void_p), p(g.log_std), p(g.stats),
        scratch.data_ptr(), scratch.numel(), env._stream()), env._h, "ppo_actor_grad")
    return g.result()


def value_grad(env, vf, buf, obs0, idx=None, vf_coef=0.5, out=None):
    """The gradient of ``vf_coef * mean((returns - V)^2)`` over one minibatch
    (``invsim_value_grad``): ``vf`` the ``ValueMLP``, everything else as
    ``ppo_actor_grad`` (``buf['returns']`` in place of the actor's arrays).
    Returns ``{"weight": [...], "bias": [...], "stats": t}``, ``stats`` float64
    ``[2]``: n and the unscaled mean squared error."""
    if not isinstance(vf, ValueMLP):
        raise TypeError("value_grad needs a ValueMLP")
    obs0, n0, obs, idx, rows, valid, (ret,) = _ppo_samples(env, vf, buf, obs0, idx, ("returns",))
    g = out if out is not None else _PPOGrads(vf, env.device)
    obj = vf.device_object(env)
    if rows == 0:
        return g.result()
    scratch = g.scratch_for(rows, env.device)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _capi.check(env._lib.invsim_value_grad(
        env._h, obj, p(obs0), n0, p(obs), p(idx), rows, p(valid), p(ret), float(vf_coef), C.cast(g.W, C.c_void_p),
        C.cast(g.B, C.c_void_p), p(g.stats), scratch.data_ptr(), scratch.numel(), env._stream()), env._h, "value_grad")
    return g.result()


class PPOLearner:
    """SB3's ``PPO.train`` for the in-library actor and critic (separate
    networks, state-independent ``log_std``): minibatch epochs whose forward,
    loss and backward are the two gradient calls above, with the optimiser in
    torch.  ``pi`` / ``vf``: the ``GaussianMLPPolicyAgent`` / ``ValueMLP`` the
    rollouts are collected with; ``actor`` / ``critic``: the ``nn.Sequential``
    modules they were built from (float32 parameters on the env's device);
    ``log_std``: the ``nn.Parameter`` ``[A]``.  The learner owns preallocated
    gradient tensors, which every parameter's ``.grad`` aliases from then on,
    the scratch, and a ``RunningMoments(1)`` for the advantages.

    ``update(buf, obs0)`` runs on the env's stream and never synchronises: the
    advantage statistics over the rollout's valid rows (``invsim_moments``, once
    per call); per epoch a device ``randperm``; per minibatch the two gradient
    calls, ``clip_grad_norm_`` over actor, critic and ``log_std`` jointly,
    ``optimizer.step()`` (default ``Adam(lr=3e-4, eps=1e-5, fused=True)``) and
    ``update_from_module`` on both networks.  It returns the per-minibatch
    statistics stacked on the device: ``{"actor": [M, 6], "critic": [M, 2]}``.

    Differences from SB3: the advantages are normalised with the statistics of
    the whole rollout's valid rows, not of each minibatch; reset rows (``valid``
    False) are in the permutation but selected out of every sum, so a minibatch
    averages over its valid samples; there is no ``clip_range_vf`` and no
    ``target_kl``."""

    def __init__(self, env, pi, vf, actor, critic, log_std, optimizer=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, n_epochs=10, batch_size=4096, normalize_advantage=True):
        if not isinstance(pi, GaussianMLPPolicyAgent):
            raise TypeError("pi must be a GaussianMLPPolicyAgent")
        if not isinstance(vf, ValueMLP):
            raise TypeError("vf must be a ValueMLP")
        if not isinstance(actor, torch.nn.Module) or not isinstance(critic, torch.nn.Module):
            raise TypeError("actor and critic must be the torch modules the networks were built from")
        if not isinstance(log_std, torch.nn.Parameter):
            raise TypeError("log_std must be a torch.nn.Parameter")
        if optimizer is not None and not isinstance(optimizer, torch.optim.Optimizer):
            raise TypeError("optimizer must be a torch.optim.Optimizer or None")
        if not float(clip_range) > 0:
            raise ValueError(f"clip_range must be > 0, got {clip_range}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be > 0 or None, got {max_grad_norm}")
        if int(n_epochs) < 1 or int(batch_size) < 1:
            raise ValueError("n_epochs and batch_size must be >= 1")
        a_params, c_params = pi._module_params(actor), vf._module_params(critic)
        if tuple(log_std.shape) != (pi.dims[-1],):
            raise ValueError(f"log_std must have shape {(pi.dims[-1],)}, got {tuple(log_std.shape)}")
        self.params = [t for w, b in a_params + c_params for t in (w, b) if t is not None] + [log_std]
        for t in self.params:
            if t.dtype != torch.float32 or t.device != env.device or not t.is_contiguous():
                raise ValueError(f"every parameter must be float32, contiguous and on {env.device}: its .grad aliases a "
                                 "tensor the gradient kernels write")
        self.env, self.pi, self.vf, self.actor, self.critic, self.log_std = env, pi, vf, actor, critic, log_std
        self.clip_range, self.ent_coef, self.vf_coef = float(clip_range), float(ent_coef), float(vf_coef)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.n_epochs, self.batch_size = int(n_epochs), int(batch_size)
        self.normalize_advantage = bool(normalize_advantage)
        self._ga, self._gc = _PPOGrads(pi, env.device, log_std=True), _PPOGrads(vf, env.device)
        for g, params in ((self._ga, a_params), (self._gc, c_params)):
            for l, (w, b) in enumerate(params):
                w.grad = g.weight[l]
                if b is not None:
                    b.grad = g.bias[l]
        log_std.grad = self._ga.log_std
        self.optimizer = optimizer if optimizer is not None else torch.optim.Adam(self.params, lr=3e-4, eps=1e-5,
                                                                                  fused=True)
        self.adv_rms = RunningMoments(1, env.device)

    def update(self, buf, obs0, perms=None):
        """One ``PPO.train``: ``n_epochs`` passes over ``buf`` in minibatches of
        ``batch_size`` (the last one of an epoch may be short).  ``perms``: the
        epochs' sample orders as int64 device tensors, one per epoch (any
        length), default a device ``randperm`` of all samples each."""
        env = self.env
        S = buf["obs"].numel() // env.obs_dim
        stats = None
        if self.normalize_advantage:
            self.adv_rms.stats.zero_()      # this rollout's statistics alone
            self.adv_rms.update(buf["advantages"], mask=buf.get("valid"), stream=env._stream())
            stats = self.adv_rms.stats
        a_stats, c_stats = [], []
        for e in range(self.n_epochs):
            perm = perms[e] if perms is not None else torch.randperm(S, device=env.device)
            for lo in range(0, perm.shape[0], self.batch_size):
                idx = perm[lo:lo + self.batch_size]
                ppo_actor_grad(env, self.pi, buf, obs0, idx, self.clip_range, self.ent_coef, stats, out=self._ga)
                value_grad(env, self.vf, buf, obs0, idx, self.vf_coef, out=self._gc)
                if self.max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm, foreach=True)
                self.optimizer.step()
                self.pi.update_from_module(env, self.actor, log_std=self.log_std)
                self.vf.update_from_module(env, self.critic)
                a_stats.append(self._ga.stats.clone())
                c_stats.append(self._gc.stats.clone())
        return {"actor": torch.stack(a_stats), "critic": torch.stack(c_stats)}


def _rollout_mlp(env, agent, K, obs, rewards, actions, metrics, obs0):
    """The closed loop of an MLPPolicyAgent: one invsim_rollout_mlp call."""
    if obs0 is None:
        raise ValueError("an MLPPolicyAgent rollout needs obs0, the observation the env last returned "
                         "(reset()'s, or the last row of the previous rollout's obs)")
    N, dev = env.num_envs, env.device
    obs0 = torch.as_tensor(obs0, device=dev)
    if tuple(obs0.shape) != (N, env.obs_dim):
        raise ValueError(f"obs0 must have shape {(N, env.obs_dim)}, got {tuple(obs0.shape)}")
    obs0 = obs0.to(env.obs_dtype).contiguous()
    metrics = env._metrics_arg(metrics)
    obj = agent.device_object(env)
    out = {}
    o = torch.empty((K, N, env.obs_dim), dtype=env.obs_dtype, device=dev) if obs else None
    if rewards:
        out["reward"] = torch.empty((K, N), dtype=torch.float64, device=dev)
        out["terminated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
        out["truncated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
    a = torch.empty((K, N, env.action_dim), dtype=env.act_dtype, device=dev) if actions else None
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _capi.check(env._lib.invsim_rollout_mlp(
        env._h, int(K), obj, obs0.data_ptr(), p(o), p(out.get("reward")), p(out.get("terminated")),
        p(out.get("truncated")), p(a), p(metrics), env._stream()), env._h, "rollout_mlp")
    if obs:
        out["obs"] = o
    if actions:
        out["actions"] = a
    return out


def rollout_policy(env, agent, K, obs=False, rewards=True, actions=False, metrics=None, obs0=None):
    """K steps of every env of ``env`` under ``agent``.  Returns a dict with
    the requested device tensors; ``metrics`` (float64 [N, M]) is accumulated in
    place when given.  The heuristic agents run in the step kernel, one launch;
    a ``TorchPolicyAgent`` runs in torch between K one-step launches and an
    ``MLPPolicyAgent`` in a kernel of its own before each (a
    ``GaussianMLPPolicyAgent``: the sampling variant of that kernel; the
    log-probabilities come with ``collect_rollout``); all need ``obs0``,
    the observation the env last returned (``actions`` then records what the
    policy produced at every step, reset steps included)."""
    if isinstance(agent, TorchPolicyAgent):
        return _rollout_torch(env, agent, int(K), obs, rewards, actions, metrics, obs0)
    if isinstance(agent, ValueMLP):
        raise TypeError("a ValueMLP is a critic, not a policy: see collect_rollout(critic=...)")
    if isinstance(agent, GaussianMLPPolicyAgent):
        return _rollout_mlp_sample(env, agent, int(K), obs, rewards, actions, metrics, obs0)
    if isinstance(agent, MLPPolicyAgent):
        return _rollout_mlp(env, agent, int(K), obs, rewards, actions, metrics, obs0)
    spec, keep = agent.device_spec(env)
    N, dev = env.num_envs, env.device
    out = {}
    o = torch.empty((K, N, env.obs_dim), dtype=env.obs_dtype, device=dev) if obs else None
    if rewards:
        out["reward"] = torch.empty((K, N), dtype=torch.float64, device=dev)
        out["terminated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
        out["truncated"] = torch.empty((K, N), dtype=torch.bool, device=dev)
    # the kernels record the agent's order of every stepped env; a NEXT_STEP
    # reset step (whose action the env ignores) keeps the 0 written here
    a = torch.zeros((K, N, env.action_dim), dtype=env.act_dtype, device=dev) if actions else None
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _capi.check(env._lib.invsim_rollout_policy(
        env._h, int(K), C.byref(spec), p(o), p(out.get("reward")), p(out.get("terminated")),
        p(out.get("truncated")), p(a), p(metrics), env._stream()), env._h, "rollout_policy")
    del keep
    if obs:
        out["obs"] = o
    if actions:
        out["actions"] = a
    return out


def metrics_dim(env):
    d = C.c_int32()
    _capi.check(env._lib.invsim_metrics_dim(env._h, C.byref(d)), env._h, "metrics_dim")
    return d.value


def summarize(family, m, main_nodes=None):
    """Per-episode summary columns from the accumulated sums, with the
    reference's float expressions."""
    m = np.asarray(m, np.float64)
    rows = {"TotalReward": m[:, 0], "Steps": m[:, 1].astype(np.int64)}
    if family == _capi.INVSIM_INVMGMT:
        # benchmark_InvManagementBacklogEnv.py:412-415
        steps, dem, sales, stock, inv = m[:, 1], m[:, 2], m[:, 3], m[:, 4], m[:, 5]
        rows["AvgServiceLevel"] = np.array([s / max(1e-6, d) if d > 1e-6 else 1.0 for s, d in zip(sales, dem)])
        rows["TotalStockoutQty"] = stock
        rows["AvgEndingInv"] = np.array([i / n if n > 0 else 0 for i, n in zip(inv, steps)], np.float64)
    elif family == _capi.INVSIM_NETINVMGMT:
        # benchmark_NetInvMgmtLostSalesEnv.py:291-296: DataFrame sums / mean of column means
        steps, dem, sales, stock = m[:, 1], m[:, 2], m[:, 3], m[:, 4]
        X = m[:, 5:]
        rows["AvgServiceLevel"] = np.array([s / max(1e-6, d) if d > 1e-6 else 1.0 for s, d in zip(sales, dem)])
        rows["TotalStockoutQty"] = stock
        rows["AvgEndingInv"] = np.array([np.sum(x / n) / x.shape[0] if n > 0 else np.nan
                                         for x, n in zip(X, steps)])
    return rows


def _gather_rows(met, n_episodes, world, rank, group):
    """All ranks' per-episode metric rows, in global episode order (one
    all_gather of a padded [ceil(n / world), M] block; RCCL for device tensors
    with the nccl backend, host tensors with gloo)."""
    import torch.distributed as dist
    from .distributed import shard_range
    nmax = -(-n_episodes // world)
    dev = met.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    pad = torch.zeros((nmax, met.shape[1]), dtype=torch.float64, device=dev)
    pad[:met.shape[0]] = met.to(dev)
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([parts[r][:shard_range(n_episodes, r, world)[1]] for r in range(world)]).cpu()


def evaluate_agent(agent, env_cls, env_config=None, n_episodes=100, seed_offset=0, device=None, group=None):
    """Batched evaluate_agent: episode i = env i seeded seed_offset + i, one
    full episode under ``agent`` in one kernel launch (a ``TorchPolicyAgent``:
    one launch per step, with the policy's torch ops between; an
    ``MLPPolicyAgent`` or ``GaussianMLPPolicyAgent``: two launches per step, issued by
    the library; the latter samples its actions).  Returns a dict of
    per-episode columns (the reference's summary DataFrame columns).

    Under torch.distributed (one process per GPU) the episodes are sharded by
    global index over the ranks of ``group`` (rank r runs episodes
    [offset_r, offset_r + n_r), seeded by global index as above) and every
    rank gets all episodes' columns, gathered in one collective; Time is the
    slowest rank's time per episode."""
    import torch.distributed as dist
    from .distributed import shard_range
    on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if on else 1
    rank = dist.get_rank(group) if on else 0
    off, n_loc = shard_range(n_episodes, rank, world)
    env = env_cls(num_envs=max(n_loc, 1), device=device, autoreset_mode="disabled", global_offset=off,
                  **(env_config or {}))
    try:
        obs0, _ = env.reset(seed=seed_offset)
        M = metrics_dim(env)
        met = torch.zeros((env.num_envs, M), dtype=torch.float64, device=env.device)
        torch.cuda.synchronize(env.device)
        t0 = time.perf_counter()
        rollout_policy(env, agent, env._horizon(), obs=False, rewards=False, metrics=met, obs0=obs0)
        torch.cuda.synchronize(env.device)
        dt = time.perf_counter() - t0
        met = met[:n_loc]
        family = env.family
        env_dev = env.device
    finally:
        env.close()
    if on:      # a 1-rank group too: the same collectives an N-GPU job runs
        met = _gather_rows(met, n_episodes, world, rank, group)
        # both collectives on the env's device (RCCL), or on the host (gloo)
        dev = env_dev if dist.get_backend(group) == "nccl" else torch.device("cpu")
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        dt = float(t.item())
    cols = summarize(family, met.cpu().numpy())
    n = n_episodes
    return {"Agent": [agent.name] * n, "Episode": np.arange(1, n + 1), **cols,
            "Time": np.full(n, dt / max(n, 1)), "Seed": seed_offset + np.arange(n), "Error": [None] * n}


def summary_table(results):
    """The reference's benchmark summary (process_and_report_results,
    benchmark_InvManagementBacklogEnv.py:474-516; the NetInvMgmt scripts'
    :333-353 are the same): per agent the mean / median / std / min / max
    episode reward, mean service level, stockout and ending inventory, time per
    episode, and episode counts, sorted by AvgReward.  ``results``: a list of
    evaluate_agent outputs.  Returns a pandas DataFrame indexed by Agent."""
    import pandas as pd
    raw = pd.concat([pd.DataFrame(r) for r in results], ignore_index=True)
    for c in ("AvgServiceLevel", "TotalStockoutQty", "AvgEndingInv"):
        if c not in raw:
            raw[c] = np.nan
    summary = raw.dropna(subset=["TotalReward"]).groupby("Agent").agg(
        AvgReward=("TotalReward", "mean"), MedianReward=("TotalReward", "median"),
        StdReward=("TotalReward", "std"), MinReward=("TotalReward", "min"), MaxReward=("TotalReward", "max"),
        AvgServiceLevel=("AvgServiceLevel", "mean"), AvgStockoutQty=("TotalStockoutQty", "mean"),
        AvgEndInv=("AvgEndingInv", "mean"), AvgTimePerEp=("Time", "mean"),
        SuccessfulEpisodes=("Episode", "count"))
    summary["TrainingTime(s)"] = 0.0                    # heuristic agents do not train
    summary["EpisodesAttempted"] = raw.groupby("Agent")["Episode"].count()
    summary["SuccessRate(%)"] = (summary["SuccessfulEpisodes"] / summary["EpisodesAttempted"]) * 100
    summary = summary.sort_values(by="AvgReward", ascending=False)
    return summary[["AvgReward", "MedianReward", "StdReward", "MinReward", "MaxReward", "AvgServiceLevel",
                    "AvgStockoutQty", "AvgEndInv", "AvgTimePerEp", "TrainingTime(s)", "SuccessfulEpisodes",
                    "EpisodesAttempted", "SuccessRate(%)"]]


def _levels_env(env_cls, env_config, n_cand, n_episodes, seed_offset, device):
    """One env of n_cand * n_episodes instances; instance c * n_episodes + r
    will run candidate c on seed seed_offset + r (the returned seed list)."""
    env = env_cls(num_envs=n_cand * n_episodes, device=device, autoreset_mode="disabled", **(env_config or {}))
    if env.family not in (_capi.INVSIM_INVMGMT, _capi.INVSIM_NETINVMGMT):
        env.close()
        raise TypeError("level policies need an InvManagement or NetInvMgmt env class")
    return env, [seed_offset + r for _ in range(n_cand) for r in range(n_episodes)]


def _levels_agent_cls(env):
    """the family's level policy: LevelsAgent (InvMgmt) or NetLevelsAgent (NetInvMgmt)"""
    return NetLevelsAgent if env.family == _capi.INVSIM_NETINVMGMT else LevelsAgent


def _levels_columns(family, met, n_cand, n_episodes):
    """summarize()'s columns as [C, R] and, under "candidates", the per-candidate
    means summary_table() reports, each [C] (StdReward: the sample standard
    deviation)."""
    cols = {k: np.ascontiguousarray(v.reshape(n_cand, n_episodes)) for k, v in summarize(family, met).items()}
    # one contiguous row at a time: the very sum np.mean takes over an evaluate_agent column
    mean = lambda a: np.array([np.mean(row) for row in a])  # noqa: E731
    cols["candidates"] = {
        "AvgReward": mean(cols["TotalReward"]),
        "StdReward": np.array([np.std(row, ddof=1) if n_episodes > 1 else np.nan for row in cols["TotalReward"]]),
        "AvgServiceLevel": mean(cols["AvgServiceLevel"]), "AvgEndingInv": mean(cols["AvgEndingInv"])}
    return cols


def evaluate_levels(levels, env_cls, env_config=None, n_episodes=100, seed_offset=0, reorder=None, device=None):
    """Score ``levels`` [C, A] (and ``reorder`` [C, A]) candidates under common
    random numbers: one env of ``C * n_episodes`` instances, instance ``c *
    n_episodes + r`` running candidate c on seed ``seed_offset + r``, one full
    episode in one launch, metrics only.  Returns a dict: ``TotalReward`` and
    the other ``summarize`` columns as ``[C, n_episodes]`` (row c equals
    ``evaluate_agent(LevelsAgent(levels[c]), ...)`` on the same seeds, bit for
    bit), and under ``"candidates"`` a dict of the per-candidate ``AvgReward``,
    ``StdReward``, ``AvgServiceLevel`` and ``AvgEndingInv``, each ``[C]`` (the
    means of those rows; the per-episode columns keep the two shared names).
    With a NetInvMgmt env class the candidates are ``NetLevelsAgent`` levels per
    reorder link and the columns are that family's ``summarize`` columns."""
    rows = lambda a: np.repeat(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a,  # noqa: E731
                                          np.float64), n_episodes, axis=0)
    lv = rows(levels)
    if lv.ndim != 2:
        raise ValueError(f"levels must be [C, A], got {np.shape(levels)}")
    n_cand = lv.shape[0] // n_episodes
    env, seeds = _levels_env(env_cls, env_config, n_cand, n_episodes, seed_offset, device)
    try:
        env.reset(seed=seeds)
        met = torch.zeros((env.num_envs, metrics_dim(env)), dtype=torch.float64, device=env.device)
        agent = _levels_agent_cls(env)(lv, None if reorder is None else rows(reorder))
        rollout_policy(env, agent, env._horizon(), obs=False, rewards=False, metrics=met)
        return _levels_columns(env.family, met.cpu().numpy(), n_cand, n_episodes)
    finally:
        env.close()


def tune_levels(env_cls, env_config=None, n_episodes=64, population=256, iterations=10, seed=0, seed_offset=0,
                init=None, elite_frac=0.1, device=None, max_level=None):
    """Cross-entropy search for the level vector with the best mean episode
    reward over seeds ``seed_offset .. seed_offset + n_episodes - 1``.

    One env of ``population * n_episodes`` instances and one levels tensor are
    made once; an iteration is ``reset(seed=<the same list>)``, an in-place
    rewrite of the levels tensor and one launch of one episode.  Candidates are
    drawn from a diagonal normal (a seeded ``torch.Generator``), clipped to
    ``[0, max_level]`` and refitted to the best ``elite_frac`` of them.
    ``max_level`` defaults per stage to ``max(3 * (L + 1) * mu, c)``: a few
    multiples of BaseStock's level, and never so low that an order of the full
    capacity ``c`` is out of reach.  Candidate 0 of every generation is the
    incumbent best (``init``, default the ``safety_factor = 1`` levels, in the
    first): the same seeds and levels give the same bits, so its score is
    reproduced exactly and the best score never decreases.  A NetInvMgmt env
    class searches ``NetLevelsAgent`` levels per reorder link: ``init`` defaults
    to ``NetLevelsAgent.from_mean_demand`` and ``max_level`` to the action
    space's ``high``.

    Returns a dict: ``levels`` [A] the best vector, ``TotalReward``
    [n_episodes] its per-episode rewards, ``history`` [iterations] the best
    ``AvgReward`` after each iteration."""
    if population < 2 or iterations < 1:
        raise ValueError("tune_levels needs population >= 2 and iterations >= 1")
    env, seeds = _levels_env(env_cls, env_config, population, n_episodes, seed_offset, device)
    try:
        A = env.action_dim
        if env.family == _capi.INVSIM_NETINVMGMT:
            base = np.asarray(NetLevelsAgent.from_mean_demand(env).levels, np.float64)
            hi = env._action_high().astype(np.float64)
        else:
            base = np.asarray((env.lead_time + 1) * env.dist_param.get("mu", 10), np.float64)
            hi = np.maximum(3.0 * base, env.supply_capacity.astype(np.float64))
        if max_level is not None:
            hi = np.broadcast_to(np.asarray(max_level, np.float64), (A,))
        hi = torch.from_numpy(np.ascontiguousarray(hi))
        best = torch.as_tensor(np.asarray(base if init is None else init, np.float64)).reshape(A).clone()
        mean, std = best.clone(), hi / 4
        gen = torch.Generator().manual_seed(int(seed))
        n_elite = max(2, int(round(elite_frac * population)))
        lv = torch.empty((env.num_envs, A), dtype=torch.float64, device=env.device)
        agent = _levels_agent_cls(env)(lv)
        met = torch.zeros((env.num_envs, metrics_dim(env)), dtype=torch.float64, device=env.device)
        history, best_rew = [], None
        for _ in range(iterations):
            cand = mean + std * torch.randn((population, A), dtype=torch.float64, generator=gen)
            cand = torch.minimum(torch.clamp(cand, min=0.0), hi)
            cand[0] = best
            env.reset(seed=seeds)
            lv.copy_(cand.repeat_interleave(n_episodes, dim=0))
            met.zero_()
            rollout_policy(env, agent, env._horizon(), obs=False, rewards=False, metrics=met)
            cols = _levels_columns(env.family, met.cpu().numpy(), population, n_episodes)
            avg = cols["candidates"]["AvgReward"]
            order = np.argsort(-avg, kind="stable")                     # (ties: the incumbent first)
            top = int(order[0])
            best, best_rew = cand[top].clone(), cols["TotalReward"][top].copy()
            history.append(float(avg[top]))
            elite = cand[torch.from_numpy(order[:n_elite].copy())]
            mean, std = elite.mean(dim=0), elite.std(dim=0).clamp_min(1e-3)
        return {"levels": best.numpy(), "TotalReward": best_rew, "history": np.asarray(history)}
    finally:
        env.close()
