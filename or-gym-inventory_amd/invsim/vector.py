"""Gymnasium-style VectorEnv base over libinvsim (one handle = N envs on one GPU).

Mirrors ``gymnasium.vector.VectorEnv``: ``num_envs``, ``single_observation_space``,
``single_action_space``, ``observation_space``, ``action_space``,
``reset(seed=, options=)`` and ``step(actions)``, with torch tensors on the GPU
in and out.  Seeding follows ``gymnasium.vector.SyncVectorEnv`` /
SB3 ``DummyVecEnv``: ``reset(seed=s)`` seeds env i with ``s + i``
(``benchmark_InvManagementBacklogEnv.py:264``); a list seeds env i with
``seed[i]``; ``None`` draws fresh OS entropy the first time and afterwards
continues the streams (gymnasium ``Env.reset(seed=None)``).

Autoreset modes (``gymnasium.vector.AutoresetMode``):

* ``"next_step"`` (default, gymnasium >= 1.0): the step after an env is done
  resets it, ignoring its action, and returns the reset obs with reward 0.
* ``"same_step"`` (SB3 VecEnv): the done step returns the reset obs, the
  terminal obs is in ``info["final_obs"]`` (mask ``info["_final_obs"]``).
* ``"disabled"``: the caller resets; stepping an InvMgmt/NetInvMgmt env past
  its horizon raises IndexError as the reference does
  (``inventory_management.py:267``).

Demand stream (``demand_stream=``): ``"numpy"`` (default) draws from numpy's
PCG64 Generator stream, bit-exact with the reference on the same seeds;
``"philox"`` is the opt-in, non-parity fast stream (rocRAND Philox4x32-10,
counter-based: no per-env generator state per step; ``include/invsim.h``).
"""
import os

import numpy as np
import torch

from . import _capi
from .spaces import batch_box


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _to_device_index(device):
    if device is None:
        return torch.cuda.current_device()
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"invsim runs on a ROCm GPU (torch 'cuda' device), got {d}")
    return d.index if d.index is not None else torch.cuda.current_device()


def _seed_words(seeds):
    seeds = [int(s) for s in seeds]
    words = np.zeros((len(seeds), 4), np.uint32)
    nw = np.zeros(len(seeds), np.int32)
    for i, s in enumerate(seeds):
        if s < 0 or s >= 2**128:
            raise ValueError("seeds must be integers in [0, 2**128)")
        k = 0
        while True:
            words[i, k] = s & 0xFFFFFFFF
            k += 1
            s >>= 32
            if s == 0:
                break
        nw[i] = k
    return words, nw


class InvSimVectorEnv:
    """Base class; subclasses build the spec and the single-env spaces."""

    family = None
    metadata = {"autoreset_mode": "next_step"}
    obs_dtype = torch.float32
    act_dtype = torch.float32

    def __init__(self, num_envs, device=None, autoreset_mode="next_step", global_offset=0,
                 record_demand=False, record_info=False, copy=True, demand_stream="numpy"):
        if not torch.cuda.is_available():
            raise RuntimeError("invsim requires a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        if autoreset_mode not in _capi.AUTORESET_MODES:
            raise ValueError(f"autoreset_mode must be one of {sorted(_capi.AUTORESET_MODES)}")
        self.num_envs = int(num_envs)
        self.global_offset = int(global_offset)
        self.device_index = _to_device_index(device)
        self.device = torch.device("cuda", self.device_index)
        self.autoreset_mode = autoreset_mode
        self.copy = bool(copy)
        self._lib = _capi.lib()
        self._h = None
        self._create()
        od, ad, dd, fam = (_capi.C.c_int32() for _ in range(4))
        _capi.check(self._lib.invsim_dims(self._h, _capi.C.byref(od), _capi.C.byref(ad),
                                          _capi.C.byref(dd), _capi.C.byref(fam)), self._h, "dims")
        self.obs_dim, self.action_dim, self.demand_dim = od.value, ad.value, dd.value
        self.observation_space = batch_box(self.single_observation_space, self.num_envs)
        self.action_space = batch_box(self.single_action_space, self.num_envs)
        self.set_demand_stream(demand_stream)
        self._seeded = False
        self._demand = None
        if record_demand:
            self._demand = torch.zeros((self.num_envs, self.demand_dim), dtype=torch.int64,
                                       device=self.device)
            _capi.check(self._lib.invsim_set_info_demand(self._h, self._demand.data_ptr()),
                        self._h, "set_info_demand")
        self._rec = None
        if record_info:
            d = _capi.C.c_int32()
            _capi.check(self._lib.invsim_info_record_dim(self._h, _capi.C.byref(d)), self._h, "info_record_dim")
            if d.value == 0:
                raise ValueError("record_info: this env family keeps no step record")
            rdt = torch.int64 if self.family == _capi.INVSIM_INVMGMT else torch.float64
            self._rec = torch.zeros((self.num_envs, d.value), dtype=rdt, device=self.device)
            _capi.check(self._lib.invsim_set_info_record(self._h, self._rec.data_ptr()), self._h, "set_info_record")
        self._out = None
        self._arng = None     # RandomAgent's action generators (seed_actions)
        self._levels = None   # LevelsAgent's attached (levels, reorder) tensors (_attach_policy_levels)
        self._mlps = []       # invsim_mlp objects of MLPPolicyAgents that met this env (destroyed in close)

    def _record_info(self, info):
        """Decode the per-step record into the reference's step-info names."""
        rec = self._rec.clone()
        if self.family == _capi.INVSIM_INVMGMT:
            m = (rec.shape[1] - 5) // 2
            info["sales"] = rec[:, :m]
            info["unfulfilled"] = rec[:, m:2 * m]
            f = rec[:, 2 * m:].view(torch.float64)
            for i, k in enumerate(("period_profit", "revenue", "procurement_cost", "holding_cost", "penalty_cost")):
                info[k] = f[:, i]
        elif self.family == _capi.INVSIM_NEWSVENDOR:
            # newsvendor.py:195-199; kinds: 0 Python float, 1 np.float32, 2 np.float64, 3 Python int
            kinds = rec[:, 4].to(torch.int64)
            for i, k in enumerate(("revenue", "purchase_cost", "holding_cost", "lost_sales_penalty")):
                info[k] = rec[:, i]
                info[k + "_kind"] = (kinds // (4 ** i)) % 4
        else:
            RL, J, E = len(self.retail_links), len(self.main_nodes), len(self.reorder_links)
            o = 0
            for k, w in (("sales", RL), ("unfulfilled", RL), ("inventory", J), ("replenishment", E),
                         ("pipeline", E), ("profit", J)):
                info[k] = rec[:, o:o + w]   # S[t], U[t+1] (retail links); X[t+1]; R[t], Y[t+1]; P[t]
                o += w
        return info

    # -- subclass hooks ------------------------------------------------------
    def _create(self):
        raise NotImplementedError

    def _horizon(self):
        raise NotImplementedError

    def _create_handle(self, fn, spec):
        h = _capi.C.c_void_p()
        rc = fn(_capi.C.byref(spec), self.num_envs, self.device_index,
                _capi.AUTORESET_MODES[self.autoreset_mode], _capi.C.byref(h))
        if rc != 0:
            raise _capi.InvsimError(f"invsim create failed ({rc}): {_capi.last_error(None)}")
        self._h = h

    # -- helpers --------------------------------------------------------------
    def _stream(self):
        # the raw hipStream_t of torch's current stream on this device (the
        # public torch.cuda.current_stream(dev).cuda_stream costs ~3 us a call)
        if _raw_stream is not None:
            return _raw_stream(self.device_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def _mask_ptr(self, mask):
        if mask is None:
            return None, None
        m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if m.shape != (self.num_envs,):
            raise ValueError(f"reset_mask must have shape ({self.num_envs},)")
        return m, m.data_ptr()

    def _alloc(self, *shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _outputs(self):
        N, O = self.num_envs, self.obs_dim
        if self.copy or self._out is None:
            self._out = (self._alloc(N, O, dtype=self.obs_dtype),
                         self._alloc(N, dtype=torch.float64),
                         self._alloc(N, dtype=torch.bool),
                         self._alloc(N, dtype=torch.bool))
        return self._out

    def _actions(self, actions, lead_shape):
        a = actions
        if (type(a) is torch.Tensor and a.dtype == self.act_dtype and a.device == self.device
                and a.is_contiguous() and a.shape == tuple(lead_shape) + (self.action_dim,)):
            return a                                         # already in the kernel's layout
        a = torch.as_tensor(actions)
        shape = tuple(lead_shape) + (self.action_dim,)
        if a.shape != shape:
            if a.numel() == int(np.prod(shape)):
                a = a.reshape(shape)
            else:
                raise ValueError(f"actions must have shape {shape}, got {tuple(a.shape)}")
        return self._convert_actions(a.to(self.device)).contiguous()

    def _convert_actions(self, a):
        return a.to(self.act_dtype)

    # -- public API ------------------------------------------------------------
    def seed(self, seed=None):
        """Re-seed the env RNGs without resetting (gymnasium seeding.np_random)."""
        s = self._stream()
        if seed is None:
            ent = np.frombuffer(os.urandom(16 * self.num_envs), dtype=np.uint32).reshape(-1, 4)
            words = torch.from_numpy(ent.copy()).to(self.device)
            nw = torch.full((self.num_envs,), 4, dtype=torch.int32, device=self.device)
            _capi.check(self._lib.invsim_seed_words(self._h, words.data_ptr(), nw.data_ptr(), None, s),
                        self._h, "seed_words")
        elif isinstance(seed, (int, np.integer)):
            seed = int(seed)
            if seed < 0 or seed >= 2**128:
                raise ValueError("seed must be in [0, 2**128)")
            _capi.check(self._lib.invsim_seed_range(self._h, seed & (2**64 - 1), seed >> 64,
                                                    self.global_offset, None, s),
                        self._h, "seed_range")
        else:
            seeds = list(seed)
            if len(seeds) != self.num_envs:
                raise ValueError(f"expected {self.num_envs} seeds, got {len(seeds)}")
            w, nw = _seed_words(seeds)
            words = torch.from_numpy(w).to(self.device)
            nwt = torch.from_numpy(nw).to(self.device)
            _capi.check(self._lib.invsim_seed_words(self._h, words.data_ptr(), nwt.data_ptr(), None, s),
                        self._h, "seed_words")
        self._seeded = True

    def reset(self, *, seed=None, options=None):
        mask = (options or {}).get("reset_mask")
        if seed is not None or not self._seeded:
            if mask is not None and seed is not None:
                raise ValueError("seed together with reset_mask is not supported; seed first")
            self.seed(seed)
        m, mp = self._mask_ptr(mask)
        obs = self._alloc(self.num_envs, self.obs_dim, dtype=self.obs_dtype)
        _capi.check(self._lib.invsim_reset(self._h, mp, obs.data_ptr(), self._stream()), self._h, "reset")
        # with a reset_mask, rows of envs that were not reset are left unwritten in `obs`
        return obs, {}

    def step(self, actions):
        a = self._actions(actions, (self.num_envs,))
        obs, rew, term, trunc = self._outputs()
        fobs = None
        if self.autoreset_mode == "same_step":
            fobs = self._alloc(self.num_envs, self.obs_dim, dtype=self.obs_dtype)
        _capi.check(self._lib.invsim_step(self._h, a.data_ptr(), obs.data_ptr(), rew.data_ptr(),
                                          term.data_ptr(), trunc.data_ptr(),
                                          fobs.data_ptr() if fobs is not None else None,
                                          self._stream()), self._h, "step")
        info = {}
        if fobs is not None:
            info["final_obs"] = fobs
            info["_final_obs"] = trunc
        if self._demand is not None:
            info["demand"] = self._demand.clone() if self.demand_dim > 1 else self._demand[:, 0].clone()
        if self._rec is not None:
            self._record_info(info)
        return obs, rew, term, trunc, info

    def rollout(self, actions):
        """K consecutive steps in ONE kernel launch.  actions [K, N, A] ->
        obs [K, N, O], reward [K, N], terminated [K, N], truncated [K, N].
        Identical to K step() calls (next_step / disabled autoreset)."""
        a = torch.as_tensor(actions)
        K = int(a.shape[0])
        a = self._actions(a, (K, self.num_envs))
        N, O = self.num_envs, self.obs_dim
        obs = self._alloc(K, N, O, dtype=self.obs_dtype)
        rew = self._alloc(K, N, dtype=torch.float64)
        term = self._alloc(K, N, dtype=torch.bool)
        trunc = self._alloc(K, N, dtype=torch.bool)
        _capi.check(self._lib.invsim_rollout(self._h, K, a.data_ptr(), obs.data_ptr(), rew.data_ptr(),
                                             term.data_ptr(), trunc.data_ptr(), self._stream()),
                    self._h, "rollout")
        return obs, rew, term, trunc

    def rollout_policy(self, agent, K, obs=False, rewards=True, actions=False, metrics=None, obs0=None):
        """K steps with the agent's actions computed in the kernel, or in torch
        for a TorchPolicyAgent (which needs obs0; see invsim.policies);
        outputs optional, metrics [N, M] accumulated."""
        from .policies import rollout_policy
        return rollout_policy(self, agent, K, obs=obs, rewards=rewards, actions=actions, metrics=metrics,
                              obs0=obs0)

    def _rollout_metrics(self, K, a, obs, rew, term, trunc, metrics):
        """invsim_rollout_metrics on tensors in the kernel's layout (any output may be None)."""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _capi.check(self._lib.invsim_rollout_metrics(self._h, int(K), a.data_ptr(), p(obs), p(rew), p(term),
                                                     p(trunc), p(metrics), self._stream()),
                    self._h, "rollout_metrics")

    def _metrics_arg(self, metrics):
        if metrics is None:
            return None
        if getattr(self, "_mdim", None) is None:
            d = _capi.C.c_int32()
            _capi.check(self._lib.invsim_metrics_dim(self._h, _capi.C.byref(d)), self._h, "metrics_dim")
            self._mdim = d.value
        if (type(metrics) is not torch.Tensor or metrics.dtype != torch.float64 or metrics.device != self.device
                or not metrics.is_contiguous() or tuple(metrics.shape) != (self.num_envs, self._mdim)):
            raise ValueError(f"metrics must be a contiguous float64 tensor [{self.num_envs}, {self._mdim}] on {self.device}")
        return metrics

    def rollout_metrics(self, actions, metrics=None, obs=True, rewards=True):
        """K consecutive steps with the caller's actions [K, N, A], as
        rollout(), that also add evaluate_agent's per-env sums to ``metrics``
        (float64 [N, M], in place), as rollout_policy() does for its in-kernel
        agents: the entry point for policies computed outside the kernels and
        for scoring open-loop action plans.  Returns a dict with the requested
        device tensors: "obs" [K, N, O]; "reward", "terminated", "truncated"
        [K, N].  next_step / disabled autoreset."""
        a = torch.as_tensor(actions)
        K = int(a.shape[0])
        a = self._actions(a, (K, self.num_envs))
        metrics = self._metrics_arg(metrics)
        N = self.num_envs
        out = {}
        o = self._alloc(K, N, self.obs_dim, dtype=self.obs_dtype) if obs else None
        if rewards:
            out["reward"] = self._alloc(K, N, dtype=torch.float64)
            out["terminated"] = self._alloc(K, N, dtype=torch.bool)
            out["truncated"] = self._alloc(K, N, dtype=torch.bool)
        self._rollout_metrics(K, a, o, out.get("reward"), out.get("terminated"), out.get("truncated"), metrics)
        if obs:
            out["obs"] = o
        return out

    def mlp_actions(self, agent, obs, raw=False):
        """One launch of an MLPPolicyAgent's network on obs [N, O] (the env's obs
        dtype): the actions [N, A] in the action dtype, or with ``raw=True`` the
        pair (actions, the float32 outputs before clipping and casting).  Env
        state is not touched."""
        o = torch.as_tensor(obs, device=self.device)
        if tuple(o.shape) != (self.num_envs, self.obs_dim):
            raise ValueError(f"obs must have shape {(self.num_envs, self.obs_dim)}, got {tuple(o.shape)}")
        o = o.to(self.obs_dtype).contiguous()
        obj = agent.device_object(self)
        a = self._alloc(self.num_envs, self.action_dim, dtype=self.act_dtype)
        r = self._alloc(self.num_envs, self.action_dim, dtype=torch.float32) if raw else None
        _capi.check(self._lib.invsim_mlp_actions(self._h, obj, o.data_ptr(), a.data_ptr(),
                                                 r.data_ptr() if raw else None, self._stream()),
                    self._h, "mlp_actions")
        return (a, r) if raw else a

    def mlp_sample(self, agent, obs):
        """One sampling launch of a GaussianMLPPolicyAgent on obs [N, O]: a dict
        with "actions" [N, A] (action dtype), "raw_actions" and "mean" [N, A]
        float32 (the sample before conversion, the network's output) and
        "log_prob" [N] float32.  Every env's action generator advances by A
        normals; env state is not touched."""
        o = torch.as_tensor(obs, device=self.device)
        if tuple(o.shape) != (self.num_envs, self.obs_dim):
            raise ValueError(f"obs must have shape {(self.num_envs, self.obs_dim)}, got {tuple(o.shape)}")
        o = o.to(self.obs_dtype).contiguous()
        obj = agent.device_object(self)
        N, A = self.num_envs, self.action_dim
        out = {"actions": self._alloc(N, A, dtype=self.act_dtype), "raw_actions": self._alloc(N, A, dtype=torch.float32),
               "mean": self._alloc(N, A, dtype=torch.float32), "log_prob": self._alloc(N, dtype=torch.float32)}
        _capi.check(self._lib.invsim_mlp_sample(self._h, obj, o.data_ptr(), out["actions"].data_ptr(),
                                                out["raw_actions"].data_ptr(), out["mean"].data_ptr(),
                                                out["log_prob"].data_ptr(), self._stream()),
                    self._h, "mlp_sample")
        return out

    def _mlp_values_into(self, critic, obs, rows, out):
        """invsim_mlp_values: `rows` contiguous obs rows (obs dtype) -> the contiguous float32 tensor `out`"""
        _capi.check(self._lib.invsim_mlp_values(self._h, critic.device_object(self), obs.data_ptr(), int(rows),
                                                out.data_ptr(), self._stream()), self._h, "mlp_values")

    def mlp_values(self, critic, obs):
        """One launch of a ValueMLP on obs [..., O] (the env's obs dtype, any
        number of leading dimensions: a whole [K, N, O] block at once): the
        values, float32 [...].  Env state is not touched."""
        o = torch.as_tensor(obs, device=self.device)
        if o.dim() < 1 or o.shape[-1] != self.obs_dim:
            raise ValueError(f"obs must have shape [..., {self.obs_dim}], got {tuple(o.shape)}")
        o = o.to(self.obs_dtype).contiguous()
        v = self._alloc(*o.shape[:-1], dtype=torch.float32)
        self._mlp_values_into(critic, o, v.numel(), v)
        return v

    # -- RandomAgent's action stream (include/invsim.h "RandomAgent") ----------
    def _action_high(self):
        """The action space's upper bounds in the action dtype (host array)."""
        sp = self.single_action_space
        return np.ascontiguousarray(np.asarray(sp.high, dtype=sp.dtype).reshape(-1))

    def _attach_action_rng(self, buf):
        _capi.check(self._lib.invsim_set_action_rng(self._h, buf.data_ptr() if buf is not None else None),
                    self._h, "set_action_rng")
        self._arng = buf

    def _attach_policy_levels(self, levels, reorder=None):
        """Attach the LEVELS policy's device tensors (float64 [N, A]); they stay
        alive here while attached.  Nothing to do when they already are.  On a
        NetInvMgmt env they are the NET_LEVELS policy's (a handle is of one
        family, so one slot holds either)."""
        cur = self._levels
        if cur is not None and cur[0] is levels and cur[1] is reorder:
            return
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        net = self.family == _capi.INVSIM_NETINVMGMT
        attach = self._lib.invsim_set_policy_net_levels if net else self._lib.invsim_set_policy_levels
        _capi.check(attach(self._h, p(levels), p(reorder)), self._h,
                    "set_policy_net_levels" if net else "set_policy_levels")
        self._levels = (levels, reorder) if levels is not None else None

    def seed_actions(self, seed):
        """Allocate, seed and attach the per-env action generators: env i draws
        its random actions from ``Generator(PCG64(SeedSequence(2**64 + seed +
        global_offset + i)))``, a stream separate from the demand generator."""
        seed = int(seed)
        if seed < 0 or seed >= 2**64:
            raise ValueError("action seed must be in [0, 2**64)")
        b = _capi.C.c_int64()
        _capi.check(self._lib.invsim_action_rng_bytes(self._h, _capi.C.byref(b)), self._h, "action_rng_bytes")
        buf = torch.zeros((4, b.value // 32), dtype=torch.int64, device=self.device)
        _capi.check(self._lib.invsim_seed_action_rng(self._h, buf.data_ptr(), seed, 1, self.global_offset,
                                                     self._stream()), self._h, "seed_action_rng")
        self._attach_action_rng(buf)

    def sample_actions(self, K):
        """K steps of random actions [K, N, A] (action dtype) from the attached
        action generators, which advance as a RandomAgent rollout of K steps would."""
        a = self._alloc(int(K), self.num_envs, self.action_dim, dtype=self.act_dtype)
        high = self._action_high()
        _capi.check(self._lib.invsim_sample_actions(self._h, int(K), high.ctypes.data, a.data_ptr(), self._stream()),
                    self._h, "sample_actions")
        return a

    def action_rng_state(self):
        """A clone of the action generators, int64 [4, Npad] (rows state hi / state
        lo / inc hi / inc lo): the action stream's checkpoint."""
        if getattr(self, "_arng", None) is None:
            raise RuntimeError("no action generators: call seed_actions(seed) first")
        return self._arng.clone()

    def set_action_rng_state(self, t):
        """Attach a copy of ``t`` (as returned by action_rng_state) as the action generators."""
        t = torch.as_tensor(t, device=self.device)
        b = _capi.C.c_int64()
        _capi.check(self._lib.invsim_action_rng_bytes(self._h, _capi.C.byref(b)), self._h, "action_rng_bytes")
        if t.dtype != torch.int64 or tuple(t.shape) != (4, b.value // 32):
            raise ValueError(f"action generator state must be int64 [4, {b.value // 32}]")
        self._attach_action_rng(t.contiguous().clone())

    def status(self, clear=True):
        """Sticky device status word (synchronous): bit 0 = an env was stepped past its
        horizon with autoreset disabled after a masked reset (the step was not applied).
        step()/rollout() already check it in that mode and raise IndexError."""
        f = _capi.C.c_uint32()
        _capi.check(self._lib.invsim_status(self._h, _capi.C.byref(f), int(clear)), self._h, "status")
        return f.value

    def set_demand_stream(self, mode):
        """"numpy" (parity, default) or "philox" (fast, NOT the reference's draws)."""
        if mode not in _capi.DEMAND_STREAMS:
            raise ValueError(f"demand_stream must be one of {sorted(_capi.DEMAND_STREAMS)}")
        _capi.check(self._lib.invsim_set_demand_stream(self._h, _capi.DEMAND_STREAMS[mode]), self._h,
                    "set_demand_stream")

    @property
    def demand_stream(self):
        """The stream the handle draws demands from ("numpy" or "philox")."""
        m = _capi.C.c_int32()
        _capi.check(self._lib.invsim_demand_stream(self._h, _capi.C.byref(m)), self._h, "demand_stream")
        return {v: k for k, v in _capi.DEMAND_STREAMS.items()}[m.value]

    @property
    def kernel_variant(self):
        """0 = generic kernel; 1 / 2 = NetInvMgmt kernel specialised for the
        reference's default / custom supply network."""
        v = _capi.C.c_int32()
        _capi.check(self._lib.invsim_kernel_variant(self._h, _capi.C.byref(v)), self._h, "kernel_variant")
        return v.value

    def position(self):
        """Opaque token of the host-side position (lock-step period, lookahead
        slot) that picks each launch's kernel; see invsim.graphs."""
        p = _capi.C.c_int64()
        _capi.check(self._lib.invsim_position(self._h, _capi.C.byref(p)), self._h, "position")
        return p.value

    def capture(self, fn, warmup=1, pool=None):
        """Record fn() (a policy's torch ops + calls on this env) as one HIP
        graph: returns an invsim.graphs.StepGraph whose replay() reruns it."""
        from .graphs import StepGraph
        return StepGraph(self, fn, warmup=warmup, pool=pool)

    # -- state -----------------------------------------------------------------
    def state_bytes(self):
        b = _capi.C.c_int64()
        _capi.check(self._lib.invsim_state_bytes(self._h, _capi.C.byref(b)), self._h, "state_bytes")
        return b.value

    def get_state(self):
        """Checkpoint: the whole device state (RNG streams included) as a uint8 tensor."""
        buf = torch.empty(self.state_bytes(), dtype=torch.uint8, device=self.device)
        _capi.check(self._lib.invsim_get_state(self._h, buf.data_ptr(), self._stream()), self._h, "get_state")
        return buf

    def set_state(self, buf):
        buf = torch.as_tensor(buf, device=self.device).contiguous()
        if buf.dtype != torch.uint8 or buf.numel() != self.state_bytes():
            raise ValueError("state blob does not match this env's layout")
        _capi.check(self._lib.invsim_set_state(self._h, buf.data_ptr(), self._stream()), self._h, "set_state")
        self._seeded = True

    def state_fields(self, blob=None):
        """Decode a state blob into {name: tensor[rows, N]} views (debug / tests)."""
        blob = self.get_state() if blob is None else blob
        out = {}
        i = 0
        dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        while True:
            name = _capi.C.create_string_buffer(32)
            off, eb, rows, stride = _capi.C.c_int64(), _capi.C.c_int32(), _capi.C.c_int32(), _capi.C.c_int64()
            rc = self._lib.invsim_state_field(self._h, i, name, _capi.C.byref(off), _capi.C.byref(eb),
                                              _capi.C.byref(rows), _capi.C.byref(stride))
            if rc != 0:
                break
            r_, st_ = rows.value, stride.value
            if st_ > 0:     # [rows][stride]
                raw = blob[off.value: off.value + r_ * st_ * eb.value].view(dt[eb.value]).view(r_, st_)
                out[name.value.decode()] = raw[:, : self.num_envs] if st_ > 1 else raw
            elif st_ < 0:   # record layout [Npad][rows] -> [rows, N] view
                raw = blob[off.value: off.value + r_ * -st_ * eb.value].view(dt[eb.value]).view(-st_, r_)
                out[name.value.decode()] = raw[: self.num_envs].t()
            i += 1
        return out

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            for m in getattr(self, "_mlps", ()):
                self._lib.invsim_mlp_destroy(m)
            self._mlps = []
            self._lib.invsim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        return f"{type(self).__name__}(num_envs={self.num_envs}, device={self.device})"
