"""GPU: the critic, GAE and parameter-update calls (include/invsim.h "Critic,
GAE and parameter updates") against their CPU restatements: invsim_gae against
tests/gae_model.py bit for bit, invsim_mlp_values against tests/mlp_model.py,
invsim_mlp_update against an object created from the new parameters, and
collect_rollout(critic=...) end to end on all three env families, per-env
periods and a captured update -> values -> GAE chain included."""
import ctypes as C

import numpy as np
import pytest
import torch

import gae_model
import gaussian_model as gm
import mlp_model
import staggered

pytestmark = pytest.mark.gpu

N, K = 197, 20                # three full 64-env groups and a last group of 5
SEED = 400
F32 = np.float32
EINVAL = -22
KEYS = ("obs", "reward", "terminated", "truncated", "actions", "raw_actions", "log_prob")
GL = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.0), (0.98, 0.0)]


# ---------------------------------------------------------------- helpers
def _cls_kw(name):
    import invsim
    if name == "im":
        return invsim.InvManagementBacklogEnv, dict(periods=7)
    if name == "nv":
        return invsim.NewsvendorEnv, dict(step_limit=6)
    from invsim.topology import default_graph
    return invsim.NetInvMgmtMasterEnv, dict(graph=default_graph(), num_periods=6, backlog=True)


def _make(gpu, name, n=N, **vec):
    cls, kw = _cls_kw(name)
    env = cls(n, device=gpu, **kw, **vec)
    obs0, _ = env.reset(seed=SEED)
    return env, obs0


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    if t.dtype == torch.bool:
        return t.to(torch.uint8).numpy()
    return t.numpy()


def _same(a, b, what, nan_ok=False):
    """the same bits (nan_ok: a NaN equals any NaN, and only a NaN: the sign and
    payload of a NaN are the arithmetic unit's, as in tests/test_gpu_mlp_policy.py)"""
    assert tuple(a.shape) == tuple(b.shape), f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    x, y = _bits(a), _bits(b)
    assert x.dtype == y.dtype, f"{what}: {x.dtype} vs {y.dtype}"
    ne = x != y
    if nan_ok:
        fa = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        fb = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
        ne &= ~(np.isnan(fa) & np.isnan(fb))
    if ne.any():
        pytest.fail(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[:4].tolist()}")


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _layers(dims, rng):
    return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (rng.standard_normal(o) * 0.25).astype(F32))
            for i, o in zip(dims[:-1], dims[1:])]


def _in_scale(O, rng):
    return dict(in_scale=(0.01 * (1 + 0.1 * rng.standard_normal(O))).astype(F32),
                in_shift=(0.1 * rng.standard_normal(O)).astype(F32))


def _critic(env, hidden=(16,), seed=21, activation="relu", scales=True):
    import invsim
    rng = np.random.default_rng(seed)
    kw = {}
    if scales:
        kw = dict(_in_scale(env.obs_dim, rng), out_scale=np.array([37.5], F32), out_shift=np.array([-3.25], F32))
    return invsim.ValueMLP(_layers([env.obs_dim] + list(hidden) + [1], rng), activation=activation, **kw)


def _actor(env, hidden=(16,), seed=11, aseed=0, log_std=None):
    import invsim
    rng = np.random.default_rng(seed)
    sp = env.single_action_space
    high = np.asarray(sp.high, dtype=np.float64).reshape(-1)
    high = np.where(np.isfinite(high), high, 1000.0)
    ls = np.log(0.2 * high).astype(F32) if log_std is None else log_std
    return invsim.GaussianMLPPolicyAgent(_layers([env.obs_dim] + list(hidden) + [env.action_dim], rng), log_std=ls,
                                         seed=aseed, activation="relu", out_scale=(1.5 * high).astype(F32),
                                         out_shift=(0.5 * high).astype(F32), **_in_scale(env.obs_dim, rng))


def _obs(env, rows, seed=1):
    """synthetic observations of the env's dtype: int64 ones include values float32 cannot hold"""
    rng = np.random.default_rng(seed)
    O = env.obs_dim
    if env.obs_dtype == torch.int64:
        o = rng.integers(0, 400, (rows, O))
        o[::23, 1] = 2 ** 24 + 1
        o[::31, 0] = -(2 ** 40) - 2 ** 15 - 1
        return torch.from_numpy(o).to(env.device)
    return torch.from_numpy(rng.uniform(0, 400, (rows, O)).astype(F32)).to(env.device)


def _model_gae(out_or_case, gamma, lam, done0=None, value0=None, values=None):
    c = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out_or_case.items()}
    d0 = done0.cpu().numpy() if isinstance(done0, torch.Tensor) else done0
    return gae_model.gae(c["reward"], c["terminated"], c["truncated"], d0, value0, values, gamma, lam)


# ---------------------------------------------------------------- 1. invsim_gae, synthetic
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2048])
@pytest.mark.parametrize("Kk", [1, 2, 3, 5, 9, 31])
def test_gae_kernel_bit_exact(gpu, Kk, n):
    """every remainder of the row blocking, partial waves and several workgroups,
    every flag pattern of gae_model.synthetic, each flag array absent"""
    import invsim
    for seed, (gamma, lam) in enumerate(GL):
        c = gae_model.synthetic(Kk, n, seed=seed)
        for drop in (None, "terminated", "truncated", "done0"):
            d = dict(c, **({drop: None} if drop else {}))
            out = invsim.policies.gae(_dev(gpu, d["reward"]), _dev(gpu, d["terminated"]), _dev(gpu, d["truncated"]),
                                      _dev(gpu, d["value0"]), _dev(gpu, d["values"]), gamma, lam,
                                      done0=_dev(gpu, d["done0"]))
            adv, ret, valid = gae_model.gae(d["reward"], d["terminated"], d["truncated"], d["done0"], d["value0"],
                                            d["values"], gamma, lam)
            what = f"K={Kk} n={n} gamma={gamma} lambda={lam} without {drop}"
            assert out["valid"].dtype == torch.bool
            _same(out["valid"], valid, f"{what}: valid")
            _same(out["advantages"], adv, f"{what}: advantages", nan_ok=True)
            _same(out["returns"], ret, f"{what}: returns", nan_ok=True)
    if n == 2048 and Kk == 31:
        assert np.isnan(adv).any() and np.isinf(adv).any() and (valid == 0).any(), "the special values reach the outputs"


def test_gae_validation_and_null_valid(gpu):
    import invsim
    from invsim import _capi
    lib = _capi.lib()
    Kk, n = 5, 130
    c = gae_model.synthetic(Kk, n, seed=2)
    t = {k: _dev(gpu, v) for k, v in c.items()}
    adv = torch.full((Kk, n), 7.0, dtype=torch.float32, device=gpu)
    ret, valid = adv.clone(), torch.full((Kk, n), 7, dtype=torch.uint8, device=gpu)
    s = torch.cuda.current_stream(gpu).cuda_stream
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(Kk=Kk, n=n, gamma=0.99, lam=0.95, **over):
        a = dict(reward=t["reward"], terminated=t["terminated"], truncated=t["truncated"], done0=t["done0"],
                 value0=t["value0"], values=t["values"], adv=adv, ret=ret, valid=valid)
        a.update(over)
        return lib.invsim_gae(p(a["reward"]), p(a["terminated"]), p(a["truncated"]), p(a["done0"]), p(a["value0"]),
                              p(a["values"]), Kk, n, gamma, lam, p(a["adv"]), p(a["ret"]), p(a["valid"]), s)
    # refused or empty: nothing is written
    assert call(Kk=-1) == EINVAL and call(n=-1) == EINVAL
    for name in ("reward", "value0", "values", "adv", "ret"):
        assert call(**{name: None}) == EINVAL, name
    assert call(Kk=0) == 0 and call(n=0) == 0
    assert call(Kk=0, reward=None, values=None, adv=None) == 0, "nothing is required of an empty block"
    torch.cuda.synchronize(gpu)
    assert bool((adv == 7).all()) and bool((ret == 7).all()) and bool((valid == 7).all())
    # valid = NULL: the same advantages and returns, valid untouched
    assert call(valid=None) == 0
    e_adv, e_ret, e_valid = gae_model.gae(c["reward"], c["terminated"], c["truncated"], c["done0"], c["value0"],
                                          c["values"], 0.99, 0.95)
    _same(adv, e_adv, "valid = NULL: advantages", nan_ok=True), _same(ret, e_ret, "valid = NULL: returns", nan_ok=True)
    assert bool((valid == 7).all())
    assert call() == 0
    _same(valid, e_valid, "valid")
    # the Python wrapper: bool flags, K = 0, shapes
    out = invsim.policies.gae(t["reward"], t["terminated"].bool(), t["truncated"].bool(), t["value0"], t["values"],
                              done0=t["done0"].bool())
    _same(out["advantages"], e_adv, "bool flags", nan_ok=True)
    empty = invsim.policies.gae(t["reward"][:0], None, None, t["value0"], t["values"][:0])
    assert all(tuple(empty[k].shape) == (0, n) for k in ("advantages", "returns", "valid"))
    with pytest.raises(ValueError):
        invsim.policies.gae(t["reward"], None, None, t["value0"][:-1], t["values"])


# ---------------------------------------------------------------- 2. invsim_mlp_values
@pytest.mark.parametrize("name", ["im", "nv", "net"])
@pytest.mark.parametrize("hidden", [(16,), (64, 64), (128,)], ids=["16", "64x64", "128"])
def test_values_bit_exact(gpu, name, hidden):
    """ReLU critics (128: the 8-wave launch), int64 and f32 observations, rows
    independent of the handle's N, with and without the scales"""
    env, _ = _make(gpu, name)
    for scales in (True, False):
        critic = _critic(env, hidden, seed=5 + scales, scales=scales)
        for rows in (0, 1, 1000, (K + 1) * N):
            obs = _obs(env, rows, seed=rows + 1)
            v = env.mlp_values(critic, obs)
            assert v.dtype == torch.float32 and tuple(v.shape) == (rows,)
            if rows:
                _same(v, mlp_model.forward(critic, obs.cpu().numpy())[:, 0], f"{name} {hidden} scales={scales} rows={rows}")
    blk = _obs(env, (K + 1) * N, seed=9).reshape(K + 1, N, env.obs_dim)
    v = env.mlp_values(critic, blk)
    assert tuple(v.shape) == (K + 1, N)
    _same(v[3], env.mlp_values(critic, blk[3]), "a [K + 1, N, O] block is its rows")


def test_values_at_31_times_2_20_rows(gpu):
    """the largest block the issue names, [31][1 048 576][33] int64 observations in
    one launch: 507 904 workgroups, byte offsets past 2^32 (8.6 GB of observations).
    The rows repeat 1000 distinct ones, so every value has a restated expectation."""
    env, _ = _make(gpu, "im", n=64)
    critic = _critic(env, (16,), seed=4)
    rows = 31 * 1048576
    base = _obs(env, 1000, seed=3)
    idx = torch.arange(rows, device=gpu) % 1000
    obs = base[idx]
    assert obs.numel() * 8 > 2 ** 32
    v = env.mlp_values(critic, obs)
    want = torch.from_numpy(mlp_model.forward(critic, base.cpu().numpy())[:, 0]).to(gpu)
    assert tuple(v.shape) == (rows,)
    ne = v.view(torch.int32) != want[idx].view(torch.int32)
    assert not bool(ne.any()), f"{int(ne.sum())} of {rows} differ, first at row {int(ne.nonzero()[0])}"


@pytest.mark.parametrize("name", ["im", "nv"])
def test_values_tanh(gpu, name):
    """the bound of test_gpu_mlp_policy.py's tanh actors: with F64 the float64
    evaluation of the network and d_ref = max |R32 - F64| of the float32
    restatement with numpy's tanh, the kernel satisfies max |v - F64| <= 4 d_ref"""
    env, _ = _make(gpu, name)
    critic = _critic(env, (64, 64), seed=8, activation="tanh")
    obs = _obs(env, 1000)
    v = env.mlp_values(critic, obs).cpu().numpy().astype(np.float64)
    o = obs.cpu().numpy()
    f64 = mlp_model.forward_f64(critic, o)[:, 0]
    d_ref = float(np.abs(mlp_model.forward(critic, o)[:, 0].astype(np.float64) - f64).max())
    d_gpu = float(np.abs(v - f64).max())
    print(f"tanh critic {name}: d_ref = {d_ref:.6e}  kernel = {d_gpu:.6e}  scale = {float(np.abs(f64).max()):.4e}")
    assert d_ref > 0
    assert d_gpu <= 4 * d_ref, (d_gpu, d_ref)


def test_value_and_actor_objects_refuse_each_other(gpu):
    import invsim
    from invsim import _capi
    (env, obs0), (other, _) = _make(gpu, "im"), _make(gpu, "im")
    actor, critic = _actor(env), _critic(env)
    a_obj, v_obj, v_other = actor.device_object(env), critic.device_object(env), critic.device_object(other)
    lib, s = env._lib, env._stream()
    A = env.action_dim
    act = torch.zeros((2, N, A), dtype=torch.int64, device=gpu)
    raw = torch.zeros((2, N, A), dtype=torch.float32, device=gpu)
    lp = torch.zeros((2, N), dtype=torch.float32, device=gpu)
    val = torch.zeros(N, dtype=torch.float32, device=gpu)
    st, gen = env.get_state(), env._arng.clone()
    o = obs0.data_ptr()
    calls = {
        "mlp_actions": lambda m: lib.invsim_mlp_actions(env._h, m, o, act.data_ptr(), raw.data_ptr(), s),
        "mlp_sample": lambda m: lib.invsim_mlp_sample(env._h, m, o, act.data_ptr(), raw.data_ptr(), None, lp.data_ptr(), s),
        "set_gaussian": lambda m: lib.invsim_mlp_set_gaussian(env._h, m, actor.std.ctypes.data, actor.log_std.ctypes.data),
        "rollout_mlp": lambda m: lib.invsim_rollout_mlp(env._h, 2, m, o, None, None, None, None, act.data_ptr(), None, s),
        "rollout_mlp_sample": lambda m: lib.invsim_rollout_mlp_sample(env._h, 2, m, o, None, None, None, None,
                                                                      act.data_ptr(), raw.data_ptr(), lp.data_ptr(), None, s),
    }
    for what, call in calls.items():
        assert call(v_obj) == EINVAL and "value network" in _capi.last_error(env._h), what
    values = lambda m, rows=N: lib.invsim_mlp_values(env._h, m, o, rows, val.data_ptr(), s)  # noqa: E731
    assert values(a_obj) == EINVAL and "actor" in _capi.last_error(env._h)
    assert values(v_other) == EINVAL and "another handle" in _capi.last_error(env._h)
    assert values(v_obj, -1) == EINVAL
    assert lib.invsim_mlp_values(env._h, v_obj, None, N, val.data_ptr(), s) == EINVAL
    assert lib.invsim_mlp_values(env._h, v_obj, o, N, None, s) == EINVAL
    assert values(v_obj, 0) == 0
    upd = lambda m, std=None, ls=None: lib.invsim_mlp_update(env._h, m, None, None, std, ls, s)  # noqa: E731
    assert upd(v_other) == EINVAL and "another handle" in _capi.last_error(env._h)
    sd = torch.ones(1, dtype=torch.float32, device=gpu)
    assert upd(v_obj, sd.data_ptr(), sd.data_ptr()) == EINVAL, "std on a value object"
    assert upd(a_obj, sd.data_ptr(), None) == EINVAL, "std without log_std"
    torch.cuda.synchronize(gpu)
    assert torch.equal(env.get_state(), st) and torch.equal(env._arng, gen)
    assert bool((act == 0).all()) and bool((raw == 0).all()) and bool((lp == 0).all()) and bool((val == 0).all())
    # create_value's own validation
    ws =[np.zeros((16, env.obs_dim), F32), np.zeros((3, 16), F32)]
    W = (C.c_void_p * 2)(*[w.ctypes.data for w in ws])
    obj = C.c_void_p()
    keep = np.asarray([env.obs_dim, 16, 3], np.int32)
    spec = _capi.MLPSpec(2, 1, 0, 0, keep.ctypes.data, C.cast(W, C.c_void_p), None, None, None, None, None, None, None)
    assert lib.invsim_mlp_create_value(env._h, C.byref(spec), C.byref(obj)) == -34 and not obj.value, "last width 3"
    keep1 = np.asarray([env.obs_dim, 16, 1], np.int32)
    spec = _capi.MLPSpec(2, 1, 0, 1, keep1.ctypes.data, C.cast(W, C.c_void_p), None, None, None, None, None, None, None)
    assert lib.invsim_mlp_create_value(env._h, C.byref(spec), C.byref(obj)) == EINVAL and not obj.value, "clip"
    # the Python surface
    with pytest.raises(TypeError):
        invsim.policies.rollout_policy(env, critic, 2, obs0=obs0)
    with pytest.raises(_capi.InvsimError):
        env.mlp_values(actor, obs0)


# ---------------------------------------------------------------- 3. invsim_mlp_update
def _module(dims, seed, gpu):
    torch.manual_seed(seed)
    mods = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(torch.nn.Linear(a, b))
        if i < len(dims) - 2:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods).to(gpu)


@pytest.mark.parametrize("hidden", [(64, 64), (17, 5)], ids=["33-64-64", "33-17-5"])
def test_update_equals_a_fresh_object(gpu, hidden):
    """after invsim_mlp_update from device tensors, actions, samples and values are
    those of an object created from the new parameters (17 and 5 are padded to 20
    and 8 on the device, 3 and 1 to 4: the padded units never reach an output)"""
    import invsim
    env, obs0 = _make(gpu, "im")
    obs = _obs(env, N)
    A, O = env.action_dim, env.obs_dim
    ls0 = np.full(A, 1.0, F32)
    old = invsim.GaussianMLPPolicyAgent.from_module(_module([O, *hidden, A], 1, gpu), log_std=ls0, seed=0)
    new_mod = _module([O, *hidden, A], 2, gpu)
    env.mlp_sample(old, obs)                                     # the old object has been used
    old.update_from_module(env, new_mod)
    fresh = invsim.GaussianMLPPolicyAgent.from_module(new_mod, log_std=ls0, seed=0)
    old._bufs.pop(env)                                           # both sample from a newly seeded generator buffer
    got = env.mlp_sample(old, obs)
    act_got, raw_got = env.mlp_actions(old, obs, raw=True)
    want = env.mlp_sample(fresh, obs)
    act_want, raw_want = env.mlp_actions(fresh, obs, raw=True)
    for k in ("actions", "raw_actions", "mean", "log_prob"):
        _same(got[k], want[k], f"sample after update: {k}")
    _same(act_got, act_want, "actions after update"), _same(raw_got, raw_want, "raw after update")
    _same(raw_got, mlp_model.forward(fresh, obs.cpu().numpy()), "and they are the model's")
    assert not torch.equal(raw_got, env.mlp_actions(
        invsim.MLPPolicyAgent.from_module(_module([O, *hidden, A], 1, gpu)), obs, raw=True)[1]), "the update changed something"
    # a second env must not silently get the stale host copy
    other, _ = _make(gpu, "im")
    with pytest.raises(RuntimeError, match="update_from_module"):
        other.mlp_actions(old, obs)
    # the critic
    c_old = invsim.ValueMLP.from_module(_module([O, *hidden, 1], 3, gpu))
    c_mod = _module([O, *hidden, 1], 4, gpu)
    env.mlp_values(c_old, obs)
    c_old.update_from_module(env, c_mod)
    c_new = invsim.ValueMLP.from_module(c_mod)
    _same(env.mlp_values(c_old, obs), env.mlp_values(c_new, obs), "values after update")
    _same(env.mlp_values(c_old, obs), mlp_model.forward(c_new, obs.cpu().numpy())[:, 0], "and they are the model's")
    # parameters that are not float32 / contiguous / on the device are copied first
    c_cpu = _module([O, *hidden, 1], 5, gpu).double().cpu()
    c_old.update_from_module(env, c_cpu)
    _same(env.mlp_values(c_old, obs), env.mlp_values(invsim.ValueMLP.from_module(c_cpu), obs), "from a CPU float64 module")


def test_update_null_entries_and_gaussian(gpu):
    import invsim
    from invsim import _capi
    env, obs0 = _make(gpu, "im")
    obs = _obs(env, N)
    A, O = env.action_dim, env.obs_dim
    lib, s = env._lib, env._stream()
    rng = np.random.default_rng(3)
    dims = [O, 17, 5, A]
    l0, l1 = _layers(dims, rng), _layers(dims, rng)
    plain = invsim.MLPPolicyAgent(l0, activation="relu")
    obj = plain.device_object(env)
    # a NULL entry keeps that layer: new weight of layer 1 and new bias of layer 2 only
    w1, b2 = _dev(gpu, l1[1][0]), _dev(gpu, l1[2][1])
    W = (C.c_void_p * 3)(None, w1.data_ptr(), None)
    B = (C.c_void_p * 3)(None, None, b2.data_ptr())
    assert lib.invsim_mlp_update(env._h, obj, C.cast(W, C.c_void_p), C.cast(B, C.c_void_p), None, None, s) == 0
    mixed = [l0[0], (l1[1][0], l0[1][1]), (l0[2][0], l1[2][1])]
    want = invsim.MLPPolicyAgent(mixed, activation="relu")
    _same(env.mlp_actions(plain, obs, raw=True)[1], mlp_model.forward(want, obs.cpu().numpy()), "NULL entries keep")
    # a NULL bias array keeps every bias
    keep_alive = _dev(gpu, l1[0][0])
    W = (C.c_void_p * 3)(keep_alive.data_ptr(), None, None)
    assert lib.invsim_mlp_update(env._h, obj, C.cast(W, C.c_void_p), None, None, None, s) == 0
    mixed[0] = (l1[0][0], l0[0][1])
    want = invsim.MLPPolicyAgent(mixed, activation="relu")
    _same(env.mlp_actions(plain, obs, raw=True)[1], mlp_model.forward(want, obs.cpu().numpy()), "NULL bias array keeps")
    # the update alone sets a Gaussian: the object had none
    env.seed_actions(0)
    out = {k: torch.zeros(sh, dtype=dt, device=gpu) for k, sh, dt in (
        ("actions", (N, A), torch.int64), ("raw", (N, A), torch.float32), ("mean", (N, A), torch.float32),
        ("lp", (N,), torch.float32))}
    sample = lambda: lib.invsim_mlp_sample(env._h, obj, obs.data_ptr(), out["actions"].data_ptr(), out["raw"].data_ptr(),  # noqa: E731
                                           out["mean"].data_ptr(), out["lp"].data_ptr(), s)
    assert sample() == EINVAL and "Gaussian" in _capi.last_error(env._h)
    gauss = invsim.GaussianMLPPolicyAgent(mixed, log_std=np.array([0.5, -1.0, 2.0], F32), seed=0, activation="relu")
    sd, ls = _dev(gpu, gauss.std), _dev(gpu, gauss.log_std)
    assert lib.invsim_mlp_update(env._h, obj, None, None, sd.data_ptr(), ls.data_ptr(), s) == 0
    assert sample() == 0
    want = env.mlp_sample(gauss, obs)                              # seeds its own buffer from the same seed
    for k, kk in (("actions", "actions"), ("raw", "raw_actions"), ("mean", "mean"), ("lp", "log_prob")):
        _same(out[k], want[kk], f"Gaussian set by the update alone: {kk}")
    # and an update replaces it: std and log_std from update_from_module's log_std (exp in torch, float32)
    ls2 = torch.tensor([0.25, 0.0, -0.75], dtype=torch.float32, device=gpu)
    mod = _module(dims, 6, gpu)
    gauss.update_from_module(env, mod, log_std=ls2)
    gauss._bufs.pop(env)
    got = env.mlp_sample(gauss, obs)
    z = gm.normals(0, 0, N, A)
    _same(got["mean"], mlp_model.forward(invsim.MLPPolicyAgent.from_module(mod), obs.cpu().numpy()), "mean of the new weights")
    _same(got["raw_actions"], gm.sample(got["mean"].cpu().numpy(), z, ls2.exp().cpu().numpy()), "sample with the new std")
    _same(got["log_prob"], gm.log_prob(z, ls2.cpu().numpy()), "log_prob with the new log_std")
    with pytest.raises(TypeError):
        plain.update_from_module(env, mod, log_std=ls2)


# ---------------------------------------------------------------- 4. collect_rollout with a critic
def _check_critic_keys(env, critic, out, obs0, gamma, lam, done0, what):
    Kk = out["reward"].shape[0]
    allobs = torch.cat([obs0[None], out["obs"]])
    v = env.mlp_values(critic, allobs) if not isinstance(critic, torch.nn.Module) else critic(
        allobs.float()).detach().reshape(Kk + 1, -1).float()
    _same(out["values"], v[:Kk], f"{what}: values"), _same(out["last_value"], v[Kk], f"{what}: last_value")
    vn = v.cpu().numpy()
    adv, ret, valid = _model_gae(out, gamma, lam, done0, vn[0], vn[1:])
    _same(out["advantages"], adv, f"{what}: advantages"), _same(out["returns"], ret, f"{what}: returns")
    _same(out["valid"], valid, f"{what}: valid")
    done = (out["terminated"] | out["truncated"])
    prev = torch.cat([(done0 if done0 is not None else torch.zeros_like(done[0]))[None], done[:-1]])
    assert torch.equal(out["valid"], ~prev), f"{what}: valid[k] is the negation of done[k - 1]"
    assert torch.equal(out["done"], done[-1]) and out["done"].dtype == torch.bool, f"{what}: done"
    assert bool((out["advantages"][~out["valid"]] == 0).all())


@pytest.mark.parametrize("name", ["im", "nv", "net"])
def test_collect_rollout_with_critic(gpu, name):
    import invsim
    collect = invsim.policies.collect_rollout
    (env, obs0), (twin, obs0_t), (third, obs0_3) = _make(gpu, name), _make(gpu, name), _make(gpu, name)
    actor, critic = _actor(env), _critic(env, (64, 64))
    out = collect(env, actor, K, obs0, critic=critic, gamma=0.98, gae_lambda=0.9)
    ref = collect(twin, actor, K, obs0_t)
    assert sorted(ref) == sorted(KEYS)
    assert sorted(out) == sorted(KEYS + ("values", "last_value", "advantages", "returns", "valid", "done"))
    for k in KEYS:
        _same(out[k], ref[k], f"{name}: {k} with and without a critic")
    assert torch.equal(env.get_state(), twin.get_state()) and torch.equal(env._arng, twin._arng)
    _check_critic_keys(env, critic, out, obs0, 0.98, 0.9, None, name)
    resets = (~out["valid"]).all(1).sum().item()
    assert resets == 2 and bool(out["valid"].all(1)[~(~out["valid"]).all(1)].all()), "two reset rows inside the call"
    assert bool((out["reward"][~out["valid"]] == 0).all())
    # a plain torch module as the critic: the same GAE from its own values
    mod = _module([env.obs_dim, 32, 1], 7, gpu)
    out3 = collect(third, actor, K, obs0_3, critic=mod, gamma=0.98, gae_lambda=0.9)
    for k in KEYS:
        _same(out3[k], ref[k], f"{name}: {k} with a torch critic")
    _check_critic_keys(third, mod, out3, obs0_3, 0.98, 0.9, None, f"{name} torch critic")
    # step on to a call that ends on a done; the next call's first row is then masked through done0
    cur, done = out["obs"][-1], out["done"]
    for _ in range(9):
        if bool(done.all()):
            break
        o1 = collect(env, actor, 1, cur, critic=critic, done0=done)
        cur, done = o1["obs"][-1], o1["done"]
    assert bool(done.all())
    nxt = collect(env, actor, 3, cur, critic=critic, done0=done)
    _check_critic_keys(env, critic, nxt, cur, 0.99, 0.95, done, f"{name} after a done")
    assert not bool(nxt["valid"][0].any()) and bool(nxt["valid"][1:].all())


def test_collect_rollout_per_env_periods(gpu):
    """half-way through an episode a masked reset (tests/staggered.py's first mask)
    staggers the periods: the reset rows differ per env, and the call ends on a done
    for one cohort only"""
    import invsim
    collect = invsim.policies.collect_rollout
    (env, obs0), (twin, obs0_t) = _make(gpu, "im"), _make(gpu, "im")
    actor, critic = _actor(env), _critic(env, (64, 64))
    mask = torch.from_numpy(staggered.schedule_masks(N, "a")[0]).to(gpu)
    cur = {}
    for e, o0, kw in ((env, obs0, dict(critic=critic)), (twin, obs0_t, {})):
        first = collect(e, actor, 3, o0, **kw)
        r_obs, _ = e.reset(options={"reset_mask": mask})
        cur[e] = torch.where(mask[:, None], r_obs, first["obs"][-1])
    assert (env.position() & 0xFFFFFFFF) == 0xFFFFFFFF, "per-env periods after the mask"
    out = collect(env, actor, K, cur[env], critic=critic)
    ref = collect(twin, actor, K, cur[twin])
    for k in KEYS:
        _same(out[k], ref[k], f"staggered: {k} with and without a critic")
    _check_critic_keys(env, critic, out, cur[env], 0.99, 0.95, None, "staggered")
    rows = (~out["valid"]).cpu().numpy()
    assert rows[:, mask.cpu().numpy()].any(0).all() and not (rows[:, 0] == rows[:, 1]).all(), "reset rows differ per env"
    done = out["done"]
    assert bool(done.any()) and not bool(done.all())
    nxt = collect(env, actor, 5, out["obs"][-1], critic=critic, done0=done)
    _check_critic_keys(env, critic, nxt, out["obs"][-1], 0.99, 0.95, done, "staggered, second call")
    assert torch.equal(nxt["valid"][0], ~done)


# ---------------------------------------------------------------- 5. capture
def test_graph_of_update_values_gae(gpu):
    """invsim_mlp_update -> invsim_mlp_values -> invsim_gae captured on one stream:
    the replay equals the eager calls, and after the weight tensors are overwritten
    in place the next replay computes with the new weights"""
    import invsim
    env, obs0 = _make(gpu, "im")
    actor = _actor(env)
    roll = invsim.policies.collect_rollout(env, actor, K, obs0)
    allobs = torch.cat([obs0[None], roll["obs"]]).contiguous()
    mod = _module([env.obs_dim, 64, 64, 1], 11, gpu)
    critic = invsim.ValueMLP.from_module(_module([env.obs_dim, 64, 64, 1], 12, gpu))
    critic.device_object(env)                     # the first meeting synchronises: before the capture
    v = torch.zeros((K + 1, N), dtype=torch.float32, device=gpu)

    def fn():
        critic.update_from_module(env, mod)
        env._mlp_values_into(critic, allobs, (K + 1) * N, v)
        return invsim.policies.gae(roll["reward"], roll["terminated"], roll["truncated"], v[0], v[1:], 0.99, 0.95,
                                   stream=env._stream())
    g = env.capture(fn, warmup=1)
    assert g.steps == 0

    def eager():
        fresh = invsim.ValueMLP.from_module(mod)
        ve = env.mlp_values(fresh, allobs)
        return ve, invsim.policies.gae(roll["reward"], roll["terminated"], roll["truncated"], ve[0], ve[1:], 0.99, 0.95)
    for rep in range(2):
        if rep:                                    # the optimiser's step: new weights in the same tensors
            with torch.no_grad():
                for p_, q_ in zip(mod.parameters(), _module([env.obs_dim, 64, 64, 1], 13, gpu).parameters()):
                    p_.copy_(q_)
        v.zero_()
        og = g.replay()
        torch.cuda.synchronize(gpu)
        ve, oe = eager()
        _same(v, ve, f"replay {rep}: values")
        for k in ("advantages", "returns", "valid"):
            _same(og[k], oe[k], f"replay {rep}: {k}")
    _same(ve, torch.from_numpy(mlp_model.forward(invsim.ValueMLP.from_module(mod), allobs.reshape(-1, env.obs_dim).cpu().numpy())
                               [:, 0].reshape(K + 1, N)), "and they are the model's, with the new weights")
