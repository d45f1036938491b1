"""The episode sink (invsim_set_episode_sink): the
evaluation harness's running returns (benchmark_InvManagementBacklogEnv.py:
371, 386, 434) folded inside the step / rollout kernels.

* fused == fold: an env with the sink attached and a twin env whose outputs
  are folded afterwards by invsim_episode_fold_groups, launch by launch, give
  the same running returns and the same per-group partials, bit for bit (the
  kernels run the fold's per-lane code on the rows they produce);
* returns == oracle: the per-env running returns equal the C oracle's rewards
  summed in step order, bit for bit, and the finished-episode statistics its
  episode sums;
* the other families (no in-kernel fold) take the fallback fold of their
  outputs, with the same bits as an explicit fold;
* resets: a reset (of every env or a masked one) with the sink attached
  restarts the reset envs' running returns and folds nothing, against the
  oracle reset at the same step.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def _twins(cls, n, seed, gpu):
    from invsim.distributed import EpisodeStats
    a, b = cls(n, device=gpu), cls(n, device=gpu)
    a.reset(seed=seed)
    b.reset(seed=seed)
    sa, sb = EpisodeStats(n, gpu), EpisodeStats(n, gpu)
    sa.attach(a)
    return a, b, sa, sb


def _im_actions(g, K, n, gpu):
    shape = (K, n, 3) if K else (n, 3)
    return torch.randint(-5, 240, shape, device=gpu, generator=g)


def _check(sa, sb, where):
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sa.ret), _bits(sb.ret)), f"{where}: running returns"
    assert np.array_equal(_bits(sa.part), _bits(sb.part)), f"{where}: group partials"


@pytest.mark.parametrize("cls_name,n", [("InvManagementBacklogEnv", 65536),      # im_split + im_roll3
                                        ("InvManagementBacklogEnv", 4099),       # im_roll3o, a partial group
                                        ("InvManagementLostSalesEnv", 32768)])   # im_roll3o (config 4 shard)
def test_sink_fused_equals_fold(gpu, cls_name, n):
    import invsim
    a, b, sa, sb = _twins(getattr(invsim, cls_name), n, 41, gpu)
    g = torch.Generator(device=gpu)
    g.manual_seed(n)
    # single steps across a NEXT_STEP reset (steps 0..29, the reset step, 0..8)
    for k in range(40):
        act = _im_actions(g, 0, n, gpu)
        a.step(act)
        _, r, te, tr, _ = b.step(act)
        sb.update_block(r.reshape(1, -1), te.reshape(1, -1), tr.reshape(1, -1))
        if k in (0, 29, 30, 39):
            _check(sa, sb, f"step {k}")
    # fused rollouts of several lengths, across resets, then steps again
    for K in (30, 17, 45, 2):
        act = _im_actions(g, K, n, gpu)
        a.rollout(act)
        _, r, te, tr = b.rollout(act)
        sb.update_block(r.contiguous(), te.contiguous(), tr.contiguous())
        _check(sa, sb, f"rollout K={K}")
    for k in range(5):
        act = _im_actions(g, 0, n, gpu)
        a.step(act)
        _, r, te, tr, _ = b.step(act)
        sb.update_block(r.reshape(1, -1), te.reshape(1, -1), tr.reshape(1, -1))
    _check(sa, sb, "steps after the rollouts")
    assert float(sa.acc[2]) == 4 * n            # four episodes finished (steps 29; rollouts 30 and 45 twice)
    sa.detach()
    a.step(_im_actions(g, 0, n, gpu))            # detached: nothing more is folded
    _check(sa, sb, "after detach")


def test_sink_policy_rollout_equals_fold(gpu):
    """in-kernel BaseStock agent (im_roll3 / im_roll3o with POL): the sink
    folds the rewards the kernel computes"""
    import invsim
    from invsim.policies import BaseStockAgent
    for n in (65536, 8192):
        a, b, sa, sb = _twins(invsim.InvManagementBacklogEnv, n, 5, gpu)
        for K in (30, 31, 7):
            a.rollout_policy(BaseStockAgent(1.0), K)
            out = b.rollout_policy(BaseStockAgent(1.0), K)
            r, te, tr = out["reward"], out["terminated"], out["truncated"]
            sb.update_block(r.contiguous(), te.contiguous(), tr.contiguous())
            _check(sa, sb, f"policy n={n} K={K}")


@pytest.mark.parametrize("cls_name", ["NewsvendorEnv", "NetInvMgmtBacklogEnv"])
def test_sink_fallback_families(gpu, cls_name):
    """families without the in-kernel fold: the library folds each launch's
    output rows (invsim_episode_fold_groups on the launch stream)"""
    import invsim
    n = 4096 + 3
    cls = getattr(invsim, cls_name)
    a, b, sa, sb = _twins(cls, n, 9, gpu)
    g = torch.Generator(device=gpu)
    g.manual_seed(1)
    A = b.action_dim
    hi = 300.0
    T = a._horizon() + 1
    for k in range(T + 3):
        act = torch.rand((n, A), device=gpu, generator=g) * hi
        a.step(act)
        _, r, te, tr, _ = b.step(act)
        sb.update_block(r.reshape(1, -1), te.reshape(1, -1), tr.reshape(1, -1))
    act = torch.rand((2 * T, n, A), device=gpu, generator=g) * hi
    a.rollout(act)
    _, r, te, tr = b.rollout(act)
    sb.update_block(r.contiguous(), te.contiguous(), tr.contiguous())
    _check(sa, sb, cls_name)
    assert float(sa.acc[2]) == 3 * n


def test_sink_returns_vs_oracle(gpu, oracle):
    """running returns bit-exact against the oracle's rewards summed in step
    order; finished-episode sums against the oracle's episodes"""
    import invsim
    from invsim.distributed import EpisodeStats
    n = 2048 + 5
    env = invsim.InvManagementBacklogEnv(n, device=gpu)
    st = EpisodeStats(n, gpu)
    env.reset(seed=123)
    st.attach(env)
    orc = oracle.OracleInvMgmt(n, backlog=True)
    orc.seed(range(123, 123 + n))
    orc.reset()
    rng = np.random.default_rng(2)
    acts = rng.integers(0, 230, size=(80, n, 3)).astype(np.int64)
    dev = torch.from_numpy(acts).to(gpu)
    env.rollout(dev[:25])                      # periods 0..24
    for k in range(25, 50):                    # 25..29, reset, 0..18
        env.step(dev[k])
    env.rollout(dev[50:80])                    # 19..29, reset, 0..17
    ret = np.zeros(n)
    fin = []
    t = 0
    for k in range(80):
        if t >= 30:
            orc.reset()
            t = 0
            continue
        _, r, tr = orc.step(acts[k])
        ret = ret + r
        t += 1
        if tr.all():
            fin.append(ret)
            ret = np.zeros(n)
    torch.cuda.synchronize()
    assert np.array_equal(st.ret.cpu().numpy().view(np.int64), ret.view(np.int64))
    fin = np.stack(fin)
    res = st.allreduce()
    assert res["episodes"] == fin.size
    assert res["sum"] == pytest.approx(fin.sum(), rel=1e-12)
    assert res["sum_sq"] == pytest.approx((fin * fin).sum(), rel=1e-12)


# ---------------------------------------------------------------- resets with a sink attached
# invsim_reset abandons the reset envs' episodes: their running return restarts
# at +0.0 and nothing is folded, as the harness's `episode_reward = 0.0` at every
# reset (benchmark_InvManagementBacklogEnv.py:368-371).
N_RST = 3 * 64 + 5          # three full groups and one of 5 envs


def _near(got, terms, where):
    """got against the f64 sum of `terms` in another order: a reordered sum of
    m terms errs by at most (m - 1) 2**-53 sum|x|; m < 400 here, under 5e-14
    sum|x|, and 1e-12 leaves about 20x."""
    terms = np.asarray(terms, np.float64).ravel()
    exp, tol = terms.sum(), 1e-12 * np.abs(terms).sum()
    assert abs(float(got) - exp) <= tol, f"{where}: {float(got)!r} != {exp!r} (tol {tol:.3g})"


def _group_terms(x, idx, n):
    """per 64-env group g, the entries of x (one per env of idx) whose env is in g"""
    idx = np.asarray(idx)
    return [x[(idx // 64) == g] for g in range((n + 63) // 64)]


def _im_oracle_acts(n, K, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-10, 270, size=(K, n, 3)).astype(np.int64)


@pytest.mark.parametrize("how", ["plain", "reseed"])
def test_sink_reset_mid_episode_vs_oracle(gpu, oracle, how):
    """a reset 12 steps into the episode: the 12 abandoned rewards leave the
    running returns, the partials keep only their reward sum, and the episode
    that then finishes is the oracle's 30 steps after its reset"""
    import invsim
    from invsim.distributed import EpisodeStats
    n = N_RST
    env = invsim.InvManagementBacklogEnv(n, device=gpu)
    st = EpisodeStats(n, gpu)
    env.reset(seed=123)
    st.attach(env)
    orc = oracle.OracleInvMgmt(n, backlog=True)
    orc.seed(range(123, 123 + n))
    orc.reset()
    acts = _im_oracle_acts(n, 42, 3)
    dev = torch.from_numpy(acts).to(gpu)
    env.rollout(dev[:12])
    for k in range(12):
        orc.step(acts[k])
    torch.cuda.synchronize()
    before = st.part.cpu().numpy().copy()
    assert np.abs(st.ret.cpu().numpy()).max() > 0          # there is something to abandon
    if how == "plain":
        obs, _ = env.reset()
    else:
        obs, _ = env.reset(seed=900)
        orc.seed(range(900, 900 + n))
    assert np.array_equal(obs.cpu().numpy(), orc.reset())
    torch.cuda.synchronize()
    ret = st.ret.cpu().numpy()
    assert not _bits(st.ret).any(), f"running returns after the reset: max |ret| = {np.abs(ret).max()!r}, not +0.0"
    part = st.part.cpu().numpy()
    assert not part[:, :3].any(), "nothing finished: no episode is folded by a reset"
    assert np.array_equal(part[:, 3].view(np.int64), before[:, 3].view(np.int64)), "reward sums change at a reset"
    exp = np.zeros(n)
    rews = []
    for k in range(12, 17):
        env.step(dev[k])
        _, r, _ = orc.step(acts[k])
        exp = exp + r
        rews.append(r)
    torch.cuda.synchronize()
    got = st.ret.cpu().numpy()
    assert np.array_equal(got.view(np.int64), exp.view(np.int64)), \
        f"running returns 5 steps after the reset: max |ret - oracle| = {np.abs(got - exp).max()!r}"
    env.rollout(dev[17:42])
    for k in range(17, 42):
        _, r, tr = orc.step(acts[k])
        exp = exp + r
    assert tr.all()
    torch.cuda.synchronize()
    assert not _bits(st.ret).any()
    res = st.allreduce()
    assert res["episodes"] == n
    _near(res["sum"], exp, "sum of episode returns")
    _near(res["sum_sq"], exp * exp, "sum of squared episode returns")


def test_sink_masked_reset_vs_oracle(gpu, oracle):
    """a masked reset 12 steps in: the reset envs' returns restart, the others
    carry on; the per-env-period launches that follow (im_run_kernel and the
    fallback fold of its rows) against one oracle per subset"""
    import invsim
    from invsim.distributed import EpisodeStats
    n = N_RST
    env = invsim.InvManagementBacklogEnv(n, device=gpu)
    st = EpisodeStats(n, gpu)
    env.reset(seed=123)
    st.attach(env)
    mask = np.zeros(n, bool)
    mask[::3] = True
    kept, rst = np.flatnonzero(~mask), np.flatnonzero(mask)
    orcs = {}
    for name, idx in (("kept", kept), ("rst", rst)):
        o = oracle.OracleInvMgmt(len(idx), backlog=True)
        o.seed([123 + int(i) for i in idx])              # each env's own seed
        o.reset()
        orcs[name] = (o, idx)
    acts = _im_oracle_acts(n, 30, 4)
    dev = torch.from_numpy(acts).to(gpu)
    exp = np.zeros(n)

    def orc_steps(k0, k1):
        for k in range(k0, k1):
            for o, idx in orcs.values():
                _, r, tr = o.step(acts[k][idx])
                exp[idx] = exp[idx] + r
        return tr

    env.rollout(dev[:12])
    orc_steps(0, 12)
    env.reset(options={"reset_mask": torch.from_numpy(mask).to(gpu)})
    orcs["rst"][0].reset()                               # InvMgmt's reset draws nothing
    exp[rst] = 0.0
    for k in range(12, 16):
        env.step(dev[k])
    env.rollout(dev[16:22])
    orc_steps(12, 22)
    torch.cuda.synchronize()
    got = st.ret.cpu().numpy()
    for name, idx in (("kept", kept), ("reset", rst)):
        assert np.array_equal(got[idx].view(np.int64), exp[idx].view(np.int64)), \
            f"running returns of the {name} envs: max |ret - oracle| = {np.abs(got[idx] - exp[idx]).max()!r}"
    assert not st.part.cpu().numpy()[:, :3].any()
    for k in range(22, 25):
        env.step(dev[k])
    env.rollout(dev[25:30])
    orc_steps(22, 30)                                    # the kept envs truncate at step 29
    torch.cuda.synchronize()
    got = st.ret.cpu().numpy()
    assert not got[kept].view(np.int64).any()
    assert np.array_equal(got[rst].view(np.int64), exp[rst].view(np.int64))
    part = st.part.cpu().numpy()
    for g, x in enumerate(_group_terms(exp[kept], kept, n)):
        assert part[g, 2] == len(x), g
        _near(part[g, 0], x, f"group {g} sum of episode returns")
        _near(part[g, 1], x * x, f"group {g} sum of squared episode returns")


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_sink_fused_equals_fold_across_reset(gpu, masked):
    """the sink's reset rule is EpisodeStats.reset_returns on the explicit fold"""
    import invsim
    n = N_RST
    a, b, sa, sb = _twins(invsim.InvManagementBacklogEnv, n, 41, gpu)
    g = torch.Generator(device=gpu)
    g.manual_seed(6)
    mask = None
    if masked:
        mask = torch.zeros(n, dtype=torch.bool, device=gpu)
        mask[::3] = True

    def steps(m, where):
        for _ in range(m):
            act = _im_actions(g, 0, n, gpu)
            a.step(act)
            _, r, te, tr, _ = b.step(act)
            sb.update_block(r.reshape(1, -1), te.reshape(1, -1), tr.reshape(1, -1))
        _check(sa, sb, where)

    steps(9, "9 steps")
    for x in (a, b):
        x.reset(options={"reset_mask": mask} if masked else None)
    sb.reset_returns(mask)
    _check(sa, sb, "reset")
    torch.cuda.synchronize()
    zeroed = sa.ret if mask is None else sa.ret[mask]
    assert not _bits(zeroed).any()
    act = _im_actions(g, 30, n, gpu)
    a.rollout(act)
    _, r, te, tr = b.rollout(act)
    sb.update_block(r.contiguous(), te.contiguous(), tr.contiguous())
    _check(sa, sb, "rollout K=30")
    steps(3, "3 steps")
    assert float(sa.acc[2]) == n


def test_sink_fallback_family_reset_vs_oracle(gpu, oracle):
    """a family without the in-kernel fold (Newsvendor): the reset rule is the
    library's, not a kernel's"""
    import invsim
    from invsim.distributed import EpisodeStats
    n = N_RST
    env = invsim.NewsvendorEnv(n, device=gpu)
    st = EpisodeStats(n, gpu)
    env.reset(seed=9)
    st.attach(env)
    orc = oracle.OracleNewsvendor(n)
    orc.seed(range(9, 9 + n))
    orc.reset()
    rng = np.random.default_rng(8)
    acts = rng.uniform(-50, 2500, size=(47, n, 1)).astype(np.float32)
    dev = torch.from_numpy(acts).to(gpu)
    for k in range(7):
        env.step(dev[k])
        orc.step(acts[k])
    torch.cuda.synchronize()
    assert np.abs(st.ret.cpu().numpy()).max() > 0
    obs, _ = env.reset()
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), orc.reset().view(np.uint32))   # its reset draws parameters
    torch.cuda.synchronize()
    assert not _bits(st.ret).any(), \
        f"running returns after the reset: max |ret| = {np.abs(st.ret.cpu().numpy()).max()!r}, not +0.0"
    env.rollout(dev[7:27])
    for k in range(27, 47):
        env.step(dev[k])
    exp = np.zeros(n)
    for k in range(7, 47):
        _, r, tr, _ = orc.step(acts[k])
        exp = exp + r
    assert tr.all()
    torch.cuda.synchronize()
    assert not _bits(st.ret).any()
    res = st.allreduce()
    assert res["episodes"] == n
    _near(res["sum"], exp, "sum of episode returns")
    _near(res["sum_sq"], exp * exp, "sum of squared episode returns")


def test_sink_refuses_missing_rewards(gpu):
    import invsim
    from invsim.distributed import EpisodeStats
    n = 256
    env = invsim.InvManagementBacklogEnv(n, device=gpu)
    env.reset(seed=0)
    st = EpisodeStats(n, gpu)
    st.attach(env)
    a = torch.zeros((n, 3), dtype=torch.int64, device=gpu)
    obs = torch.empty((n, env.obs_dim), dtype=torch.int64, device=gpu)
    rc = env._lib.invsim_step(env._h, a.data_ptr(), obs.data_ptr(), None, None, None, None, None)
    assert rc == -22                                     # INVSIM_EINVAL: no reward outputs to fold
    with pytest.raises(ValueError):
        EpisodeStats(n + 1, gpu).attach(env)
