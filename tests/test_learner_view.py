"""CPU: the numpy models the GPU tests hold the kernels to bit for bit
(mlp_model, gaussian_model, gae_model, norm_model) against the independent
float64 / extended-precision references of tests/learner_reference.py, at the
shapes and tolerances of tests/test_gpu_learner_view.py; the one measured
tolerance (the float32 network against the float64 module) is measured here;
and every comparison is shown to have teeth: a list of plausible mistakes, each
a few lines, goes through the same comparison function on the same inputs and
must be rejected."""
import ast
import os
import types

import numpy as np
import pytest
import torch

import gae_model
import gaussian_model as gm
import learner_reference as lr
import mlp_model
import norm_model as nm

F32, F64 = np.float32, np.float64
N, SEED = 197, 400
B = nm.BLOCK
GL = [(0.99, 0.95), (1.0, 1.0), (0.5, 0.0), (0.9, 1.0)]
MODELS = ("mlp_model", "gaussian_model", "gae_model", "norm_model", "random_agent_model")


def test_the_reference_imports_no_model():
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "learner_reference.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in (
                "__import__", "import_module"):
            names.add("<dynamic import>")
    assert names == {"copy", "numpy", "torch"}, names
    assert not names & set(MODELS)


# ---------------------------------------------------------------- cases
def _tanh(a):
    """float32 tanh, correctly rounded (float64's, rounded once by the caller): the
    measured tolerance then does not depend on which SIMD tanh numpy dispatches to"""
    return np.tanh(a.astype(F64))


def _reset_obs(oracle, family, n=N):
    """the env's own observations after reset(seed=SEED), from the CPU oracle"""
    if family == "im":
        o = oracle.OracleInvMgmt(n, periods=7)
    elif family == "nv":
        o = oracle.OracleNewsvendor(n, step_limit=6)
    else:
        o = oracle.OracleNet(n, graph=oracle.default_graph(), num_periods=6, backlog=True)
    o.seed(range(SEED, SEED + n))
    return o.reset()


def _network(i, family, hidden, activation, value=False, **kw):
    """(module, affines, the library's host-side agent) of case i"""
    import invsim
    f = lr.FAMILIES[family]
    out = 1 if value else len(f["high"])
    mod = lr.make_module([f["O"]] + list(hidden) + [out], activation, seed=lr.module_seed(i, activation, value), **kw)
    aff = lr.affines(family, value=value)
    cls = invsim.ValueMLP if value else invsim.MLPPolicyAgent
    return mod, aff, cls.from_module(mod, **aff)


def test_mlp_model_against_the_module_and_the_tolerance(oracle):
    """mlp_model.forward against forward64 on every network, activation and
    observation set of the GPU tests; MLP_TOL is 4 x the largest ratio seen here,
    the condition of the issue holds on every entry, and the converted actions
    are those of the reference away from the boundaries (at most 1 % are near)."""
    largest, worst_cond = 0.0, 0.0
    for i, (cid, family, hidden) in enumerate(lr.NETWORKS):
        f = lr.FAMILIES[family]
        sets = {"reset": _reset_obs(oracle, family), "synthetic": lr.synthetic_obs(family, N, seed=i + 1),
                "block": lr.synthetic_obs(family, (lr.K + 1) * N, seed=i + 50)}      # its first (K + 1) n rows: the block of n envs
        for act in lr.ACTIVATIONS:
            for value in (False, True):
                mod, aff, agent = _network(i, family, hidden, act, value)
                for sname, obs in sets.items():
                    if sname == "block" and not value:
                        continue                                 # only mlp_values takes a block
                    what = f"{cid} {act} {'critic' if value else 'actor'} {sname}"
                    ref, cond = lr.forward64(mod, obs, **aff)
                    got = mlp_model.forward(agent, obs, tanh=_tanh)
                    ratio = lr.check_forward(got, ref, cond, what)
                    worst_cond = max(worst_cond, lr.check_condition(ref, cond, what))
                    print(f"{what}: max |f32 - f64| / condition scale = {ratio:.3e}")
                    largest = max(largest, ratio)
                    if not value:
                        low = np.zeros(len(f["high"]))
                        conv = mlp_model.convert(got, low, f["high"], f["act_dtype"])
                        for n in lr.N_ENVS:                      # the GPU tests' env counts: the first n rows
                            lr.check_actions(conv[:n], ref[:n], cond[:n], low, f["high"], f["act_dtype"], f"{what} n={n}",
                                             lambda r: np.clip(r, low, f["high"]).astype(f["act_dtype"]))
    print(f"largest {largest:.3e}  MLP_TOL {lr.MLP_TOL:.3e}  MLP_TOL x condition / (1 + |ref|) <= {worst_cond:.3e}")
    assert 4 * largest <= lr.MLP_TOL <= 5 * largest, "MLP_TOL is 4 x the largest measured ratio, rounded up"


def _mutant(agent, **change):
    fields = {k: getattr(agent, k) for k in ("weights", "biases", "activation", "out_activation", "in_scale",
                                              "in_shift", "out_scale", "out_shift")}
    return types.SimpleNamespace(**dict(fields, **change))


@pytest.mark.parametrize("act", lr.ACTIVATIONS)
@pytest.mark.parametrize("name", ["activation on the output", "no biases", "in_shift sign", "no out_shift"])
def test_mlp_mutants_are_rejected(name, act):
    # outputs below zero, so that a ReLU on them shows (the cases' own are centred at +2)
    mod, aff, agent = _network(0, "im", lr.OWN["im"], act, out_bias=-2.0)
    obs = lr.synthetic_obs("im", N, seed=1)
    ref, cond = lr.forward64(mod, obs, **aff)
    lr.check_forward(mlp_model.forward(agent, obs, tanh=_tanh), ref, cond, "unmutated")
    lr.check_condition(ref, cond, "unmutated")
    bad = {"activation on the output": dict(out_activation=act),
           "no biases": dict(biases=[None] * len(agent.biases)),
           "in_shift sign": dict(in_shift=-agent.in_shift),
           "no out_shift": dict(out_shift=np.zeros_like(agent.out_shift))}[name]
    with pytest.raises(AssertionError):
        lr.check_forward(mlp_model.forward(_mutant(agent, **bad), obs, tanh=_tanh), ref, cond, name)


# ---------------------------------------------------------------- samples and log-probabilities
LOGP_CASES = [("im", 0.2), ("nv", 0.2), ("net", 0.2), ("im", 0.002)]


def _gauss_case(family, width, oracle_obs=None):
    f = lr.FAMILIES[family]
    i = [n[1] for n in lr.NETWORKS].index(family)
    mod, aff, agent = _network(i, family, lr.OWN[family], "relu")
    obs = lr.synthetic_obs(family, N, seed=i + 1)
    mean = mlp_model.forward(agent, obs)
    log_std = np.log(width * np.asarray(f["high"])).astype(F32)
    std = np.exp(log_std.astype(F64)).astype(F32)
    z = lr.action_normals(0, 0, N, len(f["high"]))
    return mean, log_std, std, z


@pytest.mark.parametrize("family,width", LOGP_CASES)
def test_gaussian_model_against_the_distribution(family, width):
    mean, log_std, std, z = _gauss_case(family, width)
    raw = gm.sample(mean, z, std)
    lp, bound = lr.log_prob64(mean, log_std, raw)
    slack = lr.check_log_prob(gm.log_prob(z, log_std), lp, bound, f"{family} {width}")
    print(f"{family} A={len(log_std)} width {width}: max error {np.abs(gm.log_prob(z, log_std) - lp).max():.3e}, "
          f"max bound {bound.max():.3e}, error / bound <= {slack:.3f}")
    # the sample is the documented stream: within one float32 ulp of mean + std * float32(z)
    want = mean.astype(F64) + std.astype(F64) * z.astype(F32).astype(F64)
    assert (np.abs(raw.astype(F64) - want) <= np.spacing(np.abs(want).astype(F32))).all()
    assert np.array_equal(z, gm.normals(0, 0, N, z.shape[1])), "the models' table is that stream"


@pytest.mark.parametrize("family,width", LOGP_CASES)
@pytest.mark.parametrize("name", ["+log_std", "no constant", "density at the mean"])
def test_log_prob_mutants_are_rejected(name, family, width):
    mean, log_std, std, z = _gauss_case(family, width)
    raw = gm.sample(mean, z, std)
    lp, bound = lr.log_prob64(mean, log_std, raw)
    zf, A = z.astype(F32), z.shape[1]
    const = F32(0.0) if name == "no constant" else F32(-lr.LOG_SQRT_2PI * A)
    sign = F32(-1.0) if name == "+log_std" else F32(1.0)
    if name == "density at the mean":
        zf = np.zeros_like(zf)
    got = (const - (F32(0.5) * zf * zf).sum(1, dtype=F32) - sign * log_std.sum(dtype=F32)).astype(F32)
    with pytest.raises(AssertionError):
        lr.check_log_prob(got, lp, bound, name)


# ---------------------------------------------------------------- GAE
def _gae_loop(c, gamma, lam, carry_through_done=False, bootstrap_terminated=False, no_truncation_bootstrap=False,
              shifted_values=False, lam_only=False, reset_is_transition=False):
    """a plain backward scan with one switch per mistake; with none set it is GAE"""
    r, te, tr = c["reward"], c["terminated"].astype(bool), c["truncated"].astype(bool)
    K, n = r.shape
    v_out = c["values"].astype(F64)
    v_in = v_out if shifted_values else np.concatenate([c["value0"].astype(F64)[None], v_out[:-1]])
    done = te | tr
    prev = np.concatenate([c["done0"].astype(bool)[None], done[:-1]])
    if reset_is_transition:
        prev = np.zeros_like(prev)
    adv, carry = np.zeros((K, n)), np.zeros(n)
    for k in range(K - 1, -1, -1):
        boot = np.ones(n, bool) if bootstrap_terminated else (~done[k] if no_truncation_bootstrap else ~te[k])
        delta = r[k] + gamma * v_out[k] * boot - v_in[k]
        keep = np.ones(n, bool) if carry_through_done else ~done[k]
        a = delta + (lam if lam_only else gamma * lam) * carry * keep
        carry = np.where(prev[k], carry if carry_through_done else 0.0, a)     # (the reset row after a done row stops it too)
        adv[k] = np.where(prev[k], 0.0, a)
    ret = np.where(prev, v_in, adv + v_in)
    return ret.astype(F32), ~prev, adv.astype(F32)


@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_gae_model_against_the_definition(K):
    seen = set()
    for seed, (gamma, lam) in enumerate(GL):
        c = lr.legal_block(K, N, seed)
        adv, ret, valid = gae_model.gae(c["reward"], c["terminated"], c["truncated"], c["done0"], c["value0"],
                                        c["values"], gamma, lam)
        slack = lr.check_gae(ret, valid, adv, c, gamma, lam, f"K={K} gamma={gamma} lambda={lam}")
        print(f"K={K} gamma={gamma} lambda={lam}: error / bound <= {slack:.3f}")
        lr.check_gae(*_gae_loop(c, gamma, lam), c, gamma, lam, "the plain scan")
        seen |= _flag_features(c)
    if K >= 9:
        assert seen == FEATURES, FEATURES - seen


FEATURES = {"done at row 0", "done at row K - 1", "terminated alone", "truncated alone", "both", "two episodes end",
            "done0", "no done0", "+-1e3"}


def _flag_features(c):
    te, tr, d0 = c["terminated"].astype(bool), c["truncated"].astype(bool), c["done0"].astype(bool)
    done = te | tr
    out = set()
    for cond, name in ((done[0].any(), "done at row 0"), (done[-1].any(), "done at row K - 1"),
                       ((te & ~tr).any(), "terminated alone"), ((tr & ~te).any(), "truncated alone"),
                       ((te & tr).any(), "both"), ((done.sum(0) >= 2).any(), "two episodes end"),
                       (d0.any(), "done0"), ((~d0).any(), "no done0"), ((np.abs(c["reward"]) == 1e3).any(), "+-1e3")):
        if cond:
            out.add(name)
    return out


@pytest.mark.parametrize("name", ["carry_through_done", "bootstrap_terminated", "no_truncation_bootstrap",
                                  "shifted_values", "lam_only", "reset_is_transition"])
def test_gae_mutants_are_rejected(name):
    c = lr.legal_block(9, N, 0)
    gamma, lam = GL[0]
    lr.check_gae(*_gae_loop(c, gamma, lam), c, gamma, lam, "unmutated")
    with pytest.raises(AssertionError):
        lr.check_gae(*_gae_loop(c, gamma, lam, **{name: True}), c, gamma, lam, name)


# ---------------------------------------------------------------- normalisation
@pytest.mark.parametrize("dtype,cols", lr.MOMENT_CASES, ids=lr.MOMENT_IDS)
@pytest.mark.parametrize("rows", lr.MOMENT_ROWS)
def test_moments_model_against_running_mean_var(rows, dtype, cols):
    x, y = lr.moment_data(dtype, cols, rows, seed=rows), lr.moment_data(dtype, cols, rows, seed=rows + 1)
    mask = np.random.default_rng(rows).random(rows) < 0.6
    mask[0] = True
    one = nm.moments(x)
    s1 = lr.check_moments(one, [x], None, B, f"rows={rows}")
    s2 = lr.check_moments(nm.moments(x, mask), [x], [mask], B, f"rows={rows} masked")
    s3 = lr.check_moments(nm.moments(y, mask, one), [x, y], [None, mask], B, f"rows={rows} two calls")
    print(f"rows={rows} {np.dtype(dtype).name} x {cols}: error / bound (mean, M2) {s1} {s2} {s3}")
    count, mean, var = lr.running_mean_var([x, y], [None, mask])
    scale, shift = nm.norm_params(nm.moments(y, mask, one), 1e-8)
    lr.check_scale_shift(scale, shift, mean, var, 1e-8, f"rows={rows}")


def _rms64(x, ddof=0, prior=1e-4):
    """update_from_moments in float64 numpy, one batch into the prior: [3, cols]"""
    x = x.astype(F64)
    bc, bm, bv = x.shape[0], x.mean(0), x.var(0, ddof=ddof)
    tot = prior + bc
    return np.stack([np.full(x.shape[1], tot), bm * bc / tot, prior + bv * bc + bm * bm * prior * bc / tot])


@pytest.mark.parametrize("name", ["n - 1", "no prior count"])
@pytest.mark.parametrize("rows", [63, 70001])
def test_moment_mutants_are_rejected(name, rows):
    x = lr.moment_data(np.int64, 33, rows, seed=rows)
    lr.check_moments(_rms64(x), [x], None, B, "unmutated")
    with pytest.raises(AssertionError):
        lr.check_moments(_rms64(x, **({"ddof": 1} if name == "n - 1" else {"prior": 0.0})), [x], None, B, name)


def test_eps_outside_the_root_is_rejected():
    x = lr.moment_data(np.int64, 33, 5 * 64 + 3, seed=2)
    st = nm.moments(x)
    count, mean, var = lr.running_mean_var([x])
    lr.check_scale_shift(*nm.norm_params(st, 1e-8), mean, var, 1e-8, "unmutated")
    v = st[2] / st[0]
    inv = 1.0 / (np.sqrt(v) + 1e-8)
    with pytest.raises(AssertionError):
        lr.check_scale_shift(inv.astype(F32), (-(st[1] * inv)).astype(F32), mean, var, 1e-8, "eps outside")


def _returns_loop(c, gamma, ret0, zero_at_done=True):
    r, done = c["reward"], (c["terminated"] | c["truncated"]).astype(bool)
    K, n = r.shape
    prev, ret = c["done0"].astype(bool), np.array(ret0, F64)
    out, valid = np.zeros((K, n)), np.zeros((K, n), bool)
    for k in range(K):
        new = ret * gamma + r[k]
        out[k], valid[k] = np.where(prev, 0.0, new), ~prev
        ret = np.where(prev, 0.0 if zero_at_done else ret, np.where(done[k] & zero_at_done, 0.0, new))
        prev = done[k]
    return out, valid, ret


@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_returns_and_rewards_models_against_the_definitions(K):
    for seed, gamma in enumerate((0.99, 1.0, 0.5, 0.97)):
        c = lr.legal_block(K, N, seed)
        ret0 = np.where(c["done0"], 0.0, np.random.default_rng(seed).uniform(-1e3, 1e3, N))
        out, valid, ret = nm.discounted_returns(c["reward"], c["terminated"], c["truncated"], c["done0"], gamma, ret0)
        slack = lr.check_returns(out, valid, c, gamma, ret0, f"K={K} gamma={gamma}", new_ret=ret)
        print(f"K={K} gamma={gamma}: error / bound <= {slack:.3f}")
        stats = nm.moments(out.reshape(-1, 1), valid.reshape(-1))
        ref, mask, _ = lr.returns_by_definition(c["reward"], c["terminated"], c["truncated"], c["done0"], ret0, gamma)
        lr.check_moments(stats, [ref.reshape(-1, 1)], [mask.reshape(-1)], B, f"K={K}: statistics of the returns")
        count, mean, var = lr.running_mean_var([ref.reshape(-1, 1)], [mask.reshape(-1)])
        for eps, clip in ((1e-8, 10.0), (1e-8, 0.5)):
            lr.check_reward_norm(nm.normalize_rewards(c["reward"], stats, eps, clip), c["reward"], var[0], eps, clip,
                                 f"K={K} clip={clip}")


def test_return_not_zeroed_at_a_done_row_is_rejected():
    c = lr.legal_block(9, N, 0)
    ret0 = np.zeros(N)
    out, valid, ret = _returns_loop(c, 0.97, ret0)
    lr.check_returns(out, valid, c, 0.97, ret0, "unmutated", new_ret=ret)
    out, valid, ret = _returns_loop(c, 0.97, ret0, zero_at_done=False)
    with pytest.raises(AssertionError):
        lr.check_returns(out, valid, c, 0.97, ret0, "not zeroed", new_ret=ret)
