"""SB3's PPO.train loss for separate actor / critic networks and a
state-independent log_std, written in torch from the formulas of
include/invsim.h ("PPO gradients") and differentiated by torch.autograd on the
CPU (TEST INFRASTRUCTURE, never shipped).  ``dtype=torch.float64`` is the
reference the gradient kernels and tests/ppo_model.py are held to; the same
code in float32 is torch's own float32 autograd, whose distance from the
float64 result sets the tolerance.  This module imports nothing from invsim and
no model file (tests/test_ppo_grad.py checks the imports); it also holds the
case generator the CPU and the GPU tests share.

Metric, per gradient tensor and for the stats vector:
    max |got - ref64| / (max |ref64| + TINY)

GRAD_TOL.  tests/test_ppo_grad.py::test_tolerance_is_four_times_torch_float32
measures the metric for torch's float32 CPU autograd of this loss on every case
of CASES (every gradient tensor and the stats of actor and critic) and asserts
GRAD_TOL == 4 x MEASURED_F32, rounded up to two digits, and that MEASURED_F32 is
what it measures (to the few per cent by which BLAS builds differ):

    largest float32-autograd value   see MEASURED_F32 below (asserted equal)
    factor                           4: the kernels sum 64 samples in sequence
                                     and then up to 256 partials, torch sums
                                     pairwise / blocked; float32 error grows at
                                     most linearly with the chain length
    the kernels' largest error / bound on an MI355X: see KERNEL_SLACK below

The end-to-end bound is the same factor on the float32 torch learner beside the
float64 one (``learner``), computed by the end-to-end GPU test on the buffers it
collected (they exist only on the GPU); the values it printed are in
LEARNER_MEASURED.

Cases.  ``old_logp`` is the float64 new log-density plus an offset from {-0.5,
-0.05, +0.05, +0.5}: with clip_range 0.2 both clip sides and the unclipped
region each hold a real share of the samples and no ratio is near a kink.  No
advantage is 0 (|adv| >= 0.05), and no return lies within 0.25 of the value: the
critic's gradient of a sample is proportional to v - returns, so where that
difference cancels, the forward pass's own float32 error (up to MLP_TOL x the
condition scale, about 2, by the "MLP actor" contract) is divided by it; a
one-sample minibatch with |v - returns| = 0.02 would turn one ulp of v into
1e-5 of the gradient, whatever computes it.  For relu networks ``make_case`` asserts that
the smallest float64 |pre-activation| over all samples exceeds 64 x MLP_TOL x
its condition scale (|W| |h| + |b|), so no float32 evaluation can land on the
other side of a kink; the seeds are chosen so that it does.  No sample is ever
left out of a comparison.
"""
import copy

import numpy as np
import torch

F32, F64 = np.float32, np.float64
TINY = 1e-30
MLP_TOL = 6.7e-6             # the float32 forward against float64, in units of the condition scale
                             # (measured in tests/learner_reference.py's docstring)
LOG_SQRT_2PI = 0.9189385332046727
CLIP_RANGE, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
MAX_GROUPS = 256             # INVSIM_PPO_MAX_GROUPS (the test reads the header and compares)

# largest metric of torch's float32 autograd over CASES (measured on this code, asserted by the CPU test)
MEASURED_F32 = 1.735e-6        # im-64x64-tanh; the single-sample case reaches 1.3e-6
GRAD_TOL = 7.0e-6
# largest kernel error / GRAD_TOL seen on an MI355X (printed by tests/test_gpu_ppo_grad.py)
KERNEL_SLACK = 0.37           # 2.59e-6, im-64x64-tanh actor; net-noscale actor 0.33; every other tensor below 0.2
# end-to-end (197 envs, K = 9, 2 epochs x 3 minibatches of 600, two iterations): largest parameter metric after the
# first minibatch; after the update library / torch float32 (the bound is 4 x the latter); largest error / bound
LEARNER_MEASURED = {"im": (3.6e-7, 3.6e-7, 3.2e-7, 0.28), "nv": (1.4e-7, 2.2e-7, 2.2e-7, 0.25),
                    "net": (3.2e-6, 3.3e-6, 1.2e-6, 0.70)}

FAMILIES = {     # the env families' observation dtype and width, and their action width
    "im": dict(obs_dtype=np.int64, O=33, A=3),
    "nv": dict(obs_dtype=np.float32, O=10, A=1),
    "net": dict(obs_dtype=np.float32, O=68, A=11),
}

# name -> family, hidden widths, hidden activation, tanh output, in_scale, out_scale, samples S, n0,
#         idx kind (None | "perm" | "repeat" | "seam"), rows of the minibatch, masked share, adv_stats, seed
CASES = {
    "im-64x64-tanh": dict(family="im", hidden=[64, 64], act="tanh", S=197, n0=0, idx=None, mask=0.0, stats=True, seed=1),
    "im-64x64-rows1": dict(family="im", hidden=[64, 64], act="tanh", S=1, n0=0, idx=None, mask=0.0, stats=False, seed=2),
    "im-64x64-rows63": dict(family="im", hidden=[64, 64], act="tanh", S=200, n0=100, idx="perm", rows=63, mask=0.2,
                            stats=True, seed=3),
    "im-64x64-rows64": dict(family="im", hidden=[64, 64], act="tanh", S=200, n0=200, idx="repeat", rows=64, mask=0.0,
                            stats=True, seed=4),
    "im-64x64-seam": dict(family="im", hidden=[64, 64], act="tanh", S=200, n0=70, idx="seam", rows=65, mask=0.2,
                          stats=False, seed=5),
    "nv-16-relu": dict(family="nv", hidden=[16], act="relu", S=197, n0=0, idx=None, mask=0.0, stats=True, seed=231),
    "nv-16-relu-noscale": dict(family="nv", hidden=[16], act="relu", in_scale=False, S=130, n0=64, idx="perm", rows=130,
                               mask=0.2, stats=False, seed=25),
    "net-64x64-tanh": dict(family="net", hidden=[64, 64], act="tanh", S=197, n0=64, idx="perm", rows=197, mask=0.1,
                           stats=True, seed=8),
    "im-linear": dict(family="im", hidden=[], act="tanh", S=65, n0=0, idx=None, mask=0.0, stats=True, seed=9),
    "im-30x7-tanh": dict(family="im", hidden=[30, 7], act="tanh", S=197, n0=0, idx="repeat", rows=150, mask=0.1,
                         stats=True, seed=10),
    "im-tanh-out": dict(family="im", hidden=[64, 64], act="tanh", out_tanh=True, S=130, n0=0, idx=None, mask=0.0,
                        stats=True, seed=11),
    "net-noscale": dict(family="net", hidden=[64, 64], act="tanh", in_scale=False, out_scale=False, S=100, n0=0,
                        idx=None, mask=0.0, stats=False, seed=12),
    "im-two-tiles-per-group": dict(family="im", hidden=[64, 64], act="tanh", S=64 * MAX_GROUPS + 65, n0=0, idx=None,
                                   mask=0.1, stats=True, seed=13),
    "im-256x256-tanh": dict(family="im", hidden=[256, 256], act="tanh", S=197, n0=0, idx=None, mask=0.0, stats=True,
                            seed=14),
}


def make_module(dims, act, out_tanh, seed):
    """nn.Sequential of Linear layers under torch's default initialisation"""
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    mods = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(torch.nn.Linear(a, b))
        if i < len(dims) - 2:
            mods.append(torch.nn.ReLU() if act == "relu" else torch.nn.Tanh())
    if out_tanh:
        mods.append(torch.nn.Tanh())
    torch.random.set_rng_state(state)
    return torch.nn.Sequential(*mods)


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def inputs(case, dtype):
    """the network inputs of every sample: the first S rows of cat([obs0, obs]), cast
    to float32 as the learner's obs.float(), then the input affine, in ``dtype``"""
    rows = case["obs"] if case["obs0"] is None else np.concatenate([case["obs0"], case["obs"]])
    x = torch.from_numpy(np.ascontiguousarray(rows[:case["S"]])).float().to(dtype)
    if case["in_scale"] is not None:
        x = x * _t(case["in_scale"], dtype) + _t(case["in_shift"], dtype)
    return x


def selected(case, idx="case"):
    """the minibatch's valid samples, in order, repeats kept: masked ones are removed"""
    idx = case["idx"] if isinstance(idx, str) else idx
    sel = np.arange(case["S"]) if idx is None else np.asarray(idx, np.int64)
    if case["valid"] is not None:
        sel = sel[case["valid"][sel]]
    return torch.from_numpy(sel)


def _apply(module, x, scale, shift, dtype):
    y = module(x)
    if scale is not None:
        y = y * _t(scale, dtype) + _t(shift, dtype)
    return y


def log_prob(mean, log_std, raw):
    z = (raw - mean) / log_std.exp()
    return -LOG_SQRT_2PI * mean.shape[-1] - (0.5 * z * z + log_std).sum(-1)


def normalised_adv(adv, stats):
    """(adv - mean) / (sqrt(M2 / (count - 1)) + 1e-8) with stats = (count, mean, M2); a count below 2: adv"""
    if stats is None or stats[0] < 2:
        return adv
    return (adv - float(stats[1])) / (float(np.sqrt(stats[2] / (stats[0] - 1.0))) + 1e-8)


def actor_loss(mean, log_std, raw, old_logp, adv, clip_range, ent_coef):
    """(loss, stats [6]) over the rows given (all valid); n = 0 gives (0, zeros)"""
    n = mean.shape[0]
    if n == 0:
        return mean.sum() * 0 + log_std.sum() * 0, torch.zeros(6, dtype=torch.float64)
    logp = log_prob(mean, log_std, raw)
    lr = logp - old_logp
    ratio = lr.exp()
    s1 = adv * ratio
    s2 = adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
    policy_loss = -torch.min(s1, s2).sum() / n
    entropy = (0.5 + LOG_SQRT_2PI + log_std).sum()
    with torch.no_grad():
        stats = torch.stack([torch.tensor(float(n), dtype=ratio.dtype), policy_loss, entropy,
                             ((ratio - 1) - lr).sum() / n, ((ratio - 1).abs() > clip_range).to(ratio.dtype).sum() / n,
                             ratio.sum() / n]).double()
    return policy_loss - ent_coef * entropy, stats


def critic_loss(v, returns, vf_coef):
    n = v.shape[0]
    if n == 0:
        return v.sum() * 0, torch.zeros(2, dtype=torch.float64)
    mse = ((returns - v) ** 2).sum() / n
    return vf_coef * mse, torch.stack([torch.tensor(float(n), dtype=v.dtype), mse.detach()]).double()


def _grads_of(loss, module, extra=()):
    lin = [m for m in module if isinstance(m, torch.nn.Linear)]
    params = [p for m in lin for p in (m.weight, m.bias)] + list(extra)
    g = torch.autograd.grad(loss, params, allow_unused=True)
    g = [torch.zeros_like(p) if x is None else x for p, x in zip(params, g)]
    out = {"weight": [x.double().numpy() for x in g[0:2 * len(lin):2]],
           "bias": [x.double().numpy() for x in g[1:2 * len(lin):2]]}
    if extra:
        out["log_std"] = g[-1].double().numpy()
    return out


def grads(case, dtype=torch.float64, idx="case", clip_range=None, old_logp=None):
    """{"actor": {"weight", "bias", "log_std", "stats"}, "critic": {"weight", "bias", "stats"}} of the
    case's minibatch (or of ``idx``): float64 numpy whatever ``dtype`` computed them"""
    clip_range = case["clip_range"] if clip_range is None else clip_range
    sel = selected(case, idx)
    x = inputs(case, dtype)[sel]
    actor, critic = copy.deepcopy(case["actor"]).to(dtype), copy.deepcopy(case["critic"]).to(dtype)
    log_std = _t(case["log_std"], dtype).requires_grad_(True)
    mean = _apply(actor, x, case["out_scale"], case["out_shift"], dtype)
    adv = _t(normalised_adv(case["adv"].astype(F64), case["adv_stats"]), dtype)[sel]
    old = _t(case["old_logp"] if old_logp is None else old_logp, dtype)[sel]
    loss, stats = actor_loss(mean, log_std, _t(case["raw"], dtype)[sel], old, adv, clip_range, case["ent_coef"])
    out = {"actor": _grads_of(loss, actor, (log_std,))}
    out["actor"]["stats"] = stats.numpy()
    v = _apply(critic, x, case["v_scale"], case["v_shift"], dtype)[:, 0]
    loss, stats = critic_loss(v, _t(case["returns"], dtype)[sel], case["vf_coef"])
    out["critic"] = _grads_of(loss, critic)
    out["critic"]["stats"] = stats.numpy()
    return out


def current_log_prob(case):
    """the float64 log-density of every sample's raw action under the case's actor"""
    with torch.no_grad():
        mean = _apply(copy.deepcopy(case["actor"]).double(), inputs(case, torch.float64), case["out_scale"],
                      case["out_shift"], torch.float64)
        return log_prob(mean, _t(case["log_std"], torch.float64), _t(case["raw"], torch.float64)).numpy()


def metric(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) + TINY)) if ref.size else 0.0


def compare(got, ref, what=""):
    """the largest metric over every gradient tensor and the stats of one network; a
    NaN anywhere in ``got`` is infinite"""
    worst = 0.0
    for k in ref:
        pairs = zip(got[k], ref[k]) if isinstance(ref[k], list) else [(got[k], ref[k])]
        for l, (g, r) in enumerate(pairs):
            g = np.asarray(g, F64)
            m = metric(g, r) if np.isfinite(g).all() else float("inf")
            worst = max(worst, m)
    return worst


def _min_preactivation_margin(module, x):
    """smallest |pre-activation| / (|W| |h| + |b|) over the layers a ReLU follows"""
    m = copy.deepcopy(module).double()
    mods, h, worst = list(m), x, np.inf
    with torch.no_grad():
        for i, l in enumerate(mods):
            if isinstance(l, torch.nn.Linear) and i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU):
                pre = l(h)
                cond = h.abs() @ l.weight.abs().T + l.bias.abs()
                worst = min(worst, float((pre.abs() / cond).min()))
            h = l(h)
    return worst


def synthetic_obs(obs_dtype, rows, O, rng, scaled):
    """with an input affine: observations in 0..400 as the envs give them (int64 ones
    include 2^24 + 1, which the float32 cast rounds); without: values of order 1"""
    if obs_dtype == np.int64:
        o = rng.integers(0, 400, (rows, O)) if scaled else rng.integers(-3, 4, (rows, O))
        if scaled and rows > 5:
            o[5::23, 1] = 2 ** 24 + 1
        return o
    return (rng.uniform(0, 400, (rows, O)) if scaled else rng.uniform(-2, 2, (rows, O))).astype(F32)


def make_case(name):
    c = dict(CASES[name])
    f = FAMILIES[c["family"]]
    O, A, S, n0, seed = f["O"], f["A"], c["S"], c["n0"], c["seed"]
    rng = np.random.default_rng(1000 + seed)
    scaled, oscaled = c.get("in_scale", True), c.get("out_scale", True)
    out = dict(name=name, family=c["family"], O=O, A=A, S=S, n0=n0, clip_range=CLIP_RANGE, ent_coef=ENT_COEF,
               vf_coef=VF_COEF, act=c["act"], out_tanh=c.get("out_tanh", False))
    out["actor"] = make_module([O] + c["hidden"] + [A], c["act"], out["out_tanh"], 10 * seed)
    out["critic"] = make_module([O] + c["hidden"] + [1], c["act"], False, 10 * seed + 1)
    # obs0 [n0, O] and an obs block of S rows, as a rollout's [K, N, O] behind its obs0: the last n0 rows are never read
    allobs = synthetic_obs(f["obs_dtype"], S + n0, O, rng, scaled)
    out["obs0"] = allobs[:n0].copy() if n0 else None
    out["obs"] = allobs[n0:].copy()
    if scaled:       # the statistics of 0..400 uniform: mean 200, std 115; the 2^24 + 1 entries become large inputs
        out["in_scale"] = np.full(O, 1 / 115.0, F32) * rng.uniform(0.8, 1.2, O).astype(F32)
        out["in_shift"] = (-200.0 * out["in_scale"]).astype(F32)
        if f["obs_dtype"] == np.int64:
            out["in_scale"][1] = F32(2.0 ** -23)         # the column that holds 2^24 + 1
            out["in_shift"][1] = F32(-1.0)
    else:
        out["in_scale"] = out["in_shift"] = None
    if oscaled:
        out["out_scale"] = rng.uniform(0.5, 2.0, A).astype(F32)
        out["out_shift"] = rng.uniform(-1.0, 1.0, A).astype(F32)
        out["v_scale"], out["v_shift"] = np.array([2.0], F32), np.array([1.0], F32)
    else:
        out["out_scale"] = out["out_shift"] = out["v_scale"] = out["v_shift"] = None
    out["log_std"] = rng.uniform(-0.5, 0.2, A).astype(F32)
    out["valid"] = None
    if c["mask"] > 0:
        out["valid"] = rng.uniform(size=S) >= c["mask"]
        out["valid"][0] = False
    kind = c["idx"]
    if kind is None:
        out["idx"] = None
    elif kind == "perm":
        out["idx"] = rng.permutation(S)[:c["rows"]].astype(np.int64)
    elif kind == "repeat":
        out["idx"] = rng.integers(0, S, c["rows"]).astype(np.int64)
        out["idx"][1] = out["idx"][0]
    else:            # a run of samples across the obs0 / obs seam
        lo = n0 - c["rows"] // 2
        out["idx"] = np.arange(lo, lo + c["rows"], dtype=np.int64)
    out["rows"] = S if out["idx"] is None else len(out["idx"])
    x64 = inputs(dict(out, obs0=out["obs0"], obs=out["obs"]), torch.float64)
    with torch.no_grad():
        mean = _apply(copy.deepcopy(out["actor"]).double(), x64, out["out_scale"], out["out_shift"], torch.float64)
        v = _apply(copy.deepcopy(out["critic"]).double(), x64, out["v_scale"], out["v_shift"], torch.float64)[:, 0]
    std = np.exp(out["log_std"].astype(F64))
    out["raw"] = (mean.numpy() + std * rng.standard_normal((S, A))).astype(F32)
    out["old_logp"] = np.zeros(S, F32)
    out["old_logp"] = (current_log_prob(out) + rng.choice([-0.5, -0.05, 0.05, 0.5], S)).astype(F32)
    a = rng.standard_normal(S)
    out["adv"] = (np.sign(a) * (0.05 + np.abs(a)) * 3.0 + 0.5).astype(F32)
    assert np.all(out["adv"] != 0)
    e = rng.standard_normal(S)
    out["returns"] = (v.numpy() + np.sign(e) * (0.25 + np.abs(e))).astype(F32)
    out["adv_stats"] = None
    if c["stats"]:
        av = out["adv"].astype(F64)[out["valid"]] if out["valid"] is not None else out["adv"].astype(F64)
        out["adv_stats"] = np.array([len(av), av.mean(), ((av - av.mean()) ** 2).sum()] if len(av) else [0.0, 0.0, 0.0])
    if c["act"] == "relu":
        for net in ("actor", "critic"):
            margin = _min_preactivation_margin(out[net], x64)
            assert margin > 64 * MLP_TOL, f"{name} {net}: a pre-activation sits {margin:.3g} of its condition scale " \
                                          f"from the ReLU kink (needs {64 * MLP_TOL:.3g}): choose another seed"
    return out


_CACHE = {}


def case_and_reference(name):
    """(case, float64 gradients of its minibatch), computed once and shared: callers leave both unchanged"""
    if name not in _CACHE:
        case = make_case(name)
        _CACHE[name] = (case, grads(case))
    return _CACHE[name]


# ---------------------------------------------------------------- the learner
def learner(actor, critic, log_std, buf, perms, batch_size, dtype, in_scale=None, in_shift=None, out_scale=None,
            out_shift=None, v_scale=None, v_shift=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
            lr=3e-4, eps=1e-5):
    """PPOLearner.update written in torch: the epochs' permutations ``perms`` in
    minibatches of ``batch_size``; the advantages normalised with the unbiased
    statistics of the rollout's valid rows; per minibatch the valid samples'
    losses, clip_grad_norm_ over all parameters jointly, Adam.  ``buf``: numpy
    arrays obs0, obs, raw, old_logp, adv, returns, valid over S samples.  Returns
    (parameters after the first minibatch, parameters at the end), float64 numpy
    lists in the order actor weights and biases, critic weights and biases, log_std."""
    actor, critic = copy.deepcopy(actor).to(dtype), copy.deepcopy(critic).to(dtype)
    log_std = torch.nn.Parameter(_t(np.asarray(log_std), dtype))
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=lr, eps=eps)
    S = len(buf["adv"])
    case = dict(obs0=buf["obs0"], obs=buf["obs"], S=S, in_scale=in_scale, in_shift=in_shift, valid=buf["valid"])
    x = inputs(case, dtype)
    av = buf["adv"].astype(F64)[buf["valid"]]
    stats = np.array([len(av), av.mean(), ((av - av.mean()) ** 2).sum()])
    adv = _t(normalised_adv(buf["adv"].astype(F64), stats), dtype)
    raw, old, ret = _t(buf["raw"], dtype), _t(buf["old_logp"], dtype), _t(buf["returns"], dtype)
    snap = lambda: [p.detach().double().numpy().copy() for p in params]  # noqa: E731
    first = None
    for perm in perms:
        for lo in range(0, S, batch_size):
            sel = selected(case, np.asarray(perm[lo:lo + batch_size]))
            mean = _apply(actor, x[sel], out_scale, out_shift, dtype)
            la, _ = actor_loss(mean, log_std, raw[sel], old[sel], adv[sel], clip_range, ent_coef)
            lc, _ = critic_loss(_apply(critic, x[sel], v_scale, v_shift, dtype)[:, 0], ret[sel], vf_coef)
            opt.zero_grad()
            (la + lc).backward()
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            opt.step()
            if first is None:
                first = snap()
    return first, snap()
