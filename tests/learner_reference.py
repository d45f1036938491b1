"""What a PPO learner computes from the library's tensors, written from the
textbook definitions in float64 / extended precision (TEST INFRASTRUCTURE, never
shipped).  The kernels and the numpy models of tests/*_model.py are both held
against these; this module imports none of those models and restates none of
the recurrences of include/invsim.h (tests/test_learner_view.py checks the
imports).

* ``forward64``            the torch module itself, in float64
* ``log_prob64``           torch.distributions.Normal(...).log_prob(...).sum(-1)
* ``gae_by_definition``    A_k = sum_l (gamma lambda)^l delta_{k+l} over the episode segment
* ``returns_by_definition`` the running discounted return as explicit sums
* ``running_mean_var``     SB3 RunningMeanStd.update_from_moments, two-pass batch moments
* ``scale_shift`` / ``reward_norm``

The second half holds the cases the CPU and the GPU tests share (networks,
weights, observations), so that the one measured tolerance is measured on
exactly what the kernels are later held to.

MLP_TOL, the float32 network against ``forward64`` in units of the condition
scale (the last layer's |W| |h| + |b|, times |out_scale|).  Measured by
tests/test_learner_view.py::test_mlp_model_against_the_module_and_the_tolerance
as max |mlp_model.forward - forward64| / condition scale, with a correctly
rounded float32 tanh, over every network below on every observation set of the
GPU tests (the reset observations, the synthetic ones and, for the critics, the
[K + 1, N, O] block):

    network (hidden)       actor relu  actor tanh  critic relu  critic tanh
    im   33-64-64-3        4.82e-07    6.62e-07    3.85e-07     6.88e-07
    nv   10-16-1           1.37e-07    3.19e-07    2.76e-07     2.71e-07
    net  68-64-64-11       5.13e-07    6.41e-07    4.84e-07     5.55e-07
    im   [256] * 4         1.38e-06    1.58e-06    7.27e-07     1.67e-06
    im   [3, 200]          6.68e-07    6.63e-07    4.59e-07     5.42e-07
    im   [5]               1.57e-07    1.76e-07    1.48e-07     1.73e-07
    im   no hidden layer   2.81e-07    2.57e-07    2.98e-07     2.75e-07

    largest 1.674e-06; MLP_TOL = 4 x that, rounded up = 6.7e-06

(4 x: the device's tanhf and numpy's tanh may differ by a few ulp per hidden
unit; ReLU kernels equal the model bit for bit.)  With these weights MLP_TOL x
condition scale stays at or below 1e-4 x (1 + |reference|) on every entry (it
reaches 8.2e-5), which the same test asserts.

The kernels on an MI355X stay inside it with the same margin: their largest
ratio is 1.77e-06 ([256] * 4, tanh), the ReLU networks give the model's figures.

Slack of the derived bounds, largest error / bound observed (numpy models on
the CPU; kernels on an MI355X):
    log-probability   A = 3: 0.25; 0.29    A = 1: 0.24; 0.30    A = 11: 0.15; 0.17
                      A = 3, log_std = log(0.002 high): 0.84; 0.80
                      (bounds at most 1.4e-5, 4.7e-6, 1.4e-4 and 8.0e-5)
    GAE returns       1.00: the final cast's half float32 ulp is the bound and is reached
    discounted return 0.72 at K = 1 falling to 0.05 at K = 31
    running moments   mean 0.007, M2 0.0014
"""
import copy

import numpy as np
import torch

LD = np.longdouble
F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24                     # unit roundoff of float32
LOG_SQRT_2PI = 0.9189385332046727    # 0.5 log(2 pi): the 0.919 of the bound

MLP_TOL = 6.7e-6


def _t64(a):
    """anything array-like -> a float64 CPU torch tensor (values unchanged)"""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))


# ---------------------------------------------------------------- the network and its Gaussian
def forward64(module, obs, in_scale=None, in_shift=None, out_scale=None, out_shift=None):
    """(output, condition scale), float64 numpy [..., out]: a float64 copy of
    ``module`` applied to ``obs.float().double() * in_scale + in_shift``, then
    ``* out_scale + out_shift``.  The float32 cast is the learner's ``obs.float()``.
    The condition scale is |W| |h| + |b| of the last Linear layer (h its input),
    times |out_scale|: the size of the terms the output is a sum of."""
    m = copy.deepcopy(module).cpu().double()
    obs = obs.detach().cpu() if isinstance(obs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(obs))
    x = obs.float().double()
    if in_scale is not None:
        x = x * _t64(in_scale) + _t64(in_shift)
    mods = list(m)
    last = max(i for i, l in enumerate(mods) if isinstance(l, torch.nn.Linear))
    with torch.no_grad():
        h = x
        for l in mods[:last]:
            h = l(h)
        lin = mods[last]
        y = lin(h)
        cond = h.abs() @ lin.weight.abs().T
        if lin.bias is not None:
            cond = cond + lin.bias.abs()
        for l in mods[last + 1:]:
            y = l(y)
        if out_scale is not None:
            y = y * _t64(out_scale) + _t64(out_shift)
            cond = cond * _t64(out_scale).abs()
    return y.numpy(), cond.numpy()


def log_prob64(mean, log_std, raw):
    """(log_prob [...], bound [...]) float64: the learner's
    ``Normal(mean, exp(log_std)).log_prob(raw).sum(-1)`` and how far a float32
    evaluation of it from a float32 sample may lie.  With z = (raw - mean) / std,
    dz = (ulp32(raw) / 2) / std + 2 u |z| (the sample is rounded once, std is a
    rounded exp) a term z^2 / 2 moves by |z| dz + dz^2 / 2, and the float32
    accumulation of 2 A + 1 terms adds (2 A + 2) u of their absolute sum."""
    mean, raw, log_std = _t64(mean), _t64(raw), _t64(log_std)
    std = log_std.exp()
    lp = torch.distributions.Normal(mean, std).log_prob(raw).sum(-1)
    A = mean.shape[-1]
    z = ((raw - mean) / std).abs()
    ulp = torch.from_numpy(np.spacing(np.abs(raw.numpy()).astype(F32)).astype(F64))
    dz = 0.5 * ulp / std + 2 * U32 * z
    bound = (z * dz + 0.5 * dz * dz).sum(-1) + (2 * A + 2) * U32 * (
        0.5 * (z * z).sum(-1) + log_std.abs().sum() + LOG_SQRT_2PI * A)
    return lp.numpy(), bound.numpy()


# ---------------------------------------------------------------- episodes inside a block of K rows
def _flags(a, shape):
    return np.zeros(shape, bool) if a is None else np.asarray(a).astype(bool).reshape(shape)


def _segments(te, tr, d0):
    """One env's K rows cut into episode segments: a list of (first, last) row
    indices, both inclusive.  A row that follows a done row (row 0 under d0) is
    the NEXT_STEP reset row: it belongs to no segment and must carry no flag."""
    K = len(te)
    segs, k = [], 0
    prev = bool(d0)
    while k < K:
        if prev:
            assert not (te[k] or tr[k]), "illegal flags: a reset row carries no flag"
            prev = False
            k += 1
            continue
        e = k
        while e < K - 1 and not (te[e] or tr[e]):
            e += 1
        segs.append((k, e))
        prev = bool(te[e] or tr[e])
        k = e + 1
    return segs


def gae_by_definition(reward, terminated, truncated, done0, value0, values, gamma, lam):
    """(returns, transition mask, sum of |terms|), [K, n]: longdouble, bool,
    longdouble.  Row k of a segment ending at row e has
    A_k = sum_{j = k..e} (gamma lambda)^(j - k) delta_j,
    delta_j = r_j + gamma V(obs after j) [not terminated_j] - V(input of j),
    and the return is A_k + V(input of k).  V(input of j) is value0 for j = 0 and
    values[j - 1] after it, V(obs after j) is values[j].  Reset rows: NaN."""
    r = np.asarray(reward).astype(LD)
    K, n = r.shape
    te, tr, d0 = _flags(terminated, (K, n)), _flags(truncated, (K, n)), _flags(done0, (n,))
    v_out = np.asarray(values).astype(LD).reshape(K, n)
    v_in = np.concatenate([np.asarray(value0).astype(LD).reshape(1, n), v_out[:-1]])
    g, gl = LD(gamma), LD(gamma) * LD(lam)
    ret = np.full((K, n), np.nan, LD)
    mag = np.zeros((K, n), LD)
    mask = np.zeros((K, n), bool)
    for i in range(n):
        for s, e in _segments(te[:, i], tr[:, i], d0[i]):
            for k in range(s, e + 1):
                terms = [v_in[k, i]]
                for j in range(k, e + 1):
                    w = gl ** (j - k)
                    terms += [w * r[j, i], -w * v_in[j, i]]
                    if not te[j, i]:
                        terms.append(w * g * v_out[j, i])
                ret[k, i] = sum(terms, LD(0))
                mag[k, i] = sum((abs(t) for t in terms), LD(0))
                mask[k, i] = True
    return ret, mask, mag


def returns_by_definition(reward, terminated, truncated, done0, ret0, gamma):
    """(out, transition mask, sum of |terms|), [K, n]: the running discounted
    return after every transition row, out_k = sum_{j = s..k} gamma^(k - j) r_j
    over its segment's rows so far, plus ret0 gamma^(k + 1) in the segment that
    row 0 continues.  Reset rows: NaN."""
    r = np.asarray(reward).astype(LD)
    K, n = r.shape
    te, tr, d0 = _flags(terminated, (K, n)), _flags(truncated, (K, n)), _flags(done0, (n,))
    r0 = np.asarray(ret0).astype(LD).reshape(n)
    g = LD(gamma)
    out = np.full((K, n), np.nan, LD)
    mag = np.zeros((K, n), LD)
    mask = np.zeros((K, n), bool)
    for i in range(n):
        for s, e in _segments(te[:, i], tr[:, i], d0[i]):
            for k in range(s, e + 1):
                terms = [g ** (k - j) * r[j, i] for j in range(s, k + 1)]
                if s == 0:
                    terms.append(r0[i] * g ** (k + 1))
                out[k, i] = sum(terms, LD(0))
                mag[k, i] = sum((abs(t) for t in terms), LD(0))
                mask[k, i] = True
    return out, mask, mag


# ---------------------------------------------------------------- running statistics
def running_mean_var(batches, masks=None, prior_count=1e-4):
    """(count, mean, var) longdouble [cols] after folding ``batches`` (a list of
    [rows, cols] arrays; ``masks``: per batch a bool [rows] or None) one by one
    into SB3's RunningMeanStd, which starts at count ``prior_count``, mean 0,
    variance 1.  update_from_moments, as published:
        delta = batch_mean - mean;  tot = count + batch_count
        new_mean = mean + delta * batch_count / tot
        M2 = var * count + batch_var * batch_count + delta^2 * count * batch_count / tot
        new_var = M2 / tot;  new_count = tot
    with the batch's mean and (population) variance taken in two passes.  A
    batch with no unmasked row changes nothing."""
    masks = [None] * len(batches) if masks is None else masks
    cols = np.asarray(batches[0]).shape[1]
    count, mean, var = LD(prior_count), np.zeros(cols, LD), np.ones(cols, LD)
    for x, m in zip(batches, masks):
        x = np.asarray(x)
        x = x.astype(LD) if m is None else x[np.asarray(m).astype(bool)].astype(LD)
        bc = LD(x.shape[0])
        if bc == 0:
            continue
        bm = x.sum(0) / bc
        bv = ((x - bm) ** 2).sum(0) / bc
        delta, tot = bm - mean, count + bc
        m2 = var * count + bv * bc + delta * delta * count * bc / tot
        mean, var, count = mean + delta * bc / tot, m2 / tot, tot
    return count, mean, var


def scale_shift(mean, var, eps):
    """(1 / sqrt(var + eps), -mean / sqrt(var + eps)), longdouble"""
    sd = np.sqrt(np.asarray(var, LD) + LD(eps))
    return 1 / sd, -np.asarray(mean, LD) / sd


def reward_norm(reward, var, eps, clip):
    """clip(r / sqrt(var + eps), -clip, clip), longdouble"""
    return np.clip(np.asarray(reward).astype(LD) / np.sqrt(LD(var) + LD(eps)), -LD(clip), LD(clip))


# ---------------------------------------------------------------- the cases both test files use
FAMILIES = {     # observation dtype and width, the action space's upper bounds, its dtype
    "im": dict(obs_dtype=np.int64, O=33, high=(100.0, 200.0, 230.0), act_dtype=np.int64),
    "nv": dict(obs_dtype=np.float32, O=10, high=(2000.0,), act_dtype=np.float32),
    "net": dict(obs_dtype=np.float32, O=68, high=(1700.0,) * 11, act_dtype=np.float32),
}
OWN = {"im": [64, 64], "nv": [16], "net": [64, 64]}
# (id, family, hidden widths): the families' own networks, then the kernel's launch shapes on im
NETWORKS = [("own-im", "im", OWN["im"]), ("own-nv", "nv", OWN["nv"]), ("own-net", "net", OWN["net"]),
            ("256x4", "im", [256] * 4),       # the 8-wave launch, both limits
            ("3-200", "im", [3, 200]),        # 12 chunks of 16 plus 2 of 4
            ("5", "im", [5]), ("linear", "im", [])]
ACTIVATIONS = ("relu", "tanh")


N_ENVS = (197, 1, 64)            # three full 64-env workgroups and five lanes of a fourth; one env; one workgroup
K = 9                            # mlp_values also takes a whole [K + 1, N, O] block


def module_seed(i, activation, value=False):
    """the torch seed of NETWORKS[i]'s weights"""
    return 100 * i + 7 * bool(value) + (activation == "tanh")


def make_module(dims, activation, seed, out_bias=2.0):
    """nn.Sequential of Linear layers (torch's default initialisation under
    ``seed``) with ``activation`` between them and none at the end.  ``out_bias``
    is added to the last layer's bias: it centres the output where the affine of
    ``affines`` wants it, and as part of the last layer it is part of the
    condition scale (an offset in out_shift would not be, and its float32
    rounding alone would then exceed any multiple of a small condition scale)."""
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    mods = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(torch.nn.Linear(a, b))
        if i < len(dims) - 2:
            mods.append(torch.nn.ReLU() if activation == "relu" else torch.nn.Tanh())
    torch.random.set_rng_state(gen_state)
    with torch.no_grad():
        mods[-1].bias += out_bias
    return torch.nn.Sequential(*mods)


def affines(family, value=False):
    """in_scale / in_shift [O] and out_scale / out_shift of a case, float32 numpy.
    The input rows are what a learner would use, scale_shift of the statistics of
    the family's synthetic observations, so the network sees inputs of order 1
    (the 2^24 + 1 entries included).  With make_module's out_bias of 2 the
    actor's outputs land inside the action range, around 0.55 high, and the
    critic's around 5, so the reference keeps away from 0 relative to its
    condition scale and few entries sit at a clip bound."""
    f = FAMILIES[family]
    _, mean, var = running_mean_var([synthetic_obs(family, 4096, seed=0)])
    scale, shift = scale_shift(mean, var, 1e-8)
    kw = dict(in_scale=scale.astype(F32), in_shift=shift.astype(F32))
    if value:
        kw.update(out_scale=np.array([2.0], F32), out_shift=np.array([1.0], F32))
    else:
        high = np.asarray(f["high"], F64)
        kw.update(out_scale=(0.25 * high).astype(F32), out_shift=(0.05 * high).astype(F32))
    return kw


def synthetic_obs(family, rows, seed):
    """observations in 0..400 of the family's dtype; int64 ones include 2^24 + 1,
    which the float32 cast rounds"""
    f = FAMILIES[family]
    rng = np.random.default_rng(seed)
    if f["obs_dtype"] == np.int64:
        o = rng.integers(0, 400, (rows, f["O"]))
        o[::23, 1] = 2 ** 24 + 1
        return o
    return rng.uniform(0, 400, (rows, f["O"])).astype(F32)


MOMENT_CASES = [(np.int64, 33), (np.float32, 68), (np.float32, 3), (np.float64, 1)]
MOMENT_IDS = ["i64-33", "f32-68", "f32-3", "f64-1"]
MOMENT_ROWS = [1, 63, 65, 5 * 64 + 3, 70001]     # 70001 x 33 int64: more than 256 workgroup nodes, a second tree launch


def moment_data(dtype, cols, rows, seed):
    """0..400 (int64 with 2^24 + 1 entries, as the observations) or -50..400, and
    an all-zero last column where there are several (a column the envs leave 0:
    its variance is the prior's, where epsilon matters)"""
    rng = np.random.default_rng(seed)
    if dtype == np.int64:
        x = rng.integers(0, 400, (rows, cols))
        x[::23, 1] = 2 ** 24 + 1
    else:
        x = rng.uniform(-50, 400, (rows, cols)).astype(dtype)
    if cols > 1:
        x[:, -1] = 0
    return x


def legal_block(K, n, seed):
    """Inputs [K, n] of a GAE / return block with legal flag sequences (no flag on
    a reset row).  Env e has pattern (e + seed) % 8: 0 no flag; 1 done at row 0;
    2 done at row K - 1; 3 two episodes ending inside the block (rows q and q + 2
    or the nearest legal rows); 4 / 5 / 6 terminated alone / truncated alone /
    both at the middle row; 7 random legal flags.  done0 on every other env (the
    phase flips every 8 envs, so every pattern meets both);
    where it is set row 0 is a reset row and carries no flag.  Rewards are finite,
    within +-1e3 with exact +-1e3 entries; values are mixed-sign float32."""
    rng = np.random.default_rng(1000 * K + n + 7919 * seed)
    te, tr = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    pat = (np.arange(n) + seed) % 8
    d0 = ((np.arange(n) + np.arange(n) // 8) % 2).astype(np.uint8)     # both values under every pattern
    mid = K // 2
    for e in range(n):
        first = 1 if d0[e] else 0                 # the first row that may carry a flag
        p = pat[e]
        if first >= K:
            continue
        if p == 1:
            tr[first, e] = 1
        elif p == 2:
            tr[K - 1, e] = 1
        elif p == 3:
            a = max(first, mid - 2)
            tr[a, e] = 1
            if a + 2 < K:
                te[a + 2, e] = 1
        elif p in (4, 5, 6):
            k = max(first, mid)
            te[k, e] = p in (4, 6)
            tr[k, e] = p in (5, 6)
        elif p == 7:
            prev = bool(d0[e])
            for k in range(K):
                if prev:
                    prev = False
                    continue
                te[k, e], tr[k, e] = rng.random() < 0.25, rng.random() < 0.25
                prev = bool(te[k, e] or tr[k, e])
    reward = rng.uniform(-1e3, 1e3, (K, n))
    hit = rng.random((K, n)) < 0.05
    reward[hit] = np.where(rng.random(int(hit.sum())) < 0.5, 1e3, -1e3)
    return dict(reward=reward, terminated=te, truncated=tr, done0=d0,
                value0=(50 * rng.standard_normal(n)).astype(F32),
                values=(50 * rng.standard_normal((K, n))).astype(F32))


def action_normals(seed, first, n, count):
    """z [n, count] float64, the documented action stream: env with global index
    g draws from Generator(PCG64(SeedSequence(2**64 + seed + g))).standard_normal"""
    return np.stack([np.random.Generator(np.random.PCG64(np.random.SeedSequence(2 ** 64 + seed + first + i)))
                     .standard_normal(count) for i in range(n)])


# ---------------------------------------------------------------- the comparisons (models, kernels and mutants alike)
def _f64(a):
    return a.detach().cpu().numpy().astype(F64) if isinstance(a, torch.Tensor) else np.asarray(a).astype(F64)


def check_forward(got, ref, cond, what, tol=MLP_TOL):
    """|got - ref| <= tol x condition scale on every entry; returns the largest ratio"""
    err = np.abs(_f64(got).reshape(ref.shape) - ref)
    assert np.isfinite(err).all(), f"{what}: not finite"
    ratio = float((err / cond).max())
    assert (err <= tol * cond).all(), f"{what}: |error| / condition scale up to {ratio:.3e} > {tol:.3e}"
    return ratio


def check_condition(ref, cond, what):
    """the tolerance means something: MLP_TOL x condition scale <= 1e-4 (1 + |reference|)"""
    worst = float((MLP_TOL * cond / (1 + np.abs(ref))).max())
    assert worst <= 1e-4, f"{what}: MLP_TOL x condition scale reaches {worst:.3e} (1 + |reference|)"
    return worst


def check_actions(got, ref, cond, low, high, dtype, what, convert):
    """converted actions equal ``convert(reference)`` wherever the reference is
    further than the tolerance from a clip bound or (int64 spaces) an integer; at
    most 1 % of the entries may be that close"""
    tol = MLP_TOL * cond
    lo, hi = np.asarray(low, F64), np.asarray(high, F64)
    near = (np.abs(ref - lo) <= tol) | (np.abs(ref - hi) <= tol)
    if np.dtype(dtype) == np.int64:
        near |= np.abs(ref - np.rint(ref)) <= tol
    assert near.mean() <= 0.01, f"{what}: {near.mean():.3%} of the entries are within the tolerance of a boundary"
    want = _f64(convert(ref))
    got = _f64(got).reshape(ref.shape)
    exact = np.dtype(dtype) == np.int64
    bad = ~near & ((got != want) if exact else (np.abs(got - want) > tol))
    assert not bad.any(), f"{what}: {int(bad.sum())} converted actions differ, first at {np.argwhere(bad)[:3].tolist()}"


def check_log_prob(got, lp, bound, what, extra=0.0):
    """|got - lp| and the learner's |exp(lp - got) - 1| within the derived bound (+ extra);
    the bound itself stays at or below 1e-3.  Returns the largest error / bound."""
    got = _f64(got).reshape(lp.shape)
    assert float(bound.max()) <= 1e-3, f"{what}: the bound reaches {float(bound.max()):.3e}"
    lim = bound + extra
    err = np.abs(got - lp)
    assert (err <= lim).all(), f"{what}: log_prob off by {float(err.max()):.3e}, bound {float(lim[err.argmax()]):.3e}"
    ratio = np.abs(np.expm1(lp - got))
    assert (ratio <= lim).all(), f"{what}: |ratio - 1| up to {float(ratio.max()):.3e}"
    return float((err / lim).max())


def check_gae(returns, valid, advantages, c, gamma, lam, what):
    """returns / valid / advantages [K, n] of the block ``c`` against gae_by_definition:
    K 2^-52 sum |terms| for a float64 scan plus half a float32 ulp for the cast"""
    K = c["reward"].shape[0]
    ref, mask, mag = gae_by_definition(c["reward"], c["terminated"], c["truncated"], c["done0"], c["value0"],
                                       c["values"], gamma, lam)
    valid = _f64(valid).astype(bool)
    assert np.array_equal(valid, mask), f"{what}: valid is not the transition mask ({int((valid != mask).sum())} rows)"
    got = _f64(returns).astype(LD)
    r32 = ref[mask].astype(F32)
    tol = K * 2.0 ** -52 * mag[mask] + 0.5 * np.spacing(np.abs(r32)).astype(LD)
    err = np.abs(got[mask] - ref[mask])
    assert (err <= tol).all(), f"{what}: returns off by up to {float((err / tol).max()):.3g} bounds"
    v_in = np.concatenate([np.asarray(c["value0"], F32)[None], np.asarray(c["values"], F32)[:-1]])
    adv = np.asarray(_f64(advantages)).astype(F32)
    assert (adv[~mask].view(np.int32) == 0).all(), f"{what}: a reset row's advantage is not +0.0"
    assert np.array_equal(_f64(returns).astype(F32)[~mask], v_in[~mask]), f"{what}: a reset row's return is not its input's value"
    a_ref = ref[mask] - v_in[mask].astype(LD)
    a_tol = tol + 0.5 * np.spacing(np.abs(a_ref.astype(F32))).astype(LD)
    assert (np.abs(adv[mask].astype(LD) - a_ref) <= a_tol).all(), f"{what}: advantages"
    return float((err / tol).max()) if mask.any() else 0.0


def check_returns(out, valid, c, gamma, ret0, what, new_ret=None):
    """discounted returns [K, n] (and the advanced running return) against
    returns_by_definition within K 2^-52 sum |terms|"""
    K = c["reward"].shape[0]
    ref, mask, mag = returns_by_definition(c["reward"], c["terminated"], c["truncated"], c["done0"], ret0, gamma)
    valid = _f64(valid).astype(bool)
    assert np.array_equal(valid, mask), f"{what}: valid is not the transition mask"
    got = _f64(out).astype(LD)
    tol = K * 2.0 ** -52 * mag
    err = np.abs(got[mask] - ref[mask])
    assert (err <= tol[mask]).all(), f"{what}: returns off by up to {float((err / tol[mask]).max()):.3g} bounds"
    assert (_f64(out)[~mask] == 0).all(), f"{what}: a reset row's running return is not 0"
    if new_ret is not None:
        done = _flags(c["terminated"], mask.shape)[-1] | _flags(c["truncated"], mask.shape)[-1]
        goes_on = mask[-1] & ~done
        want = np.where(goes_on, ref[-1], LD(0))
        assert (np.abs(_f64(new_ret).astype(LD) - want) <= np.where(goes_on, tol[-1], 0)).all(), f"{what}: the running return"
    nz = tol[mask] > 0
    return float((err[nz] / tol[mask][nz]).max()) if nz.any() else 0.0


def moments_bounds(R, blocks, folds, A, m2, B):
    """tests/test_norm.py::test_moments_agree_with_extended_precision's bound,
    unchanged: u = 2^-53, leaves of B rows, D = tree levels over the largest
    call's ``blocks`` leaves plus one per fold into the running statistics, R rows
    counted in all, A = max |x| of the column.  (E_mean, E_M2)"""
    u = 2.0 ** -53
    D = (int(np.ceil(np.log2(blocks))) if blocks > 1 else 0) + folds
    e_mean = 2 * (B + 1 + 7 * D) * u * A
    e_m2 = 2 * (B + 3 + 6 * D) * u * np.asarray(m2, F64) + 3 * D * R * A * e_mean + R * e_mean ** 2
    return e_mean, e_m2


def check_moments(stats, batches, masks, B, what, **kw):
    """statistics [3, cols] (count, mean, M2) against running_mean_var over the batches"""
    stats = _f64(stats)
    masks = [None] * len(batches) if masks is None else masks
    count, mean, var = running_mean_var(batches, masks, **kw)
    kept = [np.asarray(x) if m is None else np.asarray(x)[np.asarray(m).astype(bool)] for x, m in zip(batches, masks)]
    R = sum(k.shape[0] for k in kept)
    c_err = np.abs(stats[0].astype(LD) - count).astype(F64)          # one rounded addition per fold
    assert (c_err <= len(batches) * 2.0 ** -53 * float(count)).all(), f"{what}: count {stats[0][:3]} != {float(count)!r}"
    A = np.max([np.abs(k.astype(F64)).max(0) for k in kept if k.size], axis=0)       # per column
    blocks = max(-(-np.asarray(x).shape[0] // B) for x in batches)
    m2 = (var * count).astype(F64)
    e_mean, e_m2 = moments_bounds(R, blocks, len(batches), A, m2, B)
    err_mean = np.abs(stats[1].astype(LD) - mean).astype(F64)
    err_m2 = np.abs(stats[2].astype(LD) - var * count).astype(F64)
    assert (err_mean <= e_mean).all(), f"{what}: mean off by up to {err_mean.max():.3e}, bound {e_mean.max():.3e}"
    assert (err_m2 <= e_m2).all(), f"{what}: M2 off by {(err_m2 / e_m2).max():.3g} bounds"
    nz = e_mean > 0
    return float((err_mean[nz] / e_mean[nz]).max()) if nz.any() else 0.0, float((err_m2 / e_m2).max())


def check_scale_shift(scale, shift, mean, var, eps, what):
    """float32 rows within one float32 ulp of the float64 reference"""
    for got, ref, name in zip((scale, shift), scale_shift(mean, var, eps), ("scale", "shift")):
        got, ref = _f64(got), ref.astype(F64)
        ulp = np.spacing(np.abs(ref).astype(F32)).astype(F64)
        assert (np.abs(got - ref) <= ulp).all(), f"{what}: {name} off by {float((np.abs(got - ref) / ulp).max()):.3g} ulp"


def check_reward_norm(got, reward, var, eps, clip, what):
    """within 4 x 2^-53 relative of clip(r / sqrt(var + eps), +-clip)"""
    ref = reward_norm(reward, var, eps, clip)
    err = np.abs(_f64(got).astype(LD).reshape(ref.shape) - ref)
    assert (err <= 4 * 2.0 ** -53 * np.abs(ref)).all(), f"{what}: reward_norm off by {float(err.max()):.3e}"
