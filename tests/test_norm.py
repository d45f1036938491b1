"""CPU: the running-normalisation ABI is declared and exported, the numpy
restatement of its contract (tests/norm_model.py, which the GPU tests hold the
kernels against) equals an independently written scalar loop bit for bit and
agrees with the textbook moments in extended precision, masks and reset rows
behave as the contract says, and the Python wrappers refuse wrong shapes and
dtypes before any library call.

stable-baselines3 is not a dependency of this repository: the rule of its
RunningMeanStd (count 1e-4, mean 0, variance 1 at construction;
update_from_moments' parallel-variance formula) is restated here, not imported."""
import os
import re

import numpy as np
import pytest

import gae_model
import norm_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("invsim_moments_scratch_bytes", "invsim_moments", "invsim_discounted_returns", "invsim_normalize_rewards",
       "invsim_norm_params", "invsim_mlp_set_input_norm")
F32, F64 = np.float32, np.float64
B = nm.BLOCK
ROWS = [1, B - 1, B, B + 1, 2 * B + 1, 5 * B + 3, 37 * B + 5]


def _same(a, b, what):
    """the same bits; a NaN equals any NaN, and only a NaN"""
    x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {x.shape} {x.dtype} vs {y.shape} {y.dtype}"
    both_nan = np.zeros(x.shape, bool)
    if x.dtype.kind == "f":
        both_nan = np.isnan(x) & np.isnan(y)
        x, y = x.view(f"i{x.dtype.itemsize}"), y.view(f"i{y.dtype.itemsize}")
    ne = (x != y) & ~both_nan
    assert not ne.any(), f"{what}: {int(ne.sum())} differ, first at {np.argwhere(ne)[:4].tolist()}"


def _data(rows, cols, dtype, seed, specials=False):
    rng = np.random.default_rng(seed)
    if dtype == np.int64:
        x = rng.integers(0, 400, (rows, cols))
        x[::23, min(1, cols - 1)] = 2 ** 24 + 1                 # float32 cannot hold these
        x[::31, 0] = -(2 ** 40) - 2 ** 15 - 1
        return x
    x = rng.uniform(-50, 400, (rows, cols)).astype(dtype)
    if specials:
        vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
        hit = rng.random((rows, cols)) < 0.01
        x[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))].astype(dtype)
    return x


def test_symbols_declared_and_exported():
    from invsim import _capi
    text = open(os.path.join(ROOT, "include", "invsim.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(invsim_[a-z_0-9]+)\s*\(", src))
    lib = _capi.load_library()
    for s in NEW:
        assert s in declared, f"{s} is not declared in include/invsim.h"
        assert s in _capi.EXPORTS, f"{s} is not in _capi.EXPORTS"
        assert hasattr(lib, s), f"libinvsim.so does not export {s}"
    assert lib.invsim_abi_version() == 4 == _capi.ABI_VERSION
    assert "Running normalisation" in text
    for name, code in (("I64", _capi.DTYPE_I64), ("F32", _capi.DTYPE_F32), ("F64", _capi.DTYPE_F64)):
        assert re.search(rf"^#define\s+INVSIM_DTYPE_{name}\s+{code}\b", text, re.M), name
    assert B >= 1 and (B * 4) % 16 == 0


def test_scratch_bytes_and_host_refusals():
    """every refusal is made on the host: these run without a device"""
    import ctypes as C
    from invsim import _capi
    lib = _capi.load_library()
    n = C.c_int64(-1)
    assert lib.invsim_moments_scratch_bytes(30 * 65536, 33, C.byref(n)) == 0 and n.value >= 3 * 33 * 8
    big = C.c_int64()
    assert lib.invsim_moments_scratch_bytes(31 * 1048576, 33, C.byref(big)) == 0 and big.value > n.value
    assert lib.invsim_moments_scratch_bytes(-1, 33, C.byref(n)) == -22
    assert lib.invsim_moments_scratch_bytes(10, 0, C.byref(n)) == -22
    assert lib.invsim_moments_scratch_bytes(10, 1025, C.byref(n)) == -34
    buf = np.zeros(64, F64)
    p = buf.ctypes.data
    assert lib.invsim_moments(p, 3, 4, 1, None, p, p, 1 << 20, None) == -22, "unknown dtype"
    assert lib.invsim_moments(p, 0, -1, 1, None, p, p, 1 << 20, None) == -22
    assert lib.invsim_moments(p, 0, 4, 0, None, p, p, 1 << 20, None) == -22
    assert lib.invsim_moments(p, 0, 4, 1025, None, p, p, 1 << 20, None) == -34
    assert lib.invsim_moments(None, 0, 0, 1, None, None, None, 0, None) == 0, "rows == 0 is a no-op"
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.invsim_moments(args[0], 0, 4, 1, None, args[1], args[2], 1 << 20, None) == -22
    assert lib.invsim_moments(p, 0, 4, 1, None, p, p, 8, None) == -34, "scratch too small"
    assert lib.invsim_discounted_returns(p, None, None, None, -1, 4, 0.99, p, p, None, None) == -22
    assert lib.invsim_discounted_returns(None, None, None, None, 0, 4, 0.99, None, None, None, None) == 0
    assert lib.invsim_discounted_returns(None, None, None, None, 2, 4, 0.99, p, p, None, None) == -22
    assert lib.invsim_discounted_returns(p, None, None, None, 2, 4, 0.99, None, p, None, None) == -22
    for clip in (0.0, -1.0, float("nan")):
        assert lib.invsim_normalize_rewards(p, 4, p, 1e-8, clip, p, None) == -22, clip
    assert lib.invsim_normalize_rewards(p, -1, p, 1e-8, 10.0, p, None) == -22
    assert lib.invsim_normalize_rewards(None, 0, None, 1e-8, 10.0, None, None) == 0
    assert lib.invsim_normalize_rewards(p, 4, None, 1e-8, 10.0, p, None) == -22
    assert lib.invsim_norm_params(p, 0, 1e-8, p, p, None) == -22
    assert lib.invsim_norm_params(p, 1025, 1e-8, p, p, None) == -34
    assert lib.invsim_norm_params(None, 4, 1e-8, p, p, None) == -22
    assert lib.invsim_norm_params(p, 4, 1e-8, None, p, None) == -22
    assert lib.invsim_mlp_set_input_norm(None, None, p, p, None) == -22


# ---------------------------------------------------------------- the model against a scalar loop
def _merge_scalar(a, b):
    (na, ma, qa), (nb, mb, qb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    w = nb / n
    return n, ma + d * w, (qa + qb) + (d * d) * (na * w)


def _moments_scalar(x, mask, stats):
    """the header's text, one column, one block and one Python float operation at a time"""
    rows, cols = x.shape
    out = np.array(stats, F64)
    for c in range(cols):
        nodes = []
        for b0 in range(0, rows, B):
            idx = [r for r in range(b0, min(b0 + B, rows)) if mask is None or mask[r]]
            if not idx:
                nodes.append((0.0, 0.0, 0.0))
                continue
            n, s = float(len(idx)), 0.0
            for r in idx:
                s = s + float(x[r, c])
            mean, q = s / n, 0.0
            for r in idx:
                d = float(x[r, c]) - mean
                q = q + d * d
            nodes.append((n, mean, q))
        while len(nodes) > 1:
            up = [_merge_scalar(nodes[i], nodes[i + 1]) for i in range(0, len(nodes) - 1, 2)]
            nodes = up + ([nodes[-1]] if len(nodes) % 2 else [])
        out[:, c] = _merge_scalar(tuple(float(v) for v in out[:, c]), nodes[0])
    return out


@pytest.mark.parametrize("dtype", [np.int64, np.float32, np.float64], ids=["i64", "f32", "f64"])
@pytest.mark.parametrize("rows", ROWS)
def test_moments_model_equals_scalar_loop(rows, dtype):
    x = _data(rows, 3, dtype, seed=rows, specials=dtype != np.int64)
    rng = np.random.default_rng(rows + 1)
    off = np.ones(rows, np.uint8)
    off[B:2 * B] = 0                                             # one whole block off (where there is one)
    masks = [None, (rng.random(rows) < 0.6).astype(np.uint8), off, np.zeros(rows, np.uint8)]
    for i, mask in enumerate(masks):
        got = nm.moments(x, mask)
        _same(got, _moments_scalar(x, mask, nm.prior(3)), f"rows={rows} mask {i}")
        again = nm.moments(x[::-1], None, got)                   # the running merge: a second call on the result
        _same(again, _moments_scalar(x[::-1], None, got), f"rows={rows} mask {i}: second call")
    if dtype != np.int64 and rows == ROWS[-1]:
        assert np.isnan(got).any() or np.isnan(nm.moments(x)).any(), "the special values reach the statistics"


def test_moments_agree_with_extended_precision():
    """mean and M2 after folding a batch into the 1e-4 prior, against np.mean / np.var in
    long double combined by RunningMeanStd.update_from_moments' formula.  The bound
    counts operations (u = 2^-53, A = max |x|, R rows, D = tree levels with the final
    fold): a leaf's mean carries the B - 1 additions and one division of its sum, each
    merge level adds 7 roundings on quantities bounded by 2A (d, w, d * w, the sum; the
    children's errors combine convexly), so E_mean = 2 (B + 1 + 7 D) u A, the factor 2
    covering the second-order terms.  M2 is a sum of non-negative terms: B - 1 additions
    and 3 roundings per squared deviation in a leaf, 6 roundings per merge level, give
    the relative part 2 (B + 3 + 6 D) u M2; the squared mean differences inherit the
    means' absolute errors, |d^2 - dref^2| <= 12 A E_mean with weight n_a n_b / n <= n / 4
    and the n of a level summing to R, which adds 3 D R A E_mean; the leaves measure
    deviations from their rounded mean, which adds at most R E_mean^2."""
    LD = np.longdouble
    u = 2.0 ** -53
    for rows, dtype in ((4099, np.float64), (4099, np.int64), (B * 37 + 5, np.float32), (B, np.float64)):
        x = _data(rows, 3, dtype, seed=7)
        if dtype == np.int64:
            x = np.minimum(np.abs(x), 2 ** 24 + 1)               # keep A at the scale of the data
        got = nm.moments(x)
        xl = x.astype(LD)
        bm, bv, bc = xl.mean(0), xl.var(0), LD(rows)
        mean0, var0, count0 = LD(0), LD(1), LD(1e-4)
        delta, tot = bm - mean0, count0 + bc
        want_mean = mean0 + delta * bc / tot
        want_m2 = var0 * count0 + bv * bc + delta * delta * count0 * bc / tot
        A = float(np.abs(x).max())
        D = int(np.ceil(np.log2(-(-rows // B)))) + 1 if rows > B else 1
        e_mean = 2 * (B + 1 + 7 * D) * u * A
        e_m2 = 2 * (B + 3 + 6 * D) * u * want_m2.astype(F64) + 3 * D * rows * A * e_mean + rows * e_mean ** 2
        err_mean = np.abs(got[1].astype(LD) - want_mean).astype(F64)
        err_m2 = np.abs(got[2].astype(LD) - want_m2).astype(F64)
        print(f"rows={rows} {np.dtype(dtype).name}: mean err {err_mean.max():.3e} (bound {e_mean:.3e}), "
              f"M2 rel err {(err_m2 / want_m2.astype(F64)).max():.3e} (bound rel {(e_m2 / want_m2.astype(F64)).min():.3e})")
        assert (got[0] == 1e-4 + rows).all()
        assert (err_mean <= e_mean).all(), (rows, dtype, err_mean, e_mean)
        assert (err_m2 <= e_m2).all(), (rows, dtype, err_m2, e_m2)


def test_masks():
    rows = 4 * B
    x = _data(rows, 5, np.float64, seed=3)
    stats = nm.moments(_data(100, 5, np.float64, seed=4))
    # a fully masked call leaves the statistics bit-identical
    _same(nm.moments(x, np.zeros(rows, np.uint8), stats), stats, "fully masked")
    # rows masked inside one leaf: the leaf of the remaining rows
    m = (np.random.default_rng(0).random(B) < 0.5).astype(np.uint8)
    _same(nm.moments(x[:B], m, stats), nm.moments(x[:B][m.astype(bool)], None, stats), "rows removed inside a leaf")
    # the last block masked out: the tree ((0, 1), (2, -)) is the tree of the first three blocks
    last = np.ones(rows, np.uint8)
    last[3 * B:] = 0
    _same(nm.moments(x, last, stats), nm.moments(x[:3 * B], None, stats), "last block off")
    # a middle block masked out keeps its place in the tree: (0, (2, 3)), which removing the rows does not give
    mid = np.ones(rows, np.uint8)
    mid[B:2 * B] = 0
    lv = nm.leaves(x)
    want = nm.merge(stats, nm.merge(lv[:, 0], nm.merge(lv[:, 2], lv[:, 3])))
    _same(nm.moments(x, mid, stats), want, "middle block off")
    removed = nm.moments(np.concatenate([x[:B], x[2 * B:]]), None, stats)
    assert (removed[0] == nm.moments(x, mid, stats)[0]).all(), "the counts agree either way"


# ---------------------------------------------------------------- discounted returns, rewards, parameters
def _returns_scalar(c, gamma, ret):
    rew, te, tr, d0 = (c[k] for k in ("reward", "terminated", "truncated", "done0"))
    K, n = rew.shape
    out, valid, ret = np.zeros((K, n), F64), np.zeros((K, n), np.uint8), np.array(ret, F64)
    for e in range(n):
        acc = float(ret[e])
        prev = bool(d0[e]) if d0 is not None else False
        for k in range(K):
            done = (bool(te[k, e]) if te is not None else False) or (bool(tr[k, e]) if tr is not None else False)
            if prev:
                out[k, e], valid[k, e], acc = 0.0, 0, 0.0
            else:
                t = acc * float(gamma)
                acc = t + float(rew[k, e])
                out[k, e], valid[k, e] = acc, 1
                if done:
                    acc = 0.0
            prev = done
        ret[e] = acc
    return out, valid, ret


@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_returns_model_equals_scalar_loop_and_stops_at_reset_rows(K):
    n = 197
    for seed, gamma in enumerate((0.99, 1.0, 0.0, 0.5)):
        c = gae_model.synthetic(K, n, seed=seed)
        assert len(set(((np.arange(n) + seed) % gae_model.PATTERNS).tolist())) == gae_model.PATTERNS
        ret0 = np.random.default_rng(seed).uniform(-1e3, 1e3, n)
        for drop in (None, "terminated", "truncated", "done0"):
            d = dict(c, **({drop: None} if drop else {}))
            got = nm.discounted_returns(d["reward"], d["terminated"], d["truncated"], d["done0"], gamma, ret0)
            for g, w, what in zip(got, _returns_scalar(d, gamma, ret0), ("out", "valid", "ret")):
                _same(g, w, f"K={K} gamma={gamma} without {drop}: {what}")
    # the reset rows: masked, +0.0, and the return restarts from the reward after them
    c = gae_model.synthetic(K, n, seed=1, specials=False)
    out, valid, ret = nm.discounted_returns(c["reward"], c["terminated"], c["truncated"], c["done0"], 0.99, np.ones(n))
    done = (c["terminated"] | c["truncated"]).astype(bool)
    prev = np.concatenate([c["done0"][None].astype(bool), done[:-1]])
    assert (valid == ~prev).all()
    assert (out[prev].view(np.int64) == 0).all(), "+0.0 on reset rows"
    fresh = np.zeros_like(prev)
    fresh[1:] = prev[:-1] & ~prev[1:]                            # the first row of a new episode inside the block
    _same(out[fresh], (0.0 * 0.99 + c["reward"])[fresh], "the return restarts after a reset row")
    assert (ret[done[-1] | prev[-1]].view(np.int64) == 0).all()


def test_reward_and_parameter_models():
    rng = np.random.default_rng(5)
    r = rng.uniform(-2e3, 2e3, 500)
    r[:4] = [np.nan, np.inf, -np.inf, -0.0]
    stats = np.array([[1000.0], [3.0], [1000.0 * 250.0 ** 2]])
    out = nm.normalize_rewards(r, stats, 1e-8, 10.0)
    want = np.clip(r / np.sqrt(250.0 ** 2 + 1e-8), -10.0, 10.0)
    _same(out, want, "np.clip(reward / np.sqrt(var + eps), -clip, clip)")
    assert np.isnan(out[0]) and out[1] == 10.0 and out[2] == -10.0 and (np.abs(out[4:]) < 10).any()
    empty = np.zeros((3, 1))
    _same(nm.normalize_rewards(r[4:], empty, 0.0, 1e9), r[4:], "cnt == 0: variance 1")
    st = nm.moments(_data(300, 4, np.int64, seed=2))
    scale, shift = nm.norm_params(st, 1e-8)
    assert scale.dtype == F32 and shift.dtype == F32
    var = st[2] / st[0]
    _same(scale, (1.0 / np.sqrt(var + 1e-8)).astype(F32), "scale")
    _same(shift, (-(st[1] * (1.0 / np.sqrt(var + 1e-8)))).astype(F32), "shift")
    x = np.array([10.0, -3.0, 250.0, 7.0], F32)
    z = x.astype(F64) * scale.astype(F64) + shift.astype(F64)
    assert np.allclose(z, (x - st[1]) / np.sqrt(var + 1e-8), rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- the Python wrappers
def test_wrappers_refuse_before_any_library_call(monkeypatch):
    import torch
    import invsim
    from invsim import _capi, policies

    def no_library():
        raise AssertionError("a refusal must come before the library is touched")
    monkeypatch.setattr(_capi, "lib", no_library)
    with pytest.raises(ValueError):
        invsim.RunningMoments(0, "cpu")
    with pytest.raises(ValueError):
        invsim.RunningMoments(1025, "cpu")
    rm = invsim.RunningMoments(3, "cpu")
    _same(rm.stats.numpy(), nm.prior(3), "the prior")
    assert rm.count.shape == (3,) and float(rm.var[0]) == 1.0 and float(rm.mean[0]) == 0.0
    with pytest.raises(TypeError):
        rm.update(np.zeros((4, 3)))
    with pytest.raises(TypeError):
        rm.update(torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(TypeError):
        rm.update(torch.zeros((4, 3), dtype=torch.float16))
    with pytest.raises(ValueError):
        rm.update(torch.zeros((4, 2)))
    with pytest.raises(ValueError):
        rm.update(torch.zeros((4, 3)), mask=torch.ones(5, dtype=torch.bool))
    rm.update(torch.zeros((0, 3)))                               # no rows: nothing to do
    r = torch.zeros((5, 7), dtype=torch.float64)
    with pytest.raises(ValueError):
        policies.discounted_returns(r, None, None, torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError):
        policies.discounted_returns(r, None, None, torch.zeros(7, dtype=torch.float32))
    with pytest.raises(TypeError):
        policies.discounted_returns(r.float(), None, None, torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError):
        policies.discounted_returns(r, torch.zeros((5, 6), dtype=torch.bool), None, torch.zeros(7, dtype=torch.float64))
    st = torch.zeros((3, 1), dtype=torch.float64)
    with pytest.raises(TypeError):
        policies.normalize_rewards(r.float(), st)
    with pytest.raises(ValueError):
        policies.normalize_rewards(r, torch.zeros((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        policies.normalize_rewards(r, st, clip=0.0)
    with pytest.raises(ValueError):
        policies.normalize_rewards(r, st, out=torch.zeros((5, 6), dtype=torch.float64))
    # set_input_norm: there is no env here at all
    rng = np.random.default_rng(0)
    layers = [(rng.standard_normal((8, 33)).astype(F32), None), (rng.standard_normal((1, 8)).astype(F32), None)]
    bare = invsim.ValueMLP(layers)
    ok = torch.ones(33)
    with pytest.raises(ValueError, match="in_scale"):
        bare.set_input_norm(None, ok, ok)
    critic = invsim.ValueMLP(layers, in_scale=np.ones(33, F32), in_shift=np.zeros(33, F32))
    with pytest.raises(ValueError):
        critic.set_input_norm(None, torch.ones(32), ok)
    with pytest.raises(TypeError):
        critic.set_input_norm(None, ok.double(), ok)
    with pytest.raises(TypeError):
        critic.set_input_norm(None, np.ones(33, F32), ok)
    actor = invsim.GaussianMLPPolicyAgent([(rng.standard_normal((3, 33)).astype(F32), None)], log_std=np.zeros(3, F32), seed=0)
    with pytest.raises(TypeError, match="Normalizer"):
        invsim.collect_rollout(None, actor, 3, None, normalize=object())
