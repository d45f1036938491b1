"""CPU: the critic / GAE / parameter-update ABI is declared and exported, the
numpy restatement of invsim_gae (tests/gae_model.py, which the GPU tests hold the
kernel against) equals an independently written scalar loop bit for bit and
has GAE's closed form, and the Python wrappers refuse wrong shapes before any
library call."""
import os
import re

import numpy as np
import pytest

import gae_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("invsim_mlp_create_value", "invsim_mlp_values", "invsim_gae", "invsim_mlp_update")
F32, F64 = np.float32, np.float64
GL = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.0), (0.98, 0.0)]


def test_symbols_declared_and_exported():
    from invsim import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "invsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(invsim_[a-z_0-9]+)\s*\(", src))
    lib = _capi.load_library()
    for s in NEW:
        assert s in declared, f"{s} is not declared in include/invsim.h"
        assert s in _capi.EXPORTS, f"{s} is not in _capi.EXPORTS"
        assert hasattr(lib, s), f"libinvsim.so does not export {s}"
    assert lib.invsim_abi_version() == 4 == _capi.ABI_VERSION
    assert "Critic, GAE and parameter updates" in open(os.path.join(ROOT, "include", "invsim.h")).read()


def _scalar(c, gamma, lam):
    """the header's recurrence, one env and one Python float operation at a time"""
    rew, te, tr, d0, v0, v = (c[k] for k in ("reward", "terminated", "truncated", "done0", "value0", "values"))
    K, n = rew.shape
    adv, ret, valid = np.zeros((K, n), F32), np.zeros((K, n), F32), np.zeros((K, n), np.uint8)
    gl = float(gamma) * float(lam)
    with np.errstate(all="ignore"):
        for e in range(n):
            carry = 0.0
            for k in range(K - 1, -1, -1):
                t_k = bool(te[k, e]) if te is not None else False
                done_k = t_k or (bool(tr[k, e]) if tr is not None else False)
                if k > 0:
                    prev = (bool(te[k - 1, e]) if te is not None else False) or (bool(tr[k - 1, e]) if tr is not None else False)
                    vp = float(v[k - 1, e])
                else:
                    prev = bool(d0[e]) if d0 is not None else False
                    vp = float(v0[e])
                vn = float(v[k, e])
                if prev:
                    adv[k, e], ret[k, e], valid[k, e], carry = 0.0, F32(vp), 0, 0.0
                    continue
                b = 0.0 if t_k else float(gamma) * vn
                delta = (float(rew[k, e]) + b) - vp
                a = delta if done_k else delta + gl * carry
                carry = a
                adv[k, e], ret[k, e], valid[k, e] = F32(a), F32(a + vp), 1
    return adv, ret, valid


def _same(a, b, what):
    """the same bits; a NaN equals any NaN (the sign and payload of a NaN are the
    arithmetic unit's, not the contract's), and only a NaN"""
    x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    both_nan = np.zeros(x.shape, bool)
    if x.dtype == F32:
        both_nan = np.isnan(x) & np.isnan(y)
        x, y = x.view(np.int32), y.view(np.int32)
    ne = (x != y) & ~both_nan
    assert not ne.any(), f"{what}: {int(ne.sum())} differ, first at {np.argwhere(ne)[:4].tolist()}"


@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 31])
@pytest.mark.parametrize("gamma,lam", GL)
def test_model_equals_scalar_loop(K, gamma, lam):
    c = gae_model.synthetic(K, 320, seed=K)
    pat = (np.arange(320) + K) % gae_model.PATTERNS
    assert len(set(pat.tolist())) == gae_model.PATTERNS
    got = gae_model.gae(c["reward"], c["terminated"], c["truncated"], c["done0"], c["value0"], c["values"], gamma, lam)
    for g, w, what in zip(got, _scalar(c, gamma, lam), ("advantages", "returns", "valid")):
        _same(g, w, f"K={K} gamma={gamma} lambda={lam}: {what}")
    # each flag array absent, and done0 absent
    for drop in ("terminated", "truncated", "done0"):
        d = dict(c, **{drop: None})
        got = gae_model.gae(d["reward"], d["terminated"], d["truncated"], d["done0"], d["value0"], d["values"], gamma, lam)
        for g, w, what in zip(got, _scalar(d, gamma, lam), ("advantages", "returns", "valid")):
            _same(g, w, f"K={K} without {drop}: {what}")


def test_inputs_cover_the_special_values():
    c = gae_model.synthetic(31, 2048, seed=0)
    r = c["reward"]
    assert np.isnan(r).any() and np.isposinf(r).any() and np.isneginf(r).any()
    assert ((r == 0) & np.signbit(r)).any() and ((r == 0) & ~np.signbit(r)).any()
    te, tr = c["terminated"].astype(bool), c["truncated"].astype(bool)
    d = te | tr
    assert d[0].any() and d[-1].any() and (d[:-1] & d[1:]).any()
    assert (te & ~tr).any() and (tr & ~te).any() and (te & tr).any()
    assert 0 < c["done0"].sum() < 2048 and (c["values"] < 0).any() and (c["values"] > 0).any()


@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.5])
def test_lambda_one_is_the_discounted_return(gamma):
    """No flags, lambda = 1: advantages[k] + V(input of step k) = sum_j gamma^(j-k) r_j
    + gamma^(K-k) V_last.  The recurrence adds, per row, the terms r_j, gamma v_j and
    -v_{j-1} (the value terms telescope); the closed form is evaluated in extended
    precision, so the difference is the recurrence's own rounding: at most one
    relative 2^-53 per operation on partial sums bounded by the sum of the terms'
    magnitudes, which over K rows is within K * 2^-52 * sum |terms|."""
    K, n = 31, 300
    c = gae_model.synthetic(K, n, seed=3, specials=False)
    v0, v, r = c["value0"], c["values"], c["reward"]
    *_, a64 = gae_model.gae(r, None, None, None, v0, v, gamma, 1.0, full=True)
    LD = np.longdouble
    vin = np.concatenate([v0[None], v[:-1]]).astype(F64)          # V of each step's input
    for k in (0, 1, K // 2, K - 1):
        w = LD(gamma) ** np.arange(K - k, dtype=LD)
        want = (w[:, None] * r[k:].astype(LD)).sum(0) + LD(gamma) ** (K - k) * v[K - 1].astype(LD)
        terms = (np.abs(w[:, None] * r[k:]).sum(0) + np.abs(w[:, None] * gamma * v[k:]).sum(0)
                 + np.abs(w[:, None] * vin[k:]).sum(0))
        err = np.abs((a64[k].astype(LD) + vin[k].astype(LD)) - want)
        bound = K * 2.0 ** -52 * terms
        assert (err <= bound).all(), (k, float(err.max()), float(bound.min()))
        assert float(err.max()) < 1e-6 * float(np.abs(want).max())


def test_reset_rows_are_masked_and_stop_the_carry():
    K, n = 9, 64
    c = gae_model.synthetic(K, n, seed=0, specials=False)
    te, tr = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    tr[3] = 1                                  # every env truncates at row 3: row 4 is the reset row
    adv, ret, valid = gae_model.gae(c["reward"], te, tr, None, c["value0"], c["values"], 0.99, 0.95)
    assert (valid[4] == 0).all() and (valid[np.arange(K) != 4] == 1).all()
    assert (adv[4].view(np.int32) == 0).all(), "+0.0f, not -0.0f"
    _same(ret[4], c["values"][3], "a reset row's return is V of its input")
    # rows 0..3 do not see anything after the truncation: change every later reward and value
    c2 = gae_model.synthetic(K, n, seed=5, specials=False)
    rew2, val2 = c["reward"].copy(), c["values"].copy()
    rew2[4:], val2[4:] = c2["reward"][4:], c2["values"][4:]
    adv2, ret2, _ = gae_model.gae(rew2, te, tr, None, c["value0"], val2, 0.99, 0.95)
    _same(adv2[:4], adv[:4], "advantages before the truncation"), _same(ret2[:4], ret[:4], "returns before it")
    # the truncated row bootstraps from its own (final) observation's value
    want = (c["reward"][3] + F64(0.99) * c["values"][3].astype(F64)) - c["values"][2].astype(F64)
    _same(adv[3], want.astype(F32), "truncation bootstrap")
    # done0 masks row 0
    d0 = (np.arange(n) % 2).astype(np.uint8)
    adv3, _, valid3 = gae_model.gae(c["reward"], te, tr, d0, c["value0"], c["values"], 0.99, 0.95)
    assert (valid3[0] == 1 - d0).all() and (adv3[0, d0 == 1].view(np.int32) == 0).all()


def test_update_layout_model():
    rng = np.random.default_rng(0)
    for out, inn in ((17, 33), (5, 17), (3, 5), (64, 33), (1, 64)):
        w, b = rng.standard_normal((out, inn)).astype(F32), rng.standard_normal(out).astype(F32)
        wt, bp = gae_model.blob_layout(w, b)
        flat = np.array([gae_model.update_store(w, d) for d in range(wt.size)], F32)
        _same(flat.reshape(wt.shape), wt, f"{out}x{inn}")
        assert wt.shape[1] % 4 == 0 and (wt[:, out:] == 0).all() and (bp[out:] == 0).all()


def _seq(dims, act):
    import torch
    mods = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(torch.nn.Linear(a, b))
        if i < len(dims) - 2:
            mods.append(act())
    return torch.nn.Sequential(*mods)


def test_value_mlp_needs_one_output():
    import torch
    import invsim
    rng = np.random.default_rng(0)
    two = [(rng.standard_normal((8, 33)).astype(F32), None), (rng.standard_normal((2, 8)).astype(F32), None)]
    with pytest.raises(ValueError, match="one unit"):
        invsim.ValueMLP(two)
    with pytest.raises(ValueError, match="one unit"):
        invsim.ValueMLP.from_module(_seq([33, 8, 3], torch.nn.ReLU))
    v = invsim.ValueMLP.from_module(_seq([33, 8, 1], torch.nn.ReLU))
    assert v.dims == [33, 8, 1] and v.activation == "relu" and v.clip is False and v.out_activation is None
    with pytest.raises(TypeError):
        invsim.ValueMLP.from_module(torch.nn.Sequential(torch.nn.Linear(33, 1), torch.nn.Tanh()))


def test_update_from_module_checks_shapes_first():
    """before any library call: there is no env here at all"""
    import torch
    import invsim
    actor = invsim.GaussianMLPPolicyAgent.from_module(_seq([33, 64, 64, 3], torch.nn.Tanh), log_std=np.zeros(3, F32), seed=0)
    critic = invsim.ValueMLP.from_module(_seq([33, 64, 64, 1], torch.nn.Tanh))
    for agent, bad in ((actor, [33, 64, 32, 3]), (actor, [33, 64, 3]), (critic, [33, 64, 64, 3]), (critic, [32, 64, 64, 1])):
        with pytest.raises(ValueError):
            agent.update_from_module(None, _seq(bad, torch.nn.Tanh))
    with pytest.raises(ValueError):
        actor.update_from_module(None, _seq([33, 64, 64, 3], torch.nn.Tanh), log_std=torch.zeros(4))
