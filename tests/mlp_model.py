"""CPU restatement of the MLP actor's arithmetic contract (include/invsim.h,
"MLP actor"): numpy float32 with an exact emulation of the fused multiply-add.

fmaf(a, b, c) for float32 a, b, c: the product of two float32 values is exact
in float64 (48 significant bits); the addend is added with a TwoSum, which
gives the float64 sum s and its exact error e; when e != 0 the sum is rounded
to odd (if the last mantissa bit of s is even, s moves one ulp toward the sign
of e), and a float64 rounded to odd rounds to the correctly rounded float32
(53 >= 2 * 24 + 2 bits: no double rounding).  tests/test_mlp_policy.py checks it
against the C library's fmaf through a compiled probe.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    """elementwise float32 fma(a, b, c) with one rounding (broadcasting)"""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact
        s = p + c
        t = s - p                                   # TwoSum (Knuth): s + e == p + c exactly
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32)


def _params(agent):
    """the fields of an invsim.MLPPolicyAgent (or any object with the same ones)"""
    return agent.weights, agent.biases, agent.activation, agent.out_activation


def forward(agent, obs, tanh=np.tanh):
    """raw float32 outputs [N, A] of the contract, op by op.  `tanh`: the float32
    tanh to use (the device's tanhf is not restated; ReLU / linear networks never
    call it)."""
    W, B, act, out_act = _params(agent)
    x = np.asarray(obs).astype(F32)                 # int64 -> float32: round to nearest
    if agent.in_scale is not None:
        x = fmaf(x, agent.in_scale[None, :], agent.in_shift[None, :])
    n = len(W)
    for l in range(n):
        w = np.asarray(W[l], F32)
        acc = np.zeros((x.shape[0], w.shape[0]), F32)
        if B[l] is not None:
            acc = acc + np.asarray(B[l], F32)[None, :]
        for i in range(w.shape[1]):                 # ascending input index: the contract's order
            acc = fmaf(w[None, :, i], x[:, i, None], acc)
        kind = out_act if l == n - 1 else act
        if kind == "relu":
            acc = np.where(acc > 0, acc, F32(0.0)).astype(F32)     # NaN -> +0.0
        elif kind == "tanh":
            acc = tanh(acc).astype(F32)
        x = acc
    if agent.out_scale is not None:
        x = fmaf(x, agent.out_scale[None, :], agent.out_shift[None, :])
    return x


def forward_f64(agent, obs):
    """the same graph evaluated in float64 (the yardstick of the tanh networks)"""
    W, B, act, out_act = _params(agent)
    x = np.asarray(obs).astype(F32).astype(F64)
    if agent.in_scale is not None:
        x = x * agent.in_scale.astype(F64)[None, :] + agent.in_shift.astype(F64)[None, :]
    n = len(W)
    for l in range(n):
        w = np.asarray(W[l], F64)
        acc = np.zeros((x.shape[0], w.shape[0]), F64)
        if B[l] is not None:
            acc = acc + np.asarray(B[l], F64)[None, :]
        for i in range(w.shape[1]):
            acc = acc + w[None, :, i] * x[:, i, None]
        kind = out_act if l == n - 1 else act
        if kind == "relu":
            acc = np.where(acc > 0, acc, 0.0)
        elif kind == "tanh":
            acc = np.tanh(acc)
        x = acc
    if agent.out_scale is not None:
        x = x * agent.out_scale.astype(F64)[None, :] + agent.out_shift.astype(F64)[None, :]
    return x


def convert(raw, low, high, dtype, clip=True):
    """raw float32 [..., A] -> actions of `dtype` (np.int64 or np.float32): the
    contract's conversion, which is invsim.policies.convert_actions"""
    raw = np.asarray(raw, F32)
    with np.errstate(all="ignore"):
        if np.dtype(dtype) == np.int64:
            x = raw.astype(F64)
            if clip:
                lo, hi = np.asarray(low).astype(F64), np.asarray(high).astype(F64)
                x = np.where(x < lo, lo, x)
                x = np.where(x > hi, hi, x)
            x = np.where(x != x, 0.0, x)
            return np.trunc(x).astype(np.int64)
        if not clip:
            return raw.copy()
        lo, hi = np.asarray(low, F32), np.asarray(high, F32)
        nan = raw != raw
        x = np.where((raw > lo) | nan, raw, lo)
        return np.where((x < hi) | nan, x, hi).astype(F32)
