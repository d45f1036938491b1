"""CPU: the MLP actor's public pieces that need no GPU: the ctypes mirror of
invsim_mlp_spec against the header, MLPPolicyAgent's construction and
validation, and the CPU restatement (tests/mlp_model.py): its fmaf emulation
against the C library's through a compiled probe, its conversion against
invsim.policies.convert_actions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mlp_model
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "invsim.h")


def test_mlp_spec_layout_matches_header(tmp_path):
    from invsim import _capi
    names = [f for f, _ in _capi.MLPSpec._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(invsim_mlp_spec));']
    lines += [f'printf("{n} %zu\\n", offsetof(invsim_mlp_spec, {n}));' for n in names]
    lines += ['printf("consts %d %d %d %d %d\\n", INVSIM_MLP_NONE, INVSIM_MLP_RELU, INVSIM_MLP_TANH, '
              'INVSIM_MLP_MAX_LAYERS, INVSIM_MLP_MAX_WIDTH);', "return 0;}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.strip().split("\n"))
    assert int(got["size"]) == C.sizeof(_capi.MLPSpec)
    for n in names:
        assert int(got[n]) == getattr(_capi.MLPSpec, n).offset, n
    assert got["consts"].split() == [str(_capi.MLP_ACTIVATIONS[k]) for k in (None, "relu", "tanh")] + [
        str(_capi.MLP_MAX_LAYERS), str(_capi.MLP_MAX_WIDTH)]
    lib = _capi.load_library()
    for f in ("invsim_mlp_create", "invsim_mlp_destroy", "invsim_mlp_actions", "invsim_rollout_mlp"):
        assert f in _capi.EXPORTS and hasattr(lib, f)


def _lin(i, o, bias=True):
    return torch.nn.Linear(i, o, bias=bias)


def test_from_module():
    import invsim
    nn = torch.nn
    torch.manual_seed(1)
    seq = nn.Sequential(_lin(7, 5), nn.ReLU(), _lin(5, 4, bias=False), nn.ReLU(), _lin(4, 2))
    ag = invsim.MLPPolicyAgent.from_module(seq, clip=False, name="x")
    assert ag.dims == [7, 5, 4, 2] and ag.activation == "relu" and ag.out_activation is None
    assert ag.clip is False and ag.name == "x" and ag.biases[1] is None
    for w, m in zip(ag.weights, (seq[0], seq[2], seq[4])):
        assert w.dtype == np.float32 and w.flags["C_CONTIGUOUS"] and np.array_equal(w, m.weight.detach().numpy())
    assert np.array_equal(ag.biases[2], seq[4].bias.detach().numpy())
    sq = invsim.MLPPolicyAgent.from_module(nn.Sequential(_lin(3, 4).double(), nn.Tanh(), _lin(4, 2), nn.Tanh()))
    assert sq.activation == "tanh" and sq.out_activation == "tanh" and sq.weights[0].dtype == np.float32
    one = invsim.MLPPolicyAgent.from_module(nn.Sequential(_lin(3, 2)))
    assert one.dims == [3, 2] and one.out_activation is None
    for bad in (nn.Sequential(_lin(3, 4), nn.Sigmoid(), _lin(4, 2)),            # another module
                nn.Sequential(_lin(3, 4), nn.ReLU(), _lin(4, 4), nn.Tanh(), _lin(4, 2)),   # mixed
                nn.Sequential(_lin(3, 4), _lin(4, 2)),                           # no activation between
                nn.Sequential(nn.ReLU(), _lin(3, 2)),
                nn.Sequential(_lin(3, 4), nn.ReLU(), _lin(4, 2), nn.ReLU()),     # ReLU output
                _lin(3, 2)):                                                     # not a Sequential
        with pytest.raises(TypeError):
            invsim.MLPPolicyAgent.from_module(bad)


def test_python_side_validation(monkeypatch):
    """refused in Python, before any library call"""
    import invsim
    from invsim import _capi
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library was called"))
    z = lambda o, i: (np.zeros((o, i), np.float32), np.zeros(o, np.float32))  # noqa: E731
    with pytest.raises(ValueError, match="256"):
        invsim.MLPPolicyAgent([z(257, 3), z(2, 257)])
    invsim.MLPPolicyAgent([z(256, 3), z(2, 256)])
    with pytest.raises(ValueError, match="layers"):
        invsim.MLPPolicyAgent([z(4, 3)] + [z(4, 4)] * 4 + [z(2, 4)])
    invsim.MLPPolicyAgent([z(4, 3)] + [z(4, 4)] * 3 + [z(2, 4)])
    with pytest.raises(ValueError, match="pairs"):
        invsim.MLPPolicyAgent([z(2, 3)], in_scale=np.ones(3))
    with pytest.raises(ValueError, match="pairs"):
        invsim.MLPPolicyAgent([z(2, 3)], out_shift=np.ones(2))
    with pytest.raises(ValueError):
        invsim.MLPPolicyAgent([z(4, 3), z(2, 5)])               # widths do not chain
    with pytest.raises(ValueError):
        invsim.MLPPolicyAgent([z(2, 3)], in_scale=np.ones(4), in_shift=np.ones(4))
    with pytest.raises(ValueError):
        invsim.MLPPolicyAgent([z(2, 3)], activation="gelu")
    with pytest.raises(ValueError, match="obs0"):
        invsim.rollout_policy(None, invsim.MLPPolicyAgent([z(2, 3)]), 3)


# ---------------------------------------------------------------- fmaf emulation
def _triples(n=1 << 16):
    rng = np.random.default_rng(5)
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    parts = []
    parts.append([f(rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)) for _ in range(3)])   # random, wide range
    parts.append([f(rng.integers(-4096, 4096, n)) for _ in range(3)])                         # integer lattice: exact
    # half-ulp ties: a * b = m * 2**-24 with odd m against c = 1 (ulp 2**-23), and near misses
    m = rng.integers(-2 ** 12, 2 ** 12, n) * 2 + 1
    tie = [f(m), f(np.full(n, 2.0 ** -24)), f(rng.choice([1.0, -1.0, 1.0 + 2.0 ** -23, 3.0], n))]
    parts.append(tie)
    near = [f(m) * f(1 + 2.0 ** -23 * rng.integers(-1, 2, n)), tie[1], tie[2]]
    parts.append(near)
    # wide products whose low bits straddle the addend's half ulp
    a = f(1 + rng.integers(0, 2 ** 23, n) * 2.0 ** -23)
    b = f(1 + rng.integers(0, 2 ** 23, n) * 2.0 ** -23)
    parts.append([a, b, f(-(a.astype(np.float64) * b).astype(np.float32))])                 # cancellation: exact residue
    parts.append([a, b, f(rng.choice([2.0 ** 24, -2.0 ** 24, 2.0 ** 25, 2.0 ** -30], n))])
    # subnormal results and operands
    parts.append([f(rng.standard_normal(n) * 1e-20), f(rng.standard_normal(n) * 1e-20),
                  f(rng.standard_normal(n) * 1e-41)])
    parts.append([f(rng.standard_normal(n) * 1e-39), f(rng.standard_normal(n)), f(rng.standard_normal(n) * 1e-39)])
    # signed zeros, infinities, NaN
    sp = f([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 3.4e38, 1e-45])
    g = np.stack(np.meshgrid(sp, sp, sp, indexing="ij"), -1).reshape(-1, 3)
    parts.append([g[:, 0], g[:, 1], g[:, 2]])
    return [np.concatenate([p[k] for p in parts]) for k in range(3)]


def test_fmaf_emulation_equals_libm(tmp_path):
    a, b, c = _triples()
    src = tmp_path / "fma.c"
    src.write_text("""#include <math.h>
#include <stdio.h>
int main(int argc, char **argv) {
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    float t[3];
    if (!fi || !fo) return 1;
    while (fread(t, sizeof(float), 3, fi) == 3) { float r = fmaf(t[0], t[1], t[2]); fwrite(&r, sizeof r, 1, fo); }
    fclose(fo);
    return 0;
}
""")
    exe = tmp_path / "fma"
    subprocess.run(["gcc", "-O1", "-std=c11", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    np.stack([a, b, c], 1).astype(np.float32).tofile(tmp_path / "in.bin")
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    exp = np.fromfile(tmp_path / "out.bin", np.float32)
    got = mlp_model.fmaf(a, b, c)
    assert exp.shape == got.shape and len(got) > 500000
    nan = np.isnan(exp)
    assert np.array_equal(nan, np.isnan(got))
    bad = np.flatnonzero((got.view(np.int32) != exp.view(np.int32)) & ~nan)
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], exp[i]) for i in bad[:5]]
    # the cases that tell a fused from an unfused multiply-add are in the set
    with np.errstate(all="ignore"):
        unfused = (a * b + c).astype(np.float32)
    assert int(((unfused.view(np.int32) != exp.view(np.int32)) & ~nan).sum()) > 1000


# ---------------------------------------------------------------- conversion
@pytest.mark.parametrize("dtype", [np.int64, np.float32])
@pytest.mark.parametrize("clip", [True, False])
def test_conversion_equals_convert_actions(dtype, clip):
    from invsim.policies import convert_actions
    if dtype == np.int64:
        low, high = np.array([0, 0, -5, 0], np.int64), np.array([100, 2 ** 40, 5, 0], np.int64)
    else:
        low = np.array([0.0, 0.0, -5.0, -np.inf], np.float32)
        high = np.array([100.0, np.inf, 5.0, 0.0], np.float32)
    edge = [np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, -0.5, 0.999, -0.999, 1.5, -1.5, 99.999, 100.0, 100.5, 1e9, -1e9,
            5.0, -5.0, 5.0000005, -5.0000005, 4.9999995, 2.0 ** 40, 2.0 ** 41, 1e-45, -1e-45, 3.7, -3.7]
    if not clip:          # a cast alone: the int64 range is the caller's business
        edge = [v for v in edge if dtype == np.float32 or (np.isfinite(v) and abs(v) < 2 ** 62)]
    raw = np.repeat(np.asarray(edge, np.float32)[:, None], 4, 1)
    got = mlp_model.convert(raw, low, high, dtype, clip)
    t = torch.from_numpy(raw)
    tdt = torch.int64 if dtype == np.int64 else torch.float32
    exp = (convert_actions(t, low, high, tdt) if clip else t.to(tdt)).numpy()
    assert got.dtype == exp.dtype == np.dtype(dtype)
    w = np.int64 if dtype == np.int64 else np.int32
    assert np.array_equal(got.view(w), exp.view(w)), np.argwhere(got.view(w) != exp.view(w))[:5]
    if clip and dtype == np.float32:
        neg0 = edge.index(-0.0)
        assert np.signbit(got[neg0, 2]) and not np.signbit(got[neg0, 0]), "-0.0 inside passes; at a zero bound it is +0.0"
        assert not np.signbit(got[neg0, 3]) and np.isnan(got[0]).all()
    if clip and dtype == np.int64:
        assert (got[0] == 0).all() and got[1].tolist() == high.tolist() and got[2].tolist() == low.tolist()
