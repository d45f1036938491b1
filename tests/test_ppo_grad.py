"""CPU: the PPO gradient contract without a GPU.  The float64 reference of
tests/ppo_reference.py is independent of the library; the float32 restatement of
the kernels' arithmetic (tests/ppo_model.py) is held to it at the tolerance the
GPU tests use, and eleven plausible mistakes in that arithmetic are each
rejected by the same comparison; invsim_ppo_scratch_bytes and the Python
wrappers' argument checks run on the host."""
import ast
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import ppo_model as pm
import ppo_reference as pr
from conftest import ROOT

EINVAL, ERANGE = -22, -34
MODELS = ("ppo_model", "mlp_model", "gaussian_model", "gae_model", "norm_model", "random_agent_model", "invsim")


def test_the_reference_imports_no_model_and_no_library():
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ppo_reference.py")).read())
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


def _worst(got, ref):
    return max(pr.compare(got[net], ref[net]) for net in ref)


def test_tolerance_is_four_times_torch_float32():
    """torch's own float32 CPU autograd of the reference loss, on every case, against
    the float64 result: GRAD_TOL is 4 x the recorded largest value and at most 1e-3"""
    largest, where = 0.0, None
    for name in pr.CASES:
        case, ref = pr.case_and_reference(name)
        m = _worst(pr.grads(case, torch.float32), ref)
        print(f"{name}: torch float32 autograd, largest metric {m:.3e}")
        if m > largest:
            largest, where = m, name
    print(f"largest {largest:.4e} ({where}); MEASURED_F32 {pr.MEASURED_F32:.4e}; GRAD_TOL {pr.GRAD_TOL:.2e}")
    digits = 10.0 ** (math.floor(math.log10(4 * pr.MEASURED_F32)) - 1)
    assert pr.GRAD_TOL == pytest.approx(math.ceil(4 * pr.MEASURED_F32 / digits) * digits, rel=1e-12)
    assert 0.5 * pr.MEASURED_F32 <= largest <= 1.25 * pr.MEASURED_F32, (largest, where)
    assert pr.GRAD_TOL <= 1e-3


def test_cases_cover_the_regions():
    """both clip sides and the unclipped region hold a real share of every larger case's samples,
    and the shapes the kernel treats differently are all there"""
    rows = set()
    for name in pr.CASES:
        case, ref = pr.case_and_reference(name)
        rows.add(case["rows"])
        assert np.all(case["adv"] != 0)
        if ref["actor"]["stats"][0] >= 40:
            assert 0.2 <= ref["actor"]["stats"][4] <= 0.8, (name, ref["actor"]["stats"])
    assert {1, 63, 64, 65, 197, 64 * pr.MAX_GROUPS + 65} <= rows, rows
    kinds = {(pr.CASES[n]["idx"], pr.CASES[n]["n0"] == 0, pr.CASES[n]["n0"] == pr.CASES[n]["S"]) for n in pr.CASES}
    assert {k[0] for k in kinds} == {None, "perm", "repeat", "seam"}
    assert any(k[1] for k in kinds) and any(k[2] for k in kinds)


@pytest.mark.parametrize("name", list(pr.CASES))
def test_model_against_the_reference(name):
    case, ref = pr.case_and_reference(name)
    got = pm.grads(case)
    m = _worst(got, ref)
    print(f"{name}: float32 model, largest metric {m:.3e} (GRAD_TOL {pr.GRAD_TOL:.2e})")
    assert m <= pr.GRAD_TOL, (name, m)


MISTAKE_CASE = "im-64x64-rows63"     # masked samples, advantage statistics, both affines, tanh layers, idx


@pytest.mark.parametrize("mistake", pm.MISTAKES)
def test_plausible_mistakes_are_rejected(mistake):
    case, ref = pr.case_and_reference(MISTAKE_CASE)
    assert _worst(pm.grads(case), ref) <= pr.GRAD_TOL
    m = _worst(pm.grads(case, mistake), ref)
    print(f"{mistake}: largest metric {m:.3e}")
    assert m > 10 * pr.GRAD_TOL, (mistake, m)


def test_all_masked_and_a2c_in_the_model():
    case, _ = pr.case_and_reference(MISTAKE_CASE)
    masked = np.flatnonzero(~case["valid"])[:3]
    for impl in (pm.grads, pr.grads):
        g = impl(case, idx=masked)
        for net in g:
            assert all(not np.any(t) for t in g[net]["weight"] + g[net]["bias"] + [g[net]["stats"]])
        assert not np.any(g["actor"]["log_std"])
    # A2C: clip_range = inf with old_logp = the current log-density is -mean(adv * logp)'s gradient
    cur = pr.current_log_prob(case)
    a2c = pr.grads(case, clip_range=float("inf"), old_logp=cur)["actor"]
    assert a2c["stats"][4] == 0 and a2c["stats"][5] == pytest.approx(1.0, abs=1e-12)


# ---------------------------------------------------------------- invsim_ppo_scratch_bytes
def _scratch(lib, dims, rows):
    d = np.asarray(dims, np.int32)
    out = C.c_int64(-1)
    rc = lib.invsim_ppo_scratch_bytes(d.ctypes.data if dims is not None else None, len(d) - 1, rows, C.byref(out))
    return rc, out.value


def test_scratch_bytes_on_the_host():
    from invsim import _capi
    lib = _capi.load_library()
    header = open(os.path.join(ROOT, "include", "invsim.h")).read()
    groups = int(re.search(r"#define INVSIM_PPO_MAX_GROUPS (\d+)", header).group(1))
    assert groups == pr.MAX_GROUPS == pm.MAX_GROUPS == _capi.PPO_MAX_GROUPS
    row_bytes, lds = re.search(r"\+ dims\[n_layers\]\) \* (\d+) > (\d+)", header).groups()
    row_bytes, lds = int(row_bytes), int(lds)
    assert (row_bytes, lds) == (260, 160 * 1024)
    dims = [33, 64, 64, 3]
    last = -1
    for rows in [0, 1, 63, 64, 65, 197, 4096, 64 * groups - 1, 64 * groups, 64 * groups + 65, 1 << 21, 1 << 40]:
        rc, b = _scratch(lib, dims, rows)
        assert rc == 0 and b >= last and b % 8 == 0, (rows, rc, b)
        last = b
    assert _scratch(lib, dims, 0)[1] == 0
    assert _scratch(lib, dims, 1 << 21)[1] == _scratch(lib, dims, 64 * groups)[1]      # at most `groups` partials
    params = sum((a + 1) * b for a, b in zip(dims[:-1], dims[1:])) + dims[-1]
    assert _scratch(lib, dims, 64)[1] >= 4 * params
    for bad, rows in [([33, 0, 3], 1), ([33, 257, 3], 1), ([0, 3], 1), ([33, 64, 33], 1), ([33, 64, 3], -1),
                      ([257, 3], 1), ([33, -5, 3], 1)]:
        assert _scratch(lib, bad, rows)[0] == EINVAL, bad
    out = C.c_int64()
    d = np.asarray(dims, np.int32)
    assert lib.invsim_ppo_scratch_bytes(None, 3, 1, C.byref(out)) == EINVAL
    assert lib.invsim_ppo_scratch_bytes(d.ctypes.data, 0, 1, C.byref(out)) == EINVAL
    assert lib.invsim_ppo_scratch_bytes(d.ctypes.data, 6, 1, C.byref(out)) == EINVAL
    assert lib.invsim_ppo_scratch_bytes(d.ctypes.data, 3, 1, None) == EINVAL
    # INVSIM_ERANGE exactly where the header's inequality says
    fits = lambda dd: (sum(dd) + dd[-1]) * row_bytes <= lds  # noqa: E731
    assert fits([33, 256, 256, 3]) and fits([68, 256, 256, 11])
    seen = set()
    for dd in [[33, 256, 256, 3], [68, 256, 256, 11], [112, 256, 256, 3], [113, 256, 256, 3], [33, 256, 256, 256, 3],
               [256, 256, 256, 256, 256, 32], [33, 256, 85, 256, 3], [33, 256, 84, 256, 3], [68, 256, 256, 25],
               [68, 256, 256, 26], [33, 3]]:
        rc, _ = _scratch(lib, dd, 100)
        assert rc == (0 if fits(dd) else ERANGE), (dd, rc)
        seen.add(fits(dd))
        if not fits(dd):
            assert b"LDS" in lib.invsim_last_error(None)
    assert seen == {True, False}
    assert (sum([112, 256, 256, 3]) + 3) * row_bytes <= lds < (sum([113, 256, 256, 3]) + 3) * row_bytes


# ---------------------------------------------------------------- argument errors before any library call
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


@pytest.fixture
def host(monkeypatch):
    """an env stand-in whose library and device object raise, the networks of the im family on the host"""
    import invsim
    from invsim import _capi, policies
    monkeypatch.setattr(_capi, "lib", lambda: _NoLibrary())
    actor, critic = pr.make_module([33, 8, 3], "tanh", False, 1), pr.make_module([33, 8, 1], "tanh", False, 2)
    pi = invsim.GaussianMLPPolicyAgent.from_module(actor, log_std=np.zeros(3, np.float32), seed=0, clip=False)
    vf = invsim.ValueMLP.from_module(critic)
    for net in (pi, vf):
        monkeypatch.setattr(net, "device_object", lambda env: (_ for _ in ()).throw(AssertionError("device_object")))
    env = types.SimpleNamespace(device=torch.device("cpu"), obs_dim=33, obs_dtype=torch.int64, action_dim=3,
                                _lib=_NoLibrary(), _h=None, _stream=lambda: 0)
    S = 12
    buf = {"obs": torch.zeros((S, 33), dtype=torch.int64), "raw_actions": torch.zeros((S, 3)),
           "log_prob": torch.zeros(S), "advantages": torch.ones(S), "returns": torch.zeros(S),
           "valid": torch.ones(S, dtype=torch.bool)}
    return types.SimpleNamespace(env=env, pi=pi, vf=vf, actor=actor, critic=critic, buf=buf,
                                 log_std=torch.nn.Parameter(torch.zeros(3)), policies=policies)


def test_gradient_wrappers_check_their_arguments_first(host):
    h, p = host, host.policies
    obs0 = torch.zeros((4, 33), dtype=torch.int64)
    bad = [
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.vf, h.buf, obs0)),
        (TypeError, lambda: p.value_grad(h.env, h.pi, h.buf, obs0)),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, [h.buf], obs0)),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, {k: v for k, v in h.buf.items() if k != "advantages"}, obs0)),
        (ValueError, lambda: p.value_grad(h.env, h.vf, {k: v for k, v in h.buf.items() if k != "returns"}, obs0)),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, clip_range=0.0)),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, clip_range=float("nan"))),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, dict(h.buf, obs=h.buf["obs"].float()), obs0)),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, dict(h.buf, advantages=h.buf["advantages"].double()), obs0)),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, dict(h.buf, log_prob=torch.zeros(5)), obs0)),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, dict(h.buf, valid=torch.ones(12)), obs0)),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0.float())),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, torch.zeros((4, 32), dtype=torch.int64))),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, idx=torch.zeros(3, dtype=torch.int32))),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, idx=torch.zeros((3, 1), dtype=torch.int64))),
        (TypeError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, idx=[0, 1])),
        (ValueError, lambda: p.ppo_actor_grad(h.env, h.pi, h.buf, obs0, adv_stats=torch.zeros(3))),
        (ValueError, lambda: p.value_grad(h.env, h.vf, dict(h.buf, returns=h.buf["returns"][::2]), obs0)),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()


def test_learner_checks_its_arguments_first(host):
    h, L = host, host.policies.PPOLearner
    ok = dict(env=h.env, pi=h.pi, vf=h.vf, actor=h.actor, critic=h.critic, log_std=h.log_std)
    cuda_env = types.SimpleNamespace(**{**vars(h.env), "device": torch.device("cuda:0")})
    bad = [
        (TypeError, dict(pi=h.vf)), (TypeError, dict(vf=h.pi)), (TypeError, dict(actor=None)),
        (TypeError, dict(critic=lambda x: x)), (TypeError, dict(log_std=torch.zeros(3))),
        (TypeError, dict(optimizer="adam")), (ValueError, dict(clip_range=0.0)), (ValueError, dict(clip_range=-1.0)),
        (ValueError, dict(max_grad_norm=0.0)), (ValueError, dict(n_epochs=0)), (ValueError, dict(batch_size=0)),
        (ValueError, dict(actor=pr.make_module([33, 9, 3], "tanh", False, 1))),
        (ValueError, dict(critic=h.actor)), (ValueError, dict(log_std=torch.nn.Parameter(torch.zeros(2)))),
        (ValueError, dict(actor=pr.make_module([33, 8, 3], "tanh", False, 1).double())),
        (ValueError, dict(env=cuda_env)),        # the parameters are not on the env's device
    ]
    for exc, kw in bad:
        with pytest.raises(exc):
            L(**{**ok, **kw})
