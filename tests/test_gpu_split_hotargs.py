"""The split step kernel's argument path (im_split_kernel): its leading scalar
arguments (six base pointers, N, the packed ImHot word of the window's ring
slot / last logged row / depth and the three arrival rows) and the per-launch
values the host passes by value (alpha ** t, n, nw, the truncation flag).

Everything goes through the C ABI (the env classes) and is bit-exact: obs,
reward, both flags, the final get_state blob.  The reference is the C oracle
stepping the same seeds wherever it supports the configuration, and always a
second handle created with INVSIM_IM_SPLIT=0 (knobs are read at handle
creation), which runs the one-wave kernel: it takes none of the new arguments.

Shapes: 197 envs = four 64-env step groups with a partial last one and two
128-env lookahead workgroups with the second partial; 130 envs = three step
groups (the last of 2 envs) and two lookahead workgroups.
"""
import numpy as np
import pytest
import torch

from conftest import knob_envs
from test_gpu_parity import _eq_bits, _im_random_actions

gpu_test = pytest.mark.gpu


def _pair(monkeypatch, make):
    """(split handle, one-wave handle) of the same configuration"""
    return knob_envs(monkeypatch, "INVSIM_IM_SPLIT", ("1", "0"), make)


def _np(x):
    return x.cpu().numpy()


def _same(a, b, where):
    for name, x, y in zip(("obs", "reward", "terminated", "truncated"), a, b):
        x, y = _np(x), _np(y)
        if x.dtype.kind == "f":
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), f"{name} {where}"


class _Oracle:
    """The C oracle under NEXT_STEP autoreset: the call after a truncation is the reset"""

    def __init__(self, oracle, n, seed, **kw):
        self.orc = oracle.OracleInvMgmt(n, **kw)
        self.orc.seed(range(seed, seed + n))
        self.n, self.t, self.T = n, 0, self.orc.periods
        self.obs0 = self.orc.reset()

    def row(self, act):
        if self.t >= self.T:
            self.t = 0
            return self.orc.reset(), np.zeros(self.n), np.zeros(self.n, bool)
        o, r, tr = self.orc.step(act)
        self.t += 1
        return o, r, tr

    def reset(self):
        self.t = 0
        return self.orc.reset()

    def check(self, out, act, where):
        o, r, tr = self.row(act)
        assert _eq_bits(_np(out[0]), o), f"obs vs oracle {where}"
        assert np.array_equal(_np(out[1]).view(np.int64), r.view(np.int64)), f"reward vs oracle {where}"
        assert not _np(out[2]).any(), f"terminated {where}"
        assert np.array_equal(_np(out[3]), tr), f"truncated vs oracle {where}"

    def check_state(self, env):
        got = _np(env.state_fields()["rng"]).view(np.uint64).T
        assert np.array_equal(got, self.orc.rng_state()), "PCG64 state vs oracle"


UNKNOWN = 0xFFFFFFFF    # low word of position() once the periods come from the device (no lock-step)


def _lock_step(env):
    return env.position() & UNKNOWN != UNKNOWN


def _drive(envs, acts, orc=None, rollout_at=None, state_at=None):
    """Step every env of `envs` through acts [K][n][m1] (one invsim_step each; at
    call rollout_at one invsim_rollout of three rows instead; before call
    state_at a get_state / set_state round trip, which ends lock-step: from
    there on the per-env one-wave kernel runs on every handle), comparing every
    row with envs[0]'s and with the oracle's, then the final blobs.  Up to
    state_at every call is asserted to be made in lock-step."""
    K, k = acts.shape[0], 0
    dev = torch.from_numpy(acts).to(envs[0].device)
    locked = True
    while k < K:
        if k == state_at:
            for env in envs:
                env.set_state(env.get_state().clone())
                assert not _lock_step(env)
            locked = False
        if locked:
            assert all(_lock_step(env) for env in envs), f"lock-step before call {k}"
        if k == rollout_at:
            outs = [tuple(x.clone() for x in env.rollout(dev[k:k + 3])) for env in envs]
            for j in range(3):
                rows = [tuple(x[j] for x in o) for o in outs]
                for other in rows[1:]:
                    _same(rows[0], other, f"rollout row {k + j}")
                if orc:
                    orc.check(rows[0], acts[k + j], f"rollout row {k + j}")
            k += 3
            continue
        outs = [tuple(x.clone() for x in env.step(dev[k])[:4]) for env in envs]
        for other in outs[1:]:
            _same(outs[0], other, f"step {k}")
        if orc:
            orc.check(outs[0], acts[k], f"step {k}")
        k += 1
    blobs = [env.get_state() for env in envs]
    for b in blobs[1:]:
        assert torch.equal(blobs[0], b), "final get_state blob"
    if orc:
        orc.check_state(envs[0])


def _acts(seed, K, n, m1, c):
    rng = np.random.default_rng(seed)
    return np.stack([_im_random_actions(rng, n, m1, c) for _ in range(K)])


@gpu_test
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
def test_base_case(gpu, oracle, monkeypatch, cls_name):
    """63 steps under NEXT_STEP (two episodes, two reset steps, the first periods
    of the third), all in lock-step: the window grows while t < D and the ring
    wraps; the first step after seeding and after an interleaved three-row
    rollout (calls 40-42) takes the inline-draw variant.  Then a get_state /
    set_state round trip: the periods now come from the blob, so two steps run
    on the per-env one-wave kernel of both handles; an unmasked reset restores
    lock-step, and the first of six more split steps is the inline-draw
    variant after a set_state."""
    import invsim
    n, seed = 197, 910
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(n, device=gpu))
    orc = _Oracle(oracle, n, seed, backlog=cls_name.endswith("BacklogEnv"))
    for env in envs:
        obs, _ = env.reset(seed=seed)
        assert _eq_bits(_np(obs), orc.obs0)
    acts = _acts(1, 74, n, 3, [100, 200, 230])
    _drive(envs, acts[:66], orc, rollout_at=40)
    _drive(envs, acts[66:68], orc, state_at=0)
    e_obs = orc.reset()
    for env in envs:
        obs, _ = env.reset()
        assert _lock_step(env)
        assert _eq_bits(_np(obs), e_obs), "reset obs after the round trip"
    _drive(envs, acts[68:], orc)


_M1_1 = dict(I0=(60,), p=14, r=(10, 6), k=(0.2, 0.1), h=(0.1,), c=(90,), L=(4,))
_M1_8 = dict(periods=12, I0=(30, 40, 50, 60, 70, 80, 90, 100), r=(9, 8, 7, 6, 5, 4, 3, 2, 1),
             k=(0.3, 0.2, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02, 0.01), h=(0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04, 0.02),
             c=(60, 70, 80, 90, 100, 110, 120, 130), L=(0, 1, 2, 3, 0, 4, 2, 6), p=11, alpha=0.9,
             dist_param={"mu": 35})


@gpu_test
@pytest.mark.parametrize("kw", [
    _M1_1,                                   # M1 = 1: not packed, everything derived from ImParams
    dict(L=(2, 3, 4)),                       # 4 stages, packed, lt_max = 4
    _M1_8,                                   # M1 = 8, two zero lead times: not packed
    dict(L=(0, 2, 1), dist_param={"mu": 4}),   # packed, a stage with no arrival row at all
    dict(L=(3, 14, 2), periods=17),          # packed, lt_max = 14: the window does not fit the registers
    dict(L=(1, 5, 16), periods=19),          # 4 stages that cannot be packed (lt_max > 15)
], ids=["m1_1", "stages4", "m1_8", "zero_lt", "lt14", "lt16"])
def test_stage_counts_and_lead_times(gpu, oracle, monkeypatch, kw):
    import invsim
    n, seed = 130, 77
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu, **kw))
    orc = _Oracle(oracle, n, seed, **kw)
    for env in envs:
        obs, _ = env.reset(seed=seed)
        assert _eq_bits(_np(obs), orc.obs0)
    c = kw.get("c", (100, 200, 230))
    _drive(envs, _acts(2, 2 * orc.T + 3, n, len(c), list(c)), orc)


@gpu_test
@pytest.mark.parametrize("kw", [
    dict(dist=2, dist_param={"n": 400, "p": 0.05}),
    dict(dist=3, dist_param={"low": 0, "high": 40}),
    dict(dist=4, dist_param={"p": 0.05}),
    dict(dist=5, user_D=list(range(3, 33))),   # the load of user_D[t] under dist == 5 only
], ids=["binomial", "integers", "geometric", "user_D"])
def test_demand_kinds(gpu, oracle, monkeypatch, kw):
    import invsim
    n, seed = 130, 31
    envs = _pair(monkeypatch, lambda: invsim.InvManagementLostSalesEnv(n, device=gpu, **kw))
    orc = _Oracle(oracle, n, seed, backlog=False, **kw)
    for env in envs:
        obs, _ = env.reset(seed=seed)
        assert _eq_bits(_np(obs), orc.obs0)
    _drive(envs, _acts(3, orc.T, n, 3, [100, 200, 230]), orc)


@gpu_test
def test_philox_stream(gpu, monkeypatch):
    """the fast stream's instantiations (invmgmt_ph.hip: its own launcher);
    the oracle has no Philox stream, so the one-wave kernel is the reference"""
    import invsim
    n = 130
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu, demand_stream="philox"))
    for env in envs:
        env.reset(seed=5)
    _drive(envs, _acts(4, 33, n, 3, [100, 200, 230]))


@gpu_test
def test_episode_sink(gpu, oracle, monkeypatch):
    """the sink's loads now follow the step's up-front loads; its truncation
    test is the flag passed by value"""
    import invsim
    from invsim.distributed import EpisodeStats
    n, seed = 130, 19
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu))
    orc = _Oracle(oracle, n, seed)
    stats = []
    for env in envs:
        env.reset(seed=seed)
        st = EpisodeStats(n, gpu)
        st.attach(env)
        stats.append(st)
    acts = _acts(5, 33, n, 3, [100, 200, 230])
    _drive(envs, acts, orc)
    torch.cuda.synchronize()
    assert torch.equal(stats[0].ret.view(torch.int64), stats[1].ret.view(torch.int64)), "running returns"
    assert torch.equal(stats[0].part.view(torch.int64), stats[1].part.view(torch.int64)), "group partials"
    assert float(stats[0].part[:, 2].sum()) == n            # one finished episode per env


@gpu_test
def test_info_record(gpu, oracle, monkeypatch):
    import invsim
    n, seed = 130, 23
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu, record_demand=True,
                                                                     record_info=True))
    orc = oracle.OracleInvMgmt(n)
    orc.seed(range(seed, seed + n))
    orc.reset()
    for env in envs:
        env.reset(seed=seed)
    acts = _acts(6, 30, n, 3, [100, 200, 230])
    dev = torch.from_numpy(acts).to(gpu)
    for k in range(30):
        res = [env.step(dev[k]) for env in envs]
        infos = [{key: v.clone() for key, v in r[4].items() if torch.is_tensor(v)} for r in res]
        _same(res[0][:4], res[1][:4], f"step {k}")
        assert infos[0].keys() == infos[1].keys()
        for key in infos[0]:
            a, b = infos[0][key], infos[1][key]
            if a.dtype.is_floating_point:
                a, b = a.view(torch.int64), b.view(torch.int64)
            assert torch.equal(a, b), (key, k)
        o, r, tr, inf = orc.step(acts[k], info=True)
        assert _eq_bits(_np(res[0][0]), o), k
        assert np.array_equal(_np(res[0][1]).view(np.int64), r.view(np.int64)), k
        assert np.array_equal(_np(infos[0]["demand"]).reshape(n), inf["demand"]), k
        assert np.array_equal(_np(infos[0]["sales"]), inf["sales"]), k
        assert np.array_equal(_np(infos[0]["unfulfilled"]), inf["unfulfilled"]), k
        # the five f64 sums of both handles against numpy, recomputed from the
        # oracle's S, U and ending inventory as the reference forms them
        # (inventory_management.py:314-321; test_compat does it for one env)
        e0 = envs[0]
        S, U = inf["sales"], inf["unfulfilled"]
        rev = e0.unit_price * S
        pro = e0.unit_cost * S
        hol = e0.holding_cost * np.maximum(0, np.append(inf["ending_inventory"], np.zeros((n, 1), np.int64), axis=1))
        pen = e0.demand_cost * U
        exp = {"period_profit": (rev - pro - hol - pen).sum(axis=1), "revenue": rev.sum(axis=1),
               "procurement_cost": pro.sum(axis=1), "holding_cost": hol.sum(axis=1), "penalty_cost": pen.sum(axis=1)}
        for key, v in exp.items():
            assert v.dtype == np.float64 and v.shape == (n,)
            for h, got in enumerate(infos):
                assert np.array_equal(_np(got[key]).view(np.int64), v.view(np.int64)), (key, k, h)
    assert torch.equal(envs[0].get_state(), envs[1].get_state())


@gpu_test
def test_graph_replay(gpu):
    """one capture of an episode cycle (periods + the reset step) and two
    replays equal the eager steps: alpha ** t, n, nw, the truncation flag and
    the packed word are baked into each captured launch, as t is"""
    import invsim
    n = 130
    env = invsim.InvManagementBacklogEnv(n, device=gpu)
    twin = invsim.InvManagementBacklogEnv(n, device=gpu)
    C = env._horizon() + 1
    obs_g = env.reset(seed=11)[0].clone()
    obs_e = twin.reset(seed=11)[0].clone()

    def loop(e, obs):
        def fn():
            o, rews, dones, allobs = obs, [], [], []
            for _ in range(C):
                o, r, te, tr, _ = e.step(o[:, :3] % 97 + 5)
                rews.append(r)
                dones.append(tr)
                allobs.append(o)
            obs.copy_(o)
            return torch.stack(rews), torch.stack(dones), torch.stack(allobs)
        return fn

    g = env.capture(loop(env, obs_g), warmup=1)
    assert g.steps == C
    eager = loop(twin, obs_e)
    eager()                                                  # the twin of the capture's warm-up run
    for rep in range(2):
        rew_g, done_g, all_g = g.replay()
        rew_e, done_e, all_e = eager()
        torch.cuda.synchronize(gpu)
        assert torch.equal(rew_g.view(torch.int64), rew_e.view(torch.int64)), f"rewards, replay {rep}"
        assert torch.equal(done_g, done_e), f"truncated, replay {rep}"
        assert torch.equal(all_g, all_e), f"obs, replay {rep}"
        assert int(done_g.sum()) == n
    assert torch.equal(env.get_state(), twin.get_state())


# ---------------------------------------------------------------- CPU
PAD_CHECK = r"""
#include "kernels.hpp"
using invsim::pad_n;
// the rule as the host used it before it was shared: N rounded up to 256, at least 256
constexpr long long ref(long long n) { long long r = (n + 255) / 256 * 256; return r < 256 ? 256 : r; }
#define CHECK(n) static_assert(pad_n(n) == ref(n), "pad_n(" #n ")")
#define ALL() CHECK(1); CHECK(63); CHECK(64); CHECK(65); CHECK(197); CHECK(65536); CHECK(65605)
__host__ long long host_side(long long n) { ALL(); return pad_n(n); }
__global__ void device_side(long long *out, long long n) { ALL(); *out = pad_n(n); }
#include <cstdio>
int main() {
    const long long ns[] = {1, 63, 64, 65, 197, 65536, 65605};
    for (long long n : ns) std::printf("%lld %lld\n", n, (long long)host_side(n));
    return 0;
}
"""


def test_padding_rule_host_and_device(tmp_path):
    """pad_n (kernels.hpp) is one constexpr __host__ __device__ function: the
    static_asserts hold in the host pass and in the gfx950 device pass of one
    compilation, and the host program prints the strides, checked here against
    the rule restated in Python."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the build's compiler) not found"
    src = tmp_path / "pad_check.hip"
    src.write_text(PAD_CHECK)
    exe = tmp_path / "pad_check"
    subprocess.run([hipcc, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I", os.path.join(root, "or-gym-inventory_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(map(int, out[0::2]), map(int, out[1::2])))
    exp = {n: max(256, -(-n // 256) * 256) for n in (1, 63, 64, 65, 197, 65536, 65605)}
    assert got == exp
