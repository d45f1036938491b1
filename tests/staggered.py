"""Cohort oracle for staggered-period runs (test helper, imported by
test_staggered_model.py and test_gpu_staggered.py).

The C oracle (oracle/pyoracle.py) has no masked reset, but its envs are
independent of each other.  A *cohort* is the set of envs with the same reset
history: the harness keeps one oracle instance per cohort, seeded with its envs'
own seeds (seed + global index), and a masked reset resets the cohorts under
the mask.  The cohorts are made up front from the masks the run is going to
use (env e's key is its bit in every mask), so no generator state ever has to
be split: two cohorts that a later mask separates are simply driven alike until
then.  A mask at reset time may be any union of cohorts.

Autoreset rules around step() (as the device's one-wave kernels apply them per
env; `_Oracle.row` in test_gpu_split_hotargs.py is the lock-step restatement):

* next_step: the call after a truncation is the reset row: reset obs, reward
  0, both flags 0, no demand draw; the demand record keeps its last value.
* same_step: the done step returns the reset obs, the final obs separately.
* disabled: nobody resets.  A Newsvendor env keeps stepping its episode with
  truncated=True; an InvMgmt / NetInvMgmt cohort past its horizon is not
  stepped (`Row.raises`: the device call must raise IndexError) while the other
  cohorts step normally.
"""
import numpy as np

import agents

N = 197                       # three full 64-env groups and a last group of 5
GROUP = 64


class Row:
    """One call's expected outputs in env order.  `stepped`: envs whose env
    step ran (demand, metrics and the action record are theirs only);
    `defined`: envs whose obs / reward / flags the call defines (all but the
    skipped envs of a raising DISABLED call)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Cohort:
    def __init__(self, idx, orc):
        self.idx, self.orc, self.t = idx, orc, 0
        self.obs, self.log = None, []


def cohort_keys(masks, n):
    masks = np.asarray(masks, bool).reshape(-1, n)
    return [tuple(bool(b) for b in masks[:, e]) for e in range(n)]


class CohortOracle:
    """family 'im' | 'nv' | 'net'; kw are the oracle class's arguments."""

    def __init__(self, pyoracle, family, n, seed, masks, mode="next_step", **kw):
        assert mode in ("next_step", "same_step", "disabled")
        self.family, self.n, self.mode = family, n, mode
        cls = {"im": pyoracle.OracleInvMgmt, "nv": pyoracle.OracleNewsvendor, "net": pyoracle.OracleNet}[family]
        keys = cohort_keys(masks, n)
        self.cohorts = []
        for key in sorted(set(keys)):
            idx = np.array([e for e in range(n) if keys[e] == key], np.int64)
            orc = cls(len(idx), **kw)
            orc.seed([seed + int(e) for e in idx])
            self.cohorts.append(_Cohort(idx, orc))
        o = self.cohorts[0].orc
        self.obs_dim = o.obs_dim
        self.obs_dtype = np.int64 if family == "im" else np.float32
        if family == "im":
            self.T, self.act_dim, self.dem_dim, self.met_dim = o.periods, o.m - 1, 1, 6
            self.act_dtype = np.int64
        elif family == "nv":
            self.T, self.act_dim, self.dem_dim, self.met_dim = int(o.cfg.step_limit), 1, 1, 2
            self.act_dtype = np.float32
        else:
            self.T, self.act_dim, self.dem_dim = int(o.cfg.num_periods), o.act_dim, o.topo["RL"]
            self.met_dim = 5 + o.topo["J"]
            self.act_dtype = np.float32
        self.crossings = [0] * len(self.cohorts)     # times each cohort reached its horizon

    # ------------------------------------------------------------ tables in env order
    def _gather(self, per_cohort, shape, dtype):
        out = np.zeros((self.n,) + tuple(shape), dtype)
        for c, v in zip(self.cohorts, per_cohort):
            out[c.idx] = v
        return out

    def periods(self):
        return self._gather([c.t for c in self.cohorts], (), np.int32)

    def rng_state(self):
        return self._gather([c.orc.rng_state() for c in self.cohorts], (4,), np.uint64)

    def params(self):
        assert self.family == "nv"
        return self._gather([c.orc.params() for c in self.cohorts], (5,), np.float64)

    def past_horizon(self):
        """envs a DISABLED InvMgmt / Net step would refuse"""
        return self.periods() >= self.T

    # ------------------------------------------------------------ resets
    def _reset_cohort(self, c):
        c.obs = c.orc.reset()
        c.t, c.log = 0, []
        return c.obs

    def reset(self, mask=None):
        """(obs [N, O], mask [N]): rows of envs outside the mask are unspecified (0 here)"""
        mask = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        obs = np.zeros((self.n, self.obs_dim), self.obs_dtype)
        for c in self.cohorts:
            m = mask[c.idx]
            assert m.all() or not m.any(), "the mask cuts a cohort: list it when the harness is made"
            if m.all():
                obs[c.idx] = self._reset_cohort(c)
        return obs, mask

    # ------------------------------------------------------------ one env step of a cohort
    def _step_cohort(self, c, a, met):
        fam = self.family
        if fam == "im":
            obs, r, tr, info = c.orc.step(a, info=True)
            dem = info["demand"].reshape(-1, 1)
            c.log.append(np.maximum(np.asarray(a, np.int64).reshape(len(c.idx), -1), 0))   # action_log[t]
            if met is not None:
                m = met[c.idx]
                m[:, 0] += r
                m[:, 1] += 1
                m[:, 2] += info["demand"]
                m[:, 3] += info["sales"][:, 0]
                m[:, 4] += info["unfulfilled"][:, 0]
                m[:, 5] += np.maximum(0, info["ending_inventory"]).sum(axis=1)
                met[c.idx] = m
        elif fam == "nv":
            obs, r, tr, dem = c.orc.step(a)
            dem = dem.reshape(-1, 1)
            if met is not None:
                m = met[c.idx]
                m[:, 0] += r
                m[:, 1] += 1
                met[c.idx] = m
        else:
            obs, r, tr, info = c.orc.step(a, info=True)
            dem = info["D"].astype(np.int64)
            if met is not None:
                m = met[c.idx]
                m[:, 0] += r
                m[:, 1] += 1
                for q in range(info["D"].shape[1]):
                    m[:, 2] += info["D"][:, q]
                    m[:, 3] += info["S"][:, q]
                    m[:, 4] += info["U"][:, q]
                m[:, 5:] += info["X"]
                met[c.idx] = m
        c.t += 1
        c.obs = obs
        assert bool(tr.all()) == (c.t >= self.T) and (tr.all() or not tr.any())
        return obs, r, tr, dem

    def _policy_action(self, c, agent):
        kind = agent[0]
        if kind == "base_stock":                  # ("base_stock", sf, mu, L, c)
            _, sf, mu, L, cap = agent
            k, m1 = len(c.idx), len(L)
            log = np.stack(c.log) if c.log else np.zeros((0, k, m1), np.int64)
            return agents.base_stock(c.obs, c.t, log, L, mu, sf, cap)
        if kind == "order_up_to":                 # ("order_up_to", sf, lead_time, max_order)
            _, sf, L, mo = agent
            return agents.order_up_to(c.obs, L, sf, mo)
        if kind == "classic_nv":                  # ("classic_nv", cr_method, sf, lead_time, max_order)
            _, cr, sf, L, mo = agent
            return agents.classic_nv(c.obs, L, sf, mo, cr)
        assert kind == "constant"                 # ("constant", action vector)
        return np.broadcast_to(agent[1], (len(c.idx), len(agent[1]))).astype(self.act_dtype)

    # ------------------------------------------------------------ one call
    def row(self, actions=None, agent=None, metrics=None):
        """One step() call (or one row of a rollout) for all N envs.  With
        `agent` the cohort's action comes from its own obs, period and order
        log, and `metrics` [N, M] (float64) accumulates the stepped rows."""
        n, T, mode = self.n, self.T, self.mode
        obs = np.zeros((n, self.obs_dim), self.obs_dtype)
        rew = np.zeros(n, np.float64)
        tr = np.zeros(n, bool)
        dem = np.zeros((n, self.dem_dim), np.int64)
        stepped = np.zeros(n, bool)
        defined = np.ones(n, bool)
        fobs = np.zeros((n, self.obs_dim), self.obs_dtype)
        fmask = np.zeros(n, bool)
        acts = np.zeros((n, self.act_dim), self.act_dtype)   # a reset row records no action
        raises = False
        for ci, c in enumerate(self.cohorts):
            if mode == "next_step" and c.t >= T:
                obs[c.idx] = self._reset_cohort(c)
                continue
            if mode == "disabled" and self.family != "nv" and c.t >= T:
                raises = True
                defined[c.idx] = False
                continue
            a = self._policy_action(c, agent) if agent is not None else np.ascontiguousarray(actions[c.idx])
            acts[c.idx] = a
            o, r, t_, d = self._step_cohort(c, a, metrics)
            if c.t == T:
                self.crossings[ci] += 1
            rew[c.idx], tr[c.idx], dem[c.idx], stepped[c.idx] = r, t_, d, True
            if mode == "same_step" and t_.all():
                fobs[c.idx], fmask[c.idx] = o, True
                o = self._reset_cohort(c)
            obs[c.idx] = o
        return Row(obs=obs, reward=rew, truncated=tr, demand=dem, stepped=stepped, defined=defined,
                   final_obs=fobs, final_mask=fmask, actions=acts, raises=raises)


# ---------------------------------------------------------------- schedules
def schedule_masks(n, variant):
    """The two masks of a run.  Variant 'a': e % 3 == 0, then envs 64..127
    entirely plus e % 5 == 1 (env n - 1 = 196 is in it); variant 'b' takes
    e % 5 == 2 instead, so env n - 1 is never reset by a mask."""
    e = np.arange(n)
    m1 = e % 3 == 0
    m2 = ((e >= 64) & (e < 128)) | (e % 5 == (1 if variant == "a" else 2))
    return np.stack([m1, m2])


def random_actions(family, rng, n, act_dim, wide=False, cap=230):
    if family == "im":
        a = rng.integers(-10, cap + 40, size=(n, act_dim)).astype(np.int64)
        if wide:          # the 16-bit / 32-bit sentinels and orders past 2^32: the int64 side ring
            special = np.array([65535, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40], np.int64)
            m = rng.random(a.shape) < 0.3
            a[m] = special[rng.integers(0, len(special), size=int(m.sum()))]
        return a
    if family == "nv":
        return rng.uniform(-50, 2500, size=(n, 1)).astype(np.float32)
    a = rng.uniform(-5, 120, size=(n, act_dim)).astype(np.float32)
    m = rng.random(a.shape) < 0.1
    a[m] = np.round(a[m]) + 0.5
    return a


def script(h, rng, wide=False, calls=None, tail=5, cap=230, checkpoint=False):
    """The run every staggered test makes, as a generator of
    (op, argument, expectation):

      ("reset", mask | None, (obs, mask))    reset() / reset(options={"reset_mask": mask})
      ("step", actions, Row)
      ("rollout", actions [K, N, A], [Row] * K)
      ("policy", (agent, K), ([Row] * K, metrics [N, M]))
      ("state", None, None)                  compare rng_state() / periods() / params() now
      ("checkpoint", None, None)             with checkpoint=True: a fresh handle joins from get_state()

    Unmasked reset, a few lock-step steps, mask 1, two steps, mask 2, then
    steps through at least two horizons, an unmasked reset and `tail` lock-step
    rows.  With `calls` = an agent tuple a stretch of the steps after mask 2 is
    one rollout of K = 2 * horizon + 5 and one policy rollout of horizon + 3 rows
    (DISABLED InvMgmt / Net: as many rows as fit under the horizon).  Under
    DISABLED the caller resets: before a call, the cohorts that would overrun
    (Newsvendor: two rows past step_limit) get a masked reset, which is how a
    cohort crosses its horizon more than once in that mode."""
    n, T, fam = h.n, h.T, h.family
    m1, m2 = h.masks

    def acts(K=None):
        if K is None:
            return random_actions(fam, rng, n, h.act_dim, wide, cap)
        return np.stack([random_actions(fam, rng, n, h.act_dim, wide, cap) for _ in range(K)])

    def room(K):
        """DISABLED: masked reset of the cohorts that K more rows would overrun"""
        if h.mode != "disabled":
            return
        per = h.periods()
        m = per >= T + 2 if fam == "nv" else per + K > T
        if m.any():
            yield "reset", m, h.reset(m)

    def steps(k):
        for _ in range(k):
            yield from room(1)
            a = acts()
            yield "step", a, h.row(a)

    yield "reset", None, h.reset()
    yield from steps(min(3, T - 1))
    yield "reset", m1, h.reset(m1)
    yield from steps(2)
    yield "reset", m2, h.reset(m2)
    if checkpoint:
        yield from steps(2)
        yield "checkpoint", None, None
    if calls is not None:
        assert h.mode != "same_step"
        yield from steps(2)
        free = h.mode == "next_step" or fam == "nv"
        K = 2 * T + 5 if free else max(1, T // 2)
        yield from room(K)
        A = acts(K)
        yield "rollout", A, [h.row(A[k]) for k in range(K)]
        K = T + 3 if free else max(1, T // 2)
        yield from room(K)
        met = np.zeros((n, h.met_dim), np.float64)
        yield "policy", (calls, K), ([h.row(agent=calls, metrics=met) for _ in range(K)], met)
        yield from steps(T + 2)
    else:
        yield from steps(2 * (T + 1) + 3)
    yield "state", None, None
    yield "reset", None, h.reset()
    yield from steps(min(tail, T) if h.mode == "disabled" and fam != "nv" else tail)
    yield "state", None, None


def fault_script(h, rng):
    """The DISABLED horizon fault of an InvMgmt / Net handle, same tuples as
    script(): lock-step steps, mask 1, steps until the envs outside the mask
    stand at their horizon, then one more step: its Row has raises=True, the
    masked envs step and the others are left untouched.  A masked reset of the
    refused envs follows, and horizon + 2 more rows (the caller still resets
    whoever reaches the horizon)."""
    n, T, fam = h.n, h.T, h.family
    assert h.mode == "disabled" and fam != "nv"
    m1 = h.masks[0]

    def step():
        a = random_actions(fam, rng, n, h.act_dim)
        return "step", a, h.row(a)

    yield "reset", None, h.reset()
    for _ in range(min(3, T - 1)):
        yield step()
    yield "reset", m1, h.reset(m1)
    while h.periods().max() < T:
        yield step()
    assert h.periods().min() < T
    op = step()
    assert op[2].raises and op[2].stepped.any() and not op[2].stepped.all()
    yield op
    m = h.past_horizon()
    yield "reset", m, h.reset(m)
    for _ in range(T + 2):
        m = h.past_horizon()
        if m.any():
            yield "reset", m, h.reset(m)
        yield step()
    yield "state", None, None


def make(pyoracle, family, seed, variant="a", mode="next_step", n=N, **kw):
    masks = schedule_masks(n, variant)
    h = CohortOracle(pyoracle, family, n, seed, masks, mode, **kw)
    h.masks = masks
    return h


# ---------------------------------------------------------------- coverage (from the period table alone)
def coverage(pre, T, mode, n=N):
    """pre: [rows, N] periods before each step row.  An env "resets" in a row
    when the kernel's per-env branch leaves the plain step there: next_step
    period >= T (the reset row), same_step period == T - 1 (the done step
    resets in place), disabled period >= T (the refused lane; Newsvendor: the
    lane past step_limit).  Returns (a) a 64-env group mixes resetting and
    stepping envs in some row, (b) a group resets as a whole in a row where
    another group has stepping envs (with the masks above no group is ever
    free of the second mask's envs, so "steps as a whole" cannot be asked)."""
    pre = np.asarray(pre)
    rs = pre == T - 1 if mode == "same_step" else pre >= T
    a = b = False
    for row in rs:
        g = [row[s:s + GROUP] for s in range(0, n, GROUP)]
        a |= any(x.any() and not x.all() for x in g)
        b |= any(x.all() for x in g) and any(not x.all() for x in g)
    return bool(a), bool(b)
