"""A second statement of the InvMgmt env, in plain numpy, for checking the C
oracle where no golden reaches (tests/test_limit_cases.py) and the compat
view's histories (tests/test_gpu_limits.py).

It follows the reference's description of one period (inventory_management.py
reset, step, _get_obs) and shares nothing with the oracle or the kernels: one
env per object, the whole episode's history kept in [periods (+ 1), stages]
arrays (no rings), the arithmetic left to numpy's own array operations and
`dist` 1 demand drawn by numpy's own `Generator.poisson`.

The points a restatement gets wrong first, so they are spelled out:

* the observation's pipeline part is action_log[t - n : t] with n = min(t,
  max L), written OLDEST FIRST from the start of the window; while t < max L
  the newest row therefore moves, and the tail stays zero;
* the order a stage fills is min(request + its backlog, capacity, the
  supplier's stock at the START of the period): arrivals of this period do not
  count, and the last stage's supplier is unlimited;
* what leaves the stock of stage i >= 1 is the order stage i ITSELF had
  filled, as the reference writes it, not the one it shipped downstream;
* the backlog is added only from period 1 on (B[0] is zero anyway);
* an episode's second reset without a seed keeps the generator where it is.
"""
import numpy as np


class InvMgmtModel:
    def __init__(self, seed, periods=30, I0=(100, 150, 200), p=20, r=(15, 10, 7, 5),
                 k=(0.10, 0.075, 0.05, 0.025), h=(0.15, 0.10, 0.05), c=(100, 200, 230), L=(1, 5, 10),
                 backlog=True, mu=20, alpha=0.97):
        self.T = int(periods)
        self.I0 = np.array(list(I0), np.int32).astype(np.int64)
        self.m1 = len(self.I0)
        self.m = self.m1 + 1
        self.price = np.append(p, r[:-1]).astype(np.float32)
        self.cost = np.array(r, np.float32)
        self.penalty = np.array(k, np.float32)
        self.holding = np.append(h, 0).astype(np.float32)
        self.cap = np.array(list(c), np.int64)
        self.L = [int(x) for x in L]
        self.D = max(self.L)
        self.backlog, self.mu, self.alpha = bool(backlog), mu, alpha
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed))))
        assert len(self.cost) == len(self.penalty) == len(self.holding) == self.m
        assert len(self.cap) == len(self.L) == self.m1

    def reset(self):
        T, m1, m = self.T, self.m1, self.m
        self.t = 0
        self.I = np.zeros((T + 1, m1), np.int64)     # stock at the start of each period
        self.I[0] = self.I0
        self.R = np.zeros((T, m1), np.int64)         # orders filled (shipped) in each period
        self.B = np.zeros((T + 1, m), np.int64)      # backlog at the start of each period
        self.action_log = np.zeros((T, m1), np.int64)
        self.demand = np.zeros(T, np.int64)
        return self.obs()

    def obs(self):
        t, m1 = self.t, self.m1
        o = np.zeros(m1 * (self.D + 1), np.int64)
        o[:m1] = self.I[t]
        n = min(t, self.D)
        if n:
            o[m1:m1 + n * m1] = self.action_log[t - n:t].reshape(-1)   # oldest first
        return o

    def step(self, action):
        t, m1, m = self.t, self.m1, self.m
        ask = np.maximum(np.asarray(action), 0).astype(np.int64)
        self.action_log[t] = ask
        want = ask + self.B[t, 1:] if t >= 1 else ask.copy()
        stock = np.append(self.I[t, 1:], np.inf)              # the supplier of stage i is stage i + 1
        ship = np.minimum(np.minimum(want, self.cap), stock).astype(np.int64)
        self.R[t] = ship
        on_hand = self.I[t].copy()
        for i in range(m1):
            if t - self.L[i] >= 0:
                on_hand[i] += self.R[t - self.L[i], i]
        d = max(0, int(self.rng.poisson(lam=self.mu)))
        self.demand[t] = d
        owed = d + (int(self.B[t, 0]) if t >= 1 else 0)
        sold = min(int(on_hand[0]), owed)
        on_hand[0] -= sold
        on_hand[1:] -= ship[1:]                                # the reference takes stage i's OWN filled order from it
        sales = np.zeros(m, np.int64)
        sales[0], sales[1:] = sold, ship
        short = np.zeros(m, np.int64)
        short[0], short[1:] = owed - sold, want - ship
        self.B[t + 1] = short if self.backlog else 0
        self.I[t + 1] = on_hand
        profit = np.sum(self.price * sales - self.cost * sales
                        - self.holding * np.maximum(0, np.append(on_hand, 0)) - self.penalty * short)
        reward = float((self.alpha ** t) * profit)
        self.t = t + 1
        return self.obs(), reward, self.t >= self.T, d
