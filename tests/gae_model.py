"""CPU restatement of invsim_gae's contract (include/invsim.h "Critic, GAE and
parameter updates") and of the parameter layout invsim_mlp_update writes.

The scan runs over k in the outer loop and is vectorised over the envs: plain
float64 numpy operations, one rounding each (numpy never fuses a multiply with
an add).  Flags are uint8 / bool arrays [K, n] or None, done0 [n] or None.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def _flag(a, shape):
    return np.zeros(shape, bool) if a is None else np.asarray(a).astype(bool)


def gae(reward, terminated, truncated, done0, value0, values, gamma, lam, full=False):
    """(advantages f32 [K, n], returns f32 [K, n], valid uint8 [K, n]); with
    `full` also the float64 advantages before the cast"""
    reward = np.asarray(reward, F64)
    K, n = reward.shape
    te, tr = _flag(terminated, (K, n)), _flag(truncated, (K, n))
    d0 = _flag(done0, (n,))
    value0, values = np.asarray(value0, F32), np.asarray(values, F32)
    gamma, gl = F64(gamma), F64(gamma) * F64(lam)          # gl: one product on the host
    adv, ret = np.zeros((K, n), F32), np.zeros((K, n), F32)
    valid = np.zeros((K, n), np.uint8)
    adv64 = np.zeros((K, n), F64)
    carry = np.zeros(n, F64)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):
            done_k = te[k] | tr[k]
            prev = (te[k - 1] | tr[k - 1]) if k > 0 else d0
            vp = (values[k - 1] if k > 0 else value0).astype(F64)
            vn = values[k].astype(F64)
            b = np.where(te[k], F64(0.0), gamma * vn)
            delta = (reward[k] + b) - vp
            a = np.where(done_k, delta, delta + gl * carry)
            carry = np.where(prev, F64(0.0), a)
            adv64[k] = carry
            adv[k] = np.where(prev, F32(0.0), a.astype(F32))
            ret[k] = np.where(prev, vp.astype(F32), (a + vp).astype(F32))
            valid[k] = ~prev
    return (adv, ret, valid, adv64) if full else (adv, ret, valid)


PATTERNS = 8


def synthetic(K, n, seed, specials=True):
    """Inputs [K, n] that put every flag pattern in some env (env e has pattern
    (e + seed) % 8): 0 no flag; 1 done at k = 0; 2 done at K - 1; 3 dones in two
    consecutive rows (truncated, then terminated); 4 / 5 / 6 terminated alone /
    truncated alone / both at a middle row; 7 random flags.  done0 is set on
    every other env.  Rewards are of the envs' magnitude (+-1e3), with +-0.0,
    +-inf and NaN entries when `specials`; values are mixed-sign float32."""
    rng = np.random.default_rng(1000 * K + n + 7919 * seed)
    te, tr = np.zeros((K, n), np.uint8), np.zeros((K, n), np.uint8)
    pat = (np.arange(n) + seed) % PATTERNS
    mid = K // 2
    tr[0, pat == 1] = 1
    tr[K - 1, pat == 2] = 1
    tr[max(mid - 1, 0), pat == 3] = 1
    te[mid, pat == 3] = 1
    te[mid, pat == 4] = 1
    tr[mid, pat == 5] = 1
    te[mid, pat == 6] = 1
    tr[mid, pat == 6] = 1
    rnd = pat == 7
    te[:, rnd] = rng.random((K, int(rnd.sum()))) < 0.2
    tr[:, rnd] = rng.random((K, int(rnd.sum()))) < 0.2
    reward = rng.uniform(-1e3, 1e3, (K, n))
    if specials:
        vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
        hit = rng.random((K, n)) < 0.04
        reward[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))]
    return dict(reward=reward, terminated=te, truncated=tr, done0=((np.arange(n) + seed) % 2).astype(np.uint8),
                value0=(50 * rng.standard_normal(n)).astype(F32), values=(50 * rng.standard_normal((K, n))).astype(F32))


def blob_layout(weight, bias=None):
    """(wt [in, opad], b [opad]) as invsim_mlp_create and invsim_mlp_update lay a
    layer out on the device: the row-major [out, in] weight transposed, the output
    index padded with +0.0 to a multiple of 4"""
    w = np.asarray(weight, F32)
    out, inn = w.shape
    opad = (out + 3) // 4 * 4
    wt = np.zeros((inn, opad), F32)
    wt[:, :out] = w.T
    b = np.zeros(opad, F32)
    if bias is not None:
        b[:out] = np.asarray(bias, F32)
    return wt, b


def update_store(weight, d):
    """what invsim_mlp_update's kernel stores at flat destination index d of a
    layer's [in, opad] block: its index arithmetic, restated"""
    w = np.asarray(weight, F32)
    out, inn = w.shape
    opad = (out + 3) // 4 * 4
    i, j = divmod(d, opad)
    return w.reshape(-1)[j * inn + i] if j < out else F32(0.0)
