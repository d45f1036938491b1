"""CPU restatement of the running-normalisation contract (include/invsim.h
"Running normalisation"): invsim_moments' leaves, Merge and tree, the
discounted-return scan, the reward normalisation and the input-row parameters.

Plain float64 numpy operations, one rounding each (numpy never fuses a multiply
with an add; its division and square root are the IEEE correctly rounded ones).
The leaves are vectorised over blocks and columns with the 64 rows of a block
in the loop, the tree over the nodes of a level.  The leaf size is read from
the header, not repeated here.
"""
import os
import re

import numpy as np

F32, F64 = np.float32, np.float64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "invsim.h")
BLOCK = int(re.search(r"^#define\s+INVSIM_MOMENTS_BLOCK\s+(\d+)", open(HEADER).read(), re.M).group(1))
DTYPES = {np.dtype(np.int64): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}     # INVSIM_DTYPE_*


def prior(cols):
    """SB3's RunningMeanStd at construction: count 1e-4, mean 0, variance 1"""
    s = np.zeros((3, cols), F64)
    s[0] = s[2] = 1e-4
    return s


def leaves(x, mask=None):
    """[3, L, cols]: (n, mean, q) of every block of BLOCK consecutive rows"""
    x = np.asarray(x)
    rows, cols = x.shape
    L = -(-rows // BLOCK)
    xd = np.zeros((L * BLOCK, cols), F64)
    xd[:rows] = x.astype(F64)
    on = np.zeros(L * BLOCK, bool)
    on[:rows] = True if mask is None else np.asarray(mask).astype(bool)
    xd, on = xd.reshape(L, BLOCK, cols), on.reshape(L, BLOCK, 1)
    n = np.zeros((L, cols), F64) + on.sum(1).astype(F64)
    s = np.zeros((L, cols), F64)
    with np.errstate(all="ignore"):
        for r in range(BLOCK):
            s = np.where(on[:, r], s + xd[:, r], s)
        mean = s / n
        q = np.zeros((L, cols), F64)
        for r in range(BLOCK):
            d = xd[:, r] - mean
            q = np.where(on[:, r], q + d * d, q)
    empty = n == 0
    return np.stack([n, np.where(empty, F64(0.0), mean), np.where(empty, F64(0.0), q)])


def merge(a, b):
    """Merge(a, b) on [3, ...] records, elementwise"""
    (na, ma, qa), (nb, mb, qb) = a, b
    with np.errstate(all="ignore"):
        n = na + nb
        d = mb - ma
        w = nb / n
        mean = ma + d * w
        m2 = (qa + qb) + (d * d) * (na * w)
    both = np.stack([n, mean, m2])
    return np.where(nb == 0, a, np.where(na == 0, b, both))


def tree(nodes):
    """[3, L, cols] -> [3, cols]: pairwise by level, an unpaired last node passes up"""
    while nodes.shape[1] > 1:
        m = nodes.shape[1] // 2
        up = merge(nodes[:, 0:2 * m:2], nodes[:, 1:2 * m:2])
        nodes = np.concatenate([up, nodes[:, 2 * m:]], axis=1) if nodes.shape[1] % 2 else up
    return nodes[:, 0]


def moments(x, mask=None, stats=None):
    """the statistics after invsim_moments(x, mask) on `stats` (default: the prior); x is [rows, cols]"""
    x = np.asarray(x)
    stats = prior(x.shape[1]) if stats is None else np.asarray(stats, F64)
    if x.shape[0] == 0:
        return stats.copy()
    return merge(stats, tree(leaves(x, mask)))


def _flag(a, shape):
    return np.zeros(shape, bool) if a is None else np.asarray(a).astype(bool)


def discounted_returns(reward, terminated, truncated, done0, gamma, ret):
    """(out f64 [K, n], valid uint8 [K, n], the new ret [n])"""
    reward = np.asarray(reward, F64)
    K, n = reward.shape
    te, tr = _flag(terminated, (K, n)), _flag(truncated, (K, n))
    prev = _flag(done0, (n,))
    ret = np.asarray(ret, F64).copy()
    out, valid = np.zeros((K, n), F64), np.zeros((K, n), np.uint8)
    gamma = F64(gamma)
    with np.errstate(all="ignore"):
        for k in range(K):
            done = te[k] | tr[k]
            t = ret * gamma
            new = t + reward[k]
            out[k] = np.where(prev, F64(0.0), new)
            valid[k] = ~prev
            ret = np.where(prev | done, F64(0.0), new)
            prev = done
    return out, valid, ret


def _var(stats):
    stats = np.asarray(stats, F64)
    with np.errstate(all="ignore"):
        return np.where(stats[0] == 0, F64(1.0), stats[2] / stats[0])


def normalize_rewards(reward, stats, epsilon, clip):
    reward = np.asarray(reward, F64)
    clip = F64(clip)
    with np.errstate(all="ignore"):
        sd = np.sqrt(_var(stats)[0] + F64(epsilon))
        v = reward / sd
    return np.where(v < -clip, -clip, np.where(v > clip, clip, v))


def norm_params(stats, epsilon):
    """(scale f32 [cols], shift f32 [cols])"""
    stats = np.asarray(stats, F64)
    with np.errstate(all="ignore"):
        inv = F64(1.0) / np.sqrt(_var(stats) + F64(epsilon))
        return inv.astype(F32), (-(stats[1] * inv)).astype(F32)
