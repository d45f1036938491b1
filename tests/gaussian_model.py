"""The numpy model of the Gaussian MLP actor's sampling stage (include/invsim.h
"Gaussian MLP actor") and the table of action seeds and draw counts its GPU
tests use (TEST INFRASTRUCTURE, never shipped).

* the normals are numpy's own ``Generator.standard_normal`` on the env's action
  stream (``random_agent_model.generator``), drawn once per seed and shared;
* ``sample`` / ``log_prob`` restate the two formulas in float32 with
  ``mlp_model.fmaf``.

DRAWS is the contract between the GPU tests and the CPU test: every GPU case
takes its normals through ``normals()``, which refuses more than DRAWS[seed]
per env, and tests/test_mlp_gaussian.py checks the Python restatement of the
draw (tests/normal_model.py) against numpy over exactly these seeds, envs and
counts.
"""
import functools

import numpy as np

import mlp_model
from random_agent_model import _state_rows, generator

F32 = np.float32
N = 1024                      # envs of every case (global indices 0 .. N - 1; shards lie inside)
DRAWS = {0: 72, 7: 11}        # action seed -> the most normals any env draws under it
MAIN = dict(seed=0, n=1024, A=3, K=24)      # the main closed-loop case: 72 draws per env


@functools.lru_cache(maxsize=None)
def _all(seed):
    z = np.stack([generator(seed, g).standard_normal(DRAWS[seed]) for g in range(N)])
    z.setflags(write=False)
    return z


def normals(seed, first, n, count, skip=0):
    """z [n, count] float64: draws skip .. skip + count - 1 of envs first .. first + n - 1"""
    assert first + n <= N and skip + count <= DRAWS[seed], "a GPU case outside the table the CPU test covers"
    return _all(seed)[first:first + n, skip:skip + count]


def state_rows(seed, first, n, count):
    """[4, n] uint64 generator rows (state hi / lo, inc hi / lo) after `count` normals"""
    assert first + n <= N and count <= DRAWS[seed]
    gens = [generator(seed, first + i) for i in range(n)]
    for g in gens:
        if count:
            g.standard_normal(count)
    return _state_rows(gens)


def sample(mean, z, std):
    """raw [n, A] float32 = fmaf(std, (float)z, mean)"""
    return mlp_model.fmaf(np.asarray(std, F32)[None, :], z.astype(F32), mean)


def log_prob(z, log_std):
    """[n] float32: the contract's accumulation, a ascending"""
    zf = z.astype(F32)
    A = zf.shape[1]
    acc = np.full(zf.shape[0], F32(-0.91893853320467274178 * float(A)), F32)
    for a in range(A):
        acc = mlp_model.fmaf(F32(-0.5) * zf[:, a], zf[:, a], acc)
        acc = (acc - F32(log_std[a])).astype(F32)
    return acc
