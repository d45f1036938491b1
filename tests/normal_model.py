"""Python restatement of numpy 2.2.6 random_standard_normal over PCG64.random_raw
(TEST INFRASTRUCTURE, never shipped): the draw the Gaussian MLP actor's kernel
makes (or-gym-inventory_amd/csrc/numpy_normal.hpp), with the ziggurat tables
parsed from the generated header the kernel is built from, and unfused float64
arithmetic (Python floats never fuse).  It also counts which path every draw
took, so a test can assert that its seeds reach the slow paths.

tests/test_mlp_gaussian.py checks it against Generator.standard_normal bit for
bit; the log1p / exp here are the host libm's, as numpy's are.
"""
import math
import os
import re

import numpy as np

from random_agent_model import generator

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "or-gym-inventory_amd", "csrc",
                      "numpy_normal_tables.hpp")
PATHS = ("fast", "wedge_accept", "wedge_reject", "tail", "tail_reject")
_TABLES = None


def tables():
    """(ki [256] int, wi [256] float, fi [256] float, R, 1 / R) of the generated header"""
    global _TABLES
    if _TABLES is None:
        text = open(HEADER).read()
        arr = {m.group(1): m.group(2).replace("ULL", "").split(",")
               for m in re.finditer(r"npz_(\w+)\[256\] = \{(.*?)\};", text, re.S)}
        ki = [int(v, 16) for v in arr["ki"]]
        wi = [float.fromhex(v.strip()) for v in arr["wi"]]
        fi = [float.fromhex(v.strip()) for v in arr["fi"]]
        assert len(ki) == len(wi) == len(fi) == 256
        R = float(re.search(r"#define NPZ_NOR_R (\S+)", text).group(1))
        inv_r = float(re.search(r"#define NPZ_NOR_INV_R (\S+)", text).group(1))
        _TABLES = (ki, wi, fi, R, inv_r)
    return _TABLES


class Raw:
    """next64 / next_double over one PCG64's random_raw words, fetched in blocks"""

    def __init__(self, bit_generator, block=64):
        self.bg, self.block, self.buf, self.i = bit_generator, block, [], 0

    def next64(self):
        if self.i == len(self.buf):
            self.buf, self.i = [int(v) for v in self.bg.random_raw(self.block)], 0
        self.i += 1
        return self.buf[self.i - 1]

    def next_double(self):
        return (self.next64() >> 11) * (1.0 / 9007199254740992.0)


def standard_normal(raw, n, counts=None):
    """n draws [n] float64 from `raw`; counts (a dict over PATHS) is added to"""
    ki, wi, fi, R, inv_r = tables()
    c = dict.fromkeys(PATHS, 0)
    out = np.empty(n, np.float64)
    for j in range(n):
        while True:
            r = raw.next64()
            idx = r & 0xff
            r >>= 8
            sign = r & 1
            rabs = (r >> 1) & 0x000fffffffffffff
            x = float(rabs) * wi[idx]
            if sign:
                x = -x
            if rabs < ki[idx]:
                c["fast"] += 1
                break
            if idx == 0:
                c["tail"] += 1
                while True:
                    xx = -inv_r * math.log1p(-raw.next_double())
                    yy = -math.log1p(-raw.next_double())
                    if yy + yy > xx * xx:
                        break
                    c["tail_reject"] += 1
                x = -(R + xx) if (rabs >> 8) & 1 else R + xx
                break
            if (fi[idx - 1] - fi[idx]) * raw.next_double() + fi[idx] < math.exp(-0.5 * x * x):
                c["wedge_accept"] += 1
                break
            c["wedge_reject"] += 1
        out[j] = x
    if counts is not None:
        for k in PATHS:
            counts[k] = counts.get(k, 0) + c[k]
    return out


def env_normals(seed, g, n, counts=None):
    """the first n normals of the action stream of the env with global index g"""
    return standard_normal(Raw(generator(seed, g).bit_generator), n, counts)
