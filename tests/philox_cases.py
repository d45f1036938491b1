"""The case table of the fast demand stream's oracle tests, shared by

* tests/test_oracle.py (CPU): the oracle's restatement of the stream against
  tests/philox_model.py and rocRAND's own block function, and the FLOORS: over
  exactly the seeds and launch steps of the GPU test, the oracle's draws take
  the branches that make the comparison mean something (PTRS rejections reach
  blocks j >= 1, multiplication draws with an odd uniform count leave a held
  half for sub() to drop, the integers case runs the 32-bit path);
* tests/test_gpu_philox_oracle.py: every device path against the oracle.
"""
import functools

import numpy as np

N_ENV = 1000        # a multiple of neither 64 nor 256
FLOOR = 100         # hits of every branch named below, over a case's envs and steps

# Philox4x32-10 known answers: (counter words, key words) -> output words.  The
# Random123 known-answer inputs (zeros, ones, the digits of pi); the outputs
# were printed by rocRAND's own ten_rounds on the host
# (oracle/philox_rocrand_host.cpp), which tests/test_oracle.py runs again.
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# ---- InvMgmt demand cases: id -> (dist, dist_param of the env, base seed)
IM_STEPS = 33 + 45          # launch steps of the step + rollout drive (tests/test_gpu_philox_oracle.py _IM_PHASES)
# (first launch step, count) of the stretches that draw: launch steps 30 and 61
# are the NEXT_STEP reset steps of the 30-period episodes, which draw nothing
IM_DRAW_RANGES = ((0, 30), (31, 30), (62, 16))
IM_CASES = {
    "mu0.3": (1, {"mu": 0.3}, 1100),
    "mu9.99": (1, {"mu": 9.99}, 1200),
    "mu10": (1, {"mu": 10.0}, 1300),
    "mu20": (1, {"mu": 20}, 1400),
    "mu162.65": (1, {"mu": 162.65}, 1500),
    # tests/numpy_sampler_cases.py: the 32-bit integers path with its rejection
    # loop, BTPE with Step 52, the ziggurat's slow path
    "int_0_3x2p30": (3, {"low": 0, "high": 3 * 2**30}, 1600),
    "bin_1000_.3": (2, {"n": 1000, "p": 0.3}, 1700),
    "geo_.05": (4, {"p": 0.05}, 1800),
}
# the oracle counters that must reach FLOOR over a case's N_ENV envs x IM_STEPS launch steps
IM_FLOORS = {
    "mu0.3": ("pois_mult", "pois_mult_odd"),
    "mu9.99": ("pois_mult", "pois_mult_odd"),
    "mu10": ("pois_ptrs", "pois_ptrs_reject"),
    "mu20": ("pois_ptrs", "pois_ptrs_reject"),
    "mu162.65": ("pois_ptrs", "pois_ptrs_reject"),
    "int_0_3x2p30": ("int32_draw", "int32_reject"),
    "bin_1000_.3": ("btpe_step52", "btpe_four_log", "btpe_fproduct_reject"),
    "geo_.05": ("geom_inversion", "zig_slow", "zig_wedge_reject"),
}


def sampler_args(dist, dp):
    """(n_or_low, high exclusive, p) as pyoracle.philox_stream_counts takes them"""
    if dist == 1:
        return 0, 0, float(dp["mu"])
    if dist == 2:
        return int(dp["n"]), 0, float(dp["p"])
    if dist == 3:
        return int(dp["low"]), int(dp["high"]) + 1, 0.0
    return 0, 0, float(dp["p"])


@functools.lru_cache(maxsize=None)
def im_counts(case_id, n_env=N_ENV, steps=IM_STEPS):
    """the oracle's branch counters over env i = seed base + i, launch steps 0 .. steps - 1, stream 0"""
    import pyoracle
    dist, dp, base = IM_CASES[case_id]
    lo, hi, p = sampler_args(dist, dp)
    assert steps == IM_STEPS
    total = dict.fromkeys(pyoracle.COUNTERS, 0)
    for i in range(n_env):
        for s0, k in IM_DRAW_RANGES:
            _, cnt = pyoracle.philox_stream_counts(base + i, dist, k, s0, 0, lo, hi, p)
            for name, v in cnt.items():
                total[name] += v
    return total


# ---- Newsvendor: (lead time, step limit, mu_max), base seed
NV_CASES = {"L5": ((5, 40, 200.0), 2100), "L2_mu14": ((2, 12, 14.0), 2200), "L9": ((9, 17, 200.0), 2300)}

# ---- Net: base seeds per graph
NET_SEED = {"default": 3100, "custom": 3200, "user_d_between": 3300, "samplers": 3400}
