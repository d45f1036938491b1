"""Philox4x32-10 and the fast demand stream's generator (include/invsim.h
INVSIM_DEMAND_PHILOX) in plain Python ints: the third statement of the stream,
next to the device's (csrc/device_common.hpp PhiloxGen, rocRAND's block
function) and the oracle's (oracle/oracle.c), and the one a reader can check
against the paper (Salmon et al., SC'11) by eye."""
M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key schedule (Weyl) constants
MASK = 0xFFFFFFFF
RESET = 0xFFFFFFFF                       # draw stream of the Newsvendor reset's uniforms


def block(ctr, key):
    """ten rounds on the counter words (c0, c1, c2, c3) under the key (k0, k1)"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


class Gen:
    """key: the env's PCG64 increment high word (64 bits; low half key.x)"""

    def __init__(self, key64):
        self.key = (key64 & MASK, key64 >> 32)
        self.s, self.r, self.j, self.hold = 0, 0, 0, None

    def set_step(self, s):
        self.s = s

    def sub(self, r):
        self.r, self.j, self.hold = r, 0, None

    def next64(self):
        if self.hold is not None:
            x, self.hold = self.hold, None
            return x
        x = block((self.j, self.r, self.s & MASK, self.s >> 32), self.key)
        self.j += 1
        self.hold = (x[3] << 32) | x[2]
        return (x[1] << 32) | x[0]

    def next_double(self):
        return (self.next64() >> 11) * 2.0 ** -53
