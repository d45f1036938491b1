// The device sampler's text (csrc/numpy_normal.hpp) compiled for the host, a
// stand-alone program for sanitizer builds (tests/test_mlp_gaussian.py builds it
// with -fsanitize=address,undefined and runs it against the Python model's
// draws; nothing here is loaded into Python).
//
//   normal_host_check cases.bin
// cases.bin: u64 n_cases, then per case u64 state_hi, state_lo, inc_hi, inc_lo,
// u64 n, and n f64 draws (their bits).  Exit status 0 when every draw agrees
// bit for bit; prints "ok <cases> <draws>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define NPN_FN inline
#define NPZN_QUAL static const
#include "numpy_normal.hpp"

namespace {

// numpy's PCG64 (XSL-RR 128/64), as device_common.hpp's Pcg
struct HostPcg {
    unsigned __int128 state, inc;
    uint64_t next64() {
        const unsigned __int128 mult = ((unsigned __int128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
        state = state * mult + inc;
        const uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
        const uint64_t x = hi ^ lo;
        const unsigned rot = (unsigned)(hi >> 58);
        return (x >> rot) | (x << ((64u - rot) & 63u));
    }
    double next_double() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
};

bool read_u64(FILE *f, uint64_t *v, size_t n) { return fread(v, sizeof(uint64_t), n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    uint64_t n_cases = 0, draws = 0;
    if (!read_u64(f, &n_cases, 1)) return fprintf(stderr, "short file\n"), 2;
    for (uint64_t c = 0; c < n_cases; c++) {
        uint64_t head[5];
        if (!read_u64(f, head, 5) || head[4] > (1u << 24)) return fprintf(stderr, "bad case %llu\n", (unsigned long long)c), 2;
        std::vector<uint64_t> want(head[4]);
        if (!want.empty() && !read_u64(f, want.data(), want.size())) return fprintf(stderr, "short case\n"), 2;
        HostPcg g{((unsigned __int128)head[0] << 64) | head[1], ((unsigned __int128)head[2] << 64) | head[3]};
        for (size_t i = 0; i < want.size(); i++, draws++) {
            const double z = invsim::np_standard_normal(g);
            uint64_t got;
            memcpy(&got, &z, 8);
            if (got != want[i]) {
                fprintf(stderr, "case %llu draw %zu: %016llx, expected %016llx\n", (unsigned long long)c, i,
                        (unsigned long long)got, (unsigned long long)want[i]);
                return 1;
            }
        }
    }
    fclose(f);
    printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)draws);
    return 0;
}
