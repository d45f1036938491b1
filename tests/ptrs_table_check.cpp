// The host table of PTRS's right-hand side (csrc/ptrs_table.hpp: ptrs_const and
// rhs_table, the functions libinvsim's create calls run) in a stand-alone
// program, for plain and sanitizer builds (tests/test_ptrs_table.py; nothing
// here is loaded into Python).
//
//   ptrs_table_check LAM [LAM ...]
// Every rate is given as the 16 hex digits of its double.  All rates go into
// ONE table vector, in order, as NetInvMgmt's create does per retail link.
// Prints per rate
//   rate <lam bits> <loglam bits> <k0> <nk> <toff>
// followed by nk lines, the bits of that rate's entries read back from the
// shared vector at toff, and last "total <vector size>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ptrs_table.hpp"

namespace {

uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return fprintf(stderr, "usage: %s LAM_BITS_HEX ...\n", argv[0]), 2;
    std::vector<invsim::PtrsConst> pcs;
    std::vector<double> tab;
    for (int i = 1; i < argc; i++) {
        char *end = nullptr;
        const uint64_t b = strtoull(argv[i], &end, 16);
        if (!end || *end || strlen(argv[i]) != 16) return fprintf(stderr, "bad rate %s\n", argv[i]), 2;
        double lam;
        memcpy(&lam, &b, 8);
        pcs.push_back(invsim::ptrs_const(lam));
        invsim::rhs_table(pcs.back(), tab);
    }
    for (const invsim::PtrsConst &c : pcs) {
        printf("rate %016llx %016llx %d %d %d\n", (unsigned long long)bits(c.lam), (unsigned long long)bits(c.loglam),
               c.k0, c.nk, c.toff);
        if (c.nk < 0 || c.toff < 0 || (size_t)c.toff + (size_t)c.nk > tab.size())
            return fprintf(stderr, "window outside the table vector\n"), 1;
        for (int k = 0; k < c.nk; k++) printf("%016llx\n", (unsigned long long)bits(tab[(size_t)c.toff + k]));
    }
    printf("total %zu\n", tab.size());
    return 0;
}
