// numpy 2.2.6 Generator.standard_normal (random_standard_normal of
// distributions.c): the 256-level ziggurat over ki / wi / fi, restated for the
// Gaussian MLP actor's action noise (include/invsim.h "Gaussian MLP actor").
// One draw takes one next64 on the fast path (98.6 % of draws); a wedge draw
// takes one more uniform and an exp, a tail draw two uniforms and two log1p per
// attempt.
//
// Roundings.  numpy's build does not fuse the wedge test's multiply and add:
// (fi[idx - 1] - fi[idx]) * u + fi[idx] is two roundings, and so are the tail's
// products.  This text is built with -ffp-contract=off (csrc/Makefile), as the
// other samplers are.  log1p and exp are the device library's, not glibc's:
// the caveat numpy_dists.hpp states for the geometric sampler holds here too,
// for the 1.4 % of draws that reach them (an acceptance decided the other way
// needs a last-ulp difference to straddle the comparison; the tests compare
// every draw of their cases with numpy's).
//
// The text also compiles for the host (tests build it with sanitizers against
// model draws): NPN_FN is the functions' qualifier and NPZN_QUAL the tables'.
#pragma once
#include <math.h>
#include <stdint.h>

#include "numpy_normal_tables.hpp"

#ifndef NPN_FN
#define NPN_FN __device__ inline
#endif

namespace invsim {

// G: next64() and next_double() = (next64() >> 11) * 2**-53, numpy's next_uint64 / next_double
template <class G>
NPN_FN double np_standard_normal(G &g) {
    for (;;) {
        uint64_t r = g.next64();
        const int idx = (int)(r & 0xff);
        r >>= 8;
        const int sign = (int)(r & 0x1);
        const uint64_t rabs = (r >> 1) & 0x000fffffffffffffULL;
        double x = (double)rabs * npz_wi[idx];
        if (sign) x = -x;
        if (rabs < npz_ki[idx]) return x;        // 98.6 %: inside the rectangle
        if (idx == 0) {                          // the tail past R
            for (;;) {
                const double xx = -NPZ_NOR_INV_R * log1p(-g.next_double());
                const double yy = -log1p(-g.next_double());
                if (yy + yy > xx * xx) return ((rabs >> 8) & 0x1) ? -(NPZ_NOR_R + xx) : NPZ_NOR_R + xx;
            }
        } else if ((npz_fi[idx - 1] - npz_fi[idx]) * g.next_double() + npz_fi[idx] < exp(-0.5 * x * x)) {
            return x;                            // the wedge
        }
    }
}

}  // namespace invsim
