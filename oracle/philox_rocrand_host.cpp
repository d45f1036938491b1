// rocRAND's own Philox4x32-10 block function run on the host (test
// infrastructure only; tests/test_oracle.py compiles and runs it).  The
// device's fast stream calls the same ten_rounds (csrc/device_common.hpp
// PhiloxBlock); it is __host__ __device__, so no GPU is involved here.
//
// stdin: one "c0 c1 c2 c3 k0 k1" line of hex words per block;
// stdout: the four output words per line.
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_philox4x32_10.h>

#include <cstdio>

struct Block : rocrand_device::philox4x32_10_engine {
    __host__ Block() {}   // the counter and key are arguments, the engine's own state is unused
    __host__ uint4 run(uint4 c, uint2 k) { return this->ten_rounds(c, k); }
};

int main() {
    unsigned c0, c1, c2, c3, k0, k1;
    Block b;
    while (std::scanf("%x %x %x %x %x %x", &c0, &c1, &c2, &c3, &k0, &k1) == 6) {
        const uint4 x = b.run(make_uint4(c0, c1, c2, c3), make_uint2(k0, k1));
        std::printf("%08x %08x %08x %08x\n", x.x, x.y, x.z, x.w);
    }
    return 0;
}
