// Running normalisation (include/invsim.h "Running normalisation" states every
// operation): per-column moments of a [rows][cols] block as a fixed binary tree
// of Welford / Chan merges over leaves of INVSIM_MOMENTS_BLOCK rows, the
// discounted-return scan, and the three small kernels that turn the statistics
// into normalised rewards and into the network's input rows.  f64 throughout,
// every operation rounded separately (the library is built with
// -ffp-contract=off); no atomics, so the result does not depend on scheduling.
//
// moments_leaf_kernel.  The reduction reads x once and is bound by that read.
// A workgroup owns an aligned group of W = T * MOM_PASSES consecutive leaves
// (W a power of two) and, for wide rows, one chunk of CC columns.  Per pass it
// copies T leaves (at most MOM_TILE_BYTES of x, contiguous in memory when the
// chunk is the whole row: 16 B per lane, coalesced) into LDS, then lanes are
// (leaf, column) pairs that walk their 64 rows in LDS twice: the sum in
// ascending row order, then the squared deviations from the rounded mean.  A
// leaf's LDS image is followed by one row of padding, so that the lanes of
// different leaves at the same row (the only lanes there are when cols == 1)
// fall on consecutive banks instead of one.  The W leaf results stay in LDS
// and are merged pairwise, level by level, into the group's node: one
// [3][cols] record per workgroup goes to scratch.  moments_tree_kernel merges
// aligned groups of 256 nodes the same way; its last launch (one group) also
// computes stats = Merge(stats, batch).  Absent nodes right of a ragged end
// are (0, 0, 0), which Merge hands on unchanged: the contract's "an unpaired
// last node passes up".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "../../include/invsim.h"
#include "norm.hpp"

namespace invsim {
namespace {

constexpr int MOM_B = INVSIM_MOMENTS_BLOCK;
constexpr int MOM_THREADS = 256;
// bytes of x per pass, leaves per pass at most, passes per workgroup (profiles/normalize/table.md)
#ifndef MOM_TILE_BYTES
#define MOM_TILE_BYTES 32768
#endif
#ifndef MOM_PASSES
#define MOM_PASSES 4
#endif
constexpr int MOM_MAX_T = 64;
constexpr int TREE_NODES = 256, TREE_COLS = 4;
static_assert((MOM_PASSES & (MOM_PASSES - 1)) == 0, "a workgroup's leaves are an aligned power-of-two group");
static_assert(MOM_B * 4 % 16 == 0, "a 16-byte load never straddles two leaves");

struct MomGeom {
    int32_t T, CC, chunks;      // leaves per pass, columns per chunk, column chunks
    int64_t groups;             // workgroups along the rows = nodes the leaf kernel writes
    size_t lds;
};

MomGeom mom_geom(int64_t rows, int32_t cols, int esz) {
    MomGeom g{1, cols, 1, 0, 0};
    const int64_t leaf_bytes = (int64_t)MOM_B * cols * esz;
    if (leaf_bytes <= MOM_TILE_BYTES) {
        while (g.T * 2 <= MOM_MAX_T && g.T * 2 * leaf_bytes <= MOM_TILE_BYTES) g.T *= 2;
    } else {
        g.chunks = (int32_t)((leaf_bytes + MOM_TILE_BYTES - 1) / MOM_TILE_BYTES);
        g.CC = (cols + g.chunks - 1) / g.chunks;
        g.chunks = (cols + g.CC - 1) / g.CC;
    }
    const int64_t leaves = (rows + MOM_B - 1) / MOM_B, W = (int64_t)g.T * MOM_PASSES;
    g.groups = (leaves + W - 1) / W;
    g.lds = (size_t)W * g.CC * 3 * sizeof(double) + ((size_t)g.T * (MOM_B + 1) * g.CC * esz + 7) / 8 * 8 + (size_t)g.T * MOM_B;
    return g;
}

// a = Merge(a, b) on [3] records (count, mean, M2)
__device__ __forceinline__ void mom_merge(double *a, const double *b) {
    const double nb = b[0], na = a[0];
    if (nb == 0.0) return;
    if (na == 0.0) {
        a[0] = nb, a[1] = b[1], a[2] = b[2];
        return;
    }
    const double n = na + nb;
    const double d = b[1] - a[1];
    const double w = nb / n;
    const double mean = a[1] + d * w;
    const double m2 = (a[2] + b[2]) + (d * d) * (na * w);
    a[0] = n, a[1] = mean, a[2] = m2;
}

// P is [nodes][stride][3] in LDS, nodes a power of two: node 0 becomes the root of the pairwise tree
__device__ __forceinline__ void mom_tree(double *P, int nodes, int stride, int cc) {
    for (int st = 1; st < nodes; st <<= 1) {
        __syncthreads();
        const int pairs = (nodes / (2 * st)) * cc;
        for (int i = threadIdx.x; i < pairs; i += MOM_THREADS) {
            const int nd = (i / cc) * 2 * st, c = i % cc;
            mom_merge(P + ((size_t)nd * stride + c) * 3, P + ((size_t)(nd + st) * stride + c) * 3);
        }
    }
    __syncthreads();
}

template <typename E>
__global__ void __launch_bounds__(MOM_THREADS)
moments_leaf_kernel(const E *__restrict__ x, const uint8_t *__restrict__ mask, int64_t rows, int32_t cols, int32_t T,
                    int32_t CC, int32_t vec, double *__restrict__ part) {
    extern __shared__ double mom_lds[];
    constexpr int B = MOM_B;
    const int W = T * MOM_PASSES;
    double *P = mom_lds;                                              // [W][CC][3]
    E *tile = reinterpret_cast<E *>(P + (size_t)W * CC * 3);          // [T][B + 1][CC]
    uint8_t *m = reinterpret_cast<uint8_t *>(mom_lds) + (size_t)W * CC * 3 * sizeof(double) +
                 ((size_t)T * (B + 1) * CC * sizeof(E) + 7) / 8 * 8;  // [T][B]: the row counts
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * CC;
    const int cc = min(CC, cols - c0);
    const int64_t row_g = (int64_t)blockIdx.x * W * B;
    for (int p = 0; p < MOM_PASSES; ++p) {
        const int64_t row0 = row_g + (int64_t)p * T * B;
        const int64_t left = rows - row0;
        const int nrow = left <= 0 ? 0 : (int)(left < (int64_t)T * B ? left : (int64_t)T * B);
        if (p) __syncthreads();                                       // the walks of the pass before are over
        for (int i = tid; i < T * B; i += MOM_THREADS) m[i] = (i < nrow && (!mask || mask[row0 + i] != 0)) ? 1 : 0;
        if (vec) {                                                    // CC == cols: the pass is one contiguous run of x
            constexpr int NV = 16 / (int)sizeof(E);
            const int nel = nrow * CC, nvec = nel / NV, leaf_el = B * CC;
            const E *src = x + row0 * cols;
            const uint4 *src4 = reinterpret_cast<const uint4 *>(src);
            for (int i = tid; i < nvec; i += MOM_THREADS) {
                const uint4 v = src4[i];
                E e[NV];
                __builtin_memcpy(e, &v, 16);
                const int ei = i * NV;
                E *d = tile + ei + (ei / leaf_el) * CC;
#pragma unroll
                for (int j = 0; j < NV; ++j) d[j] = e[j];
            }
            for (int ei = nvec * NV + tid; ei < nel; ei += MOM_THREADS) tile[ei + (ei / leaf_el) * CC] = src[ei];
        } else {
            const int nel = nrow * cc;
            for (int i = tid; i < nel; i += MOM_THREADS) {
                const int r = i / cc, c = i - r * cc;
                tile[(size_t)(r + r / B) * CC + c] = x[(row0 + r) * cols + c0 + c];
            }
        }
        __syncthreads();
        if (tid < T * cc) {
            const int b = tid / cc, c = tid - b * cc;
            const E *col = tile + (size_t)b * (B + 1) * CC + c;
            const uint8_t *on = m + b * B;
            double n = 0.0, s = 0.0;
#pragma unroll 8
            for (int r = 0; r < B; ++r) {
                const double v = (double)col[(size_t)r * CC];
                s = on[r] ? s + v : s;
                n = on[r] ? n + 1.0 : n;
            }
            double mean = 0.0, q = 0.0;
            if (n > 0.0) {
                mean = s / n;
#pragma unroll 8
                for (int r = 0; r < B; ++r) {
                    const double d = (double)col[(size_t)r * CC] - mean;
                    q = on[r] ? q + d * d : q;
                }
            }
            double *o = P + ((size_t)(p * T + b) * CC + c) * 3;
            o[0] = n, o[1] = mean, o[2] = q;
        }
    }
    mom_tree(P, W, CC, cc);
    if (tid < cc)
        for (int k = 0; k < 3; ++k) part[((int64_t)blockIdx.x * 3 + k) * cols + c0 + tid] = P[tid * 3 + k];
}

// in [n][3][cols] -> out [ceil(n / 256)][3][cols]; with fold (one group): out is stats, = Merge(stats, root)
__global__ void __launch_bounds__(MOM_THREADS)
moments_tree_kernel(const double *__restrict__ in, int64_t n, int32_t cols, double *out, int32_t fold) {
    __shared__ double P[TREE_NODES * TREE_COLS * 3];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * TREE_COLS;
    const int cc = min(TREE_COLS, cols - c0);
    const int64_t n0 = (int64_t)blockIdx.x * TREE_NODES;
    for (int i = tid; i < TREE_NODES * 3 * TREE_COLS; i += MOM_THREADS) {
        const int nd = i / (3 * TREE_COLS), k = (i / TREE_COLS) % 3, c = i % TREE_COLS;
        double v = 0.0;
        if (n0 + nd < n && c < cc) v = in[((n0 + nd) * 3 + k) * cols + c0 + c];
        P[(nd * TREE_COLS + c) * 3 + k] = v;
    }
    mom_tree(P, TREE_NODES, TREE_COLS, cc);
    if (tid < cc) {
        const int c = c0 + tid;
        if (fold) {
            double a[3] = {out[c], out[(int64_t)cols + c], out[2 * (int64_t)cols + c]};
            mom_merge(a, P + tid * 3);
            out[c] = a[0], out[(int64_t)cols + c] = a[1], out[2 * (int64_t)cols + c] = a[2];
        } else {
            for (int k = 0; k < 3; ++k) out[((int64_t)blockIdx.x * 3 + k) * cols + c] = P[tid * 3 + k];
        }
    }
}

// Rows per block of the scan: every load of a block is issued before its first operation, as in gae_kernel.
constexpr int DR_ROWS = 8, DR_THREADS = 256;

__global__ void __launch_bounds__(DR_THREADS)
discounted_returns_kernel(const double *__restrict__ rew, const uint8_t *__restrict__ term,
                          const uint8_t *__restrict__ trunc, const uint8_t *__restrict__ done0, int32_t K, int64_t N,
                          double gamma, double *__restrict__ ret, double *__restrict__ out, uint8_t *__restrict__ valid) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    constexpr int U = DR_ROWS;
    double acc = ret[e];
    bool prev = done0 ? done0[e] != 0 : false;
    for (int k0 = 0; k0 < K; k0 += U) {
        double r[U];
        uint8_t te[U], tr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {               // rows k0 + u, clamped into the arrays
            const int64_t i = (int64_t)min(k0 + u, K - 1) * N + e;
            r[u] = rew[i];
            te[u] = term ? term[i] : (uint8_t)0;
            tr[u] = trunc ? trunc[i] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u;                   // wave-uniform
            if (k >= K) break;
            const bool done = (te[u] | tr[u]) != 0;
            const int64_t i = (int64_t)k * N + e;
            double o;
            if (prev) {                             // the row after a finished episode: no transition
                o = 0.0;
                acc = 0.0;
            } else {
                const double t = acc * gamma;
                acc = t + r[u];
                o = acc;
                if (done) acc = 0.0;
            }
            out[i] = o;
            if (valid) valid[i] = prev ? 0 : 1;
            prev = done;
        }
    }
    ret[e] = acc;
}

__device__ __forceinline__ double norm_var(const double *stats, int32_t cols, int32_t c) {
    const double cnt = stats[c];
    return cnt == 0.0 ? 1.0 : stats[2 * (int64_t)cols + c] / cnt;
}

__global__ void __launch_bounds__(256)
normalize_rewards_kernel(const double *rew, int64_t count, const double *__restrict__ stats, double epsilon, double clip,
                         double *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double sd = __dsqrt_rn(norm_var(stats, 1, 0) + epsilon);
    const double v = rew[i] / sd;
    out[i] = v < -clip ? -clip : (v > clip ? clip : v);
}

__global__ void __launch_bounds__(256)
norm_params_kernel(const double *__restrict__ stats, int32_t cols, double epsilon, float *__restrict__ scale,
                   float *__restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    const double inv = 1.0 / __dsqrt_rn(norm_var(stats, cols, c) + epsilon);
    scale[c] = (float)inv;
    if (shift) shift[c] = (float)(-(stats[(int64_t)cols + c] * inv));
}

__global__ void __launch_bounds__(256)
mlp_set_rows_kernel(float *__restrict__ dst_scale, float *__restrict__ dst_shift, const float *__restrict__ scale,
                    const float *__restrict__ shift, int32_t n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dst_scale[i] = scale[i];
    dst_shift[i] = shift[i];
}

template <typename E>
hipError_t leaf_launch(const void *x, int64_t rows, int32_t cols, const uint8_t *mask, double *part, hipStream_t s) {
    const MomGeom g = mom_geom(rows, cols, (int)sizeof(E));
    if (g.groups > 0x7fffffff) return hipErrorInvalidValue;
    const int32_t vec = g.chunks == 1 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    hipLaunchKernelGGL(moments_leaf_kernel<E>, dim3((unsigned)g.groups, (unsigned)g.chunks), dim3(MOM_THREADS), g.lds, s,
                       static_cast<const E *>(x), mask, rows, cols, g.T, g.CC, vec, part);
    return hipGetLastError();
}

}  // namespace

int64_t moments_scratch_bytes(int64_t rows, int32_t cols) {
    // the 8-byte dtypes have the fewest leaves per workgroup, hence the most nodes
    int64_t n = mom_geom(rows, cols, 8).groups, nodes = n;
    while (n > TREE_NODES) {
        n = (n + TREE_NODES - 1) / TREE_NODES;
        nodes += n;
    }
    return nodes * 3 * cols * (int64_t)sizeof(double);
}

hipError_t moments_launch(const void *x, int32_t dtype, int64_t rows, int32_t cols, const uint8_t *mask, double *stats,
                          double *scratch, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipError_t e;
    int esz = 8;
    if (dtype == INVSIM_DTYPE_I64) {
        e = leaf_launch<int64_t>(x, rows, cols, mask, scratch, s);
    } else if (dtype == INVSIM_DTYPE_F32) {
        esz = 4;
        e = leaf_launch<float>(x, rows, cols, mask, scratch, s);
    } else {
        e = leaf_launch<double>(x, rows, cols, mask, scratch, s);
    }
    if (e != hipSuccess) return e;
    int64_t n = mom_geom(rows, cols, esz).groups;
    const unsigned cy = (unsigned)((cols + TREE_COLS - 1) / TREE_COLS);
    double *in = scratch;
    while (n > TREE_NODES) {
        const int64_t up = (n + TREE_NODES - 1) / TREE_NODES;
        double *out = in + n * 3 * cols;
        hipLaunchKernelGGL(moments_tree_kernel, dim3((unsigned)up, cy), dim3(MOM_THREADS), 0, s, in, n, cols, out, 0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        in = out, n = up;
    }
    hipLaunchKernelGGL(moments_tree_kernel, dim3(1, cy), dim3(MOM_THREADS), 0, s, in, n, cols, stats, 1);
    return hipGetLastError();
}

hipError_t discounted_returns_launch(const double *rew, const uint8_t *term, const uint8_t *trunc, const uint8_t *done0,
                                     int32_t K, int64_t N, double gamma, double *ret, double *out, uint8_t *valid,
                                     hipStream_t s) {
    if (K <= 0 || N <= 0) return hipSuccess;
    const int64_t blocks = (N + DR_THREADS - 1) / DR_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(discounted_returns_kernel, dim3((unsigned)blocks), dim3(DR_THREADS), 0, s, rew, term, trunc, done0, K,
                       N, gamma, ret, out, valid);
    return hipGetLastError();
}

hipError_t normalize_rewards_launch(const double *rew, int64_t count, const double *stats, double epsilon, double clip,
                                    double *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(normalize_rewards_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rew, count, stats, epsilon, clip,
                       out);
    return hipGetLastError();
}

hipError_t norm_params_launch(const double *stats, int32_t cols, double epsilon, float *scale, float *shift, hipStream_t s) {
    hipLaunchKernelGGL(norm_params_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, stats, cols, epsilon, scale,
                       shift);
    return hipGetLastError();
}

hipError_t mlp_set_rows_launch(float *dst_scale, float *dst_shift, const float *scale, const float *shift, int32_t n,
                               hipStream_t s) {
    hipLaunchKernelGGL(mlp_set_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst_scale, dst_shift, scale,
                       shift, n);
    return hipGetLastError();
}

}  // namespace invsim
