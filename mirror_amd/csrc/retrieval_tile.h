// The exact-f32 tile product shared by the retrieval kernels (retrieval.hip: ranks, retrieval_topk.hip: top-k): a workgroup of 4 waves
// (2 x 2) forms a 128 x 128 tile of S = q k^T, each wave 2 x 2 accumulators of 32 x 32 (v_mfma_f32_32x32x2_f32), the K loop over D through a
// double-buffered LDS stage of 16 with the remainder in D zero-filled.  Every element is ONE k-ordered f32 fmaf chain from 0
// (fmaf(0, 0, acc) = acc), which retr_chain restates for a single row pair, so whatever is decided on these numbers does not depend on
// the tiling.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RT_TILE = 128;          // tile edge in rows of q and of k
constexpr int RT_BK = 16;             // K step through LDS: 8 MFMAs of k = 2
constexpr int RT_LD = RT_BK + 1;      // LDS row stride in floats: 32 rows at one k fall into 32 banks
constexpr int RT_THREADS = 256;
constexpr int RT_QUADS = RT_TILE * RT_BK / 4 / RT_THREADS;   // 16-byte pieces of one operand tile per thread

// a . b over D as ONE k-ordered f32 fmaf chain from 0 in this lane: bit for bit what the MFMA tile forms for the same row pair
__device__ __forceinline__ float retr_chain(const float* __restrict__ a, const float* __restrict__ b, int D, int vec) {
    float acc = 0.f;
    int c = 0;
    if (vec) {
        for (; c + 4 <= D; c += 4) {
            const f4_t x = *reinterpret_cast<const f4_t*>(a + c), y = *reinterpret_cast<const f4_t*>(b + c);
            acc = fmaf(x[0], y[0], acc);
            acc = fmaf(x[1], y[1], acc);
            acc = fmaf(x[2], y[2], acc);
            acc = fmaf(x[3], y[3], acc);
        }
    }
    for (; c < D; c++) acc = fmaf(a[c], b[c], acc);
    return acc;
}

// this thread's pieces of rows [row0, row0 + 128) x columns [k0, k0 + 16) of x [n x D]; zero outside the matrix
__device__ __forceinline__ void retr_load(f4_t (&r)[RT_QUADS], const float* __restrict__ x, int n, int D, int row0, int k0, int vec,
                                          int tid) {
#pragma unroll
    for (int u = 0; u < RT_QUADS; u++) {
        const int c = tid + u * RT_THREADS;
        const int row = row0 + (c >> 2), kk = k0 + (c & 3) * 4;
        f4_t v = {0.f, 0.f, 0.f, 0.f};
        if (row < n) {
            const float* p = x + (int64_t)row * D + kk;
            if (vec && kk + 4 <= D) {
                v = *reinterpret_cast<const f4_t*>(p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (kk + e < D) v[e] = p[e];
            }
        }
        r[u] = v;
    }
}

__device__ __forceinline__ void retr_store(const f4_t (&r)[RT_QUADS], float* __restrict__ tile, int tid) {
#pragma unroll
    for (int u = 0; u < RT_QUADS; u++) {
        const int c = tid + u * RT_THREADS;
        float* p = tile + (c >> 2) * RT_LD + (c & 3) * 4;
#pragma unroll
        for (int e = 0; e < 4; e++) p[e] = r[u][e];
    }
}

// acc = rows [row0, row0 + 128) of q times rows [col0, col0 + 128) of k, from zero.  Called by all 256 threads; ends with a barrier
// behind the last read of the stages.  Accumulator register r of lane l of wave (wm, wn) = (wave >> 1, wave & 1), block (i, j):
// tile row wm 64 + i 32 + (r & 3) + 8 (r >> 2) + 4 (l >> 5), tile column wn 64 + j 32 + (l & 31).
__device__ __forceinline__ void retr_product(f32x16 (&acc)[2][2], const float* __restrict__ q, const float* __restrict__ k, int nq,
                                             int nk, int D, int row0, int col0, int vec, float (&s_a)[2][RT_TILE * RT_LD],
                                             float (&s_b)[2][RT_TILE * RT_LD]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nt = (D + RT_BK - 1) / RT_BK;
    f4_t ra[RT_QUADS], rb[RT_QUADS];
    retr_load(ra, q, nq, D, row0, 0, vec, tid);
    retr_load(rb, k, nk, D, col0, 0, vec, tid);
    retr_store(ra, s_a[0], tid);
    retr_store(rb, s_b[0], tid);
    if (nt > 1) {
        retr_load(ra, q, nq, D, row0, RT_BK, vec, tid);
        retr_load(rb, k, nk, D, col0, RT_BK, vec, tid);
    }
    __syncthreads();

    // lane l feeds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31] of each k = 2 step
    const int frag = (lane & 31) * RT_LD + (lane >> 5);
    for (int t = 0; t < nt; t++) {
        const int cur = t & 1;
        if (t + 1 < nt) {          // stage cur ^ 1 was last read before the barrier that ended step t - 1
            retr_store(ra, s_a[cur ^ 1], tid);
            retr_store(rb, s_b[cur ^ 1], tid);
            if (t + 2 < nt) {
                retr_load(ra, q, nq, D, row0, (t + 2) * RT_BK, vec, tid);
                retr_load(rb, k, nk, D, col0, (t + 2) * RT_BK, vec, tid);
            }
        }
        const float* at = s_a[cur] + wm * 64 * RT_LD + frag;
        const float* bt = s_b[cur] + wn * 64 * RT_LD + frag;
#pragma unroll
        for (int s = 0; s < RT_BK / 2; s++) {
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; i++) af[i] = at[i * 32 * RT_LD + 2 * s];
#pragma unroll
            for (int j = 0; j < 2; j++) bf[j] = bt[j * 32 * RT_LD + 2 * s];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
}

}  // namespace
