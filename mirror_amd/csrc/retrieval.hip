// Cross-modal retrieval ranks (recall@k / median rank of the CLIP-style alignment, train_mirror.py:1382-1526): for every query the
// number of keys whose dot-product similarity is not below the positive's, WITHOUT the nq x nk similarity matrix.
//
// Two launches on the caller's stream, nothing allocated, nothing waits on the host (graph capturable):
//   1. retr_pos_kernel: d[i] = q_i . k_target[i] as the k-ordered f32 fmaf chain from 0 that v_mfma_f32_32x32x2_f32 forms
//      (one rounding per product), into the workspace; ranks[i] = 1.
//   2. retr_tile_kernel: a workgroup owns a 128 x 128 tile of S = q k^T: 4 waves as 2 x 2, each 2 x 2 accumulators of 32 x 32, the K
//      loop over D through a double-buffered LDS stage of 16 (the remainder in D zero-filled: fmaf(0, 0, acc) = acc, so the chain
//      of step 1 is reproduced bit for bit).  No split-K.  Epilogue: compare every accumulator with its row's d, count per row
//      with wave ballots (the 32 columns of a row half sit in 32 lanes), add the two column waves in LDS and issue ONE integer
//      atomic per row and tile.  Rows >= nq, columns >= nk and the column j == target[i] are excluded by index.
// A key row bit-identical to the positive's therefore ties with it exactly and counts against the query, as does every NaN.
//
// Grouped positives (mh_retrieval_ranks_grouped: several slides of one RNA sample): the positives of query i are the keys of its group,
// the rank is that of the BEST of them among the keys of other groups.  The same two launches:
//   1. retr_gpos_kernel: one wave per query finds where its group starts in the group-sorted keys (a search 64 probes wide), forms each positive's
//      similarity as the same one-lane chain (lane l takes positives l, l + 64, ...) and reduces with a NaN-propagating max.
//   2. retr_tile_kernel<true>: the same tile product; the epilogue excludes by 64-bit group id (the rows' ids in LDS, each lane's two
//      column ids and count flags in registers) where the ungrouped instance excludes the one column target[i].
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int RT_GROUP = 8;           // row tiles per group of the tile order (see retr_tile_kernel)

__global__ void __launch_bounds__(RT_THREADS) retr_pos_kernel(const float* __restrict__ q, const float* __restrict__ k, int nq, int nk,
                                                              int D, const int64_t* __restrict__ target, int vec,
                                                              float* __restrict__ d, int32_t* __restrict__ ranks) {
    const int i = blockIdx.x * RT_THREADS + threadIdx.x;
    if (i >= nq) return;
    const int64_t t = target ? target[i] : (int64_t)i;
    float acc;
    if (t < 0 || t >= nk) {
        acc = __builtin_nanf("");     // no such key: nothing is read, every key counts against the query
    } else {
        acc = retr_chain(q + (int64_t)i * D, k + t * D, D, vec);
    }
    d[i] = acc;
    ranks[i] = 1;
}

// max that keeps a NaN from either side (fmaxf drops it)
__device__ __forceinline__ float retr_nanmax(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// One wave per query (blockDim.x == RT_THREADS, whole waves): d[i] = max over the keys of query i's group of q_i . k_j, NaN if the group has no key or any of them is NaN.
// sgroup: the keys' group ids in ascending order, perm[p]: the key row that sorted position p came from.
__global__ void __launch_bounds__(RT_THREADS) retr_gpos_kernel(const float* __restrict__ q, const float* __restrict__ k, int nq, int nk,
                                                               int D, const int64_t* __restrict__ qgroup,
                                                               const int64_t* __restrict__ sgroup, const int64_t* __restrict__ perm,
                                                               int vec, float* __restrict__ d, int32_t* __restrict__ ranks) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nq) return;                                  // wave-uniform
    const int64_t g = qgroup[i];
    // the first position with sgroup >= g lies in [lo, hi]: each round 64 lanes probe 64 evenly spaced positions of the interval and
    // a ballot keeps the one gap it falls into (3 rounds at nk = 2^18 where a one-lane bisection is 18 dependent loads)
    int lo = 0, hi = nk;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + (lane + 1) * step - 1;
        const bool below = idx < hi && sgroup[idx] < g;   // true on a prefix of the lanes: sgroup ascends
        const int c = __popcll(__ballot(below));
        lo += c * step;                                   // the last probe below g was lo + c step - 1
        hi = lo + step - 1 < hi ? lo + step - 1 : hi;     // and the next one, if inside, is not below
    }
    const float* a = q + (int64_t)i * D;
    float best = -INFINITY;
    bool any = false;
    for (int p = lo + lane;; p += 64) {                   // the group's keys follow from lo on: stop at the first other id
        const bool in = p < nk && sgroup[p] == g;
        if (in) {
            const int64_t t = perm[p];
            // a row outside [0, nk) is not a permutation's: nothing is read for it and the query's best positive is NaN
            const float s = t < 0 || t >= nk ? __builtin_nanf("") : retr_chain(a, k + t * D, D, vec);
            best = retr_nanmax(best, s);
        }
        const unsigned long long m = __ballot(in);
        any = any || m != 0;
        if (m != ~0ull) break;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = retr_nanmax(best, __shfl_xor(best, o));
    if (lane == 0) {
        d[i] = any ? best : __builtin_nanf("");           // an empty group: every counted key counts against the query
        ranks[i] = 1;
    }
}

// GROUPED = false: the one excluded column of row i is target[i] (qgroup, kgroup, kcount unused).  GROUPED = true: column j is excluded
// from row i when kgroup[j] == qgroup[i] (all 64 bits) or kcount[j] == 0 (kcount NULL: every key counts); target unused.
template <bool GROUPED>
__global__ void __launch_bounds__(RT_THREADS) retr_tile_kernel(const float* __restrict__ q, const float* __restrict__ k, int nq, int nk,
                                                               int D, const int64_t* __restrict__ target,
                                                               const int64_t* __restrict__ qgroup, const int64_t* __restrict__ kgroup,
                                                               const uint8_t* __restrict__ kcount, int vec, int tiles_m,
                                                               int tiles_n, const float* __restrict__ d, int32_t* __restrict__ ranks) {
    __shared__ float s_a[2][RT_TILE * RT_LD];
    __shared__ float s_b[2][RT_TILE * RT_LD];
    __shared__ float s_d[RT_TILE];
    __shared__ int s_t[GROUPED ? 1 : RT_TILE];
    __shared__ int64_t s_g[GROUPED ? RT_TILE : 1];
    __shared__ int s_cnt[2][RT_TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // Blocks b and b + 8 share an XCD (and its L2): give each XCD a contiguous run of tile ids, and number the tiles in groups of
    // RT_GROUP row tiles, rows fastest, so that the blocks in flight on one XCD share a few row panels and a few column panels.
    const int nwg = gridDim.x;
    const int xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
    const int per_group = RT_GROUP * tiles_n;
    const int first_m = (wgid / per_group) * RT_GROUP;
    const int gm = tiles_m - first_m < RT_GROUP ? tiles_m - first_m : RT_GROUP;
    const int tile_m = first_m + (wgid % per_group) % gm, tile_n = (wgid % per_group) / gm;
    const int row0 = tile_m * RT_TILE, col0 = tile_n * RT_TILE;

    if (tid < RT_TILE) {
        const int row = row0 + tid;
        float dv = 0.f;
        if constexpr (GROUPED) {
            int64_t g = 0;                                // rows >= nq are dropped at the atomic, whatever they count
            if (row < nq) {
                dv = d[row];
                g = qgroup[row];
            }
            s_g[tid] = g;
        } else {
            int t = -1;
            if (row < nq) {
                dv = d[row];
                const int64_t t64 = target ? target[row] : (int64_t)row;
                t = t64 >= 0 && t64 < nk ? (int)t64 : -1;
            }
            s_t[tid] = t;
        }
        s_d[tid] = dv;
    }

    f32x16 acc[2][2];
    retr_product(acc, q, k, nq, nk, D, row0, col0, vec, s_a, s_b);

    // accumulator register r of lane l: column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of its 32 x 32 block.  A ballot gives
    // the 32 columns of that row in its low half (rows of l >> 5 == 0) and those of the row 4 below in its high half.  Lane L of
    // the wave ends up with the count of the wave's row L.
    const int half = lane >> 5;
    int col[2];
#pragma unroll
    for (int j = 0; j < 2; j++) col[j] = col0 + wn * 64 + j * 32 + (lane & 31);
    int64_t kg[2] = {0, 0};
    bool counts[2] = {false, false};                      // this lane's columns that exist and are counted
    if constexpr (GROUPED) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (col[j] < nk) {
                kg[j] = kgroup[col[j]];
                counts[j] = kcount ? kcount[col[j]] != 0 : true;
            }
        }
    }
    int mine = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int rl = i * 32 + (r & 3) + 8 * (r >> 2);      // wave-local row of the low half
            const float dv = s_d[wm * 64 + rl + 4 * half];
            int tg = 0;
            int64_t qg = 0;
            if constexpr (GROUPED) qg = s_g[wm * 64 + rl + 4 * half];
            else tg = s_t[wm * 64 + rl + 4 * half];
            int lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                bool beats;
                if constexpr (GROUPED) beats = counts[j] && kg[j] != qg && !(acc[i][j][r] < dv);
                else beats = col[j] < nk && col[j] != tg && !(acc[i][j][r] < dv);
                const unsigned long long m = __ballot(beats);
                lo += __popc((unsigned)m);
                hi += __popc((unsigned)(m >> 32));
            }
            if (lane == rl) mine = lo;
            if (lane == rl + 4) mine = hi;
        }
    }
    s_cnt[wn][wm * 64 + lane] = mine;
    __syncthreads();
    if (tid < RT_TILE) {
        const int c = s_cnt[0][tid] + s_cnt[1][tid];
        if (row0 + tid < nq && c) atomicAdd(&ranks[row0 + tid], c);
    }
}

}  // namespace

extern "C" int64_t mh_retrieval_workspace_bytes(int64_t nq, int64_t nk, int D) {
    (void)nk;
    (void)D;
    return nq > 0 ? nq * (int64_t)sizeof(float) : 0;     // the positives' similarities
}

extern "C" int mh_retrieval_ranks(const float* q, const float* k, int64_t nq, int64_t nk, int D, const int64_t* target, int32_t* ranks,
                                  void* workspace, mh_stream s) {
    MH_REQUIRE(q && k && ranks && workspace, "mh_retrieval_ranks: null pointer");
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20) && nk >= 1 && nk <= (1 << 20), "mh_retrieval_ranks: nq = %lld, nk = %lld outside [1, 2^20]",
               (long long)nq, (long long)nk);
    MH_REQUIRE(D >= 1 && D <= 4096, "mh_retrieval_ranks: D = %d outside [1, 4096]", D);
    MH_REQUIRE(target || nq == nk, "mh_retrieval_ranks: no target needs nq == nk (got %lld, %lld)", (long long)nq, (long long)nk);
    MH_REQUIRE(((uintptr_t)workspace & 3) == 0, "mh_retrieval_ranks: workspace must be 4-byte aligned");
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(k, 4);
    float* d = (float*)workspace;
    hipLaunchKernelGGL(retr_pos_kernel, dim3(mh_cdiv(nq, RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)s, q, k, (int)nq, (int)nk, D,
                       target, vec, d, ranks);
    MH_LAUNCH_CHECK("mh_retrieval_ranks");
    const int tiles_m = mh_cdiv(nq, RT_TILE), tiles_n = mh_cdiv(nk, RT_TILE);
    hipLaunchKernelGGL(retr_tile_kernel<false>, dim3((unsigned)tiles_m * (unsigned)tiles_n), dim3(RT_THREADS), 0, (hipStream_t)s, q, k,
                       (int)nq, (int)nk, D, target, (const int64_t*)nullptr, (const int64_t*)nullptr, (const uint8_t*)nullptr, vec, tiles_m,
                       tiles_n, (const float*)d, ranks);
    MH_LAUNCH_CHECK("mh_retrieval_ranks");
    return MH_OK;
}

extern "C" int mh_retrieval_ranks_grouped(const float* q, const float* k, int64_t nq, int64_t nk, int D, const int64_t* qgroup,
                                          const int64_t* kgroup, const int64_t* kgroup_sorted, const int64_t* kperm,
                                          const uint8_t* kcount, int32_t* ranks, void* workspace, mh_stream s) {
    MH_REQUIRE(q && k && ranks && workspace, "mh_retrieval_ranks_grouped: null pointer");
    MH_REQUIRE(qgroup && kgroup && kgroup_sorted && kperm, "mh_retrieval_ranks_grouped: null group ids");
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20) && nk >= 1 && nk <= (1 << 20),
               "mh_retrieval_ranks_grouped: nq = %lld, nk = %lld outside [1, 2^20]", (long long)nq, (long long)nk);
    MH_REQUIRE(D >= 1 && D <= 4096, "mh_retrieval_ranks_grouped: D = %d outside [1, 4096]", D);
    MH_REQUIRE(((uintptr_t)workspace & 3) == 0, "mh_retrieval_ranks_grouped: workspace must be 4-byte aligned");
    MH_REQUIRE((((uintptr_t)qgroup | (uintptr_t)kgroup | (uintptr_t)kgroup_sorted | (uintptr_t)kperm) & 7) == 0,
               "mh_retrieval_ranks_grouped: group ids must be 8-byte aligned");
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(k, 4);
    float* d = (float*)workspace;
    hipLaunchKernelGGL(retr_gpos_kernel, dim3(mh_cdiv(nq, RT_THREADS / 64)), dim3(RT_THREADS), 0, (hipStream_t)s, q, k, (int)nq, (int)nk,
                       D, qgroup, kgroup_sorted, kperm, vec, d, ranks);
    MH_LAUNCH_CHECK("mh_retrieval_ranks_grouped");
    const int tiles_m = mh_cdiv(nq, RT_TILE), tiles_n = mh_cdiv(nk, RT_TILE);
    hipLaunchKernelGGL(retr_tile_kernel<true>, dim3((unsigned)tiles_m * (unsigned)tiles_n), dim3(RT_THREADS), 0, (hipStream_t)s, q, k,
                       (int)nq, (int)nk, D, (const int64_t*)nullptr, qgroup, kgroup, kcount, vec, tiles_m, tiles_n, (const float*)d, ranks);
    MH_LAUNCH_CHECK("mh_retrieval_ranks_grouped");
    return MH_OK;
}
