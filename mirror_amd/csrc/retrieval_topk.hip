// Top-k retrieval (mh_retrieval_topk) and the kNN vote on its result (mh_knn_scores): for every query the kk eligible keys with the largest
// q_i . k_j, WITHOUT the nq x nk similarity matrix.  The product is retrieval.hip's (retrieval_tile.h: every similarity is the k-ordered
// f32 fmaf chain from 0), the epilogue selects where that one counts.
//
// A candidate is ONE 64-bit word: the similarity's bits made monotone (sign flipped for positives, all bits for negatives) in the high
// half, the complement of the key index in the low half.  Larger word = larger similarity, then smaller index: the total order of the
// header is an unsigned compare, and no two candidates of a query are equal.  0 is the empty slot (its high half would be a negative
// NaN's, and a NaN is never a candidate).
//
// Two launches on the caller's stream, nothing allocated, nothing waits on the host (graph capturable):
//   1. topk_tile_kernel: a workgroup owns 128 query rows and one of `parts` strips of the key tiles and walks the strip.  Each row's
//      running list (kk words, descending) lives in LDS.  After a tile's product every lane compares its 64 accumulators with its
//      rows' current kk-th word (two LDS addresses per wave and read: a broadcast) and keeps a bit per survivor.  A row whose list is not
//      full yet (a strip's first tile) has no kk-th word and would pass every key on: there each wave first finds, with ballots from the
//      top bit down, the 14-bit bucket of the kk-th largest of its own 64 keys of that row and drops what lies below it.  Rows are then served in
//      four passes of 32: a pass that has a survivor dumps the monotone bits of its survivors into a 32 x 128 word buffer (the slot is the
//      column, so nothing is appended and no atomic is needed), and each wave merges 8 rows: a row without a survivor costs one read and a
//      ballot; otherwise every survivor is broadcast once (v_readlane) and list entries and survivors count the words above them, which
//      is their new slot.  A pass without survivors is skipped by all four waves.  The strip's lists go to the workspace [nq, parts, kk].
//   2. topk_merge_kernel: one wave per query selects the kk largest of its parts x kk words, one per round, and decodes them.
// Deterministic: no atomics at all; the selected set and its order depend on the words only, not on the tiling or on `parts`.
//
// mh_knn_scores: one wave per query; lane s forms slot s's weight, lane 0 adds them in slot order into the wave's class row in LDS.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int TK_MAXK = 64;           // one list entry per lane in the merge
constexpr int TK_SEL = 14;            // bits of the monotone similarity the first-tile filter resolves: sign, exponent, 5 of the mantissa
constexpr int TK_PASS = 32;           // rows per pass of the epilogue (one accumulator block's rows)
constexpr int TK_MAXPARTS = 128;      // strips the library chooses at most (a caller may give more)

__device__ __forceinline__ uint32_t topk_mono(float v) {
    uint32_t u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;                        // -0 orders as +0 (the chain from +0 never forms it)
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float topk_unmono(uint32_t m) { return __uint_as_float(m ^ ((m >> 31) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ uint64_t topk_word(uint32_t mono, int col) { return ((uint64_t)mono << 32) | (uint32_t)~(uint32_t)col; }

__device__ __forceinline__ uint64_t topk_bcast(uint64_t v, int src) {     // src wave-uniform
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// Merge row `list` (kk words, descending, 0 = empty) with the survivors among the 128 words of `cand` (monotone bits, 0 = none; slot c is
// key col0 + c); *thr is kept equal to list[kk - 1].  One wave, all lanes.
__device__ __forceinline__ void topk_merge_row(uint64_t* __restrict__ list, uint64_t* __restrict__ thr, const uint32_t* __restrict__ cand, int kk,
                                               int col0, int lane) {
    const uint32_t h0 = cand[lane], h1 = cand[lane + 64];
    const unsigned long long m0 = __ballot(h0 != 0), m1 = __ballot(h1 != 0);
    if ((m0 | m1) == 0) return;
    const uint64_t c0 = h0 ? topk_word(h0, col0 + lane) : 0, c1 = h1 ? topk_word(h1, col0 + lane + 64) : 0;
    const uint64_t e = lane < kk ? list[lane] : 0;
    int re = lane, r0 = 0, r1 = 0;                        // words above: the list entry starts with those of the list
#pragma unroll
    for (int half = 0; half < 2; half++) {
        unsigned long long m = half ? m1 : m0;
        while (m) {
            const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            m &= m - 1;
            const uint64_t x = topk_bcast(half ? c1 : c0, b);
            const int above = __popcll(__ballot(e > x));  // list entries above this survivor
            re += x > e;
            r0 += x > c0;
            r1 += x > c1;
            if (lane == b) {
                if (half) r1 += above;
                else r0 += above;
            }
        }
    }
    if (e != 0 && re < kk) list[re] = e;                  // every lane read its entry before any of these stores
    if (c0 != 0 && r0 < kk) list[r0] = c0;
    if (c1 != 0 && r1 < kk) list[r1] = c1;
    if (e != 0 && re == kk - 1) *thr = e;                 // the row's new kk-th word, if it has kk by now
    if (c0 != 0 && r0 == kk - 1) *thr = c0;
    if (c1 != 0 && r1 == kk - 1) *thr = c1;
}

template <bool GROUPED>
__global__ void __launch_bounds__(RT_THREADS, 3) topk_tile_kernel(const float* __restrict__ q, const float* __restrict__ k, int nq, int nk,
                                                               int D, int kk, const int64_t* __restrict__ qgroup,
                                                               const int64_t* __restrict__ kgroup, int vec, int tiles_n, int parts,
                                                               uint64_t* __restrict__ partial) {
    __shared__ float s_a[2][RT_TILE * RT_LD];
    __shared__ float s_b[2][RT_TILE * RT_LD];
    __shared__ int64_t s_g[GROUPED ? RT_TILE : 1];
    __shared__ int s_flag[2][4];
    __shared__ uint64_t s_thr[RT_TILE];                   // every row's kk-th word (0: fewer than kk so far), at an address that does not depend on kk
    extern __shared__ uint64_t s_list[];                  // [128][kk]
    // the survivors' buffer lies over the q stages: those are idle between a product's last barrier and the next product
    static_assert(TK_PASS * RT_TILE <= 2 * RT_TILE * RT_LD, "the survivors' buffer must fit the q stages");
    uint32_t* s_cand = reinterpret_cast<uint32_t*>(&s_a[0][0]);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int part = blockIdx.x % parts, tile_m = blockIdx.x / parts;
    const int row0 = tile_m * RT_TILE;
    const int t_begin = (int)((int64_t)part * tiles_n / parts), t_end = (int)((int64_t)(part + 1) * tiles_n / parts);

    for (int e = tid; e < RT_TILE * kk; e += RT_THREADS) s_list[e] = 0;
    if (tid < 8) s_flag[tid >> 2][tid & 3] = 0;
    if (tid < RT_TILE) s_thr[tid] = 0;
    if constexpr (GROUPED) {
        if (tid < RT_TILE) s_g[tid] = row0 + tid < nq ? qgroup[row0 + tid] : 0;
    }
    // the first barrier inside retr_product orders these stores before the first epilogue

    for (int t = t_begin; t < t_end; t++) {
        const int col0 = t * RT_TILE, par = (t - t_begin) & 1;
        f32x16 acc[2][2];
        retr_product(acc, q, k, nq, nk, D, row0, col0, vec, s_a, s_b);

        int col[2];
        bool ok[2];                                       // this lane's columns that exist
        int64_t kg[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 2; j++) {
            col[j] = col0 + wn * 64 + j * 32 + (lane & 31);
            ok[j] = col[j] < nk;
            if constexpr (GROUPED) {
                if (ok[j]) kg[j] = kgroup[col[j]];
            }
        }
        // bit 2 r + j of surv[i]: accumulator (i, j, r) is eligible and above its row's kk-th word
        uint32_t surv[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const uint64_t thr = s_thr[rl];
                int64_t qg = 0;
                if constexpr (GROUPED) qg = s_g[rl];
                uint32_t mono[2];                         // 0: not eligible
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float v = acc[i][j][r];
                    bool in = ok[j] && v == v;            // rows >= nq (zero-filled) keep lists too: they are never written out
                    if constexpr (GROUPED) in = in && kg[j] != qg;
                    mono[j] = in ? topk_mono(v) : 0u;
                }
                // A row whose list is not full yet (a strip's first tile) would pass all 128 keys on to the merge.  Its keys in this wave
                // (32 lanes x 2, the row of the other half-wave in the other half of each ballot) below the bucket of their own kk-th
                // largest cannot be among the kk best of anything that contains them: find that bucket from the top TK_SEL bits down.
                uint32_t floor_ = 0;
                if (__ballot(thr == 0) != 0) {
#pragma unroll 1
                    for (int b = 31; b >= 32 - TK_SEL; b--) {
                        const uint32_t trial = floor_ | (1u << b);
                        const unsigned long long b0 = __ballot(mono[0] >= trial), b1 = __ballot(mono[1] >= trial);
                        const int lo = __popc((uint32_t)b0) + __popc((uint32_t)b1), hi = __popc((uint32_t)(b0 >> 32)) + __popc((uint32_t)(b1 >> 32));
                        if ((half ? hi : lo) >= kk) floor_ = trial;
                    }
                    floor_ = thr == 0 ? floor_ : 0u;
                }
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (mono[j] != 0 && mono[j] >= floor_ && topk_word(mono[j], col[j]) > thr) surv[i] |= 1u << (2 * r + j);
            }
            if (__ballot(surv[i] != 0) != 0 && lane == 0) s_flag[par][wm * 2 + i] = 1;
        }
        if (tid < 4) s_flag[par ^ 1][tid] = 0;            // last read in the epilogue of the tile before: barriers of this product lie between
        __syncthreads();

#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (s_flag[par][p] == 0) continue;            // the same for all threads
            if (wm == (p >> 1)) {
                const int i = p & 1;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int r32 = (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const bool s = (surv[i] >> (2 * r + j)) & 1u;
                        s_cand[r32 * RT_TILE + wn * 64 + j * 32 + (lane & 31)] = s ? topk_mono(acc[i][j][r]) : 0u;
                    }
                }
            }
            __syncthreads();
#pragma unroll 1
            for (int u = 0; u < TK_PASS / 4; u++) {
                const int r32 = wave * (TK_PASS / 4) + u;
                topk_merge_row(s_list + (p * TK_PASS + r32) * kk, s_thr + p * TK_PASS + r32, s_cand + r32 * RT_TILE, kk, col0, lane);
            }
            __syncthreads();
        }
    }
    // the last pass, or the last product, ended with a barrier (t_end > t_begin: parts <= tiles_n)
    for (int e = tid; e < RT_TILE * kk; e += RT_THREADS) {
        const int row = row0 + e / kk, s = e % kk;
        if (row < nq) partial[((int64_t)row * parts + part) * kk + s] = s_list[e];
    }
}

// one wave per query: the kk largest of its n = parts kk words, largest first
__global__ void __launch_bounds__(RT_THREADS) topk_merge_kernel(const uint64_t* __restrict__ partial, int nq, int n, int kk,
                                                                int32_t* __restrict__ idx, float* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= nq) return;                                  // wave-uniform
    const uint64_t* w = partial + (int64_t)i * n;
    uint64_t prev = ~0ull;                                // above every word: an all-ones high half would be a NaN's
    for (int s = 0; s < kk; s++) {
        uint64_t best = 0;
        if (prev != 0) {
            for (int e = lane; e < n; e += 64) {
                const uint64_t x = w[e];
                if (x < prev && x > best) best = x;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)best, o), hi = __shfl_xor((uint32_t)(best >> 32), o);
                const uint64_t x = ((uint64_t)hi << 32) | lo;
                best = x > best ? x : best;
            }
        }
        prev = best;
        if (lane == 0) {
            idx[(int64_t)i * kk + s] = best ? (int32_t)~(uint32_t)best : -1;
            val[(int64_t)i * kk + s] = best ? topk_unmono((uint32_t)(best >> 32)) : -INFINITY;
        }
    }
}

constexpr int KNN_MAXC = 1024;

__global__ void __launch_bounds__(RT_THREADS) knn_scores_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                                const int64_t* __restrict__ labels, int nq, int nk, int kk, int C,
                                                                float inv_t, float* __restrict__ scores) {
    extern __shared__ float s_acc[];                      // [4][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * (RT_THREADS / 64) + wave;
    if (i >= nq) return;                                  // wave-uniform, no block barrier below
    float* acc = s_acc + wave * C;
    for (int c = lane; c < C; c += 64) acc[c] = 0.f;
    __builtin_amdgcn_wave_barrier();
    // slot `lane`: its class (-1: contributes nothing) and weight
    int cls = -1;
    float wgt = 0.f;
    const float v0 = val[(int64_t)i * kk];
    if (lane < kk) {
        const int j = idx[(int64_t)i * kk + lane];
        if (j >= 0 && j < nk) {
            const int64_t l = labels[j];
            if (l >= 0 && l < C) {
                const float v = val[(int64_t)i * kk + lane];
                cls = (int)l;
                wgt = expf((v == v0 ? 0.f : v - v0) * inv_t);
            }
        }
    }
    float total = 0.f;
    for (int s = 0; s < kk; s++) {                        // slot order, one lane: a fixed order of additions
        const int c = __builtin_amdgcn_readlane(cls, s);
        const float x = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(wgt), s));
        if (c >= 0) {
            if (lane == 0) acc[c] += x;
            total += x;
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int c = lane; c < C; c += 64) scores[(int64_t)i * C + c] = total > 0.f ? acc[c] / total : 0.f;
}

int topk_cus() {
    static const int cus = [] {
        hipDeviceProp_t p;
        int d = 0;
        (void)hipGetDevice(&d);
        return hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    }();
    return cus;
}

// parts > 0: as given, up to the number of key tiles.  0: as many strips as the chip holds workgroups at once (3 per CU by registers, fewer
// where the lists' LDS, 1 KiB per neighbour on top of 36 KiB, allows fewer: a second round of workgroups would run beside idle CUs), but
// strips of at least 2 tiles where the bank allows it (a strip's first tile fills the lists).  Measured: DESIGN.md 6u.
int topk_parts(int64_t nq, int64_t nk, int kk, int parts) {
    const int tiles_m = mh_cdiv(nq, RT_TILE), tiles_n = mh_cdiv(nk, RT_TILE);
    if (parts <= 0) {
        const int per_cu = kk <= 17 ? 3 : (kk <= 44 ? 2 : 1);
        parts = per_cu * topk_cus() / tiles_m;
        const int by_len = tiles_n / 2;
        parts = parts < by_len ? parts : by_len;
        parts = parts < TK_MAXPARTS ? parts : TK_MAXPARTS;
        parts = parts > 1 ? parts : 1;
    }
    return parts < tiles_n ? parts : tiles_n;
}

}  // namespace

extern "C" int64_t mh_retrieval_topk_workspace_bytes(int64_t nq, int64_t nk, int D, int kk, int parts) {
    (void)D;
    if (nq <= 0 || nk <= 0 || kk <= 0) return 0;
    return nq * topk_parts(nq, nk, kk, parts) * (int64_t)kk * (int64_t)sizeof(uint64_t);
}

extern "C" int mh_retrieval_topk(const float* q, const float* k, int64_t nq, int64_t nk, int D, int kk, const int64_t* qgroup,
                                 const int64_t* kgroup, int parts, int32_t* idx, float* val, void* workspace, mh_stream s) {
    MH_REQUIRE(q && k && idx && val && workspace, "mh_retrieval_topk: null pointer");
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20) && nk >= 1 && nk <= (1 << 20), "mh_retrieval_topk: nq = %lld, nk = %lld outside [1, 2^20]",
               (long long)nq, (long long)nk);
    MH_REQUIRE(D >= 1 && D <= 4096, "mh_retrieval_topk: D = %d outside [1, 4096]", D);
    MH_REQUIRE(kk >= 1 && kk <= TK_MAXK, "mh_retrieval_topk: kk = %d outside [1, %d]", kk, TK_MAXK);
    MH_REQUIRE(parts >= 0, "mh_retrieval_topk: parts = %d is negative", parts);
    MH_REQUIRE((qgroup != nullptr) == (kgroup != nullptr), "mh_retrieval_topk: qgroup and kgroup go together");
    MH_REQUIRE((((uintptr_t)qgroup | (uintptr_t)kgroup | (uintptr_t)workspace) & 7) == 0,
               "mh_retrieval_topk: group ids and workspace must be 8-byte aligned");
    static const bool lds_ok = [] {
        const int cap = RT_TILE * TK_MAXK * (int)sizeof(uint64_t);
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_tile_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, cap) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_tile_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, cap) == hipSuccess;
    }();
    MH_REQUIRE(lds_ok, "mh_retrieval_topk: the device refused %d bytes of dynamic LDS", RT_TILE * TK_MAXK * (int)sizeof(uint64_t));
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(k, 4);
    const int tiles_m = mh_cdiv(nq, RT_TILE), tiles_n = mh_cdiv(nk, RT_TILE);
    const int np = topk_parts(nq, nk, kk, parts);
    uint64_t* partial = (uint64_t*)workspace;
    const size_t lds = (size_t)RT_TILE * kk * sizeof(uint64_t);
    if (qgroup) {
        hipLaunchKernelGGL(topk_tile_kernel<true>, dim3((unsigned)tiles_m * (unsigned)np), dim3(RT_THREADS), lds, (hipStream_t)s, q, k,
                           (int)nq, (int)nk, D, kk, qgroup, kgroup, vec, tiles_n, np, partial);
    } else {
        hipLaunchKernelGGL(topk_tile_kernel<false>, dim3((unsigned)tiles_m * (unsigned)np), dim3(RT_THREADS), lds, (hipStream_t)s, q, k,
                           (int)nq, (int)nk, D, kk, (const int64_t*)nullptr, (const int64_t*)nullptr, vec, tiles_n, np, partial);
    }
    MH_LAUNCH_CHECK("mh_retrieval_topk");
    hipLaunchKernelGGL(topk_merge_kernel, dim3(mh_cdiv(nq, RT_THREADS / 64)), dim3(RT_THREADS), 0, (hipStream_t)s,
                       (const uint64_t*)partial, (int)nq, np * kk, kk, idx, val);
    MH_LAUNCH_CHECK("mh_retrieval_topk");
    return MH_OK;
}

extern "C" int mh_knn_scores(const int32_t* idx, const float* val, const int64_t* labels, int64_t nq, int64_t nk, int kk, int C,
                             float inv_temperature, float* scores, mh_stream s) {
    MH_REQUIRE(idx && val && labels && scores, "mh_knn_scores: null pointer");
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20) && nk >= 1 && nk <= (1 << 20), "mh_knn_scores: nq = %lld, nk = %lld outside [1, 2^20]",
               (long long)nq, (long long)nk);
    MH_REQUIRE(kk >= 1 && kk <= TK_MAXK, "mh_knn_scores: kk = %d outside [1, %d]", kk, TK_MAXK);
    MH_REQUIRE(C >= 1 && C <= KNN_MAXC, "mh_knn_scores: C = %d outside [1, %d]", C, KNN_MAXC);
    MH_REQUIRE(inv_temperature >= 0.f && inv_temperature < INFINITY, "mh_knn_scores: inv_temperature = %g must be finite and >= 0",
               (double)inv_temperature);
    MH_REQUIRE(((uintptr_t)labels & 7) == 0, "mh_knn_scores: labels must be 8-byte aligned");
    hipLaunchKernelGGL(knn_scores_kernel, dim3(mh_cdiv(nq, RT_THREADS / 64)), dim3(RT_THREADS), (size_t)(RT_THREADS / 64) * C * sizeof(float),
                       (hipStream_t)s, idx, val, labels, (int)nq, (int)nk, kk, C, inv_temperature, scores);
    MH_LAUNCH_CHECK("mh_knn_scores");
    return MH_OK;
}
