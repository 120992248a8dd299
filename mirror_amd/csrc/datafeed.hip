// On-device batch draw (include/mirror_hip.h "data feed draws"): the token draw of datasets/dataset_pretrain.py:157-161,
// dataset_subtyping.py:187-200 and dataset_survival.py:293-314 for a whole batch in one launch, and the slide-id draw of
// utils/loader.py:15-26 (WeightedRandomSampler over class-balanced weights) in one launch.
//
// The stream.  Philox4x32-10 under key = (lo32(seed), hi32(seed)), like the dropout and noise streams; those have c2 = c3 = 0, the
// draws set bit 31 of c3, so a draw never shares a block with them under the same seed:
//     counter = (lo32(blk), kind, lo32(draw), 0x80000000 | hi32(draw))        kind = 0 token draws, 1 slide-id draws; draw < 2^63
// Element e of a draw is word e & 3 of block blk = e >> 2.
#include "common.h"

#define DF_THREADS 1024
#define DF_MAXKEYS 16384                 // 8-byte keys in LDS: 128 KiB of the CU's 160
#define DF_MAXN 8192
#define DF_LDS_BYTES (16 + DF_MAXKEYS * 8)
#define DF_MAXTRIES 40                   // the threshold search halves an interval of 2^32: 33 steps end it

__device__ __forceinline__ void draw_block(uint32_t (&w)[4], uint32_t blk, uint32_t kind, uint64_t draw, uint64_t seed) {
    w[0] = blk; w[1] = kind; w[2] = (uint32_t)draw; w[3] = 0x80000000u | (uint32_t)(draw >> 32);
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Stages j = min(k / 2, 64) .. 1 of the phases k = k_first .. k_last of the bitonic network, on the 128 consecutive keys [c0, c0 + 128):
// they pair keys inside the chunk only, so one wave holds the chunk two keys per lane (elements c0 + lane and c0 + 64 + lane) and
// exchanges through lane shuffles — no LDS traffic and no workgroup barrier between these stages.
__device__ __forceinline__ void sort_chunk(unsigned long long* keys, int c0, int lane, int k_first, int k_last) {
    unsigned long long x0 = keys[c0 + lane], x1 = keys[c0 + 64 + lane];
    const int e0 = c0 + lane, e1 = e0 + 64;
    for (int k = k_first; k <= k_last; k <<= 1) {
        int j = k >> 1;
        if (j >= 64) {
            j = 32;
            if ((x0 > x1) == ((e0 & k) == 0)) { const unsigned long long t = x0; x0 = x1; x1 = t; }
        }
        for (; j > 0; j >>= 1) {
            const unsigned long long p0 = __shfl_xor(x0, j, 64), p1 = __shfl_xor(x1, j, 64);
            const bool lower = (lane & j) == 0;               // this lane holds the pair's lower element
            const bool min0 = lower == ((e0 & k) == 0), min1 = lower == ((e1 & k) == 0);
            x0 = (p0 < x0) == min0 ? p0 : x0;
            x1 = (p1 < x1) == min1 ? p1 : x1;
        }
    }
    keys[c0 + lane] = x0;
    keys[c0 + 64 + lane] = x1;
}

// bitonic network over keys[0, P) (P a power of two >= 128), ascending; every thread of the workgroup takes part.  Stages with
// j >= 128 go through LDS behind a barrier each; the rest of a phase runs in sort_chunk (P = 8192: 28 barriers instead of 91).
__device__ __forceinline__ void sort_keys(unsigned long long* keys, int P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = wave * 128; c0 < P; c0 += (DF_THREADS / 64) * 128) sort_chunk(keys, c0, lane, 2, 128);
    __syncthreads();
    for (int k = 256; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 128; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += DF_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], c = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > c) == up) { keys[lo] = c; keys[hi] = a; }
            }
            __syncthreads();
        }
        for (int c0 = wave * 128; c0 < P; c0 += (DF_THREADS / 64) * 128) sort_chunk(keys, c0, lane, k, k);
        __syncthreads();
    }
}

// One workgroup per batch slot.  Every branch below is uniform over the workgroup (it depends on the slot's n and on LDS words read
// behind a barrier), so the barriers inside are reached by all threads.
__global__ __launch_bounds__(DF_THREADS) void sample_rows_kernel(const long* __restrict__ slot_slide, const long* __restrict__ length,
                                                                 const long* __restrict__ start, long* __restrict__ rows, int N, long S,
                                                                 uint64_t seed, uint64_t offset, const uint64_t* __restrict__ dev_base,
                                                                 float slack) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long df_lds[];
    unsigned* cnt = reinterpret_cast<unsigned*>(df_lds);        // candidate counter of the threshold path (16 bytes reserved)
    unsigned long long* keys = df_lds + 2;
    const int b = blockIdx.x, tid = threadIdx.x;
    long* out = rows + (long)b * N;
    const long sl = slot_slide[b];
    if (sl < 0 || sl >= S) {                                    // no such slide: -1 in every row (mh_gather_rows clamps to the bank)
        for (int i = tid; i < N; i += DF_THREADS) out[i] = -1;
        return;
    }
    const long n64 = length[sl], st = start[sl];
    if (n64 <= 0 || n64 >= (1l << 31)) {                        // empty slide, or too long for a 31-bit index: start[sl] repeated
        for (int i = tid; i < N; i += DF_THREADS) out[i] = st;
        return;
    }
    const uint32_t n = (uint32_t)n64;
    const uint64_t draw = offset + (dev_base ? *dev_base : 0ull) + (uint64_t)b;

    if (n < (uint32_t)N) {                                      // with replacement: multiply-shift of one word per row
        for (int q = tid; q * 4 < N; q += DF_THREADS) {
            uint32_t w[4];
            draw_block(w, (uint32_t)q, 0u, draw, seed);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (q * 4 + e < N) out[q * 4 + e] = st + (long)(((uint64_t)w[e] * n) >> 32);
        }
        return;
    }

    const uint32_t nblk = (n + 3) >> 2;
    // The threshold pass below sorts about `want` candidates.  A slide whose n keys fit a sort of that size (a power of two >= 128)
    // skips the pass and sorts all of them; a longer one (every slide above DF_MAXKEYS rows among them) takes the pass.
    const double want = (double)N + (double)slack * sqrt((double)N);
    int P = 128, Pw = 128;
    while ((double)Pw < want && Pw < DF_MAXKEYS) Pw <<= 1;
    while ((uint32_t)P < n && P < DF_MAXKEYS) P <<= 1;
    if (n <= DF_MAXKEYS && P <= Pw) {                           // every key into LDS
        for (uint32_t q = tid; q * 4 < (uint32_t)P; q += DF_THREADS) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (q < nblk) draw_block(w, q, 0u, draw, seed);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t j = q * 4 + e;
                if (j < (uint32_t)P) keys[j] = j < n ? ((unsigned long long)w[e] << 32) | j : ~0ull;
            }
        }
        __syncthreads();
    } else {
        // keep the keys whose word lies below a threshold T: any T that lets between N and DF_MAXKEYS keys through gives the
        // definition's result, since the N smallest keys are among them.  First T: an expected N + slack sqrt(N) candidates.
        // Too few -> T grows by a quarter, too many -> the middle of the interval [lo, hi] known to hold a good T.
        const int lane = tid & 63;
        const uint32_t iters = (nblk + DF_THREADS - 1) / DF_THREADS;
        uint64_t lo = 0, hi = 1ull << 32;                       // count(lo) < N, count(hi) > DF_MAXKEYS
        uint64_t T = (uint64_t)fmin(want * 4294967296.0 / (double)n, 4294967295.0);
        T = T < 1 ? 1 : (T > hi - 1 ? hi - 1 : T);
        unsigned c = 0;
        for (int tries = 0; tries < DF_MAXTRIES; tries++) {
            if (tid == 0) *cnt = 0u;
            __syncthreads();
            for (uint32_t it = 0; it < iters; it++) {
                const uint32_t q = it * DF_THREADS + tid;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (q < nblk) draw_block(w, q, 0u, draw, seed);
                bool pass[4];
                unsigned long long m[4];
                unsigned total = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    pass[e] = q * 4 + e < n && (uint64_t)w[e] < T;
                    m[e] = __ballot(pass[e]);
                    total += __popcll(m[e]);
                }
                if (total == 0) continue;                       // wave-uniform
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(cnt, total);    // LDS counter: the order of the candidates is free, the sort fixes it
                base = __shfl(base, 0, 64);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const unsigned pos = base + __popcll(m[e] & ((1ull << lane) - 1ull));
                    if (pass[e] && pos < DF_MAXKEYS) keys[pos] = ((unsigned long long)w[e] << 32) | (q * 4 + e);
                    base += __popcll(m[e]);
                }
            }
            __syncthreads();
            c = *cnt;
            if (c >= (unsigned)N && c <= DF_MAXKEYS) break;
            if (c < (unsigned)N) {
                lo = T;
                const uint64_t mid = lo + (hi - lo + 1) / 2, grown = T + (T >> 2) + 1;
                T = grown < mid ? grown : mid;
            } else {
                hi = T;
                T = lo + (hi - lo) / 2;
            }
            if (hi - lo < 2) break;                             // more than DF_MAXKEYS - N equal words: not a Philox output
            __syncthreads();                                    // everyone has read *cnt before it is cleared
        }
        if (c > DF_MAXKEYS) c = DF_MAXKEYS;
        for (P = 128; (unsigned)P < c; P <<= 1) {}
        for (int j = c + tid; j < P; j += DF_THREADS) keys[j] = ~0ull;
        __syncthreads();
    }
    sort_keys(keys, P);
    for (int i = tid; i < N; i += DF_THREADS) {
        const unsigned long long k = keys[i];
        out[i] = k == ~0ull ? st : st + (long)(k & 0xffffffffull);         // padding only after a failed search (see above)
    }
}

extern "C" int mh_sample_rows(const int64_t* slot_slide, const int64_t* length, const int64_t* start, int64_t* rows, int B, int N, int64_t S,
                              uint64_t seed, uint64_t offset, const uint64_t* dev_base, float slack, mh_stream s) {
    MH_REQUIRE(B >= 0, "mh_sample_rows: B=%d", B);
    MH_REQUIRE(N >= 0 && N <= DF_MAXN, "mh_sample_rows: N=%d unsupported (max %d)", N, DF_MAXN);
    MH_REQUIRE(S >= 0 && slack >= 0.f && slack <= 1e6f, "mh_sample_rows: S=%ld slack=%g", (long)S, (double)slack);
    MH_REQUIRE(offset + (uint64_t)B < (1ull << 63) && offset < (1ull << 63), "mh_sample_rows: draw ids must stay below 2^63");
    if (B == 0 || N == 0) return MH_OK;
    MH_REQUIRE(slot_slide && length && start && rows, "mh_sample_rows: null table");
    static const bool big = [] {       // above 64 KB of dynamic LDS the kernel needs the opt-in, once per process
        return hipFuncSetAttribute(reinterpret_cast<const void*>(sample_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DF_LDS_BYTES) == hipSuccess;
    }();
    MH_REQUIRE(big, "mh_sample_rows: %d bytes of LDS refused", DF_LDS_BYTES);
    hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(DF_THREADS), (size_t)DF_LDS_BYTES, (hipStream_t)s, (const long*)slot_slide,
                       (const long*)length, (const long*)start, (long*)rows, N, (long)S, seed, offset, dev_base, slack);
    MH_LAUNCH_CHECK("mh_sample_rows");
    return MH_OK;
}

// out[i] = #{k : cdf[k] <= u_i} clamped to S - 1, u_i = 53 bits of elements 2 i and 2 i + 1.  One thread per Philox block = two outputs.
__global__ __launch_bounds__(256) void sample_weighted_kernel(const double* __restrict__ cdf, long S, long* __restrict__ out, long count,
                                                              uint64_t seed, uint64_t offset, const uint64_t* __restrict__ dev_base) {
    const uint64_t draw = offset + (dev_base ? *dev_base : 0ull);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 2 < count; q += (long)gridDim.x * 256) {
        uint32_t w[4];
        draw_block(w, (uint32_t)q, 1u, draw, seed);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (q * 2 + h >= count) break;
            const uint64_t bits = ((uint64_t)(w[2 * h] >> 5) << 26) | (uint64_t)(w[2 * h + 1] >> 6);
            const double u = (double)bits * 1.1102230246251565e-16;          // 2^-53: exact, u in [0, 1)
            long lo = 0, hi = S;                                             // first k with cdf[k] > u
            while (lo < hi) {
                const long mid = lo + ((hi - lo) >> 1);
                if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
            }
            out[q * 2 + h] = lo < S ? lo : S - 1;
        }
    }
}

extern "C" int mh_sample_weighted(const double* cdf, int64_t S, int64_t* out, int64_t count, uint64_t seed, uint64_t offset,
                                  const uint64_t* dev_base, mh_stream s) {
    MH_REQUIRE(S >= 1 && count >= 0 && count <= (1ll << 32), "mh_sample_weighted: S=%ld count=%ld", (long)S, (long)count);
    MH_REQUIRE(offset < (1ull << 63), "mh_sample_weighted: draw ids must stay below 2^63");
    if (count == 0) return MH_OK;
    MH_REQUIRE(cdf && out, "mh_sample_weighted: null table");
    hipLaunchKernelGGL(sample_weighted_kernel, dim3((unsigned)min((long)mh_cdiv(mh_cdiv(count, 2), 256), 2048L)), dim3(256), 0, (hipStream_t)s,
                       cdf, (long)S, (long*)out, (long)count, seed, offset, dev_base);
    MH_LAUNCH_CHECK("mh_sample_weighted");
    return MH_OK;
}
