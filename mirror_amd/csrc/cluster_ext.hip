// The cluster probe's seeding, silhouette and matched accuracy (mirror_amd/cluster.py; include/mirror_hip.h "cluster probe: seeding,
// silhouette, matched accuracy").  Like kmeans.hip: every entry point launches on the caller's stream, allocates nothing, never waits on
// the host and uses no float atomics; every sum has a fixed order, so two runs agree bit for bit.
//
//   mh_silhouette      the hot path.  Per label row five launches: (1) one workgroup counts the clusters and sorts the rows by cluster id,
//                      stable (a counting sort: LDS histogram, then one wave places 64 rows at a time by ballot ranks); (2) the rows of y
//                      are gathered into that order, with q = retr_chain(row, row); (3) kmeans_assign_kernel's loop over the SORTED rows:
//                      a workgroup owns 128 rows and walks its group of key tiles (one of P contiguous groups, so that a few
//                      thousand rows fill the chip) in ascending order through retrieval_tile.h's exact-f32 product;
//                      behind every product the tile goes through LDS 64 rows at a time and four threads per row scan 32 columns each,
//                      turning every product into an f64 distance and keeping a running f64 sum that is flushed where the cluster id
//                      changes (sorted: a cluster is a contiguous column range).  A run that touches an end of the thread's 32 columns
//                      may continue in a neighbour's: those (at most two per thread) go through LDS and one thread per row adds them in
//                      column order; a run strictly inside belongs to this thread alone and goes to S directly.  S f64 [P, n, K] lives in
//                      the workspace, each workgroup on its own 128 rows of its own slice; (4) a thread per row adds the P slices in
//                      group order, forms a, b and s and scatters it back; (5) one workgroup adds the samples over mh_colmean's strips.  The product is formed once per label row.
//   mh_kmeanspp_init   D^2 seeding (Arthur and Vassilvitskii) for R restarts at once: per centre one launch that folds the newest centre
//                      into m = min |y_i - c|^2 (f64 [R, n], a thread per row, a strip's rows added in row order as in
//                      mh_kmeans_inertia) and one that adds the strips, draws u from the data feed's Philox stream (kind 2), finds the
//                      strip and then the row whose running sum passes u T, and copies that row.
//   mh_cluster_match   one workgroup per restart: the maximum-weight assignment of clusters to classes on the integer contingency
//                      counts by shortest augmenting paths with int64 potentials (a serial outer loop, the minimum over the columns
//                      workgroup-parallel, ties to the smaller column).
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int CX_MAXK = 1024;         // clusters
constexpr int CX_MAXC = 1024;         // label classes of the matching
constexpr int CX_MAXCELLS = 65536;    // K C of the matching: the tally's limit
constexpr int CX_MAXD = 4096;
constexpr int CX_MAXR = 65535;
constexpr int CX_HALF = RT_TILE / 2;  // rows per pass of the silhouette epilogue
constexpr int CX_LD = RT_TILE + 1;    // LDS row stride of the spilled half tile
constexpr int CX_QUARTER = RT_TILE / 4;         // key columns per scanning thread
constexpr int CX_MAXPARTS = 128;      // row strips: mh_colmean's partition
constexpr int CX_MINSIDE = 256;       // min(K, C) when K C <= 65536
constexpr int CX_LDSCELLS = 4096;     // contingency cells kept in LDS by the matching

__device__ __forceinline__ double cx_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

int cx_parts(int64_t n) {             // mh_colmean's strips: at least 64 rows, 128 strips at the most
    const int64_t p = (n + 63) / 64;
    return (int)(p < 1 ? 1 : (p > CX_MAXPARTS ? CX_MAXPARTS : p));
}

int cx_geometry(const char* who, int64_t n, int R, int K, int D) {
    MH_REQUIRE(K >= 1 && K <= CX_MAXK, "%s: K = %d outside [1, %d]", who, K, CX_MAXK);
    MH_REQUIRE(D >= 1 && D <= CX_MAXD, "%s: D = %d outside [1, %d]", who, D, CX_MAXD);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %lld outside [1, 2^20]", who, (long long)n);
    MH_REQUIRE(R >= 1 && R <= CX_MAXR, "%s: R = %d outside [1, %d]", who, R, CX_MAXR);
    return MH_OK;
}

// ------------------------------------------------------------------ silhouette
struct SilWs {
    float* ys;          // [n, D] the rows in cluster order
    double* S;          // [P, n, K] sums of distances per group of key tiles, by sorted row
    double* sorig;      // [n] the samples in the caller's row order
    float* qn;          // [n] retr_chain(row, row), by sorted row
    int32_t* order;     // [n] sorted position -> caller's row
    int32_t* slab;      // [n] cluster id by sorted position (K: outside)
    int32_t* cnt;       // [K + 1] members; [K]: the rows outside
};

int64_t cx_up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// The key tiles of a row tile are cut into P contiguous groups, a workgroup each, so that a cohort of a few thousand rows still fills the
// chip: P ceil(n / 128) reaches 1024 workgroups where the tiles allow it, P <= 16, and the slices beyond the first stay within 64 MiB:
// (P - 1) n K 8 <= 2^26.  So S is [n, K] and at most 64 MiB more; P = 1 from n = 2^17 on, and wherever n K >= 2^23.
constexpr int CX_SPLIT_TARGET = 1024, CX_MAXSPLIT = 16;
constexpr int64_t CX_SPLIT_BYTES = (int64_t)1 << 26;
int sil_splits(int64_t n, int K) {
    const int64_t tiles = (n + RT_TILE - 1) / RT_TILE;
    int64_t P = (CX_SPLIT_TARGET + tiles - 1) / tiles;
    P = P > CX_MAXSPLIT ? CX_MAXSPLIT : P;
    P = P > tiles ? tiles : P;
    const int64_t extra = CX_SPLIT_BYTES / (n * K * 8);   // whole slices that fit the budget
    P = P > 1 + extra ? 1 + extra : P;
    return (int)(P < 1 ? 1 : P);
}

int64_t sil_layout(int64_t n, int K, int D, char* base, SilWs* w) {
    int64_t o = 0;
    const int64_t o_ys = o;    o += cx_up16(n * D * 4);
    const int64_t o_S = o;     o += cx_up16((int64_t)sil_splits(n, K) * n * K * 8);
    const int64_t o_so = o;    o += cx_up16(n * 8);
    const int64_t o_q = o;     o += cx_up16(n * 4);
    const int64_t o_ord = o;   o += cx_up16(n * 4);
    const int64_t o_lab = o;   o += cx_up16(n * 4);
    const int64_t o_cnt = o;   o += cx_up16((int64_t)(K + 1) * 4);
    if (w) {
        w->ys = (float*)(base + o_ys);
        w->S = (double*)(base + o_S);
        w->sorig = (double*)(base + o_so);
        w->qn = (float*)(base + o_q);
        w->order = (int32_t*)(base + o_ord);
        w->slab = (int32_t*)(base + o_lab);
        w->cnt = (int32_t*)(base + o_cnt);
    }
    return o;
}

// (1) the members of every cluster and the stable order by cluster id; rows outside [0, K) sort last and get their NaN here
__global__ void __launch_bounds__(RT_THREADS) sil_order_kernel(const int32_t* __restrict__ lab, int n, int K, int32_t* __restrict__ order,
                                                               int32_t* __restrict__ slab, int32_t* __restrict__ cnt,
                                                               double* __restrict__ sorig, double* __restrict__ sil,
                                                               int32_t* __restrict__ bad) {
    __shared__ int s_cnt[CX_MAXK + 1];
    __shared__ int s_pos[CX_MAXK + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k <= K; k += RT_THREADS) s_cnt[k] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += RT_THREADS) {
        const int l = lab[i];
        const int key = (l >= 0 && l < K) ? l : K;
        atomicAdd(&s_cnt[key], 1);
        if (key == K) {
            sorig[i] = cx_nan();
            if (sil) sil[i] = cx_nan();
        }
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k <= K; k++) {
            s_pos[k] = acc;
            acc += s_cnt[k];
        }
        *bad = s_cnt[K];
    }
    __syncthreads();
    for (int k = tid; k <= K; k += RT_THREADS) cnt[k] = s_cnt[k];
    if (tid >= 64) return;
    // one wave places 64 rows at a time: the lanes of one cluster id take consecutive places in lane (= row) order
    volatile int* vpos = s_pos;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        int key = -1;
        if (i < n) {
            const int l = lab[i];
            key = (l >= 0 && l < K) ? l : K;
        }
        const int first = key >= 0 ? vpos[key] : 0;
        unsigned long long todo = __ballot(key >= 0), mine = 0ull;
        while (todo) {                                    // wave-uniform: one step per distinct id among the 64 rows
            const int lead = __ffsll((long long)todo) - 1;
            const int kk = __shfl(key, lead, 64);
            const unsigned long long m = __ballot(key == kk);
            if (key == kk) mine = m;
            todo &= ~m;
        }
        if (key >= 0) {
            const int p = first + __popcll(mine & ((1ull << lane) - 1ull));
            order[p] = i;
            slab[p] = key;
            if ((mine >> lane) == 1ull) vpos[key] = first + __popcll(mine);      // the last lane of this id moves its place on
        }
    }
}

// (2) ys[p] = y[order[p]], q[p] = the product's own chain of that row with itself
__global__ void __launch_bounds__(64) sil_gather_kernel(const float* __restrict__ y, const int32_t* __restrict__ order, int D, int vec,
                                                        float* __restrict__ ys, float* __restrict__ qn) {
    const int p = blockIdx.x;
    const float* src = y + (int64_t)order[p] * D;
    float* dst = ys + (int64_t)p * D;
    for (int d = threadIdx.x; d < D; d += 64) dst[d] = src[d];
    if (threadIdx.x == 0) qn[p] = retr_chain(src, src, D, vec);
}

// (3) the all-pairs pass over the sorted rows
__global__ void __launch_bounds__(RT_THREADS, 2) sil_tile_kernel(const float* __restrict__ ys, const float* __restrict__ qn,
                                                                 const int32_t* __restrict__ slab, const int32_t* __restrict__ cnt,
                                                                 int n, int K, int D, int vec, int cosine, int P, double* S) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    static_assert(CX_HALF * CX_LD <= 4 * RT_TILE * RT_LD, "half a tile must fit the stages");
    __shared__ int s_cl[RT_TILE];                         // cluster id and q of the tile's columns
    __shared__ float s_q[RT_TILE];
    __shared__ int s_pk[CX_HALF * 8];                     // per (row of the half tile, quarter): the head and the tail run
    __shared__ double s_pv[CX_HALF * 8];
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int nv = n - cnt[K];                            // the rows that take part: sorted positions [0, nv)
    const int row0 = blockIdx.x * RT_TILE;
    if (row0 >= nv) return;                               // the whole workgroup
    const int rl = tid & (CX_HALF - 1), quarter = tid >> 6;
    const int mine = nv - row0 < RT_TILE ? nv - row0 : RT_TILE;
    const int tiles = (nv + RT_TILE - 1) / RT_TILE, part = blockIdx.y;    // this workgroup's key tiles: group `part` of P
    const int col_lo = (int)((int64_t)part * tiles / P) * RT_TILE, col_hi = (int)((int64_t)(part + 1) * tiles / P) * RT_TILE;
    S += (int64_t)part * n * K;                           // and its own slice of S
    for (int64_t j = tid; j < (int64_t)mine * K; j += RT_THREADS) S[(int64_t)row0 * K + j] = 0.0;
    __syncthreads();

    int gi[2];
    double qi[2];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        gi[pass] = row0 + pass * CX_HALF + rl;
        qi[pass] = gi[pass] < nv ? (double)qn[gi[pass]] : 0.0;
    }
    for (int col0 = col_lo; col0 < col_hi; col0 += RT_TILE) {
        f32x16 acc[2][2];
        retr_product(acc, ys, ys, nv, nv, D, row0, col0, vec, s_a, s_b);  // ends with a barrier behind the last read of the stages
        if (tid < RT_TILE) {
            const bool in = col0 + tid < nv;
            s_cl[tid] = in ? slab[col0 + tid] : -1;
            s_q[tid] = in ? qn[col0 + tid] : 0.f;
        }
        const int k0 = col0 + quarter * CX_QUARTER;
        const int kn = nv - k0 < CX_QUARTER ? nv - k0 : CX_QUARTER;       // columns >= nv are never looked at (kn <= 0: none)
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            if (wm == pass) {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++)
#pragma unroll
                        for (int q = 0; q < 16; q++)
                            s_t[(i * 32 + (q & 3) + 8 * (q >> 2) + 4 * half) * CX_LD + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][q];
            }
            __syncthreads();
            int hk = -1, tk = -1;
            double hv = 0.0, tv = 0.0;
            const int g = gi[pass];
            if (g < nv && kn > 0) {
                const float* sc = s_t + rl * CX_LD + quarter * CX_QUARTER;
                const int* cl = s_cl + quarter * CX_QUARTER;
                const float* cq = s_q + quarter * CX_QUARTER;
                double* Sg = S + (int64_t)g * K;
                int cur = cl[0];
                double run = 0.0;
                bool first = true;
                for (int c = 0; c < kn; c++) {            // ascending columns
                    const int lj = cl[c];
                    if (lj != cur) {
                        if (first) {
                            hk = cur;
                            hv = run;
                            first = false;
                        } else {
                            Sg[cur] += run;               // a run strictly inside these 32 columns: no other thread has this cluster
                        }
                        cur = lj;
                        run = 0.0;
                    }
                    if (k0 + c != g) {                    // the pair i = j is left out by index
                        const double s = (double)sc[c];
                        double d;
                        if (cosine) {
                            d = 1.0 - s;
                        } else {
                            const double t = fma(-2.0, s, qi[pass] + (double)cq[c]);
                            d = sqrt(t < 0.0 ? 0.0 : t);  // a NaN stays a NaN
                        }
                        run += d;
                    }
                }
                if (first) {
                    hk = cur;
                    hv = run;
                } else {
                    tk = cur;
                    tv = run;
                }
            }
            s_pk[(rl * 4 + quarter) * 2] = hk;
            s_pv[(rl * 4 + quarter) * 2] = hv;
            s_pk[(rl * 4 + quarter) * 2 + 1] = tk;
            s_pv[(rl * 4 + quarter) * 2 + 1] = tv;
            __syncthreads();
            if (tid < CX_HALF && g < nv) {                // tid = rl: this row's eight runs in column order, equal ids joined first
                double* Sg = S + (int64_t)g * K;
                int ak = -1;
                double av = 0.0;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int k = s_pk[tid * 8 + e];
                    if (k < 0) continue;
                    if (k != ak) {
                        if (ak >= 0) Sg[ak] += av;
                        ak = k;
                        av = s_pv[tid * 8 + e];
                    } else {
                        av += s_pv[tid * 8 + e];
                    }
                }
                if (ak >= 0) Sg[ak] += av;
            }
            __syncthreads();                              // the next pass, or the next product, overwrites the half tile
        }
    }

}

// the sample of every sorted row from the P slices of S: a wave per row, lane l the clusters l, l + 64, .. (coalesced), each cluster's
// slices added in group order; the minimum over the lanes does not depend on an order.  Scattered back to the caller's row order
__global__ void __launch_bounds__(RT_THREADS) sil_sample_kernel(const double* __restrict__ S, const int32_t* __restrict__ slab,
                                                                const int32_t* __restrict__ cnt, const int32_t* __restrict__ order, int n,
                                                                int K, int P, double* __restrict__ sorig, double* __restrict__ sil) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= n - cnt[K]) return;                          // the whole wave
    const int li = slab[g], nl = cnt[li];
    double b = 0.0, own = 0.0;
    int others = 0, nan = 0;
    for (int k = lane; k < K; k += 64) {
        const int nk = cnt[k];
        if (nk == 0) continue;
        double tot = 0.0;
        for (int p = 0; p < P; p++) tot += S[((int64_t)p * n + g) * K + k];
        if (k == li) {
            own = tot;
            continue;
        }
        const double v = tot / (double)nk;
        nan |= v != v;
        if (others == 0 || v < b) b = v;
        others++;
    }
    own = __shfl(own, li & 63, 64);                       // the lane that holds the row's own cluster
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(b, o, 64);
        const int oo = __shfl_xor(others, o, 64);
        nan |= __shfl_xor(nan, o, 64);
        if (oo > 0 && (others == 0 || ob < b)) b = ob;
        others += oo;
    }
    if (lane != 0) return;
    double s;
    if (others == 0) {
        s = cx_nan();                                     // fewer than two clusters: not defined
    } else if (nl == 1) {
        s = 0.0;
    } else {
        const double a = own / (double)(nl - 1);
        const double mx = a > b ? a : b;
        s = mx == 0.0 ? 0.0 : (b - a) / mx;
        if (nan || a != a) s = cx_nan();
    }
    const int64_t o = order[g];
    sorig[o] = s;
    if (sil) sil[o] = s;
}

// (5) the mean over the rows that take part: a thread per strip in row order, thread 0 the strips in strip order
__global__ void __launch_bounds__(CX_MAXPARTS) sil_mean_kernel(const double* __restrict__ sorig, const int32_t* __restrict__ lab, int n,
                                                               int K, int parts, double* __restrict__ mean) {
    __shared__ double s_sum[CX_MAXPARTS];
    __shared__ int s_num[CX_MAXPARTS];
    const int p = threadIdx.x;
    if (p < parts) {
        const int64_t r0 = (int64_t)p * n / parts, r1 = (int64_t)(p + 1) * n / parts;
        double acc = 0.0;
        int num = 0;
        for (int64_t i = r0; i < r1; i++) {
            const int l = lab[i];
            if (l >= 0 && l < K) {
                acc += sorig[i];
                num++;
            }
        }
        s_sum[p] = acc;
        s_num[p] = num;
    }
    __syncthreads();
    if (p == 0) {
        double acc = 0.0;
        int num = 0;
        for (int q = 0; q < parts; q++) {
            acc += s_sum[q];
            num += s_num[q];
        }
        *mean = num > 0 ? acc / (double)num : cx_nan();
    }
}

// ------------------------------------------------------------------ k-means++ seeding
// u_j of a restart: elements 2 j and 2 j + 1 of its draw under kind 2 (datafeed.hip's counter layout), 53 bits as mh_sample_weighted
__device__ __forceinline__ double kpp_uniform(uint64_t seed, uint64_t draw, int j) {
    uint32_t w[4] = {(uint32_t)(j >> 1), 2u, (uint32_t)draw, 0x80000000u | (uint32_t)(draw >> 32)};
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t a = (j & 1) ? w[2] : w[0], b = (j & 1) ? w[3] : w[1];
    const uint64_t bits = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
    return (double)bits * 1.1102230246251565e-16;         // 2^-53: exact, u in [0, 1)
}

// m = min(m, |y_i - c|^2) against centre j - 1 (j = 1: m = that distance), and the strip's sum in row order
__global__ void __launch_bounds__(RT_THREADS) kpp_dist_kernel(const float* __restrict__ y, int64_t n, int K, int D, int j, int parts,
                                                              const int64_t* __restrict__ rows, double* __restrict__ m,
                                                              double* __restrict__ partial) {
    __shared__ double s_term[RT_THREADS];
    const int tid = threadIdx.x, part = blockIdx.x, r = blockIdx.y;
    const int64_t r0 = (int64_t)part * n / parts, r1 = (int64_t)(part + 1) * n / parts;
    const float* c = y + rows[(int64_t)r * K + j - 1] * D;
    double* mr = m + (int64_t)r * n;
    double acc = 0.0;
    for (int64_t base = r0; base < r1; base += RT_THREADS) {
        const int64_t i = base + tid;
        double t = 0.0;
        if (i < r1) {
            const float* xr = y + i * D;
            for (int d = 0; d < D; d++) {
                const double e = (double)xr[d] - (double)c[d];
                t = fma(e, e, t);
            }
            if (!(t == t)) t = 0.0;                       // a NaN distance counts as weight 0
            if (j > 1) {
                const double old = mr[i];
                t = old < t ? old : t;
            }
            mr[i] = t;
        }
        s_term[tid] = t;
        __syncthreads();
        if (tid == 0) {
            const int cntr = r1 - base < RT_THREADS ? (int)(r1 - base) : RT_THREADS;
            for (int q = 0; q < cntr; q++) acc += s_term[q];              // row order
        }
        __syncthreads();
    }
    if (tid == 0) partial[(int64_t)r * parts + part] = acc;
}

// centre j of every restart: the draw, the strip, the row; then the bit copy of that row
__global__ void __launch_bounds__(RT_THREADS) kpp_pick_kernel(const float* __restrict__ y, int64_t n, int K, int D, int j, int parts,
                                                              uint64_t seed, uint64_t offset, const double* __restrict__ m,
                                                              const double* __restrict__ partial, int64_t* __restrict__ rows,
                                                              float* __restrict__ cent) {
    __shared__ double s_term[RT_THREADS];
    __shared__ double s_before, s_target;
    __shared__ int s_strip, s_last;
    __shared__ long long s_pick;
    const int tid = threadIdx.x, r = blockIdx.x;
    const double u = kpp_uniform(seed, offset + (uint64_t)r, j);
    const double* mr = m + (int64_t)r * n;
    if (tid == 0) {
        s_pick = (long long)(u * (double)n);              // centre 0, and T = 0
        s_strip = -1;
        s_last = -1;
        if (j > 0) {
            const double* pr = partial + (int64_t)r * parts;
            double T = 0.0;
            for (int p = 0; p < parts; p++) T += pr[p];   // strip order
            if (T > 0.0) {
                const double t = u * T;
                double before = 0.0;
                int strip = -2;                           // -2: rounding left no strip whose running sum passes t
                for (int p = 0; p < parts; p++) {
                    const double next = before + pr[p];
                    if (next > t) {
                        strip = p;
                        break;
                    }
                    before = next;
                }
                s_strip = strip;
                s_before = before;
                s_target = t;
            }
        }
    }
    __syncthreads();
    int strip = s_strip;                                  // the same for the whole workgroup
    if (strip >= 0) {
        const int64_t r0 = (int64_t)strip * n / parts, r1 = (int64_t)(strip + 1) * n / parts;
        const double before = s_before, t = s_target;
        double local = 0.0;                               // the strip's own running sum, as kpp_dist_kernel added it
        for (int64_t base = r0; base < r1; base += RT_THREADS) {
            s_term[tid] = base + tid < r1 ? mr[base + tid] : 0.0;
            __syncthreads();
            if (tid == 0) {
                const int cntr = r1 - base < RT_THREADS ? (int)(r1 - base) : RT_THREADS;
                for (int q = 0; q < cntr; q++) {
                    local += s_term[q];
                    if (before + local > t) {
                        s_pick = base + q;
                        s_last = 0;
                        break;
                    }
                }
            }
            __syncthreads();
            if (s_last == 0) break;
        }
        if (s_last != 0) strip = -2;                      // cannot happen (the strip's sum repeats bit for bit); the rule still holds
        __syncthreads();
    }
    if (strip == -2) {                                    // the last row with a positive weight
        if (tid == 0) s_last = -1;
        __syncthreads();
        int last = -1;
        for (int64_t i = tid; i < n; i += RT_THREADS)
            if (mr[i] > 0.0) last = (int)i;
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
        if (tid == 0 && s_last >= 0) s_pick = s_last;
        __syncthreads();
    }
    long long pick = s_pick;
    pick = pick < 0 ? 0 : (pick >= n ? n - 1 : pick);
    if (tid == 0) rows[(int64_t)r * K + j] = pick;
    const float* src = y + pick * D;
    float* dst = cent + ((int64_t)r * K + j) * D;
    for (int d = tid; d < D; d += RT_THREADS) dst[d] = src[d];
}

// ------------------------------------------------------------------ matched accuracy
constexpr long long CX_INF = 1ll << 60;

__global__ void __launch_bounds__(RT_THREADS) cluster_match_kernel(const int32_t* __restrict__ cont, int K, int C,
                                                                   int32_t* __restrict__ match, int64_t* __restrict__ hits) {
    __shared__ long long s_u[CX_MINSIDE + 1], s_v[CX_MAXK + 1], s_minv[CX_MAXK + 1];
    __shared__ int s_p[CX_MAXK + 1], s_way[CX_MAXK + 1], s_used[CX_MAXK + 1];
    __shared__ int s_cell[CX_LDSCELLS];
    __shared__ long long s_rv[RT_THREADS / 64];
    __shared__ int s_rj[RT_THREADS / 64];
    __shared__ unsigned long long s_hits;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* cr = cont + (int64_t)blockIdx.x * K * C;
    const bool tr = K > C;                                // the smaller side takes the rows of the assignment problem
    const int nr = tr ? C : K, nc = tr ? K : C;
    const bool small = K * C <= CX_LDSCELLS;
    if (small)
        for (int q = tid; q < K * C; q += RT_THREADS) s_cell[q] = cr[q];
    const int32_t* cell = small ? s_cell : cr;
    for (int q = tid; q <= nr; q += RT_THREADS) s_u[q] = 0;
    for (int q = tid; q <= nc; q += RT_THREADS) {
        s_v[q] = 0;
        s_p[q] = 0;
        s_way[q] = 0;
    }
    if (tid == 0) s_hits = 0ull;
    __syncthreads();

    for (int i = 1; i <= nr; i++) {                       // rows and columns count from 1; column 0 is the root of the path
        for (int q = tid; q <= nc; q += RT_THREADS) {
            s_minv[q] = CX_INF;
            s_used[q] = 0;
        }
        if (tid == 0) s_p[0] = i;
        int j0 = 0;
        __syncthreads();
        while (true) {
            const int i0 = s_p[j0];
            const long long ui = s_u[i0];
            long long best = CX_INF;
            int bj = 0x7fffffff;
            for (int q = 1 + tid; q <= nc; q += RT_THREADS) {             // ascending: a thread keeps the smaller column of a tie
                if (s_used[q] || q == j0) continue;
                const int w = tr ? cell[(q - 1) * C + (i0 - 1)] : cell[(i0 - 1) * C + (q - 1)];
                const long long cur = -(long long)w - ui - s_v[q];        // the cost is minus the count
                long long mv = s_minv[q];
                if (cur < mv) {
                    mv = cur;
                    s_minv[q] = cur;
                    s_way[q] = j0;
                }
                if (mv < best) {
                    best = mv;
                    bj = q;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long ov = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (ov < best || (ov == best && oj < bj)) {
                    best = ov;
                    bj = oj;
                }
            }
            if (lane == 0) {
                s_rv[wave] = best;
                s_rj[wave] = bj;
            }
            __syncthreads();
            long long delta = s_rv[0];
            int j1 = s_rj[0];
#pragma unroll
            for (int w = 1; w < RT_THREADS / 64; w++)
                if (s_rv[w] < delta || (s_rv[w] == delta && s_rj[w] < j1)) {
                    delta = s_rv[w];
                    j1 = s_rj[w];
                }
            for (int q = tid; q <= nc; q += RT_THREADS) {
                if (s_used[q] || q == j0) {               // the columns of the tree: their rows are distinct
                    s_u[s_p[q]] += delta;
                    s_v[q] -= delta;
                } else {
                    s_minv[q] -= delta;
                }
            }
            if (tid == 0) s_used[j0] = 1;
            j0 = j1 <= nc ? j1 : 0;                       // nr <= nc: a column outside the tree always exists
            __syncthreads();
            if (j0 == 0 || s_p[j0] == 0) break;           // a free column: the path ends
        }
        __syncthreads();                                  // every wave has read s_p[j0] before thread 0 rewrites the path
        if (tid == 0) {
            while (j0) {
                const int j1 = s_way[j0];
                s_p[j0] = s_p[j1];
                j0 = j1;
            }
        }
        __syncthreads();
    }

    int32_t* mo = match + (int64_t)blockIdx.x * K;
    unsigned long long mine = 0ull;
    for (int q = 1 + tid; q <= nc; q += RT_THREADS) {
        const int row = s_p[q];
        if (tr) {                                         // columns are clusters
            mo[q - 1] = row ? row - 1 : -1;
            if (row) mine += (unsigned long long)cell[(q - 1) * C + (row - 1)];
        } else if (row) {                                 // rows are clusters: every one of them is matched
            mo[row - 1] = q - 1;
            mine += (unsigned long long)cell[(row - 1) * C + (q - 1)];
        }
    }
    if (mine) atomicAdd(&s_hits, mine);                   // integers: the order is free
    __syncthreads();
    if (tid == 0) hits[blockIdx.x] = (int64_t)s_hits;
}

}  // namespace

extern "C" int64_t mh_silhouette_workspace_bytes(int64_t n, int K, int D) {
    if (n <= 0 || K <= 0 || D <= 0) return 0;
    return sil_layout(n, K, D, nullptr, nullptr);
}

extern "C" int mh_silhouette(const float* y, const int32_t* lab, int64_t n, int R, int K, int D, int metric, double* sil, double* mean,
                             int32_t* bad, void* workspace, mh_stream s) {
    if (int rc = cx_geometry("mh_silhouette", n, R, K, D)) return rc;
    MH_REQUIRE(metric == MH_KMEANS_EUCLIDEAN || metric == MH_KMEANS_COSINE, "mh_silhouette: metric = %d", metric);
    MH_REQUIRE(y && lab && mean && bad && workspace, "mh_silhouette: null pointer");
    MH_REQUIRE((((uintptr_t)sil | (uintptr_t)mean) & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
               "mh_silhouette: sil and mean must be 8-byte aligned, the workspace 16-byte aligned");
    SilWs w;
    sil_layout(n, K, D, (char*)workspace, &w);
    const int vec = D % 4 == 0;                           // the sorted copy is 16-byte aligned
    const int vecy = vec && mh_quad_ok(y, 4);
    const int parts = cx_parts(n), P = sil_splits(n, K);
    for (int r = 0; r < R; r++) {
        const int32_t* lr = lab + (int64_t)r * n;
        double* sr = sil ? sil + (int64_t)r * n : nullptr;
        hipLaunchKernelGGL(sil_order_kernel, dim3(1), dim3(RT_THREADS), 0, (hipStream_t)s, lr, (int)n, K, w.order, w.slab, w.cnt, w.sorig,
                           sr, bad + r);
        MH_LAUNCH_CHECK("mh_silhouette");
        hipLaunchKernelGGL(sil_gather_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)s, y, (const int32_t*)w.order, D, vecy, w.ys,
                           w.qn);
        MH_LAUNCH_CHECK("mh_silhouette");
        hipLaunchKernelGGL(sil_tile_kernel, dim3(mh_cdiv(n, RT_TILE), P), dim3(RT_THREADS), 0, (hipStream_t)s, (const float*)w.ys,
                           (const float*)w.qn, (const int32_t*)w.slab, (const int32_t*)w.cnt, (int)n, K, D, vec,
                           metric == MH_KMEANS_COSINE ? 1 : 0, P, w.S);
        MH_LAUNCH_CHECK("mh_silhouette");
        hipLaunchKernelGGL(sil_sample_kernel, dim3(mh_cdiv(n, RT_THREADS / 64)), dim3(RT_THREADS), 0, (hipStream_t)s, (const double*)w.S,
                           (const int32_t*)w.slab, (const int32_t*)w.cnt, (const int32_t*)w.order, (int)n, K, P, w.sorig, sr);
        MH_LAUNCH_CHECK("mh_silhouette");
        hipLaunchKernelGGL(sil_mean_kernel, dim3(1), dim3(CX_MAXPARTS), 0, (hipStream_t)s, (const double*)w.sorig, lr, (int)n, K, parts,
                           mean + r);
        MH_LAUNCH_CHECK("mh_silhouette");
    }
    return MH_OK;
}

extern "C" int64_t mh_kmeanspp_workspace_bytes(int64_t n, int R) {
    if (n <= 0 || R <= 0) return 0;
    return (int64_t)R * (n + cx_parts(n)) * (int64_t)sizeof(double);
}

extern "C" int mh_kmeanspp_init(const float* y, int64_t n, int R, int K, int D, uint64_t seed, uint64_t offset, int64_t* rows, float* cent,
                                void* workspace, mh_stream s) {
    if (int rc = cx_geometry("mh_kmeanspp_init", n, R, K, D)) return rc;
    MH_REQUIRE((int64_t)R * K <= (1 << 20), "mh_kmeanspp_init: R = %d restarts of K = %d centres outside 2^20 centres", R, K);
    MH_REQUIRE(offset < (1ull << 63) && offset + (uint64_t)R < (1ull << 63), "mh_kmeanspp_init: draw ids must stay below 2^63");
    MH_REQUIRE(y && rows && cent && workspace, "mh_kmeanspp_init: null pointer");
    MH_REQUIRE((((uintptr_t)rows | (uintptr_t)workspace) & 7) == 0, "mh_kmeanspp_init: rows and workspace must be 8-byte aligned");
    const int parts = cx_parts(n);
    double* m = (double*)workspace;
    double* partial = m + (int64_t)R * n;
    for (int j = 0; j < K; j++) {
        if (j > 0) {
            hipLaunchKernelGGL(kpp_dist_kernel, dim3(parts, R), dim3(RT_THREADS), 0, (hipStream_t)s, y, n, K, D, j, parts,
                               (const int64_t*)rows, m, partial);
            MH_LAUNCH_CHECK("mh_kmeanspp_init");
        }
        hipLaunchKernelGGL(kpp_pick_kernel, dim3(R), dim3(RT_THREADS), 0, (hipStream_t)s, y, n, K, D, j, parts, seed, offset,
                           (const double*)m, (const double*)partial, rows, cent);
        MH_LAUNCH_CHECK("mh_kmeanspp_init");
    }
    return MH_OK;
}

extern "C" int mh_cluster_match(const int32_t* cont, int R, int K, int C, int32_t* match, int64_t* hits, mh_stream s) {
    MH_REQUIRE(K >= 1 && K <= CX_MAXK, "mh_cluster_match: K = %d outside [1, %d]", K, CX_MAXK);
    MH_REQUIRE(C >= 1 && C <= CX_MAXC, "mh_cluster_match: C = %d outside [1, %d]", C, CX_MAXC);
    MH_REQUIRE((int64_t)K * C <= CX_MAXCELLS, "mh_cluster_match: K C = %lld cells outside [1, %d]", (long long)K * C, CX_MAXCELLS);
    MH_REQUIRE(R >= 1 && R <= (1 << 20), "mh_cluster_match: R = %d outside [1, 2^20]", R);
    MH_REQUIRE(cont && match && hits, "mh_cluster_match: null pointer");
    MH_REQUIRE(((uintptr_t)hits & 7) == 0, "mh_cluster_match: hits must be 8-byte aligned");
    hipLaunchKernelGGL(cluster_match_kernel, dim3((unsigned)R), dim3(RT_THREADS), 0, (hipStream_t)s, cont, K, C, match, hits);
    MH_LAUNCH_CHECK("mh_cluster_match");
    return MH_OK;
}
