// k-means of frozen embeddings and its agreement with labels (mirror_amd/cluster.py): Lloyd's iteration over R restarts at once, the
// restarts in the role the episodes have in fewshot.hip.  Five entry points, each one launch (mh_kmeans_inertia: two) on the caller's
// stream, nothing allocated, no host wait, no float atomics anywhere: every sum has a fixed order, so two runs agree bit for bit.
//
//   mh_kmeans_assign   the hot path.  A workgroup owns 128 rows of one restart and walks that restart's ceil(K / 128) key tiles in
//                      ascending order through retrieval_tile.h's exact-f32 product.  Behind every product the tile goes through LDS
//                      64 rows at a time, as in mh_fewshot_predict (stride 129: spills and scans both hit 32 distinct banks), and four
//                      threads per row scan 32 columns each, ascending, with a strict compare; a thread carries its (row, quarter)'s best
//                      across the tiles in registers.  The four quarters of a row interleave in k, so the last step compares the index
//                      as well: the smaller k wins a tie.  No [n, R K] matrix in HBM.  `changed` is one integer atomic per workgroup.
//   mh_kmeans_update   one workgroup per (restart, cluster): it reads assign[r, :] 256 rows at a time, compacts the members in row order
//                      (ballot + prefix), and every thread adds the members' values of its columns in that order in f64.  The mean is
//                      rounded to f32 once; |c|^2 of the ROUNDED centroid in f64 (per thread in column order, a fixed butterfly, the
//                      four waves in order) gives the bias, or the cosine scale.
//   mh_kmeans_bias     -|c|^2 / 2 of centroids the update did not produce (a start, a caller's own), in the update's order of additions.
//   mh_kmeans_inertia  a workgroup per (row strip of mh_colmean's partition, restart): one thread per row forms |x - c|^2 in f64 over
//                      ascending d, thread 0 adds the rows in row order; a second launch adds the strips in strip order.
//   mh_kmeans_tally    one workgroup per restart: the contingency counts by integer atomics on the workgroup's own slice of `cont` (K C
//                      reaches 65536 cells: more than LDS holds), the marginals by LDS atomics; NMI, ARI and purity in f64 from the
//                      integers: a thread per cluster adds its row of cells in label order, thread 0 the clusters in cluster order.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int KM_MAXK = 1024;         // clusters per restart
constexpr int KM_MAXC = 1024;         // label classes of the tally
constexpr int KM_MAXCELLS = 65536;    // K C of the tally
constexpr int KM_MAXD = 4096;
constexpr int KM_MAXR = 65535;        // restarts: one grid row each
constexpr int KM_DREG = KM_MAXD / RT_THREADS;   // a centroid's elements per thread
constexpr int KM_HALF = RT_TILE / 2;  // rows per pass of the assign epilogue
constexpr int KM_LD = RT_TILE + 1;    // LDS row stride of the spilled half tile
constexpr int KM_QUARTER = RT_TILE / 4;         // key columns per scanning thread
constexpr int KM_MAXPARTS = 128;      // row strips of the inertia: mh_colmean's partition

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double block_sum256_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------ assignment
__global__ void __launch_bounds__(RT_THREADS, 2) kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                      const float* __restrict__ bias, int n, int K, int D, int vec,
                                                                      const int32_t* prev, int32_t* assign, float* __restrict__ score,
                                                                      int32_t* __restrict__ changed) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    static_assert(KM_HALF * KM_LD + RT_TILE <= 4 * RT_TILE * RT_LD, "half a tile and its biases must fit the stages");
    __shared__ int s_changed;
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + KM_HALF * KM_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, r = blockIdx.y;
    const float* cr = cent + (int64_t)r * K * D;
    const float* br = bias ? bias + (int64_t)r * K : nullptr;
    const int rl = tid & (KM_HALF - 1), quarter = tid >> 6;               // the (row of the half tile, 32 columns) this thread scans
    if (tid == 0) s_changed = 0;

    float bv[2] = {0.f, 0.f};                             // this thread's best of passes 0 and 1, carried across the key tiles
    int bk[2] = {-1, -1};
    for (int col0 = 0; col0 < K; col0 += RT_TILE) {
        f32x16 acc[2][2];
        retr_product(acc, x, cr, n, K, D, row0, col0, vec, s_a, s_b);     // ends with a barrier behind the last read of the stages
        if (tid < RT_TILE) s_bias[tid] = (br && col0 + tid < K) ? br[col0 + tid] : 0.f;
        const int k0 = col0 + quarter * KM_QUARTER;
        const int kn = K - k0 < KM_QUARTER ? K - k0 : KM_QUARTER;         // columns >= K are never looked at (kn <= 0: none)
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            if (wm == pass) {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++)
#pragma unroll
                        for (int q = 0; q < 16; q++)
                            s_t[(i * 32 + (q & 3) + 8 * (q >> 2) + 4 * half) * KM_LD + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][q];
            }
            __syncthreads();
            const float* sc = s_t + rl * KM_LD + quarter * KM_QUARTER;
            const float* sb = s_bias + quarter * KM_QUARTER;
            for (int c = 0; c < kn; c++) {                // ascending, strict: within a thread ties go to the smaller k
                float v = sc[c];
                if (br) v += sb[c];
                if (v == v && (bk[pass] < 0 || v > bv[pass])) {
                    bk[pass] = k0 + c;
                    bv[pass] = v;
                }
            }
            __syncthreads();                              // the next pass, or the next product, overwrites the half tile
        }
    }

    // the four quarters of a row: [tile row][quarter] values, then indices
    float* s_v = s_t;
    float* s_k = s_t + RT_TILE * 4;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        s_v[(pass * KM_HALF + rl) * 4 + quarter] = bv[pass];
        s_k[(pass * KM_HALF + rl) * 4 + quarter] = __int_as_float(bk[pass]);
    }
    __syncthreads();
    if (tid < RT_TILE && row0 + tid < n) {
        int best = -1;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = __float_as_int(s_k[tid * 4 + q]);
            const float w = s_v[tid * 4 + q];
            if (k >= 0 && (best < 0 || w > v || (w == v && k < best))) {
                best = k;
                v = w;
            }
        }
        const int64_t o = (int64_t)r * n + row0 + tid;
        const bool diff = prev && prev[o] != best;        // prev may be assign itself: read before the store, by the same thread
        assign[o] = best;
        if (score) score[o] = best >= 0 ? v : __uint_as_float(0x7fc00000u);
        if (diff) atomicAdd(&s_changed, 1);
    }
    __syncthreads();
    if (tid == 0 && prev && s_changed) atomicAdd(&changed[r], s_changed);
}

// ------------------------------------------------------------------ update
__global__ void __launch_bounds__(RT_THREADS) kmeans_update_kernel(const float* __restrict__ x, const int32_t* __restrict__ assign, int n,
                                                                   int K, int D, int cosine, float* __restrict__ cent,
                                                                   float* __restrict__ bias, int32_t* __restrict__ count) {
    __shared__ int s_idx[RT_THREADS];                     // the members of the current 256 rows, in row order
    __shared__ int s_wave[RT_THREADS / 64];
    __shared__ double s_red[RT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x % K;
    const int32_t* ar = assign + (int64_t)(blockIdx.x / K) * n;
    double acc[KM_DREG];
#pragma unroll
    for (int u = 0; u < KM_DREG; u++) acc[u] = 0.0;
    int total = 0;
    for (int base = 0; base < n; base += RT_THREADS) {
        const int i = base + tid;
        const bool mine = i < n && ar[i] == k;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, cnt = 0;
#pragma unroll
        for (int w = 0; w < RT_THREADS / 64; w++) {
            if (w < wave) off += s_wave[w];
            cnt += s_wave[w];
        }
        if (mine) s_idx[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
        __syncthreads();                                  // also: s_wave is next written behind this barrier, s_idx behind the next one
        if (cnt == 0) continue;                           // the same for the whole workgroup
        total += cnt;
#pragma unroll
        for (int u = 0; u < KM_DREG; u++) {
            const int d = tid + u * RT_THREADS;
            if (d < D) {
                double a = acc[u];
                int j = 0;
                for (; j + 4 <= cnt; j += 4) {            // four loads in flight, the additions still in row order
                    const float a0 = x[(int64_t)s_idx[j] * D + d], a1 = x[(int64_t)s_idx[j + 1] * D + d];
                    const float a2 = x[(int64_t)s_idx[j + 2] * D + d], a3 = x[(int64_t)s_idx[j + 3] * D + d];
                    a += (double)a0;
                    a += (double)a1;
                    a += (double)a2;
                    a += (double)a3;
                }
                for (; j < cnt; j++) a += (double)x[(int64_t)s_idx[j] * D + d];
                acc[u] = a;
            }
        }
    }
    if (total == 0) {                                     // an empty cluster keeps its centroid and its bias
        if (tid == 0) count[blockIdx.x] = 0;
        return;
    }
    const double members = (double)total;
    float v[KM_DREG];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < KM_DREG; u++) {
        v[u] = tid + u * RT_THREADS < D ? (float)(acc[u] / members) : 0.f;
        ss = fma((double)v[u], (double)v[u], ss);
    }
    ss = block_sum256_f64(ss, s_red);
    const double nrm = fmax(sqrt(ss), 1e-12);
    float* out = cent + (int64_t)blockIdx.x * D;
#pragma unroll
    for (int u = 0; u < KM_DREG; u++) {
        const int d = tid + u * RT_THREADS;
        if (d < D) out[d] = cosine ? (float)((double)v[u] / nrm) : v[u];
    }
    if (tid == 0) {
        count[blockIdx.x] = total;
        if (bias) bias[blockIdx.x] = (float)(-0.5 * ss);
    }
}

// bias = -|c|^2 / 2 of centroids that did not come out of the update (a start, a caller's own): the update's order of additions
__global__ void __launch_bounds__(RT_THREADS) kmeans_bias_kernel(const float* __restrict__ cent, int D, float* __restrict__ bias) {
    __shared__ double s_red[RT_THREADS / 64];
    const float* c = cent + (int64_t)blockIdx.x * D;
    double ss = 0.0;
    for (int d = threadIdx.x; d < D; d += RT_THREADS) ss = fma((double)c[d], (double)c[d], ss);
    ss = block_sum256_f64(ss, s_red);
    if (threadIdx.x == 0) bias[blockIdx.x] = (float)(-0.5 * ss);
}

// ------------------------------------------------------------------ inertia
int inertia_parts(int64_t n) {                            // mh_colmean's strips: at least 64 rows, 128 strips at the most
    const int64_t p = (n + 63) / 64;
    return (int)(p < 1 ? 1 : (p > KM_MAXPARTS ? KM_MAXPARTS : p));
}

__global__ void __launch_bounds__(RT_THREADS) kmeans_inertia_part_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                         const int32_t* __restrict__ assign, int64_t n, int K, int D,
                                                                         int parts, double* __restrict__ partial) {
    __shared__ double s_term[RT_THREADS];
    const int tid = threadIdx.x, part = blockIdx.x, r = blockIdx.y;
    const int64_t r0 = (int64_t)part * n / parts, r1 = (int64_t)(part + 1) * n / parts;
    const int32_t* ar = assign + (int64_t)r * n;
    const float* cr = cent + (int64_t)r * K * D;
    double acc = 0.0;
    for (int64_t base = r0; base < r1; base += RT_THREADS) {
        const int64_t i = base + tid;
        double t = 0.0;                                   // an unassigned row adds +0, which changes nothing
        if (i < r1) {
            const int a = ar[i];
            if (a >= 0 && a < K) {
                const float* xr = x + i * D;
                const float* c = cr + (int64_t)a * D;
                for (int d = 0; d < D; d++) {
                    const double e = (double)xr[d] - (double)c[d];
                    t = fma(e, e, t);
                }
            }
        }
        s_term[tid] = t;
        __syncthreads();
        if (tid == 0) {
            const int m = r1 - base < RT_THREADS ? (int)(r1 - base) : RT_THREADS;
            for (int j = 0; j < m; j++) acc += s_term[j];                 // row order
        }
        __syncthreads();
    }
    if (tid == 0) partial[(int64_t)r * parts + part] = acc;
}

__global__ void __launch_bounds__(RT_THREADS) kmeans_inertia_fold_kernel(const double* __restrict__ partial, int R, int parts,
                                                                         double* __restrict__ inertia) {
    const int r = blockIdx.x * RT_THREADS + threadIdx.x;
    if (r >= R) return;
    double acc = 0.0;
    for (int p = 0; p < parts; p++) acc += partial[(int64_t)r * parts + p];
    inertia[r] = acc;
}

// ------------------------------------------------------------------ tally
__global__ void __launch_bounds__(RT_THREADS) kmeans_tally_kernel(const int32_t* __restrict__ assign, const int64_t* __restrict__ labels,
                                                                  int n, int K, int C, int32_t* cont, int32_t* __restrict__ bad,
                                                                  double* __restrict__ summary) {
    __shared__ int s_a[KM_MAXK], s_b[KM_MAXC];            // members of every cluster, of every label
    __shared__ double s_logb[KM_MAXC];
    __shared__ double s_mi[KM_MAXK];                      // per cluster: its cells' share of the mutual information,
    __shared__ long long s_sq[KM_MAXK];                   // the sum of their squares,
    __shared__ int s_mx[KM_MAXK];                         // and the largest of them
    __shared__ int s_bad;
    const int tid = threadIdx.x, r = blockIdx.x;
    int32_t* cr = cont + (int64_t)r * K * C;
    const int32_t* ar = assign + (int64_t)r * n;
    for (int j = tid; j < K * C; j += RT_THREADS) cr[j] = 0;
    for (int j = tid; j < K; j += RT_THREADS) s_a[j] = 0;
    for (int j = tid; j < C; j += RT_THREADS) s_b[j] = 0;
    if (tid == 0) s_bad = 0;
    __threadfence();
    __syncthreads();
    for (int i = tid; i < n; i += RT_THREADS) {
        const int64_t y = labels[i];
        const int a = ar[i];
        if (y >= 0 && y < C && a >= 0 && a < K) {
            atomicAdd(&cr[a * C + (int)y], 1);
            atomicAdd(&s_a[a], 1);
            atomicAdd(&s_b[(int)y], 1);
        } else {
            atomicAdd(&s_bad, 1);
        }
    }
    __threadfence();
    __syncthreads();
    const int total = n - s_bad;
    const double N = (double)total, logN = log(N);
    for (int c = tid; c < C; c += RT_THREADS) s_logb[c] = s_b[c] > 0 ? log((double)s_b[c]) : 0.0;
    __syncthreads();
    for (int k = tid; k < K; k += RT_THREADS) {
        double mi = 0.0;
        long long sq = 0;
        int mx = 0;
        if (s_a[k] > 0) {
            const double loga = log((double)s_a[k]);
            for (int c = 0; c < C; c++) {                 // label order; the cells were written by atomics: read them where those live
                const int v = __hip_atomic_load(&cr[k * C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v > 0) {
                    sq += (long long)v * v;
                    mx = v > mx ? v : mx;
                    const double t = ((double)v / N) * (((log((double)v) - loga) - s_logb[c]) + logN);
                    mi += fabs(t) < 2.220446049250313e-16 ? 0.0 : t;
                }
            }
        }
        s_mi[k] = mi;
        s_sq[k] = sq;
        s_mx[k] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        bad[r] = s_bad;
        double mi = 0.0, ha = 0.0, hb = 0.0;
        long long sq = 0, sa = 0, sb = 0, hit = 0;
        int nk = 0, nc = 0;
        for (int k = 0; k < K; k++) {                     // cluster order
            mi += s_mi[k];
            sq += s_sq[k];
            hit += s_mx[k];
            if (s_a[k] > 0) {
                nk++;
                sa += (long long)s_a[k] * s_a[k];
                ha -= ((double)s_a[k] / N) * (log((double)s_a[k]) - logN);
            }
        }
        for (int c = 0; c < C; c++) {                     // label order
            if (s_b[c] > 0) {
                nc++;
                sb += (long long)s_b[c] * s_b[c];
                hb -= ((double)s_b[c] / N) * (s_logb[c] - logN);
            }
        }
        // NMI as sklearn's normalized_mutual_info_score("arithmetic"): 1 when neither side splits the rows (or there are none), 0 when
        // exactly one does not or the information is 0
        double nmi;
        if (nk <= 1 && nc <= 1) nmi = 1.0;
        else if (nk == 1 || nc == 1) nmi = 0.0;
        else {
            mi = mi > 0.0 ? mi : 0.0;
            nmi = mi == 0.0 ? 0.0 : mi / (0.5 * (ha + hb));
        }
        // ARI as adjusted_rand_score: the pair counts are exact integers (N <= 2^20: below 2^41), their products go through f64
        const long long tot = total;
        const long long tp = sq - tot, fp = sb - sq, fn = sa - sq, tn = tot * tot - fp - fn - sq;
        double ari = 1.0;
        if (fp != 0 || fn != 0) {
            const double dtp = (double)tp, dfp = (double)fp, dfn = (double)fn, dtn = (double)tn;
            ari = 2.0 * (dtp * dtn - dfn * dfp) / ((dtp + dfn) * (dfn + dtn) + (dtp + dfp) * (dfp + dtn));
        }
        summary[3 * (int64_t)r + 0] = nmi;
        summary[3 * (int64_t)r + 1] = ari;
        summary[3 * (int64_t)r + 2] = total > 0 ? (double)hit / N : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// the limits the k-means entry points share; 0: fine
int kmeans_geometry(const char* who, int64_t n, int R, int K, int D) {
    MH_REQUIRE(K >= 1 && K <= KM_MAXK, "%s: K = %d outside [1, %d]", who, K, KM_MAXK);
    MH_REQUIRE(D >= 1 && D <= KM_MAXD, "%s: D = %d outside [1, %d]", who, D, KM_MAXD);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %lld outside [1, 2^20]", who, (long long)n);
    MH_REQUIRE(R >= 1 && R <= KM_MAXR && (int64_t)R * K <= (1 << 20), "%s: R = %d restarts of K = %d keys outside [1, %d] restarts, 2^20 keys",
               who, R, K, KM_MAXR);
    return MH_OK;
}

}  // namespace

extern "C" int mh_kmeans_assign(const float* x, const float* cent, const float* bias, int64_t n, int R, int K, int D, const int32_t* prev,
                                int32_t* assign, float* score, int32_t* changed, mh_stream s) {
    if (int rc = kmeans_geometry("mh_kmeans_assign", n, R, K, D)) return rc;
    MH_REQUIRE(x && cent && assign, "mh_kmeans_assign: null pointer");
    MH_REQUIRE((prev != nullptr) == (changed != nullptr), "mh_kmeans_assign: prev and changed go together");
    const int vec = D % 4 == 0 && mh_quad_ok(x, 4) && mh_quad_ok(cent, 4);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(mh_cdiv(n, RT_TILE), R), dim3(RT_THREADS), 0, (hipStream_t)s, x, cent, bias, (int)n, K, D,
                       vec, prev, assign, score, changed);
    MH_LAUNCH_CHECK("mh_kmeans_assign");
    return MH_OK;
}

extern "C" int64_t mh_kmeans_update_workspace_bytes(int64_t n, int R, int K, int D) {
    (void)n, (void)R, (void)K, (void)D;
    return 0;                                             // the scan-and-compact update keeps its members in LDS
}

extern "C" int mh_kmeans_update(const float* x, const int32_t* assign, int64_t n, int R, int K, int D, int metric, float* cent, float* bias,
                                int32_t* count, void* workspace, mh_stream s) {
    (void)workspace;
    if (int rc = kmeans_geometry("mh_kmeans_update", n, R, K, D)) return rc;
    MH_REQUIRE(metric == MH_KMEANS_EUCLIDEAN || metric == MH_KMEANS_COSINE, "mh_kmeans_update: metric = %d", metric);
    MH_REQUIRE(x && assign && cent && count, "mh_kmeans_update: null pointer");
    MH_REQUIRE((bias != nullptr) == (metric == MH_KMEANS_EUCLIDEAN), "mh_kmeans_update: the bias goes with the euclidean metric only");
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)R * (unsigned)K), dim3(RT_THREADS), 0, (hipStream_t)s, x, assign, (int)n, K, D,
                       metric == MH_KMEANS_COSINE ? 1 : 0, cent, bias, count);
    MH_LAUNCH_CHECK("mh_kmeans_update");
    return MH_OK;
}

extern "C" int mh_kmeans_bias(const float* cent, int R, int K, int D, float* bias, mh_stream s) {
    if (int rc = kmeans_geometry("mh_kmeans_bias", 1, R, K, D)) return rc;
    MH_REQUIRE(cent && bias, "mh_kmeans_bias: null pointer");
    hipLaunchKernelGGL(kmeans_bias_kernel, dim3((unsigned)R * (unsigned)K), dim3(RT_THREADS), 0, (hipStream_t)s, cent, D, bias);
    MH_LAUNCH_CHECK("mh_kmeans_bias");
    return MH_OK;
}

extern "C" int64_t mh_kmeans_inertia_workspace_bytes(int64_t n, int R) {
    if (n <= 0 || R <= 0) return 0;
    return (int64_t)inertia_parts(n) * R * (int64_t)sizeof(double);
}

extern "C" int mh_kmeans_inertia(const float* x, const float* cent, const int32_t* assign, int64_t n, int R, int K, int D, double* inertia,
                                 void* workspace, mh_stream s) {
    if (int rc = kmeans_geometry("mh_kmeans_inertia", n, R, K, D)) return rc;
    MH_REQUIRE(x && cent && assign && inertia && workspace, "mh_kmeans_inertia: null pointer");
    MH_REQUIRE((((uintptr_t)workspace | (uintptr_t)inertia) & 7) == 0, "mh_kmeans_inertia: inertia and workspace must be 8-byte aligned");
    const int parts = inertia_parts(n);
    hipLaunchKernelGGL(kmeans_inertia_part_kernel, dim3(parts, R), dim3(RT_THREADS), 0, (hipStream_t)s, x, cent, assign, n, K, D, parts,
                       (double*)workspace);
    MH_LAUNCH_CHECK("mh_kmeans_inertia");
    hipLaunchKernelGGL(kmeans_inertia_fold_kernel, dim3(mh_cdiv(R, RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)s,
                       (const double*)workspace, R, parts, inertia);
    MH_LAUNCH_CHECK("mh_kmeans_inertia");
    return MH_OK;
}

extern "C" int mh_kmeans_tally(const int32_t* assign, const int64_t* labels, int64_t n, int R, int K, int C, int32_t* cont, int32_t* bad,
                               double* summary, mh_stream s) {
    MH_REQUIRE(K >= 1 && K <= KM_MAXK, "mh_kmeans_tally: K = %d outside [1, %d]", K, KM_MAXK);
    MH_REQUIRE(C >= 1 && C <= KM_MAXC, "mh_kmeans_tally: C = %d outside [1, %d]", C, KM_MAXC);
    MH_REQUIRE((int64_t)K * C <= KM_MAXCELLS, "mh_kmeans_tally: K C = %lld cells outside [1, %d]", (long long)K * C, KM_MAXCELLS);
    MH_REQUIRE(R >= 1 && R <= (1 << 20), "mh_kmeans_tally: R = %d outside [1, 2^20]", R);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_kmeans_tally: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(assign && labels && cont && bad && summary, "mh_kmeans_tally: null pointer");
    MH_REQUIRE((((uintptr_t)labels | (uintptr_t)summary) & 7) == 0, "mh_kmeans_tally: labels and summary must be 8-byte aligned");
    hipLaunchKernelGGL(kmeans_tally_kernel, dim3((unsigned)R), dim3(RT_THREADS), 0, (hipStream_t)s, assign, labels, (int)n, K, C, cont, bad,
                       summary);
    MH_LAUNCH_CHECK("mh_kmeans_tally");
    return MH_OK;
}
