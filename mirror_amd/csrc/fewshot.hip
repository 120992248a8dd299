// Few-shot prototype probe of frozen embeddings (mirror_amd/fewshot.py): the nearest-centroid classifier of SimpleShot over E random
// support draws at once.  Five entry points, each one launch (mh_colmean: two) on the caller's stream, nothing allocated, no host wait,
// no float atomics anywhere: every sum has a fixed order, so two runs agree bit for bit.
//
//   mh_colmean          mu[d] = mean of the pool's column d: row strips summed in row order in f64, the strips then in strip order.
//   mh_center_l2norm    y = (x - mu) / max(|x - mu|, eps), one wave per row.
//   mh_fewshot_protos   one workgroup per (episode, class slot): the K support rows summed in k order in f32, times 1 / K; the bias
//                       -|p|^2 / 2 (euclidean) or the prototype normalised again (cosine); pad slots 0 / -inf.
//   mh_fewshot_predict  the hot path.  The prototypes of ALL episodes are the keys of retrieval_tile.h's exact-f32 128 x 128 product (Cp
//                       is a power of two <= 64, so an episode's Cp keys never straddle a tile); the epilogue turns every run of Cp key
//                       columns into one class per query row.  In retr_product's accumulator layout a lane owns one key column and 16
//                       query rows, so that reduction crosses lanes (and the two wn waves at Cp = 64): the tile goes through LDS, 64 rows
//                       at a time (64 x 129 floats fit the four stages of the product, which are idle behind its last barrier), and
//                       one thread scans each (row, run) in ascending class order with a strict compare: the smaller class wins a tie.
//                       Stride 129: a spill instruction's 32 lanes of one half write 32 consecutive floats of one row, a scan's 32 lanes
//                       read 32 consecutive rows at one column, (row 129 + c) mod 32 = (row + c) mod 32: both hit 32 distinct banks.
//                       No [nq, E Cp] matrix in HBM, no scratch.
//   mh_fewshot_tally    one workgroup per episode: int32 confusion counts in LDS (integer atomics), stored; the three summary numbers
//                       in f64 from the integer counts in class order.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int FS_MAXC = 64;           // classes: one run of Cp <= 64 key columns lies inside one 128-key tile
constexpr int FS_MAXK = 1024;         // shots: the support indices of one prototype in LDS
constexpr int FS_MAXD = 4096;
constexpr int FS_DREG = FS_MAXD / RT_THREADS;   // a prototype's elements per thread
constexpr int FS_HALF = RT_TILE / 2;  // rows per pass of the predict epilogue
constexpr int FS_LD = RT_TILE + 1;    // LDS row stride of the spilled half tile
constexpr int CM_MAXPARTS = 128;      // row strips of the column mean

// ------------------------------------------------------------------ preparation
// strip `part` of column d: rows [part n / parts, (part + 1) n / parts) in row order, f64
__global__ void __launch_bounds__(RT_THREADS) colmean_part_kernel(const float* __restrict__ x, int64_t n, int D, int parts,
                                                                  double* __restrict__ partial) {
    const int d = blockIdx.x * RT_THREADS + threadIdx.x, part = blockIdx.y;
    if (d >= D) return;
    const int64_t r0 = (int64_t)part * n / parts, r1 = (int64_t)(part + 1) * n / parts;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; r++) acc += (double)x[r * D + d];
    partial[(int64_t)part * D + d] = acc;
}

__global__ void __launch_bounds__(RT_THREADS) colmean_fold_kernel(const double* __restrict__ partial, int64_t n, int D, int parts,
                                                                  float* __restrict__ mu) {
    const int d = blockIdx.x * RT_THREADS + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int p = 0; p < parts; p++) acc += partial[(int64_t)p * D + d];
    mu[d] = (float)(acc / (double)n);
}

int colmean_parts(int64_t n) {
    const int64_t p = (n + 63) / 64;                      // strips of at least 64 rows
    return (int)(p < 1 ? 1 : (p > CM_MAXPARTS ? CM_MAXPARTS : p));
}

// one wave per row: the squares of x - mu summed per lane in column order, then across the lanes by the fixed butterfly of wave_sum
__global__ void __launch_bounds__(RT_THREADS) center_l2norm_kernel(const float* __restrict__ x, const float* __restrict__ mu,
                                                                   float* __restrict__ y, int64_t n, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;                                 // wave-uniform, no block barrier below
    const float* xr = x + row * D;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float v = xr[d] - mu[d];
        ss = fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    const float inv = 1.f / fmaxf(sqrtf(ss), eps);
    float* yr = y + row * D;
    for (int d = lane; d < D; d += 64) yr[d] = (xr[d] - mu[d]) * inv;
}

// ------------------------------------------------------------------ prototypes
__global__ void __launch_bounds__(RT_THREADS) fewshot_protos_kernel(const float* __restrict__ y, int64_t n, const int64_t* __restrict__ rows,
                                                                    const int64_t* __restrict__ perm, int C, int Cp, int K, int D,
                                                                    int cosine, float* __restrict__ protos, float* __restrict__ bias) {
    __shared__ int s_row[FS_MAXK];
    __shared__ int s_bad;
    __shared__ float red[RT_THREADS / 64];
    const int tid = threadIdx.x;
    const int e = blockIdx.x / Cp, c = blockIdx.x % Cp;
    float* out = protos + (int64_t)blockIdx.x * D;
    if (c >= C) {                                         // a pad slot (the same for the whole workgroup)
        for (int d = tid; d < D; d += RT_THREADS) out[d] = 0.f;
        if (tid == 0 && bias) bias[blockIdx.x] = -INFINITY;
        return;
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const int64_t* r = rows + ((int64_t)e * C + c) * K;
    for (int k = tid; k < K; k += RT_THREADS) {
        int64_t j = r[k];
        if (perm && j >= 0 && j < n) j = perm[j];
        const bool ok = j >= 0 && j < n;
        s_row[k] = ok ? (int)j : 0;
        if (!ok) s_bad = 1;                               // every writer stores the same value
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    const float inv_k = 1.f / (float)K;
    float v[FS_DREG];
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < FS_DREG; u++) {
        const int d = tid + u * RT_THREADS;
        float acc = 0.f;
        if (d < D) {
            int k = 0;
            for (; k + 4 <= K; k += 4) {                  // four loads in flight, the additions still in k order
                const float a0 = y[(int64_t)s_row[k] * D + d], a1 = y[(int64_t)s_row[k + 1] * D + d];
                const float a2 = y[(int64_t)s_row[k + 2] * D + d], a3 = y[(int64_t)s_row[k + 3] * D + d];
                acc += a0;
                acc += a1;
                acc += a2;
                acc += a3;
            }
            for (; k < K; k++) acc += y[(int64_t)s_row[k] * D + d];
            acc *= inv_k;
        }
        v[u] = acc;
        ss = fmaf(acc, acc, ss);
    }
    ss = block_sum256(ss, red);                           // per thread in d order, the butterfly, the four waves in order
    const float nan = __uint_as_float(0x7fc00000u);
    float scale = 1.f;
    if (cosine) scale = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int u = 0; u < FS_DREG; u++) {
        const int d = tid + u * RT_THREADS;
        if (d < D) out[d] = bad ? nan : v[u] * scale;
    }
    if (tid == 0 && bias) bias[blockIdx.x] = bad ? nan : -0.5f * ss;
}

// ------------------------------------------------------------------ prediction
__global__ void __launch_bounds__(RT_THREADS, 3) fewshot_predict_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                                        const float* __restrict__ bias, int nq, int nk, int D, int C,
                                                                        int cshift, int vec, int32_t* __restrict__ pred) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    static_assert(FS_HALF * FS_LD + RT_TILE <= 4 * RT_TILE * RT_LD, "half a tile and its biases must fit the stages");
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + FS_HALF * FS_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Cp = 1 << cshift;

    f32x16 acc[2][2];
    retr_product(acc, q, p, nq, nk, D, row0, col0, vec, s_a, s_b);      // ends with a barrier behind the last read of the stages

    if (tid < RT_TILE) s_bias[tid] = (bias && col0 + tid < nk) ? bias[col0 + tid] : 0.f;
    const int tasks = FS_HALF << (7 - cshift);            // 64 rows x (128 / Cp) runs
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        s_t[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * FS_LD + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
        }
        __syncthreads();
        for (int t = tid; t < tasks; t += RT_THREADS) {
            const int rl = t & (FS_HALF - 1), run = t >> 6;
            const int row = row0 + pass * FS_HALF + rl, key0 = col0 + run * Cp;
            if (row >= nq || key0 >= nk) continue;        // nk = E Cp: a run lies inside the keys or outside them
            const float* sc = s_t + rl * FS_LD + run * Cp;
            const float* sb = s_bias + run * Cp;
            int best = -1;
            float bv = 0.f;
            for (int c = 0; c < C; c++) {                 // pads (c >= C) are never looked at; ascending, strict: ties to the smaller class
                float v = sc[c];
                if (bias) v += sb[c];
                if (v == v && (best < 0 || v > bv)) {
                    best = c;
                    bv = v;
                }
            }
            pred[(int64_t)(key0 >> cshift) * nq + row] = best;
        }
        __syncthreads();                                  // the next pass overwrites the half tile
    }
}

// ------------------------------------------------------------------ tally
__global__ void __launch_bounds__(RT_THREADS) fewshot_tally_kernel(const int32_t* __restrict__ pred, const int64_t* __restrict__ labels,
                                                                   int nq, int C, int32_t* __restrict__ conf, int32_t* __restrict__ bad,
                                                                   double* __restrict__ summary) {
    __shared__ int s_conf[FS_MAXC * FS_MAXC];
    __shared__ int s_n[FS_MAXC];                          // rows of every label, a prediction of -1 included
    __shared__ int s_tp[FS_MAXC], s_pr[FS_MAXC];
    __shared__ int s_bad;
    const int tid = threadIdx.x, e = blockIdx.x;
    for (int k = tid; k < C * C; k += RT_THREADS) s_conf[k] = 0;
    if (tid < FS_MAXC) s_n[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const int32_t* pe = pred + (int64_t)e * nq;
    for (int i = tid; i < nq; i += RT_THREADS) {
        const int64_t y = labels[i];
        const int p = pe[i];
        const bool yok = y >= 0 && y < C;
        if (yok) atomicAdd(&s_n[(int)y], 1);
        if (yok && p >= 0 && p < C) atomicAdd(&s_conf[(int)y * C + p], 1);
        else atomicAdd(&s_bad, 1);
    }
    __syncthreads();
    for (int k = tid; k < C * C; k += RT_THREADS) conf[(int64_t)e * C * C + k] = s_conf[k];
    if (tid < C) {
        int pr = 0;
        for (int y = 0; y < C; y++) pr += s_conf[y * C + tid];
        s_pr[tid] = pr;
        s_tp[tid] = s_conf[tid * C + tid];
    }
    __syncthreads();
    if (tid == 0) {
        bad[e] = s_bad;
        int64_t trace = 0, valid = 0;
        double bsum = 0.0, fsum = 0.0;
        int bcnt = 0, fcnt = 0;
        for (int c = 0; c < C; c++) {                     // class order
            trace += s_tp[c];
            valid += s_n[c];
            if (s_n[c] > 0) {
                bsum += (double)s_tp[c] / (double)s_n[c];
                bcnt++;
            }
            if (s_n[c] + s_pr[c] > 0) {
                fsum += 2.0 * (double)s_tp[c] / (double)(s_n[c] + s_pr[c]);
                fcnt++;
            }
        }
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        summary[3 * (int64_t)e + 0] = valid > 0 ? 100.0 * (double)trace / (double)valid : nan;
        summary[3 * (int64_t)e + 1] = bcnt > 0 ? 100.0 * (bsum / (double)bcnt) : nan;
        summary[3 * (int64_t)e + 2] = fcnt > 0 ? fsum / (double)fcnt : nan;
    }
}

// the limits every few-shot entry point shares; 0: fine
int fewshot_geometry(const char* who, int E, int C, int Cp, int D) {
    MH_REQUIRE(C >= 2 && C <= FS_MAXC, "%s: C = %d outside [2, %d]", who, C, FS_MAXC);
    MH_REQUIRE(Cp >= C && Cp <= FS_MAXC && (Cp & (Cp - 1)) == 0 && Cp < 2 * C,
               "%s: Cp = %d is not the next power of two >= C = %d", who, Cp, C);
    MH_REQUIRE(D >= 1 && D <= FS_MAXD, "%s: D = %d outside [1, %d]", who, D, FS_MAXD);
    MH_REQUIRE(E >= 1 && (int64_t)E * Cp <= (1 << 20), "%s: E = %d episodes of Cp = %d keys outside [1, 2^20] keys", who, E, Cp);
    return MH_OK;
}

}  // namespace

extern "C" int64_t mh_colmean_workspace_bytes(int64_t n, int D) {
    if (n <= 0 || D <= 0) return 0;
    return (int64_t)colmean_parts(n) * D * (int64_t)sizeof(double);
}

extern "C" int mh_colmean(const float* x, int64_t n, int D, float* mu, void* workspace, mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_colmean: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(D >= 1 && D <= FS_MAXD, "mh_colmean: D = %d outside [1, %d]", D, FS_MAXD);
    MH_REQUIRE(x && mu && workspace, "mh_colmean: null pointer");
    MH_REQUIRE(((uintptr_t)workspace & 7) == 0, "mh_colmean: workspace must be 8-byte aligned");
    const int parts = colmean_parts(n);
    hipLaunchKernelGGL(colmean_part_kernel, dim3(mh_cdiv(D, RT_THREADS), parts), dim3(RT_THREADS), 0, (hipStream_t)s, x, n, D, parts,
                       (double*)workspace);
    MH_LAUNCH_CHECK("mh_colmean");
    hipLaunchKernelGGL(colmean_fold_kernel, dim3(mh_cdiv(D, RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)s, (const double*)workspace, n,
                       D, parts, mu);
    MH_LAUNCH_CHECK("mh_colmean");
    return MH_OK;
}

extern "C" int mh_center_l2norm(const float* x, const float* mu, float* y, int64_t n, int D, float eps, mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_center_l2norm: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(D >= 1 && D <= FS_MAXD, "mh_center_l2norm: D = %d outside [1, %d]", D, FS_MAXD);
    MH_REQUIRE(eps > 0.f && eps < INFINITY, "mh_center_l2norm: eps = %g must be positive and finite", (double)eps);
    MH_REQUIRE(x && mu && y, "mh_center_l2norm: null pointer");
    hipLaunchKernelGGL(center_l2norm_kernel, dim3(mh_cdiv(n, RT_THREADS / 64)), dim3(RT_THREADS), 0, (hipStream_t)s, x, mu, y, n, D, eps);
    MH_LAUNCH_CHECK("mh_center_l2norm");
    return MH_OK;
}

extern "C" int mh_fewshot_protos(const float* y, int64_t n, const int64_t* rows, const int64_t* perm, int E, int C, int Cp, int K, int D,
                                 int metric, float* protos, float* bias, mh_stream s) {
    if (int rc = fewshot_geometry("mh_fewshot_protos", E, C, Cp, D)) return rc;
    MH_REQUIRE(K >= 1 && K <= FS_MAXK, "mh_fewshot_protos: K = %d outside [1, %d]", K, FS_MAXK);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_fewshot_protos: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(metric == MH_FEWSHOT_EUCLIDEAN || metric == MH_FEWSHOT_COSINE, "mh_fewshot_protos: metric = %d", metric);
    MH_REQUIRE(y && rows && protos, "mh_fewshot_protos: null pointer");
    MH_REQUIRE((bias != nullptr) == (metric == MH_FEWSHOT_EUCLIDEAN), "mh_fewshot_protos: the bias goes with the euclidean metric only");
    MH_REQUIRE((((uintptr_t)rows | (uintptr_t)perm) & 7) == 0, "mh_fewshot_protos: rows and perm must be 8-byte aligned");
    hipLaunchKernelGGL(fewshot_protos_kernel, dim3((unsigned)E * (unsigned)Cp), dim3(RT_THREADS), 0, (hipStream_t)s, y, n, rows, perm, C, Cp,
                       K, D, metric == MH_FEWSHOT_COSINE ? 1 : 0, protos, bias);
    MH_LAUNCH_CHECK("mh_fewshot_protos");
    return MH_OK;
}

extern "C" int mh_fewshot_predict(const float* q, const float* protos, const float* bias, int64_t nq, int E, int C, int Cp, int D,
                                  int32_t* pred, mh_stream s) {
    if (int rc = fewshot_geometry("mh_fewshot_predict", E, C, Cp, D)) return rc;
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20), "mh_fewshot_predict: nq = %lld outside [1, 2^20]", (long long)nq);
    MH_REQUIRE(q && protos && pred, "mh_fewshot_predict: null pointer");
    const int nk = E * Cp;
    int cshift = 0;
    while ((1 << cshift) < Cp) cshift++;
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(protos, 4);
    hipLaunchKernelGGL(fewshot_predict_kernel, dim3(mh_cdiv(nq, RT_TILE), mh_cdiv(nk, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, q,
                       protos, bias, (int)nq, nk, D, C, cshift, vec, pred);
    MH_LAUNCH_CHECK("mh_fewshot_predict");
    return MH_OK;
}

extern "C" int mh_fewshot_tally(const int32_t* pred, const int64_t* labels, int64_t nq, int E, int C, int32_t* conf, int32_t* bad,
                                double* summary, mh_stream s) {
    MH_REQUIRE(C >= 2 && C <= FS_MAXC, "mh_fewshot_tally: C = %d outside [2, %d]", C, FS_MAXC);
    MH_REQUIRE(E >= 1 && E <= (1 << 20), "mh_fewshot_tally: E = %d outside [1, 2^20]", E);
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20), "mh_fewshot_tally: nq = %lld outside [1, 2^20]", (long long)nq);
    MH_REQUIRE(pred && labels && conf && bad && summary, "mh_fewshot_tally: null pointer");
    MH_REQUIRE((((uintptr_t)labels | (uintptr_t)summary) & 7) == 0, "mh_fewshot_tally: labels and summary must be 8-byte aligned");
    hipLaunchKernelGGL(fewshot_tally_kernel, dim3((unsigned)E), dim3(RT_THREADS), 0, (hipStream_t)s, pred, labels, (int)nq, C, conf, bad,
                       summary);
    MH_LAUNCH_CHECK("mh_fewshot_tally");
    return MH_OK;
}
