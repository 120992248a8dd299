// Cross-validated recursive gene elimination (mirror_amd/geneselect.py): J = folds + 1 one-vs-rest squared-hinge machines (LinearSVC's
// default loss) over the SAME standardised rows, the folds side by side as jobs, with a per-job mask of the features still in play.
// Nothing allocated, no host wait, no float atomics: every sum has a fixed order, so two runs agree bit for bit.
//
// Layout (mh_linprobe_*'s): Cp = the next power of two >= C; weights f32 [J x Cp x D], bias f32 [J x Cp]; no entry point here reads what
// a pad slot c >= C holds.  The weights of an eliminated feature are exactly 0, so the product needs no mask.
//
//   mh_colstats        mu and rstd per column: mh_colmean's strips of rows in f64, added in strip order, then a second pass over the
//                      centred values x - mu (f64) for the population variance; rstd = 0 where it is 0.
//   mh_standardize     y = (x - mu) rstd, elementwise; may write in place.
//   mh_gsel_rowsq      sum of y_id^2 over a job's active columns: one wave per row, a lane adds its columns d = lane, lane + 64, .. in that
//                      order, the lanes by the fixed butterfly of wave_sum (mh_center_l2norm's order).
//   mh_gsel_grad       two launches.  (1) retrieval_tile.h's exact-f32 128 x 128 product with the contraction cut into Z slices of ks
//                      columns (gs_product_range: retr_product over [kbeg, kend)); every slice is ONE k-ordered f32 fmaf chain from 0 and
//                      is STORED to workspace [Z x n x J Cp] from the accumulator registers.  (2) one thread per (row, job) adds the
//                      slices in slice order, then the bias, and forms the hinge, the logit gradient, the loss term and the class.
//   mh_gsel_eliminate  one workgroup per job: a radix select over the bits of the importances (four passes of 8 bits, LDS histograms),
//                      then one pass in index order that breaks the tie at the threshold by prefix counts and removes.
//
// mh_gsel_step lives in linprobe.hip: it is mh_linprobe_step's kernel with the mask as a template parameter.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int GS_MAXC = 64;
constexpr int GS_MAXD = 1 << 18;
constexpr int GS_MAXPARTS = 128;      // row strips of the column statistics: mh_colmean's partition
constexpr int GS_SLICE_MIN = 256;     // the shortest slice of the contraction worth a workgroup: 16 stages of the product
constexpr int GS_WG_TARGET = 768;     // 256 CUs x 3 resident workgroups (35 KB of LDS each)
constexpr int GS_MAXZ = 128;
constexpr int GS_JB = 16;             // jobs per workgroup of the fold
constexpr int GS_ET = 1024;           // threads of the elimination: 16 waves
constexpr int GS_EW = GS_ET / 64;

int gs_parts(int64_t n) {
    const int64_t p = (n + 63) / 64;                      // strips of at least 64 rows
    return (int)(p < 1 ? 1 : (p > GS_MAXPARTS ? GS_MAXPARTS : p));
}

// ------------------------------------------------------------------ column statistics
// strip `part` of column d: rows [part n / parts, (part + 1) n / parts) in row order, f64; mu NULL: the values, else the squares of x - mu
__global__ void __launch_bounds__(RT_THREADS) colstats_part_kernel(const float* __restrict__ x, const float* __restrict__ mu, int64_t n,
                                                                   int D, int parts, double* __restrict__ partial) {
    const int d = blockIdx.x * RT_THREADS + threadIdx.x, part = blockIdx.y;
    if (d >= D) return;
    const int64_t r0 = (int64_t)part * n / parts, r1 = (int64_t)(part + 1) * n / parts;
    double acc = 0.0;
    if (mu) {
        const double m = (double)mu[d];
        for (int64_t r = r0; r < r1; r++) {
            const double v = (double)x[r * D + d] - m;
            acc += v * v;
        }
    } else {
        for (int64_t r = r0; r < r1; r++) acc += (double)x[r * D + d];
    }
    partial[(int64_t)part * D + d] = acc;
}

// rstd 0: out[d] = the mean; rstd 1: out[d] = 1 / sqrt(the mean), 0 where the mean is not positive
__global__ void __launch_bounds__(RT_THREADS) colstats_fold_kernel(const double* __restrict__ partial, int64_t n, int D, int parts,
                                                                   int rstd, float* __restrict__ out) {
    const int d = blockIdx.x * RT_THREADS + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int p = 0; p < parts; p++) acc += partial[(int64_t)p * D + d];
    const double m = acc / (double)n;
    out[d] = rstd ? (m > 0.0 ? (float)(1.0 / sqrt(m)) : 0.f) : (float)m;
}

__global__ void __launch_bounds__(RT_THREADS) standardize_kernel(const float* x, const float* __restrict__ mu,
                                                                 const float* __restrict__ rstd, float* y, int64_t n, int D) {
    const int d = blockIdx.x * RT_THREADS + threadIdx.x;
    if (d >= D) return;
    const float m = mu[d], r = rstd[d];
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) y[row * D + d] = (x[row * D + d] - m) * r;
}

// one wave per row, every job of this grid row in turn
__global__ void __launch_bounds__(RT_THREADS) gsel_rowsq_kernel(const float* __restrict__ y, int64_t n, int D,
                                                                const uint8_t* __restrict__ mask, int J, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;                                 // wave-uniform, no block barrier below
    const float* yr = y + row * D;
    for (int j = blockIdx.y; j < J; j += gridDim.y) {
        const uint8_t* m = mask + (int64_t)j * D;
        float ss = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float v = yr[d];
            if (m[d]) ss = fmaf(v, v, ss);
        }
        ss = wave_sum(ss);
        if (lane == 0) out[(int64_t)j * n + row] = ss;
    }
}

// ------------------------------------------------------------------ the product over a range of the contraction
// retr_load with the columns cut at kend instead of D
__device__ __forceinline__ void gs_load(f4_t (&r)[RT_QUADS], const float* __restrict__ x, int n, int D, int row0, int k0, int kend, int vec,
                                        int tid) {
#pragma unroll
    for (int u = 0; u < RT_QUADS; u++) {
        const int c = tid + u * RT_THREADS;
        const int row = row0 + (c >> 2), kk = k0 + (c & 3) * 4;
        f4_t v = {0.f, 0.f, 0.f, 0.f};
        if (row < n) {
            const float* p = x + (int64_t)row * D + kk;
            if (vec && kk + 4 <= kend) {
                v = *reinterpret_cast<const f4_t*>(p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (kk + e < kend) v[e] = p[e];
            }
        }
        r[u] = v;
    }
}

// retr_product over the columns [kbeg, kend) of both operands (kbeg a multiple of 16, kend <= D): the same stages, the same fragment
// layout, the same accumulator layout; every element is ONE k-ordered f32 fmaf chain from 0 over that range.  Ends with a barrier.
__device__ __forceinline__ void gs_product_range(f32x16 (&acc)[2][2], const float* __restrict__ q, const float* __restrict__ k, int nq,
                                                 int nk, int D, int row0, int col0, int kbeg, int kend, int vec,
                                                 float (&s_a)[2][RT_TILE * RT_LD], float (&s_b)[2][RT_TILE * RT_LD]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nt = (kend - kbeg + RT_BK - 1) / RT_BK;
    f4_t ra[RT_QUADS], rb[RT_QUADS];
    gs_load(ra, q, nq, D, row0, kbeg, kend, vec, tid);
    gs_load(rb, k, nk, D, col0, kbeg, kend, vec, tid);
    retr_store(ra, s_a[0], tid);
    retr_store(rb, s_b[0], tid);
    if (nt > 1) {
        gs_load(ra, q, nq, D, row0, kbeg + RT_BK, kend, vec, tid);
        gs_load(rb, k, nk, D, col0, kbeg + RT_BK, kend, vec, tid);
    }
    __syncthreads();

    const int frag = (lane & 31) * RT_LD + (lane >> 5);
    for (int t = 0; t < nt; t++) {
        const int cur = t & 1;
        if (t + 1 < nt) {          // stage cur ^ 1 was last read before the barrier that ended step t - 1
            retr_store(ra, s_a[cur ^ 1], tid);
            retr_store(rb, s_b[cur ^ 1], tid);
            if (t + 2 < nt) {
                gs_load(ra, q, nq, D, row0, kbeg + (t + 2) * RT_BK, kend, vec, tid);
                gs_load(rb, k, nk, D, col0, kbeg + (t + 2) * RT_BK, kend, vec, tid);
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

// slice blockIdx.z of the tile (blockIdx.x, blockIdx.y) to part [Z x n x nk]; a lane owns one column: 32 consecutive floats per row
__global__ void __launch_bounds__(RT_THREADS, 3) gsel_partial_kernel(const float* __restrict__ y, const float* __restrict__ w, int n,
                                                                     int nk, int D, int ks, int vec, float* __restrict__ part) {
    __shared__ float s_a[2][RT_TILE * RT_LD];
    __shared__ float s_b[2][RT_TILE * RT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int kbeg = blockIdx.z * ks, kend = min(D, kbeg + ks);

    f32x16 acc[2][2];
    gs_product_range(acc, y, w, n, nk, D, row0, col0, kbeg, kend, vec, s_a, s_b);

    float* out = part + (int64_t)blockIdx.z * n * nk;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = row0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (row >= n) continue;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int col = col0 + wn * 64 + j * 32 + (lane & 31);
                if (col < nk) out[(int64_t)row * nk + col] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------ slices folded; hinge, logit gradient, loss, class
__global__ void __launch_bounds__(RT_THREADS) gsel_fold_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                               const int64_t* __restrict__ labels, const int32_t* __restrict__ fold,
                                                               const int32_t* __restrict__ heldout, const float* __restrict__ rscale,
                                                               int n, int nk, int J, int C, int cshift, int Z, float* __restrict__ G,
                                                               double* __restrict__ loss_part, int32_t* __restrict__ pred) {
    __shared__ float s_l[GS_JB][RT_TILE + 1];             // the loss term of (job, row): writers walk the jobs, readers the rows
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * RT_TILE, job0 = blockIdx.y * GS_JB;
    const int Cp = 1 << cshift;
    const int64_t zs = (int64_t)n * nk;
    for (int t = tid; t < RT_TILE * GS_JB; t += RT_THREADS) {
        const int jl = t & (GS_JB - 1), rl = t / GS_JB;
        const int row = row0 + rl, job = job0 + jl;
        float ls = 0.f;
        if (row < n && job < J) {
            const int64_t l64 = labels[row];
            const int f = fold[row];
            const bool train = l64 >= 0 && l64 < C && f >= 0 && f != heldout[job];
            const int lab = (int)l64;
            const float r2 = 2.f * rscale[job];
            const float* p = part + (int64_t)row * nk + (job << cshift);
            const float* b = bias + (job << cshift);
            float* g = G + (int64_t)row * nk + (job << cshift);
            int best = -1;
            float bv = 0.f;
            for (int c = 0; c < C; c++) {
                float v = p[c];
                for (int z = 1; z < Z; z++) v += p[z * zs + c];                 // slice order
                v += b[c];
                if (v == v && (best < 0 || v > bv)) {     // ascending, strict: ties to the smaller class; a NaN is not eligible
                    best = c;
                    bv = v;
                }
                float gc = 0.f;
                if (train) {
                    const bool own = c == lab;
                    const float m = own ? 1.f - v : 1.f + v;                    // 1 - t v, t = +1 for the row's class
                    if (!(m <= 0.f)) {                    // the hinge is active, or NaN: a NaN stays
                        ls = fmaf(m, m, ls);
                        gc = own ? -(r2 * m) : r2 * m;
                    }
                }
                g[c] = gc;
            }
            for (int c = C; c < Cp; c++) g[c] = 0.f;
            if (pred) pred[(int64_t)job * n + row] = best;
        }
        s_l[jl][rl] = ls;
    }
    if (!loss_part) return;
    __syncthreads();
    if (tid < GS_JB && job0 + tid < J) {
        double s = 0.0;
        for (int rl = 0; rl < RT_TILE; rl++) s += (double)s_l[tid][rl];         // row order
        loss_part[(int64_t)blockIdx.x * J + job0 + tid] = (double)rscale[job0 + tid] * s;
    }
}

// ------------------------------------------------------------------ elimination
// imp_d of job weights W [Cp x D]: the fmaf chain from 0 of the squares in class order
__device__ __forceinline__ float gs_imp(const float* W, int C, int D, int d) {
    float a = 0.f;
    for (int c = 0; c < C; c++) {
        const float w = W[(int64_t)c * D + d];
        a = fmaf(w, w, a);
    }
    return a;
}

__global__ void __launch_bounds__(GS_ET) gsel_eliminate_kernel(float* Wx, float* Wz, uint8_t* mask, int32_t* elim_round, int C, int Cp,
                                                               int D, int k, int round, float* importance) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_wave[GS_EW];
    __shared__ unsigned s_active, s_prefix, s_need;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j = blockIdx.x;
    float* Wxj = Wx + j * Cp * D;
    float* Wzj = Wz + j * Cp * D;
    uint8_t* m = mask + j * D;

    if (tid == 0) s_active = 0u;
    __syncthreads();
    unsigned cnt = 0u;
    for (int d = tid; d < D; d += GS_ET) {
        const bool a = m[d] != 0;
        cnt += a ? 1u : 0u;
        if (importance) importance[j * D + d] = a ? gs_imp(Wxj, C, D, d) : 0.f;
    }
    if (cnt) atomicAdd(&s_active, cnt);
    __syncthreads();
    const unsigned active = s_active;
    const unsigned kk = (unsigned)k < active ? (unsigned)k : active;
    if (kk == 0u) return;                                 // the same for the whole workgroup
    const bool all = kk == active;

    // the threshold T: fewer than kk active keys lie below it, at least kk at or below it; `need` of the keys equal to T go
    unsigned prefix = 0u, need = kk;
    if (!all) {
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) s_hist[tid] = 0u;
            __syncthreads();
            for (int d = tid; d < D; d += GS_ET) {
                if (!m[d]) continue;
                const unsigned key = __float_as_uint(gs_imp(Wxj, C, D, d));
                if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0u, b = 0u;
                for (; b < 255u; b++) {                   // the matching keys number at least `need`: the walk ends inside the table
                    const unsigned h = s_hist[b];
                    if (cum + h >= need) break;
                    cum += h;
                }
                s_prefix = prefix | (b << shift);
                s_need = need - cum;
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
            __syncthreads();                              // the next pass clears the table and rewrites both
        }
    }
    const unsigned T = prefix;

    // index order: chunk by chunk, the keys equal to T counted by ballot inside a wave, the waves and the chunks before it added in order
    unsigned base = 0u;
    for (int d0 = 0; d0 < D; d0 += GS_ET) {
        const int d = d0 + tid;
        const bool a = d < D && m[d] != 0;
        const unsigned key = a ? __float_as_uint(gs_imp(Wxj, C, D, d)) : 0u;
        const bool tie = a && !all && key == T;
        const unsigned long long bal = __ballot(tie);
        const unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned off = base, total = 0u;
        for (int w = 0; w < GS_EW; w++) {
            const unsigned c = s_wave[w];
            if (w < wave) off += c;
            total += c;
        }
        if (a && (all || key < T || (tie && off + before < need))) {
            m[d] = 0;
            elim_round[j * D + d] = round;
            for (int c = 0; c < C; c++) {
                Wxj[(int64_t)c * D + d] = 0.f;
                Wzj[(int64_t)c * D + d] = 0.f;
            }
        }
        base += total;
        __syncthreads();                                  // the next chunk rewrites the wave counts
    }
}

// the limits the gsel entry points share; 0: fine
int gsel_geometry(const char* who, int64_t n, int D, int J, int C, int Cp) {
    MH_REQUIRE(C >= 2 && C <= GS_MAXC, "%s: C = %d outside [2, %d]", who, C, GS_MAXC);
    MH_REQUIRE(Cp >= C && Cp <= GS_MAXC && (Cp & (Cp - 1)) == 0 && Cp < 2 * C, "%s: Cp = %d is not the next power of two >= C = %d", who,
               Cp, C);
    MH_REQUIRE(D >= 1 && D <= GS_MAXD, "%s: D = %d outside [1, 2^18]", who, D);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %lld outside [1, 2^20]", who, (long long)n);
    MH_REQUIRE(J >= 1 && (int64_t)J * Cp <= (1 << 20), "%s: J = %d jobs of Cp = %d keys outside [1, 2^20] keys", who, J, Cp);
    MH_REQUIRE(n * J * Cp <= (1ll << 28), "%s: n J Cp = %lld x %d x %d logit gradients, 2^28 at the most", who, (long long)n, J, Cp);
    return MH_OK;
}

int gs_shift(int Cp) {
    int s = 0;
    while ((1 << s) < Cp) s++;
    return s;
}

// (Z, ks): the slices of the contraction and their length, from the shape alone
void gs_slices(int64_t n, int64_t nk, int D, int* Z, int* ks) {
    const int64_t tiles = ((n + RT_TILE - 1) / RT_TILE) * ((nk + RT_TILE - 1) / RT_TILE);
    int64_t zmax = GS_WG_TARGET / tiles;
    zmax = zmax < 1 ? 1 : (zmax > GS_MAXZ ? GS_MAXZ : zmax);
    int64_t z0 = (D + GS_SLICE_MIN - 1) / GS_SLICE_MIN;
    z0 = z0 > zmax ? zmax : z0;
    const int len = (int)(((D + z0 - 1) / z0 + RT_BK - 1) / RT_BK * RT_BK);
    *ks = len;
    *Z = (D + len - 1) / len;
}

}  // namespace

extern "C" int64_t mh_colstats_workspace_bytes(int64_t n, int D) {
    if (n <= 0 || D <= 0) return 0;
    return (int64_t)gs_parts(n) * D * (int64_t)sizeof(double);
}

extern "C" int mh_colstats(const float* x, int64_t n, int D, float* mu, float* rstd, void* workspace, mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_colstats: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(D >= 1 && D <= GS_MAXD, "mh_colstats: D = %d outside [1, 2^18]", D);
    MH_REQUIRE(x && mu && rstd && workspace, "mh_colstats: null pointer");
    MH_REQUIRE(((uintptr_t)workspace & 7) == 0, "mh_colstats: workspace must be 8-byte aligned");
    const int parts = gs_parts(n);
    const dim3 gp(mh_cdiv(D, RT_THREADS), parts), gf(mh_cdiv(D, RT_THREADS));
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(colstats_part_kernel, gp, dim3(RT_THREADS), 0, (hipStream_t)s, x, (const float*)nullptr, n, D, parts, ws);
    MH_LAUNCH_CHECK("mh_colstats");
    hipLaunchKernelGGL(colstats_fold_kernel, gf, dim3(RT_THREADS), 0, (hipStream_t)s, (const double*)ws, n, D, parts, 0, mu);
    MH_LAUNCH_CHECK("mh_colstats");
    hipLaunchKernelGGL(colstats_part_kernel, gp, dim3(RT_THREADS), 0, (hipStream_t)s, x, (const float*)mu, n, D, parts, ws);
    MH_LAUNCH_CHECK("mh_colstats");
    hipLaunchKernelGGL(colstats_fold_kernel, gf, dim3(RT_THREADS), 0, (hipStream_t)s, (const double*)ws, n, D, parts, 1, rstd);
    MH_LAUNCH_CHECK("mh_colstats");
    return MH_OK;
}

extern "C" int mh_standardize(const float* x, const float* mu, const float* rstd, float* y, int64_t n, int D, mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_standardize: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(D >= 1 && D <= GS_MAXD, "mh_standardize: D = %d outside [1, 2^18]", D);
    MH_REQUIRE(x && mu && rstd && y, "mh_standardize: null pointer");
    hipLaunchKernelGGL(standardize_kernel, dim3(mh_cdiv(D, RT_THREADS), (unsigned)(n < 4096 ? n : 4096)), dim3(RT_THREADS), 0,
                       (hipStream_t)s, x, mu, rstd, y, n, D);
    MH_LAUNCH_CHECK("mh_standardize");
    return MH_OK;
}

extern "C" int mh_gsel_rowsq(const float* y, int64_t n, int D, const uint8_t* mask, int J, float* out, mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "mh_gsel_rowsq: n = %lld outside [1, 2^20]", (long long)n);
    MH_REQUIRE(D >= 1 && D <= GS_MAXD, "mh_gsel_rowsq: D = %d outside [1, 2^18]", D);
    MH_REQUIRE(J >= 1 && J <= (1 << 19) && n * J <= (1ll << 28), "mh_gsel_rowsq: J = %d jobs over n = %lld rows (J <= 2^19, n J <= 2^28)", J,
               (long long)n);
    MH_REQUIRE(y && mask && out, "mh_gsel_rowsq: null pointer");
    hipLaunchKernelGGL(gsel_rowsq_kernel, dim3(mh_cdiv(n, RT_THREADS / 64), J < 1024 ? J : 1024), dim3(RT_THREADS), 0, (hipStream_t)s, y, n,
                       D, mask, J, out);
    MH_LAUNCH_CHECK("mh_gsel_rowsq");
    return MH_OK;
}

extern "C" int mh_gsel_slices(int64_t n, int nk, int D) {
    if (n < 1 || n > (1 << 20) || nk < 1 || nk > (1 << 20) || D < 1 || D > GS_MAXD) return 0;
    int Z, ks;
    gs_slices(n, nk, D, &Z, &ks);
    return Z;
}

extern "C" int64_t mh_gsel_grad_workspace_bytes(int64_t n, int J, int Cp, int D) {
    if (n < 1 || n > (1 << 20) || J < 1 || Cp < 1 || (int64_t)J * Cp > (1 << 20) || D < 1 || D > GS_MAXD) return 0;
    int Z, ks;
    gs_slices(n, (int64_t)J * Cp, D, &Z, &ks);
    return (int64_t)Z * n * J * Cp * (int64_t)sizeof(float);
}

extern "C" int mh_gsel_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* labels, const int32_t* fold,
                            const int32_t* heldout, const float* rscale, int J, int C, int Cp, float* G, double* loss_part, int32_t* pred,
                            void* workspace, mh_stream s) {
    if (int rc = gsel_geometry("mh_gsel_grad", n, D, J, C, Cp)) return rc;
    MH_REQUIRE(y && Wz && bz && labels && fold && heldout && rscale && G && workspace, "mh_gsel_grad: null pointer");
    MH_REQUIRE((((uintptr_t)labels | (uintptr_t)loss_part) & 7) == 0, "mh_gsel_grad: labels and loss_part must be 8-byte aligned");
    MH_REQUIRE(((uintptr_t)workspace & 3) == 0, "mh_gsel_grad: workspace must be 4-byte aligned");
    const int nk = J * Cp;
    int Z, ks;
    gs_slices(n, nk, D, &Z, &ks);
    const int vec = D % 4 == 0 && mh_quad_ok(y, 4) && mh_quad_ok(Wz, 4);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(gsel_partial_kernel, dim3(mh_cdiv(n, RT_TILE), mh_cdiv(nk, RT_TILE), Z), dim3(RT_THREADS), 0, (hipStream_t)s, y, Wz,
                       (int)n, nk, D, ks, vec, part);
    MH_LAUNCH_CHECK("mh_gsel_grad");
    hipLaunchKernelGGL(gsel_fold_kernel, dim3(mh_cdiv(n, RT_TILE), mh_cdiv(J, GS_JB)), dim3(RT_THREADS), 0, (hipStream_t)s,
                       (const float*)part, bz, labels, fold, heldout, rscale, (int)n, nk, J, C, gs_shift(Cp), Z, G, loss_part, pred);
    MH_LAUNCH_CHECK("mh_gsel_grad");
    return MH_OK;
}

extern "C" int mh_gsel_eliminate(float* Wx, float* Wz, uint8_t* mask, int32_t* elim_round, int J, int C, int Cp, int D, int k, int round,
                                 float* importance, mh_stream s) {
    if (int rc = gsel_geometry("mh_gsel_eliminate", 1, D, J, C, Cp)) return rc;
    MH_REQUIRE(k >= 0, "mh_gsel_eliminate: k = %d is negative", k);
    MH_REQUIRE(round >= 0, "mh_gsel_eliminate: round = %d is negative (-1 marks a feature still in play)", round);
    MH_REQUIRE(Wx && Wz && mask && elim_round, "mh_gsel_eliminate: null pointer");
    if (k == 0 && !importance) return MH_OK;
    hipLaunchKernelGGL(gsel_eliminate_kernel, dim3(J), dim3(GS_ET), 0, (hipStream_t)s, Wx, Wz, mask, elim_round, C, Cp, D, k, round,
                       importance);
    MH_LAUNCH_CHECK("mh_gsel_eliminate");
    return MH_OK;
}
