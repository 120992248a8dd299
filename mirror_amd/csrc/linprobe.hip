// Linear probe of frozen embeddings (mirror_amd/linprobe.py): J = (folds + 1) x strengths independent L2-regularised softmax
// regressions over the SAME prepared rows, one full-batch FISTA iteration = two launches on the caller's stream.  Nothing allocated, no
// host wait, no float atomics: every sum has a fixed order, so two runs agree bit for bit.
//
// Layout (mh_fewshot_protos's): Cp = the next power of two >= C; weights f32 [J x Cp x D], bias f32 [J x Cp]; pad slots c >= C hold
// weight 0 and bias -inf, so a job's Cp keys never straddle a 128-key tile.
//
//   mh_linprobe_grad   the J Cp weight rows of the look-ahead point Z are the keys of retrieval_tile.h's exact-f32 128 x 128 product;
//                      the epilogue is mh_fewshot_predict's: the tile goes through LDS 64 rows at a time and one thread owns each
//                      (row, job): bias added, the maximum, lse = max + logf(sum expf(v - max)) in class order in f32, and the
//                      logit gradient r_j (p_c - [c = label]) written back over the logits in LDS (0 for rows outside train_j and for
//                      pad columns); the half tile is then stored to G [n x J Cp] with 128 consecutive floats per row.  CE of every
//                      (row, job) goes to a second LDS table; one thread per job adds them in row order in f64.
//   mh_linprobe_step   dW = G^T y + lambda Wz and db = G^T 1 as ONE product contracted over the rows: a workgroup of 4 waves (2 x 2)
//                      owns a 128 (key) x 128 (column) tile of [J Cp x (D + 1)], each wave 2 x 2 accumulators of 32 x 32
//                      (v_mfma_f32_32x32x2_f32), and walks rows 0 .. n - 1 in ascending order through a double-buffered LDS stage
//                      of 16 rows (rows past n zero-filled: fmaf(0, 0, acc) = acc).  Every element is ONE row-ordered f32 fmaf chain
//                      from 0; column D of the right operand is a column of ones formed in the load.  The epilogue runs from the
//                      accumulator registers (a lane owns one column: 32 lanes write 32 consecutive floats of one weight row):
//                          g  = fmaf(lambda_j, Wz, acc)        (bias: g = acc, it is not penalised)
//                          X' = fmaf(-eta_j, g, Wz)
//                          Z' = fmaf(beta, X' - X, X')
//                      stored over Wx / Wz (bx / bz) in place: every element has exactly one owner, and the main loop reads G and y
//                      only.  Pad slots are skipped outright (-inf - (-inf) = NaN).  max |g| per key row by integer LDS max on the
//                      bits of |g| (order-free; a NaN is larger than every number and survives), then per job of the tile.
//                      No split over n: J Cp = 160, D = 512 is 2 x 5 workgroups.
//   mh_linprobe_proba  the product and the per-(row, job) softmax of mh_linprobe_grad (lp_spill_half, lp_lse, lp_prob: the same
//                      device functions, so the same bits) over query rows: p_c = expf(v_c - lse) is what the half tile keeps, and it
//                      is stored to P [E x nq x C] WITHOUT the pad columns, job by job, 64 C consecutive floats per job of the key
//                      tile.  lse - v_label of the rows with a label in [0, C) goes through the CE table to nll_part as the loss does.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int LP_MAXC = 64;
constexpr int LP_MAXD = 4096;
constexpr int LP_HALF = RT_TILE / 2;  // rows per pass of the grad epilogue
constexpr int LP_LDT = RT_TILE + 1;   // LDS row stride of the spilled half tile (fewshot.hip says why 129)
constexpr int LP_LDC = LP_HALF + 1;   // stride of the CE table [run][row]: writers walk the rows, readers the runs
constexpr int LP_BK = 16;             // rows per LDS stage of the step kernel: 8 MFMAs of k = 2
constexpr int LP_LD = RT_TILE + 32;   // its LDS row stride: the two k of one MFMA step lie 160 floats = 32 banks apart
constexpr int LP_QUADS = LP_BK * RT_TILE / 4 / RT_THREADS;

// ------------------------------------------------------------------ logits, softmax, logit gradient
// rows [pass 64, pass 64 + 64) of the 128 x 128 accumulator tile to s_t [64][LP_LDT]: the two waves with wm == pass own them
__device__ __forceinline__ void lp_spill_half(const f32x16 (&acc)[2][2], float* __restrict__ s_t, int pass, int wm, int wn, int half,
                                              int lane) {
    if (wm != pass) return;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                s_t[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * LP_LDT + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
}

// one (row, job): v_c = sc[c] + sb[c] stored back over sc, c < C (pads are never looked at); returns lse = m + logf(sum_c expf(v_c - m)),
// m = max_c v_c, in class order in f32.  With lp_prob the ONE statement of the softmax that both kernels below use.
__device__ __forceinline__ float lp_lse(float* __restrict__ sc, const float* __restrict__ sb, int C) {
    float m = -INFINITY;
    for (int c = 0; c < C; c++) {
        const float v = sc[c] + sb[c];
        sc[c] = v;
        m = fmaxf(m, v);
    }
    float sum = 0.f;
    for (int c = 0; c < C; c++) sum += expf(sc[c] - m);
    return m + logf(sum);
}

__device__ __forceinline__ float lp_prob(float v, float lse) { return expf(v - lse); }

__global__ void __launch_bounds__(RT_THREADS, 3) linprobe_grad_kernel(const float* __restrict__ y, const float* __restrict__ w,
                                                                      const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ fold, const int32_t* __restrict__ heldout,
                                                                      const float* __restrict__ rscale, int n, int nk, int D, int C,
                                                                      int cshift, int vec, float* __restrict__ G,
                                                                      double* __restrict__ loss_part) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    __shared__ float s_ce[RT_TILE / 2 * LP_LDC];          // CE of (run, row) of the current half; at most 64 runs (Cp = 2)
    static_assert(LP_HALF * LP_LDT + RT_TILE <= 4 * RT_TILE * RT_LD, "half a tile and its biases must fit the stages");
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + LP_HALF * LP_LDT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Cp = 1 << cshift, J = nk >> cshift;
    const int runs = RT_TILE >> cshift;                   // jobs of this key tile

    f32x16 acc[2][2];
    retr_product(acc, y, w, n, nk, D, row0, col0, vec, s_a, s_b);       // ends with a barrier behind the last read of the stages

    if (tid < RT_TILE) s_bias[tid] = col0 + tid < nk ? bias[col0 + tid] : 0.f;
    const int tasks = LP_HALF * runs;
    double lsum = 0.0;                                    // thread `run` < runs: this row tile's CE of job col0 / Cp + run, in row order
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        lp_spill_half(acc, s_t, pass, wm, wn, half, lane);
        __syncthreads();
        for (int t = tid; t < tasks; t += RT_THREADS) {
            const int rl = t & (LP_HALF - 1), run = t >> 6;
            const int row = row0 + pass * LP_HALF + rl, job = (col0 >> cshift) + run;
            if (job >= J) continue;                       // nk = J Cp: a run lies inside the keys or outside them
            float* sc = s_t + rl * LP_LDT + run * Cp;
            float ce = 0.f;
            bool train = false;
            int lab = -1;
            float r = 0.f;
            if (row < n) {
                const int64_t l64 = labels[row];
                const int f = fold[row];
                train = l64 >= 0 && l64 < C && f >= 0 && f != heldout[job];
                lab = (int)l64;
                r = rscale[job];
            }
            if (train) {
                const float lse = lp_lse(sc, s_bias + run * Cp, C);
                ce = lse - sc[lab];
                for (int c = 0; c < C; c++) sc[c] = r * (lp_prob(sc[c], lse) - (c == lab ? 1.f : 0.f));
                for (int c = C; c < Cp; c++) sc[c] = 0.f;
            } else {
                for (int c = 0; c < Cp; c++) sc[c] = 0.f;
            }
            s_ce[run * LP_LDC + rl] = ce;
        }
        __syncthreads();
        for (int t = tid; t < LP_HALF * RT_TILE; t += RT_THREADS) {     // 128 consecutive floats of one row of G per half wave pair
            const int rl = t >> 7, c = t & (RT_TILE - 1);
            const int row = row0 + pass * LP_HALF + rl;
            if (row < n && col0 + c < nk) G[(int64_t)row * nk + col0 + c] = s_t[rl * LP_LDT + c];
        }
        if (loss_part && tid < runs && (col0 >> cshift) + tid < J) {
            for (int rl = 0; rl < LP_HALF; rl++) lsum += (double)s_ce[tid * LP_LDC + rl];
        }
        __syncthreads();                                  // the next pass overwrites the half tile and the CE table
    }
    if (loss_part && tid < runs && (col0 >> cshift) + tid < J) {
        const int job = (col0 >> cshift) + tid;
        loss_part[(int64_t)blockIdx.x * J + job] = (double)rscale[job] * lsum;
    }
}

// ------------------------------------------------------------------ class probabilities of query rows, and their log-loss
__global__ void __launch_bounds__(RT_THREADS, 3) linprobe_proba_kernel(const float* __restrict__ q, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                                       int n, int nk, int D, int C, int cshift, int vec,
                                                                       float* __restrict__ P, double* __restrict__ nll_part) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // as linprobe_grad_kernel: the stages, then the spilled half tile
    __shared__ float s_ce[RT_TILE / 2 * LP_LDC];          // lse - v_label of (run, row) of the current half
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + LP_HALF * LP_LDT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Cp = 1 << cshift, J = nk >> cshift;
    const int job0 = col0 >> cshift;
    const int runs = min(RT_TILE >> cshift, J - job0);    // jobs of this key tile: nk = J Cp, a run lies inside the keys or outside

    f32x16 acc[2][2];
    retr_product(acc, q, w, n, nk, D, row0, col0, vec, s_a, s_b);

    if (tid < RT_TILE) s_bias[tid] = col0 + tid < nk ? bias[col0 + tid] : 0.f;
    double lsum = 0.0;                                    // thread `run` < runs: this row tile's log-loss under job job0 + run, in row order
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        lp_spill_half(acc, s_t, pass, wm, wn, half, lane);
        __syncthreads();
        const int rbase = row0 + pass * LP_HALF;
        const int rows = min(LP_HALF, n - rbase);         // <= 0: this half lies past the last row
        for (int t = tid; t < LP_HALF * runs; t += RT_THREADS) {
            const int rl = t & (LP_HALF - 1), run = t >> 6;
            float* sc = s_t + rl * LP_LDT + run * Cp;
            float ce = 0.f;
            if (rl < rows) {
                const float lse = lp_lse(sc, s_bias + run * Cp, C);
                if (labels) {
                    const int64_t l64 = labels[rbase + rl];
                    if (l64 >= 0 && l64 < C) ce = lse - sc[(int)l64];
                }
                for (int c = 0; c < C; c++) sc[c] = lp_prob(sc[c], lse);
            }
            s_ce[run * LP_LDC + rl] = ce;
        }
        __syncthreads();
        const int per = rows * C;                         // job by job: rows x C consecutive floats of P [E x n x C]
        for (int run = 0; run < runs && per > 0; run++) {
            float* dst = P + ((int64_t)(job0 + run) * n + rbase) * C;
            for (int t = tid; t < per; t += RT_THREADS) {
                const int rl = t / C, c = t - rl * C;
                dst[t] = s_t[rl * LP_LDT + run * Cp + c];
            }
        }
        if (nll_part && tid < runs) {
            for (int rl = 0; rl < LP_HALF; rl++) lsum += (double)s_ce[tid * LP_LDC + rl];
        }
        __syncthreads();                                  // the next pass overwrites the half tile and the CE table
    }
    if (nll_part && tid < runs) nll_part[(int64_t)blockIdx.x * J + job0 + tid] = lsum;
}

// ------------------------------------------------------------------ weight gradient and the FISTA update
// this thread's pieces of rows [i0, i0 + LP_BK) x columns [c0, c0 + 128) of src [nrows x ncols]; zero outside, 1 at column `ones`
__device__ __forceinline__ void lp_load(f4_t (&r)[LP_QUADS], const float* __restrict__ src, int nrows, int ncols, int i0, int c0, int vec,
                                        int ones, int tid) {
#pragma unroll
    for (int u = 0; u < LP_QUADS; u++) {
        const int q = tid + u * RT_THREADS;
        const int row = i0 + (q >> 5), col = c0 + (q & 31) * 4;
        f4_t v = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows) {
            const float* p = src + (int64_t)row * ncols + col;
            if (vec && col + 4 <= ncols) {
                v = *reinterpret_cast<const f4_t*>(p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if (col + e < ncols) v[e] = p[e];
                    else if (col + e == ones) v[e] = 1.f;
                }
            }
        }
        r[u] = v;
    }
}

__device__ __forceinline__ void lp_store(const f4_t (&r)[LP_QUADS], float* __restrict__ tile, int tid) {
#pragma unroll
    for (int u = 0; u < LP_QUADS; u++) {
        const int q = tid + u * RT_THREADS;
        *reinterpret_cast<f4_t*>(tile + (q >> 5) * LP_LD + (q & 31) * 4) = r[u];
    }
}

// MASKED (mh_gsel_step): a (job, column) with mask[job, column] = 0 is neither read for the update nor written and takes no part in the
// maximum; fit_intercept = 0 does the same to the bias column.  MASKED = false is mh_linprobe_step: both arguments are unused.
// BIAS = false (mh_coxprobe_step: the partial likelihood has no intercept) leaves the bias column alone outright: bx and bz are never
// dereferenced and may be null.
template <bool MASKED, bool BIAS = true>
__global__ void __launch_bounds__(RT_THREADS, 2) linprobe_step_kernel(const float* __restrict__ y, const float* __restrict__ G,
                                                                      float* __restrict__ Wx, float* __restrict__ bx,
                                                                      float* __restrict__ Wz, float* __restrict__ bz,
                                                                      const float* __restrict__ lam, const float* __restrict__ eta,
                                                                      float beta, int n, int nk, int D, int C, int cshift, int vec_g,
                                                                      int vec_y, float* __restrict__ gmax_part,
                                                                      const uint8_t* __restrict__ mask, int fit_intercept) {
    __shared__ __attribute__((aligned(16))) float s_g[2][LP_BK * LP_LD];
    __shared__ __attribute__((aligned(16))) float s_y[2][LP_BK * LP_LD];
    __shared__ unsigned s_max[RT_TILE];                   // bits of max |g| per key row of the tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int key0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Cp = 1 << cshift, J = nk >> cshift;

    if (tid < RT_TILE) s_max[tid] = 0u;                   // read behind the barriers of the loop below

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nt = (n + LP_BK - 1) / LP_BK;
    f4_t rg[LP_QUADS], ry[LP_QUADS];
    lp_load(rg, G, n, nk, 0, key0, vec_g, -1, tid);
    lp_load(ry, y, n, D, 0, col0, vec_y, D, tid);
    lp_store(rg, s_g[0], tid);
    lp_store(ry, s_y[0], tid);
    if (nt > 1) {
        lp_load(rg, G, n, nk, LP_BK, key0, vec_g, -1, tid);
        lp_load(ry, y, n, D, LP_BK, col0, vec_y, D, tid);
    }
    __syncthreads();

    // lane l feeds A[key l & 31][row l >> 5] and B[row l >> 5][column l & 31] of each step of two rows
    const int frag = half * LP_LD + (lane & 31);
    for (int t = 0; t < nt; t++) {
        const int cur = t & 1;
        if (t + 1 < nt) {          // stage cur ^ 1 was last read before the barrier that ended step t - 1
            lp_store(rg, s_g[cur ^ 1], tid);
            lp_store(ry, s_y[cur ^ 1], tid);
            if (t + 2 < nt) {
                lp_load(rg, G, n, nk, (t + 2) * LP_BK, key0, vec_g, -1, tid);
                lp_load(ry, y, n, D, (t + 2) * LP_BK, col0, vec_y, D, tid);
            }
        }
        const float* at = s_g[cur] + wm * 64 + frag;
        const float* bt = s_y[cur] + wn * 64 + frag;
#pragma unroll
        for (int s = 0; s < LP_BK / 2; s++) {
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; i++) af[i] = at[2 * s * LP_LD + i * 32];
#pragma unroll
            for (int j = 0; j < 2; j++) bf[j] = bt[2 * s * LP_LD + j * 32];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // accumulator register r of block (i, j): tile key wm 64 + i 32 + (r & 3) + 8 (r >> 2) + 4 half, tile column wn 64 + j 32 + (l & 31)
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int key = key0 + kl;
            if (key >= nk || (key & (Cp - 1)) >= C) continue;           // outside the keys, or a pad slot: untouched
            const int job = key >> cshift;
            const float e = eta[job], l = lam[job];
            unsigned gm = 0u;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int col = col0 + wn * 64 + j * 32 + (lane & 31);
                if (col > D) continue;
                const bool isb = col == D;
                if (!BIAS && isb) continue;
                if (MASKED && (isb ? !fit_intercept : !mask[(int64_t)job * D + col])) continue;
                float* px = isb ? bx + key : Wx + (int64_t)key * D + col;
                float* pz = isb ? bz + key : Wz + (int64_t)key * D + col;
                const float z = *pz, x = *px;
                const float g = isb ? acc[i][j][r] : fmaf(l, z, acc[i][j][r]);
                const float xn = fmaf(-e, g, z);
                *px = xn;
                *pz = fmaf(beta, xn - x, xn);
                const unsigned gb = __float_as_uint(fabsf(g));
                gm = gb > gm ? gb : gm;
            }
            if (gmax_part) atomicMax(&s_max[kl], gm);
        }
    }
    if (gmax_part) {
        __syncthreads();
        const int job = (key0 >> cshift) + tid;
        if (tid < (RT_TILE >> cshift) && job < J) {
            unsigned m = 0u;
            for (int c = 0; c < C; c++) {
                const unsigned v = s_max[tid * Cp + c];
                m = v > m ? v : m;
            }
            gmax_part[(int64_t)blockIdx.y * J + job] = __uint_as_float(m);
        }
    }
}

// the limits both entry points share; 0: fine
int linprobe_geometry(const char* who, int64_t n, int D, int J, int C, int Cp, int maxd = LP_MAXD) {
    MH_REQUIRE(C >= 2 && C <= LP_MAXC, "%s: C = %d outside [2, %d]", who, C, LP_MAXC);
    MH_REQUIRE(Cp >= C && Cp <= LP_MAXC && (Cp & (Cp - 1)) == 0 && Cp < 2 * C, "%s: Cp = %d is not the next power of two >= C = %d", who,
               Cp, C);
    MH_REQUIRE(D >= 1 && D <= maxd, "%s: D = %d outside [1, %d]", who, D, maxd);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %lld outside [1, 2^20]", who, (long long)n);
    MH_REQUIRE(J >= 1 && (int64_t)J * Cp <= (1 << 20), "%s: J = %d jobs of Cp = %d keys outside [1, 2^20] keys", who, J, Cp);
    MH_REQUIRE(n * J * Cp <= (1ll << 28), "%s: n J Cp = %lld x %d x %d logit gradients, 2^28 at the most", who, (long long)n, J, Cp);
    return MH_OK;
}

int lp_shift(int Cp) {
    int s = 0;
    while ((1 << s) < Cp) s++;
    return s;
}

}  // namespace

extern "C" int mh_linprobe_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* labels,
                                const int32_t* fold, const int32_t* heldout, const float* rscale, int J, int C, int Cp, float* G,
                                double* loss_part, mh_stream s) {
    if (int rc = linprobe_geometry("mh_linprobe_grad", n, D, J, C, Cp)) return rc;
    MH_REQUIRE(y && Wz && bz && labels && fold && heldout && rscale && G, "mh_linprobe_grad: null pointer");
    MH_REQUIRE((((uintptr_t)labels | (uintptr_t)loss_part) & 7) == 0, "mh_linprobe_grad: labels and loss_part must be 8-byte aligned");
    const int nk = J * Cp;
    const int vec = D % 4 == 0 && mh_quad_ok(y, 4) && mh_quad_ok(Wz, 4);
    hipLaunchKernelGGL(linprobe_grad_kernel, dim3(mh_cdiv(n, RT_TILE), mh_cdiv(nk, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, y, Wz, bz,
                       labels, fold, heldout, rscale, (int)n, nk, D, C, lp_shift(Cp), vec, G, loss_part);
    MH_LAUNCH_CHECK("mh_linprobe_grad");
    return MH_OK;
}

extern "C" int mh_linprobe_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* bx, float* Wz, float* bz,
                                const float* lam, const float* eta, float beta, int J, int C, int Cp, float* gmax_part, mh_stream s) {
    if (int rc = linprobe_geometry("mh_linprobe_step", n, D, J, C, Cp)) return rc;
    MH_REQUIRE(beta >= 0.f && beta <= 1.f, "mh_linprobe_step: beta = %g outside [0, 1]", (double)beta);
    MH_REQUIRE(y && G && Wx && bx && Wz && bz && lam && eta, "mh_linprobe_step: null pointer");
    const int nk = J * Cp;
    const int vec_g = nk % 4 == 0 && mh_quad_ok(G, 4);
    const int vec_y = D % 4 == 0 && mh_quad_ok(y, 4);
    hipLaunchKernelGGL(linprobe_step_kernel<false>, dim3(mh_cdiv(nk, RT_TILE), mh_cdiv(D + 1, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s,
                       y, G, Wx, bx, Wz, bz, lam, eta, beta, (int)n, nk, D, C, lp_shift(Cp), vec_g, vec_y, gmax_part,
                       (const uint8_t*)nullptr, 1);
    MH_LAUNCH_CHECK("mh_linprobe_step");
    return MH_OK;
}

// geneselect.hip's step: the kernel above with the mask, at that file's limits (D up to 2^18)
extern "C" int mh_gsel_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* bx, float* Wz, float* bz, const float* lam,
                            const float* eta, float beta, const uint8_t* mask, int fit_intercept, int J, int C, int Cp, float* gmax_part,
                            mh_stream s) {
    if (int rc = linprobe_geometry("mh_gsel_step", n, D, J, C, Cp, 1 << 18)) return rc;
    MH_REQUIRE(beta >= 0.f && beta <= 1.f, "mh_gsel_step: beta = %g outside [0, 1]", (double)beta);
    MH_REQUIRE(fit_intercept == 0 || fit_intercept == 1, "mh_gsel_step: fit_intercept = %d is neither 0 nor 1", fit_intercept);
    MH_REQUIRE(y && G && Wx && bx && Wz && bz && lam && eta && mask, "mh_gsel_step: null pointer");
    const int nk = J * Cp;
    const int vec_g = nk % 4 == 0 && mh_quad_ok(G, 4);
    const int vec_y = D % 4 == 0 && mh_quad_ok(y, 4);
    hipLaunchKernelGGL(linprobe_step_kernel<true>, dim3(mh_cdiv(nk, RT_TILE), mh_cdiv(D + 1, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s,
                       y, G, Wx, bx, Wz, bz, lam, eta, beta, (int)n, nk, D, C, lp_shift(Cp), vec_g, vec_y, gmax_part, mask, fit_intercept);
    MH_LAUNCH_CHECK("mh_gsel_step");
    return MH_OK;
}

// coxprobe.hip's step: the kernel above with one key per job (C = Cp = 1: `key & (Cp - 1)` is 0, the per-job maximum runs over one key)
// and no bias column, at that file's limits
extern "C" int mh_coxprobe_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* Wz, const float* lam, const float* eta,
                                float beta, int J, float* gmax_part, mh_stream s) {
    MH_REQUIRE(D >= 1 && D <= LP_MAXD, "mh_coxprobe_step: D = %d outside [1, %d]", D, LP_MAXD);
    MH_REQUIRE(n >= 1 && n <= 65536, "mh_coxprobe_step: n = %lld outside [1, 65536]", (long long)n);
    MH_REQUIRE(J >= 1 && n * J <= (1ll << 24), "mh_coxprobe_step: n J = %lld x %d score gradients outside [1, 2^24]", (long long)n, J);
    MH_REQUIRE(beta >= 0.f && beta <= 1.f, "mh_coxprobe_step: beta = %g outside [0, 1]", (double)beta);
    MH_REQUIRE(y && G && Wx && Wz && lam && eta, "mh_coxprobe_step: null pointer");
    const int vec_g = J % 4 == 0 && mh_quad_ok(G, 4);
    const int vec_y = D % 4 == 0 && mh_quad_ok(y, 4);
    hipLaunchKernelGGL((linprobe_step_kernel<false, false>), dim3(mh_cdiv(J, RT_TILE), mh_cdiv(D + 1, RT_TILE)), dim3(RT_THREADS), 0,
                       (hipStream_t)s, y, G, Wx, (float*)nullptr, Wz, (float*)nullptr, lam, eta, beta, (int)n, J, D, 1, 0, vec_g, vec_y,
                       gmax_part, (const uint8_t*)nullptr, 0);
    MH_LAUNCH_CHECK("mh_coxprobe_step");
    return MH_OK;
}

extern "C" int mh_linprobe_proba(const float* q, int64_t nq, int D, const float* W, const float* b, int E, int C, int Cp,
                                 const int64_t* labels, float* P, double* nll_part, mh_stream s) {
    if (int rc = linprobe_geometry("mh_linprobe_proba", nq, D, E, C, Cp)) return rc;
    MH_REQUIRE(labels || !nll_part, "mh_linprobe_proba: nll_part needs labels");
    MH_REQUIRE(q && W && b && P, "mh_linprobe_proba: null pointer");
    MH_REQUIRE((((uintptr_t)labels | (uintptr_t)nll_part) & 7) == 0, "mh_linprobe_proba: labels and nll_part must be 8-byte aligned");
    const int nk = E * Cp;
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(W, 4);
    hipLaunchKernelGGL(linprobe_proba_kernel, dim3(mh_cdiv(nq, RT_TILE), mh_cdiv(nk, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, q, W, b,
                       labels, (int)nq, nk, D, C, lp_shift(Cp), vec, P, nll_part);
    MH_LAUNCH_CHECK("mh_linprobe_proba");
    return MH_OK;
}
