// Survival linear probe of frozen embeddings (mirror_amd/survprobe.py): J = (folds + 1) x strengths independent L2-regularised
// discrete-time hazard regressions over the SAME prepared rows.  The FISTA iteration is mh_survprobe_grad followed by mh_linprobe_step
// (linprobe.hip, unchanged, with M in the role of C); the held-out folds are scored from mh_survprobe_risk.  Nothing allocated, no host
// wait, no float atomics: every sum has a fixed order, so two runs agree bit for bit.
//
// Layout (mh_linprobe_*'s): Mp = the next power of two >= M; weights f32 [J x Mp x D], bias f32 [J x Mp]; a job's Mp keys never straddle
// a 128-key tile.  Neither kernel reads a pad slot t >= M of the weights' products or of the bias, so what the pads hold is free.
//
//   mh_survprobe_grad  the J Mp weight rows of the look-ahead point Z are the keys of retrieval_tile.h's exact-f32 128 x 128 product;
//                      the epilogue is mh_linprobe_grad's: the tile goes through LDS 64 rows at a time and one thread owns each
//                      (row, job).  For the bins t <= T_i of a training row: v = product + bias, e = expf(-|v|),
//                      softplus(v) = max(v, 0) + log1pf(e), sigmoid(v) = 1 / (1 + e) or e / (1 + e) by the sign of v; the logit
//                      gradient r_j w_i (sigmoid(v_t) - [t = T_i] e_i) is written back over the logit in LDS, exactly 0 for t > T_i,
//                      for pad columns and for rows outside train_j; the half tile is then stored to G [n x J Mp] with 128 consecutive
//                      floats per row.  w_i nll_i of every (row, job) goes to a second LDS table; one thread per job adds them in row
//                      order in f64.
//   mh_survprobe_risk  the same product with the S Mp weight rows of one fold's jobs as keys; the epilogue walks the M bins in order:
//                      surv *= sigmoid(-v_t), sum += surv, risk = -sum (mh_surv_risk's definition, no clamp).  The logits are never
//                      stored; risk is [S x nq], so the 64 lanes of a wave store 64 consecutive floats of one job.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int SP_MAXM = 64;
constexpr int SP_MAXD = 4096;
constexpr int SP_HALF = RT_TILE / 2;  // rows per pass of the epilogues
constexpr int SP_LDT = RT_TILE + 1;   // LDS row stride of the spilled half tile (fewshot.hip says why 129)
constexpr int SP_LDN = SP_HALF + 1;   // stride of the nll table [run][row]: writers walk the rows, readers the runs

// e = expf(-|v|) serves both: softplus(v) = max(v, 0) + log1pf(e) and sigmoid(v) = (v >= 0 ? 1 : e) / (1 + e); a NaN v gives NaN twice
__device__ __forceinline__ float sp_sigmoid(float v, float e) { return (v >= 0.f ? 1.f : e) / (1.f + e); }

// ------------------------------------------------------------------ logits, hazard NLL, logit gradient
__global__ void __launch_bounds__(RT_THREADS, 3) survprobe_grad_kernel(const float* __restrict__ y, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, const int64_t* __restrict__ bins,
                                                                       const uint8_t* __restrict__ event, const int32_t* __restrict__ fold,
                                                                       const int32_t* __restrict__ heldout,
                                                                       const float* __restrict__ rscale, float w_cens, int n, int nk, int D,
                                                                       int M, int mshift, int vec, float* __restrict__ G,
                                                                       double* __restrict__ loss_part) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    __shared__ float s_nll[RT_TILE / 2 * SP_LDN];         // w_i nll_i of (run, row) of the current half; at most 64 runs (Mp = 2)
    static_assert(SP_HALF * SP_LDT + RT_TILE <= 4 * RT_TILE * RT_LD, "half a tile and its biases must fit the stages");
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + SP_HALF * SP_LDT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Mp = 1 << mshift, J = nk >> mshift;
    const int runs = RT_TILE >> mshift;                   // jobs of this key tile

    f32x16 acc[2][2];
    retr_product(acc, y, w, n, nk, D, row0, col0, vec, s_a, s_b);       // ends with a barrier behind the last read of the stages

    if (tid < RT_TILE) s_bias[tid] = col0 + tid < nk ? bias[col0 + tid] : 0.f;
    const int tasks = SP_HALF * runs;
    double lsum = 0.0;                                    // thread `run` < runs: this row tile's loss of job col0 / Mp + run, in row order
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        s_t[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * SP_LDT + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
        }
        __syncthreads();
        for (int t = tid; t < tasks; t += RT_THREADS) {
            const int rl = t & (SP_HALF - 1), run = t >> 6;
            const int row = row0 + pass * SP_HALF + rl, job = (col0 >> mshift) + run;
            if (job >= J) continue;                       // nk = J Mp: a run lies inside the keys or outside them
            float* sc = s_t + rl * SP_LDT + run * Mp;
            float wnll = 0.f;
            int last = -1;                                // the bins 0 .. last carry a term; -1: the row does not train in this job
            float rw = 0.f, wi = 0.f, ev = 0.f;
            if (row < n) {
                const int64_t b64 = bins[row];
                const uint8_t e = event[row];
                const int f = fold[row];
                if (b64 >= 0 && b64 < M && e <= 1 && f >= 0 && f != heldout[job]) {
                    last = (int)b64;
                    ev = (float)e;
                    wi = e ? 1.f : w_cens;
                    rw = rscale[job] * wi;
                }
            }
            if (last >= 0) {
                const float* sb = s_bias + run * Mp;
                float nll = 0.f;
                for (int b = 0; b <= last; b++) {         // bin order; bins past T_i and pads are never looked at
                    const float v = sc[b] + sb[b];
                    const float tgt = b == last ? ev : 0.f;
                    const float e = expf(-fabsf(v));
                    nll += fmaxf(v, 0.f) + log1pf(e) - tgt * v;
                    sc[b] = rw * (sp_sigmoid(v, e) - tgt);
                }
                wnll = wi * nll;
            }
            for (int b = last + 1; b < Mp; b++) sc[b] = 0.f;
            s_nll[run * SP_LDN + rl] = wnll;
        }
        __syncthreads();
        for (int t = tid; t < SP_HALF * RT_TILE; t += RT_THREADS) {     // 128 consecutive floats of one row of G per half wave pair
            const int rl = t >> 7, c = t & (RT_TILE - 1);
            const int row = row0 + pass * SP_HALF + rl;
            if (row < n && col0 + c < nk) G[(int64_t)row * nk + col0 + c] = s_t[rl * SP_LDT + c];
        }
        if (loss_part && tid < runs && (col0 >> mshift) + tid < J) {
            for (int rl = 0; rl < SP_HALF; rl++) lsum += (double)s_nll[tid * SP_LDN + rl];
        }
        __syncthreads();                                  // the next pass overwrites the half tile and the nll table
    }
    if (loss_part && tid < runs && (col0 >> mshift) + tid < J) {
        const int job = (col0 >> mshift) + tid;
        loss_part[(int64_t)blockIdx.x * J + job] = (double)rscale[job] * lsum;
    }
}

// ------------------------------------------------------------------ risk of held-out rows
__global__ void __launch_bounds__(RT_THREADS, 3) survprobe_risk_kernel(const float* __restrict__ q, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, int nq, int nk, int D, int M,
                                                                       int mshift, int vec, float* __restrict__ risk) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    static_assert(SP_HALF * SP_LDT + RT_TILE <= 4 * RT_TILE * RT_LD, "half a tile and its biases must fit the stages");
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];
    float* s_bias = s_t + SP_HALF * SP_LDT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;
    const int Mp = 1 << mshift;

    f32x16 acc[2][2];
    retr_product(acc, q, w, nq, nk, D, row0, col0, vec, s_a, s_b);      // ends with a barrier behind the last read of the stages

    if (tid < RT_TILE) s_bias[tid] = col0 + tid < nk ? bias[col0 + tid] : 0.f;
    const int tasks = SP_HALF << (7 - mshift);            // 64 rows x (128 / Mp) runs
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        s_t[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * SP_LDT + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
        }
        __syncthreads();
        for (int t = tid; t < tasks; t += RT_THREADS) {
            const int rl = t & (SP_HALF - 1), run = t >> 6;
            const int row = row0 + pass * SP_HALF + rl, key0 = col0 + run * Mp;
            if (row >= nq || key0 >= nk) continue;        // nk = S Mp: a run lies inside the keys or outside them
            const float* sc = s_t + rl * SP_LDT + run * Mp;
            const float* sb = s_bias + run * Mp;
            float surv = 1.f, sum = 0.f;
            for (int b = 0; b < M; b++) {                 // bin order; pads are never looked at
                const float v = -(sc[b] + sb[b]);
                surv *= sp_sigmoid(v, expf(-fabsf(v)));   // 1 - hazard = sigmoid(-logit)
                sum += surv;
            }
            risk[(int64_t)(key0 >> mshift) * nq + row] = -sum;          // a wave: 64 consecutive rows of one job
        }
        __syncthreads();                                  // the next pass overwrites the half tile
    }
}

// the limits of mh_linprobe_grad / mh_linprobe_step with M in the role of C; 0: fine
int survprobe_geometry(const char* who, int64_t n, int D, int J, int M, int Mp) {
    MH_REQUIRE(M >= 2 && M <= SP_MAXM, "%s: M = %d outside [2, %d]", who, M, SP_MAXM);
    MH_REQUIRE(Mp >= M && Mp <= SP_MAXM && (Mp & (Mp - 1)) == 0 && Mp < 2 * M, "%s: Mp = %d is not the next power of two >= M = %d", who,
               Mp, M);
    MH_REQUIRE(D >= 1 && D <= SP_MAXD, "%s: D = %d outside [1, %d]", who, D, SP_MAXD);
    MH_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %lld outside [1, 2^20]", who, (long long)n);
    MH_REQUIRE(J >= 1 && (int64_t)J * Mp <= (1 << 20), "%s: J = %d jobs of Mp = %d keys outside [1, 2^20] keys", who, J, Mp);
    return MH_OK;
}

int sp_shift(int Mp) {
    int s = 0;
    while ((1 << s) < Mp) s++;
    return s;
}

}  // namespace

extern "C" int mh_survprobe_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* bins,
                                 const uint8_t* event, const int32_t* fold, const int32_t* heldout, const float* rscale, float w_cens,
                                 int J, int M, int Mp, float* G, double* loss_part, mh_stream s) {
    if (int rc = survprobe_geometry("mh_survprobe_grad", n, D, J, M, Mp)) return rc;
    MH_REQUIRE(n * J * Mp <= (1ll << 28), "mh_survprobe_grad: n J Mp = %lld x %d x %d logit gradients, 2^28 at the most", (long long)n, J,
               Mp);
    MH_REQUIRE(w_cens >= 0.f && w_cens <= 1.f, "mh_survprobe_grad: w_cens = %g outside [0, 1]", (double)w_cens);
    MH_REQUIRE(y && Wz && bz && bins && event && fold && heldout && rscale && G, "mh_survprobe_grad: null pointer");
    MH_REQUIRE((((uintptr_t)bins | (uintptr_t)loss_part) & 7) == 0, "mh_survprobe_grad: bins and loss_part must be 8-byte aligned");
    const int nk = J * Mp;
    const int vec = D % 4 == 0 && mh_quad_ok(y, 4) && mh_quad_ok(Wz, 4);
    hipLaunchKernelGGL(survprobe_grad_kernel, dim3(mh_cdiv(n, RT_TILE), mh_cdiv(nk, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, y, Wz,
                       bz, bins, event, fold, heldout, rscale, w_cens, (int)n, nk, D, M, sp_shift(Mp), vec, G, loss_part);
    MH_LAUNCH_CHECK("mh_survprobe_grad");
    return MH_OK;
}

extern "C" int mh_survprobe_risk(const float* q, int64_t nq, int D, const float* W, const float* b, int S, int M, int Mp, float* risk,
                                 mh_stream s) {
    if (int rc = survprobe_geometry("mh_survprobe_risk", nq, D, S, M, Mp)) return rc;
    MH_REQUIRE(q && W && b && risk, "mh_survprobe_risk: null pointer");
    const int nk = S * Mp;
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(W, 4);
    hipLaunchKernelGGL(survprobe_risk_kernel, dim3(mh_cdiv(nq, RT_TILE), mh_cdiv(nk, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, q, W, b,
                       (int)nq, nk, D, M, sp_shift(Mp), vec, risk);
    MH_LAUNCH_CHECK("mh_survprobe_risk");
    return MH_OK;
}
