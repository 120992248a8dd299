// Downstream survival step (train_survival.py): the discrete-time survival losses of losses/nll_surv.py and
// losses/cross_entropy_surv.py, their logit gradients, the validation risk score (train_survival.py:1431-1433) and the pair counts
// of the censored concordance index (train_survival.py:1460-1465).
//
// N (batch) and M (num_bins) are small here (16 x 4 at the survival template), so the losses run one lane per row and walk the M
// bins in the reference's order: every intermediate is formed as the reference's torch expression forms it (clamp of the
// sigmoid, log of 1 - h, cumprod left to right), so the results track torch's f32 rounding.  Sums over rows are one block's
// fixed-order reduction: bitwise reproducible, no atomics.  Nothing is allocated and nothing waits on the host (graph capturable).
#include "common.h"

namespace {

constexpr int SV_THREADS = 256;

__device__ __forceinline__ int64_t sv_time(const void* p, int dt, int64_t r) {
    return dt == MH_SV_I32 ? (int64_t)((const int32_t*)p)[r] : ((const int64_t*)p)[r];
}

// censoring[r] == 1 / == 0 as the reference compares it (`censoring == 1`, `censoring == 0`) for each storage dtype
__device__ __forceinline__ void sv_cens(const void* p, int dt, int64_t r, bool& is1, bool& is0) {
    switch (dt) {
        case MH_SV_U8: { const uint8_t v = ((const uint8_t*)p)[r]; is1 = v == 1; is0 = v == 0; break; }
        case MH_SV_I32: { const int32_t v = ((const int32_t*)p)[r]; is1 = v == 1; is0 = v == 0; break; }
        case MH_SV_I64: { const int64_t v = ((const int64_t*)p)[r]; is1 = v == 1; is0 = v == 0; break; }
        default: { const float v = ((const float*)p)[r]; is1 = v == 1.0f; is0 = v == 0.0f; break; }
    }
}

__device__ __forceinline__ float sv_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct SvArgs {
    const float* x; int64_t ld;
    const void* t; int dt_t;
    const void* c; int dt_c;
    int N, M, kind;
    float lo, hi, w_all, w_unc;
};

// loss of one row, exactly the reference's expression (NaN for a CE row whose uncensored target lies outside [0, M])
__device__ float sv_row_loss(const SvArgs& a, int r) {
    const float* x = a.x + (int64_t)r * a.ld;
    const int64_t T = sv_time(a.t, a.dt_t, r);
    bool unc, cen;
    sv_cens(a.c, a.dt_c, r, unc, cen);
    if (a.kind == MH_SURV_NLL) {
        // losses/nll_surv.py:37-94: masked sums of log h / log(1 - h) over the bins, alpha mix of the two per-sample losses
        float s_lt = 0.f, s_ev = 0.f, s_le = 0.f;
        for (int j = 0; j < a.M; j++) {
            const float h = fminf(fmaxf(sv_sigmoid(x[j]), a.lo), a.hi);
            const float l1mh = logf(1.0f - h);
            if (j < T) s_lt += l1mh;
            if (j == T) s_ev += logf(h);
            if (j <= T) s_le += l1mh;
        }
        const float unc_nll = -(s_lt + s_ev);
        const float nll = unc ? unc_nll : (cen ? -s_le : 0.f);
        return a.w_all * nll + a.w_unc * (unc ? unc_nll : 0.f);
    }
    // losses/cross_entropy_surv.py:46-105: categorical distribution over M + 1 outcomes, renormalised, -log of the target class
    const int64_t tgt = unc ? T : (int64_t)a.M;
    float S = 1.0f, psum = 0.f, pt = 0.f;
    for (int j = 0; j < a.M; j++) {
        const float h = fminf(fmaxf(sv_sigmoid(x[j]), a.lo), a.hi);
        const float p = h * S;
        S = S * (1.0f - h);
        psum += p;
        if (j == tgt) pt = p;
    }
    psum += S;
    if (tgt == a.M) pt = S;
    if (tgt < 0 || tgt > a.M) return __builtin_nanf("");
    const float chosen = fmaxf(pt / fmaxf(psum, a.lo), a.lo);
    return -logf(chosen);
}

__global__ void __launch_bounds__(SV_THREADS) surv_loss_fwd_kernel(SvArgs a, float coef, float* __restrict__ rows, float* __restrict__ out) {
    __shared__ float red[SV_THREADS / 64];
    float acc = 0.f;
    for (int r = threadIdx.x; r < a.N; r += SV_THREADS) {
        const float l = sv_row_loss(a, r);
        if (rows) rows[r] = l;
        acc += l;
    }
    const float tot = block_sum256(acc, red);
    if (out && threadIdx.x == 0) out[0] = coef * tot;
}

// dlogits of one row per lane.  The derivative of the reference's expression as written: the clamp of the sigmoid passes the
// gradient only where lo <= sigmoid(x) <= hi (torch's clamp backward), and CE differentiates through p / clamp(p_sum) and the
// clamp of the chosen probability.  dx (contiguous [N, M]) doubles as the row's scratch for the survival prefix S_j.
__global__ void __launch_bounds__(SV_THREADS) surv_loss_bwd_kernel(SvArgs a, const float* __restrict__ g, int g_per_row, float gcoef,
                                                                   float* __restrict__ dx) {
    const int r = blockIdx.x * SV_THREADS + threadIdx.x;
    if (r >= a.N) return;
    const float* x = a.x + (int64_t)r * a.ld;
    float* d = dx + (int64_t)r * a.M;
    const int64_t T = sv_time(a.t, a.dt_t, r);
    bool unc, cen;
    sv_cens(a.c, a.dt_c, r, unc, cen);
    const float u = gcoef * g[g_per_row ? r : 0];
    if (a.kind == MH_SURV_NLL) {
        // d loss / d nll: w_all + w_unc for an uncensored row, w_all for a censored one, 0 otherwise
        const float k = unc ? a.w_all + a.w_unc : (cen ? a.w_all : 0.f);
        const float gn = u * k;
        for (int j = 0; j < a.M; j++) {
            const float s = sv_sigmoid(x[j]);
            const float h = fminf(fmaxf(s, a.lo), a.hi);
            // -(d log h [event bin] + d log(1 - h) [survived bins]) / dh
            float gh = 0.f;
            if (unc && j == T) gh -= gn / h;
            if ((unc && j < T) || (cen && j <= T)) gh += gn / (1.0f - h);
            d[j] = (s >= a.lo && s <= a.hi) ? gh * (1.0f - s) * s : 0.f;
        }
        return;
    }
    const int64_t tgt = unc ? T : (int64_t)a.M;
    if (tgt < 0 || tgt > a.M) {
        for (int j = 0; j < a.M; j++) d[j] = __builtin_nanf("");
        return;
    }
    // forward sweep: S_j = prod_{i <= j} (1 - h_i) into d[j]; p_sum; p_t
    float S = 1.0f, psum = 0.f, pt = 0.f;
    for (int j = 0; j < a.M; j++) {
        const float h = fminf(fmaxf(sv_sigmoid(x[j]), a.lo), a.hi);
        const float p = h * S;
        S = S * (1.0f - h);
        d[j] = S;
        psum += p;
        if (j == tgt) pt = p;
    }
    psum += S;
    if (tgt == a.M) pt = S;
    const float ps = fmaxf(psum, a.lo);
    const float pd = pt / ps;
    // loss = -log(clamp(pd, lo)): gradient through the clamp only where pd >= lo; through clamp(p_sum, lo) only where p_sum >= lo
    const float gc = pd >= a.lo ? -u / fmaxf(pd, a.lo) : 0.f;
    const float gA = gc / ps;                                          // d / d p_t (the numerator)
    const float gB = psum >= a.lo ? -gc * pt / (ps * ps) : 0.f;        // d / d p_k for every k (the normaliser)
    // reverse sweep (torch's cumprod backward for an input without zeros: reversed cumsum of g_S * S, divided by the input)
    float acc = 0.f, h_next = 0.f;
    for (int j = a.M - 1; j >= 0; j--) {
        const float s = sv_sigmoid(x[j]);
        const float h = fminf(fmaxf(s, a.lo), a.hi);
        const float Sj = d[j];
        const float Sprev = j > 0 ? d[j - 1] : 1.0f;
        // S_j feeds p_{j+1} = h_{j+1} * S_j, or p_M = S_{M-1} for the last bin
        const float gS = j + 1 < a.M ? ((j + 1 == tgt ? gA : 0.f) + gB) * h_next : ((tgt == a.M ? gA : 0.f) + gB);
        acc += gS * Sj;
        const float gp = (j == tgt ? gA : 0.f) + gB;
        const float gh = gp * Sprev - acc / (1.0f - h);
        d[j] = (s >= a.lo && s <= a.hi) ? gh * (1.0f - s) * s : 0.f;
        h_next = h;
    }
}

// risk[r] = -sum_j prod_{i <= j} (1 - sigmoid(x_ri))   (train_survival.py:1431-1433: no clamp)
__global__ void __launch_bounds__(SV_THREADS) surv_risk_kernel(const float* __restrict__ x, int64_t ld, int N, int M, float* __restrict__ risk) {
    const int r = blockIdx.x * SV_THREADS + threadIdx.x;
    if (r >= N) return;
    const float* xr = x + (int64_t)r * ld;
    float S = 1.0f, sum = 0.f;
    for (int j = 0; j < M; j++) {
        S = S * (1.0f - sv_sigmoid(xr[j]));
        sum += S;
    }
    risk[r] = -sum;
}

// Concordance pair counts: lane = sample i (an event), blockIdx.y = a chunk of CI_CHUNK samples j staged through LDS in tiles of
// SV_THREADS.  Per-lane counts stay below CI_CHUNK, waves sum them exactly and add them with integer atomics (order-free).
constexpr int CI_CHUNK = 1024;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(SV_THREADS) cindex_counts_kernel(const uint8_t* __restrict__ ev, const double* __restrict__ tm,
                                                                   const float* __restrict__ est, int64_t n, float tol,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ double s_t[SV_THREADS];
    __shared__ float s_e[SV_THREADS];
    __shared__ uint8_t s_ev[SV_THREADS];
    const int64_t i = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    const bool act = i < n && ev[i] != 0;
    const double ti = act ? tm[i] : 0.0;
    const float ei = act ? est[i] : 0.f;
    int con = 0, dis = 0, tie = 0, ttime = 0, comp = 0;
    const int64_t j0 = (int64_t)blockIdx.y * CI_CHUNK;
    const int64_t j1 = j0 + CI_CHUNK < n ? j0 + CI_CHUNK : n;
    for (int64_t base = j0; base < j1; base += SV_THREADS) {
        const int64_t j = base + threadIdx.x;
        __syncthreads();
        if (j < j1) {
            s_t[threadIdx.x] = tm[j];
            s_e[threadIdx.x] = est[j];
            s_ev[threadIdx.x] = ev[j];
        }
        __syncthreads();
        const int cnt = (int)(j1 - base < SV_THREADS ? j1 - base : SV_THREADS);
        if (!act) continue;
        for (int k = 0; k < cnt; k++) {
            const double tj = s_t[k];
            const bool cens_j = s_ev[k] == 0;
            const bool same = tj == ti;
            if (!(tj > ti || (same && cens_j))) continue;
            comp++;
            ttime += same;              // same time and censored (the only way a same-time pair is comparable)
            const float ej = s_e[k];
            if (fabsf(ej - ei) <= tol) tie++;
            else if (ej < ei) con++;
            else dis++;
        }
    }
    const int v[5] = {con, dis, tie, ttime, comp};
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int w = wave_sum_i(v[q]);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&counts[q], (unsigned long long)w);
    }
}

int sv_check(const char* name, const float* x, int64_t ld, const void* t, int dt_t, const void* c, int dt_c, int N, int M, int kind) {
    MH_REQUIRE(x && t && c, "%s: logits / event_times / censoring must be non-null", name);
    MH_REQUIRE(N >= 1 && M >= 1 && ld >= M, "%s: bad shape N=%d M=%d ld=%lld", name, N, M, (long long)ld);
    MH_REQUIRE(dt_t == MH_SV_I32 || dt_t == MH_SV_I64, "%s: event_times must be int32 or int64 (code %d)", name, dt_t);
    MH_REQUIRE(dt_c >= MH_SV_U8 && dt_c <= MH_SV_F32, "%s: bad censoring dtype code %d", name, dt_c);
    MH_REQUIRE(kind == MH_SURV_NLL || kind == MH_SURV_CE, "%s: bad kind %d", name, kind);
    return MH_OK;
}

}  // namespace

extern "C" int mh_surv_loss_fwd(const float* logits, int64_t ld, const void* event_times, int dt_t, const void* censoring, int dt_c,
                                int N, int M, int kind, float lo, float hi, float w_all, float w_unc, float coef, float* loss_rows,
                                float* out, mh_stream s) {
    int rc = sv_check("mh_surv_loss_fwd", logits, ld, event_times, dt_t, censoring, dt_c, N, M, kind);
    if (rc) return rc;
    MH_REQUIRE(loss_rows || out, "mh_surv_loss_fwd: neither loss_rows nor out given");
    const SvArgs a = {logits, ld, event_times, dt_t, censoring, dt_c, N, M, kind, lo, hi, w_all, w_unc};
    hipLaunchKernelGGL(surv_loss_fwd_kernel, dim3(1), dim3(SV_THREADS), 0, (hipStream_t)s, a, coef, loss_rows, out);
    MH_LAUNCH_CHECK("mh_surv_loss_fwd");
    return MH_OK;
}

extern "C" int mh_surv_loss_bwd(const float* logits, int64_t ld, const void* event_times, int dt_t, const void* censoring, int dt_c,
                                int N, int M, int kind, float lo, float hi, float w_all, float w_unc, const float* g, int g_per_row,
                                float gcoef, float* dlogits, mh_stream s) {
    int rc = sv_check("mh_surv_loss_bwd", logits, ld, event_times, dt_t, censoring, dt_c, N, M, kind);
    if (rc) return rc;
    MH_REQUIRE(g && dlogits, "mh_surv_loss_bwd: g / dlogits must be non-null");
    const SvArgs a = {logits, ld, event_times, dt_t, censoring, dt_c, N, M, kind, lo, hi, w_all, w_unc};
    hipLaunchKernelGGL(surv_loss_bwd_kernel, dim3(mh_cdiv(N, SV_THREADS)), dim3(SV_THREADS), 0, (hipStream_t)s, a, g, g_per_row, gcoef,
                       dlogits);
    MH_LAUNCH_CHECK("mh_surv_loss_bwd");
    return MH_OK;
}

extern "C" int mh_surv_risk(const float* logits, int64_t ld, int N, int M, float* risk, mh_stream s) {
    MH_REQUIRE(logits && risk, "mh_surv_risk: logits / risk must be non-null");
    MH_REQUIRE(N >= 1 && M >= 1 && ld >= M, "mh_surv_risk: bad shape N=%d M=%d ld=%lld", N, M, (long long)ld);
    hipLaunchKernelGGL(surv_risk_kernel, dim3(mh_cdiv(N, SV_THREADS)), dim3(SV_THREADS), 0, (hipStream_t)s, logits, ld, N, M, risk);
    MH_LAUNCH_CHECK("mh_surv_risk");
    return MH_OK;
}

extern "C" int mh_cindex_counts(const uint8_t* event, const double* time, const float* estimate, int64_t n, float tied_tol,
                                int64_t* counts, mh_stream s) {
    MH_REQUIRE(event && time && estimate && counts, "mh_cindex_counts: null pointer");
    MH_REQUIRE(n >= 1 && n <= ((int64_t)1 << 26), "mh_cindex_counts: n = %lld out of range", (long long)n);
    if (hipMemsetAsync(counts, 0, 5 * sizeof(int64_t), (hipStream_t)s) != hipSuccess) {
        mh_set_error("mh_cindex_counts: hipMemsetAsync failed");
        return MH_EHIP;
    }
    const dim3 grid(mh_cdiv(n, SV_THREADS), mh_cdiv(n, CI_CHUNK));
    hipLaunchKernelGGL(cindex_counts_kernel, grid, dim3(SV_THREADS), 0, (hipStream_t)s, event, time, estimate, n, tied_tol,
                       (unsigned long long*)counts);
    MH_LAUNCH_CHECK("mh_cindex_counts");
    return MH_OK;
}
