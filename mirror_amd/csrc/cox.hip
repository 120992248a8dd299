// Continuous-time survival: the Cox proportional-hazards partial-likelihood loss (Breslow / Efron ties) with its logit gradient,
// and the two-group log-rank statistics.  Both are all-pairs passes over (time, event, score), the shape of cindex_counts_kernel
// (survival.hip): one row per lane, the other index staged through LDS in tiles of CX_THREADS.
//
// Cox, for scores r [N] f32, times t [N] f64, e_i = (censoring_i == 1), m = max_j r_j, w_j = exp(r_j - m) in f64:
//   S_i = sum_j [t_j >= t_i] w_j      D_i = sum_j [t_j == t_i][e_j] w_j      d_i = sum_j [t_j == t_i][e_j]
//   l_i = sum_{j < i} [t_j == t_i][e_j]
//   f_i = 0 (Breslow), l_i / d_i on event rows (Efron);   den_i = S_i - f_i D_i;   loss_i = e_i (log den_i + m - r_i)
//   d loss / d r_k = w_k sum_i q_i ([t_k > t_i] + [t_k == t_i](1 - e_k f_i)) - g_k e_k,   q_i = g_i e_i / den_i
// Summed over a tie group in index order this is the textbook Efron / Breslow partial likelihood.  Nothing N x N is ever stored
// and exp never sees a positive argument.  All sums are f64 in a fixed order (per row four partial sums, each over ascending j,
// added in a fixed order; rows folded by one block), so the results are bitwise reproducible; only the final stores round to f32.
// No atomics, no allocation, no host wait: graph capturable.  The number of events and the "mean" divisor stay on the device.
#include <cmath>

#include "common.h"

namespace {

constexpr int CX_THREADS = 256;
constexpr int CX_ROWS = 64;                          // rows of a pair-pass block: one per lane of a wave
constexpr int CX_PARTS = CX_THREADS / CX_ROWS;       // the waves that split each tile of the other index
static_assert(CX_PARTS == 4, "the pair passes add four partial sums");
constexpr int CX_MAX_N = 65536;

// workspace (f64): [0] = m, [1] = n_events, then w [N], den [N], f [N], loss rows [N]
constexpr int CX_HDR = 2;
__host__ __device__ inline int64_t cx_ws_doubles(int64_t N) { return CX_HDR + 4 * N; }

// censoring[r] == 1 for each storage dtype, as survival.hip compares it
__device__ __forceinline__ bool cx_event(const void* p, int dt, int64_t r) {
    switch (dt) {
        case MH_SV_U8: return ((const uint8_t*)p)[r] == 1;
        case MH_SV_I32: return ((const int32_t*)p)[r] == 1;
        case MH_SV_I64: return ((const int64_t*)p)[r] == 1;
        default: return ((const float*)p)[r] == 1.0f;
    }
}

__device__ __forceinline__ double cx_nan() { return __builtin_nan(""); }

// fixed-order block sum / max of CX_THREADS doubles through LDS (red: CX_THREADS doubles); every thread gets the result
__device__ __forceinline__ double cx_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = CX_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double cx_block_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = CX_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    return red[0];
}

// m (NaN when any logit is NaN: it then propagates into every w), n_events and w, by one block
__global__ void __launch_bounds__(CX_THREADS) cox_prep_kernel(const float* __restrict__ x, int64_t ld, const void* __restrict__ c, int dt_c,
                                                              int N, double* __restrict__ ws) {
    __shared__ double red[CX_THREADS];
    double mx = -INFINITY, bad = 0.0, nev = 0.0;
    for (int j = threadIdx.x; j < N; j += CX_THREADS) {
        const double r = (double)x[(int64_t)j * ld];
        if (r != r) bad = 1.0;
        else mx = fmax(mx, r);
        nev += cx_event(c, dt_c, j) ? 1.0 : 0.0;
    }
    mx = cx_block_max(mx, red);
    bad = cx_block_max(bad, red);
    nev = cx_block_sum(nev, red);       // integers below 2^53: exact in any order
    const double m = bad != 0.0 ? cx_nan() : mx;
    if (threadIdx.x == 0) {
        ws[0] = m;
        ws[1] = nev;
    }
    double* w = ws + CX_HDR;
    for (int j = threadIdx.x; j < N; j += CX_THREADS) w[j] = exp((double)x[(int64_t)j * ld] - m);
}

// A block owns CX_ROWS rows, one per lane; every j tile of CX_THREADS is split between its four waves (wave p takes slots
// 64 p .. 64 p + 63 of each tile), so a wave walks N / 4 values of j and N / 64 blocks spread over the chip.  Each wave adds its j in
// ascending order, the four partial sums are added as ((p0 + p1) + p2) + p3: a fixed order.
// Slots past N hold t = NaN (in no comparison), w = 0, e = 0, so the inner loop has no bound.
__global__ void __launch_bounds__(CX_THREADS) cox_fwd_kernel(const float* __restrict__ x, int64_t ld, const double* __restrict__ tm,
                                                             const void* __restrict__ c, int dt_c, int N, int efron,
                                                             float* __restrict__ rows, double* __restrict__ ws) {
    __shared__ double s_t[CX_THREADS];
    __shared__ double s_w[CX_THREADS];
    __shared__ uint8_t s_e[CX_THREADS];
    __shared__ double p_S[CX_PARTS][CX_ROWS];
    __shared__ double p_D[CX_PARTS][CX_ROWS];
    __shared__ int p_d[CX_PARTS][CX_ROWS];
    __shared__ int p_l[CX_PARTS][CX_ROWS];
    const double* w = ws + CX_HDR;
    const int lane = threadIdx.x & (CX_ROWS - 1), part = threadIdx.x / CX_ROWS;
    const int i = blockIdx.x * CX_ROWS + lane;
    const bool in = i < N;
    const double ti = in ? tm[i] : cx_nan();
    double S = 0.0, D = 0.0;
    int d = 0, l = 0;
    for (int base = 0; base < N; base += CX_THREADS) {
        const int j = base + threadIdx.x;
        __syncthreads();
        s_t[threadIdx.x] = j < N ? tm[j] : cx_nan();
        s_w[threadIdx.x] = j < N ? w[j] : 0.0;
        s_e[threadIdx.x] = j < N && cx_event(c, dt_c, j) ? 1 : 0;
        __syncthreads();
        const int k0 = part * CX_ROWS;
#pragma unroll 8
        for (int k = k0; k < k0 + CX_ROWS; k++) {
            const double tj = s_t[k], wj = s_w[k];
            const bool ev = tj == ti && s_e[k] != 0;
            S += tj >= ti ? wj : 0.0;
            D += ev ? wj : 0.0;
            d += ev;
            l += ev && base + k < i;
        }
    }
    p_S[part][lane] = S;
    p_D[part][lane] = D;
    p_d[part][lane] = d;
    p_l[part][lane] = l;
    __syncthreads();
    if (part != 0 || !in) return;
    S = ((p_S[0][lane] + p_S[1][lane]) + p_S[2][lane]) + p_S[3][lane];
    D = ((p_D[0][lane] + p_D[1][lane]) + p_D[2][lane]) + p_D[3][lane];
    d = p_d[0][lane] + p_d[1][lane] + p_d[2][lane] + p_d[3][lane];
    l = p_l[0][lane] + p_l[1][lane] + p_l[2][lane] + p_l[3][lane];
    const bool ei = cx_event(c, dt_c, i);
    const double f = efron && ei ? (double)l / (double)d : 0.0;       // an event row with a real time counts itself: d >= 1
    const double den = S - f * D;
    double loss = ei ? log(den) + ws[0] - (double)x[(int64_t)i * ld] : 0.0;
    if (ti != ti) loss = cx_nan();
    double* den_o = ws + CX_HDR + N;
    double* f_o = den_o + N;
    double* loss_o = f_o + N;
    den_o[i] = den;
    f_o[i] = ti != ti ? 0.0 : f;
    loss_o[i] = loss;
    if (rows) rows[i] = (float)loss;
}

// out[0] = coef * sum_i loss_i: lane t adds rows t, t + 256, .. in that order, then the fixed tree.  coef: 1 ("sum"),
// 1 / max(n_events, 1) ("mean"), 1 / N ("batch").
__device__ __forceinline__ double cx_coef(int reduction, int N, const double* ws) {
    if (reduction == MH_COX_RED_MEAN) return 1.0 / fmax(ws[1], 1.0);
    if (reduction == MH_COX_RED_BATCH) return 1.0 / (double)N;
    return 1.0;
}

__global__ void __launch_bounds__(CX_THREADS) cox_fold_kernel(int N, int reduction, const double* __restrict__ ws, float* __restrict__ out) {
    __shared__ double red[CX_THREADS];
    const double* loss = ws + CX_HDR + 3 * (int64_t)N;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += CX_THREADS) acc += loss[i];
    const double tot = cx_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = (float)(cx_coef(reduction, N, ws) * tot);
}

// Row k per lane over tiles of i, split between the waves as above: A = sum_i q_i [t_k > t_i], B = sum_i q_i [t_k == t_i],
// C = sum_i q_i f_i [t_k == t_i].  Empty slots and rows with a NaN time hold t = NaN and q = 0.
__global__ void __launch_bounds__(CX_THREADS) cox_bwd_kernel(const double* __restrict__ tm, const void* __restrict__ c, int dt_c, int N,
                                                             int reduction, const float* __restrict__ g, int g_per_row,
                                                             const double* __restrict__ ws, float* __restrict__ dx, int64_t ld_d) {
    __shared__ double s_t[CX_THREADS];
    __shared__ double s_q[CX_THREADS];
    __shared__ double s_qf[CX_THREADS];
    __shared__ double p_A[CX_PARTS][CX_ROWS];
    __shared__ double p_B[CX_PARTS][CX_ROWS];
    __shared__ double p_C[CX_PARTS][CX_ROWS];
    const double* w = ws + CX_HDR;
    const double* den = w + N;
    const double* fr = den + N;
    const double coef = reduction == MH_COX_RED_NONE ? 1.0 : cx_coef(reduction, N, ws);
    const int lane = threadIdx.x & (CX_ROWS - 1), part = threadIdx.x / CX_ROWS;
    const int k = blockIdx.x * CX_ROWS + lane;
    const bool in = k < N;
    const double tk = in ? tm[k] : cx_nan();
    double A = 0.0, B = 0.0, Cf = 0.0;
    for (int base = 0; base < N; base += CX_THREADS) {
        const int i = base + threadIdx.x;
        __syncthreads();
        double t = cx_nan(), q = 0.0, f = 0.0;
        if (i < N) {
            t = tm[i];
            f = fr[i];
            if (t == t && cx_event(c, dt_c, i)) q = coef * (double)g[g_per_row ? i : 0] / den[i];
        }
        s_t[threadIdx.x] = t;
        s_q[threadIdx.x] = q;
        s_qf[threadIdx.x] = q * f;
        __syncthreads();
        const int j0 = part * CX_ROWS;
#pragma unroll 8
        for (int j = j0; j < j0 + CX_ROWS; j++) {
            const double t2 = s_t[j], q2 = s_q[j];
            const bool eq = tk == t2;
            A += tk > t2 ? q2 : 0.0;
            B += eq ? q2 : 0.0;
            Cf += eq ? s_qf[j] : 0.0;
        }
    }
    p_A[part][lane] = A;
    p_B[part][lane] = B;
    p_C[part][lane] = Cf;
    __syncthreads();
    if (part != 0 || !in) return;
    A = ((p_A[0][lane] + p_A[1][lane]) + p_A[2][lane]) + p_A[3][lane];
    B = ((p_B[0][lane] + p_B[1][lane]) + p_B[2][lane]) + p_B[3][lane];
    Cf = ((p_C[0][lane] + p_C[1][lane]) + p_C[2][lane]) + p_C[3][lane];
    const bool ek = cx_event(c, dt_c, k);
    const double gk = ek ? coef * (double)g[g_per_row ? k : 0] : 0.0;
    double r = w[k] * (A + B - (ek ? Cf : 0.0)) - gk;
    if (tk != tk) r = cx_nan();
    dx[(int64_t)k * ld_d] = (float)r;
}

// Log-rank: an event row with no earlier event row at its time owns that time's term.  One block walks the rows in chunks of
// CX_THREADS and thread 0 adds the chunk sums in chunk order; rows with a NaN time are ignored.
__global__ void __launch_bounds__(CX_THREADS) logrank_kernel(const uint8_t* __restrict__ ev, const double* __restrict__ tm,
                                                             const uint8_t* __restrict__ grp, int n, double* __restrict__ stats) {
    __shared__ double s_t[CX_THREADS];
    __shared__ uint8_t s_e[CX_THREADS];
    __shared__ uint8_t s_g[CX_THREADS];
    __shared__ double red[CX_THREADS];
    double O1 = 0.0, E1 = 0.0, V = 0.0, nev = 0.0;
    for (int row0 = 0; row0 < n; row0 += CX_THREADS) {
        const int i = row0 + threadIdx.x;
        const double ti = i < n ? tm[i] : cx_nan();
        const bool act = i < n && ev[i] != 0 && ti == ti;
        int cn = 0, cn1 = 0, cd = 0, cd1 = 0, earlier = 0;
        for (int base = 0; base < n; base += CX_THREADS) {
            const int j = base + threadIdx.x;
            __syncthreads();
            s_t[threadIdx.x] = j < n ? tm[j] : cx_nan();
            s_e[threadIdx.x] = j < n && ev[j] != 0 ? 1 : 0;
            s_g[threadIdx.x] = j < n && grp[j] != 0 ? 1 : 0;
            __syncthreads();
            if (!act) continue;
#pragma unroll 16
            for (int k = 0; k < CX_THREADS; k++) {
                const double tj = s_t[k];
                const int g1 = s_g[k];
                const int ge = tj >= ti;
                const int de = tj == ti && s_e[k] != 0;
                cn += ge;
                cn1 += ge & g1;
                cd += de;
                cd1 += de & g1;
                earlier += de && base + k < i;
            }
        }
        double o = 0.0, e = 0.0, v = 0.0;
        if (act && earlier == 0) {
            const double dn = cn, dn1 = cn1, dd = cd;
            o = cd1;
            e = dd * dn1 / dn;
            if (cn > 1) v = dn1 * (dn - dn1) * dd * (dn - dd) / (dn * dn * (dn - 1.0));
        }
        const double so = cx_block_sum(o, red), se = cx_block_sum(e, red), sv = cx_block_sum(v, red);
        const double sn = cx_block_sum(act ? 1.0 : 0.0, red);
        O1 += so;
        E1 += se;
        V += sv;
        nev += sn;
    }
    if (threadIdx.x == 0) {
        stats[0] = O1;
        stats[1] = E1;
        stats[2] = V;
        stats[3] = nev;
    }
}

int cx_check(const char* name, const float* x, int64_t ld, const double* t, const void* c, int dt_c, int N, int ties, int reduction,
             const void* ws) {
    MH_REQUIRE(x && t && c && ws, "%s: logits / time / censoring / workspace must be non-null", name);
    MH_REQUIRE(N >= 1 && N <= CX_MAX_N, "%s: N = %d outside [1, %d]", name, N, CX_MAX_N);
    MH_REQUIRE(ld >= 1, "%s: bad row stride %lld", name, (long long)ld);
    MH_REQUIRE(dt_c >= MH_SV_U8 && dt_c <= MH_SV_F32, "%s: bad censoring dtype code %d", name, dt_c);
    MH_REQUIRE(ties == MH_COX_BRESLOW || ties == MH_COX_EFRON, "%s: bad ties %d", name, ties);
    MH_REQUIRE(reduction >= MH_COX_RED_NONE && reduction <= MH_COX_RED_BATCH, "%s: bad reduction %d", name, reduction);
    MH_REQUIRE(((uintptr_t)t & 7) == 0 && ((uintptr_t)ws & 7) == 0, "%s: time / workspace must be 8-byte aligned", name);
    return MH_OK;
}

}  // namespace

extern "C" int64_t mh_cox_workspace_bytes(int N) { return N >= 1 && N <= CX_MAX_N ? cx_ws_doubles(N) * (int64_t)sizeof(double) : -1; }

extern "C" int mh_cox_loss_fwd(const float* logits, int64_t ld, const double* time, const void* censoring, int dt_c, int N, int ties,
                               int reduction, float* loss_rows, float* out, void* workspace, mh_stream s) {
    int rc = cx_check("mh_cox_loss_fwd", logits, ld, time, censoring, dt_c, N, ties, reduction, workspace);
    if (rc) return rc;
    MH_REQUIRE(loss_rows || out, "mh_cox_loss_fwd: neither loss_rows nor out given");
    MH_REQUIRE(!out || reduction != MH_COX_RED_NONE, "mh_cox_loss_fwd: out needs a reduction other than none");
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(cox_prep_kernel, dim3(1), dim3(CX_THREADS), 0, (hipStream_t)s, logits, ld, censoring, dt_c, N, ws);
    MH_LAUNCH_CHECK("mh_cox_loss_fwd (prep)");
    hipLaunchKernelGGL(cox_fwd_kernel, dim3(mh_cdiv(N, CX_ROWS)), dim3(CX_THREADS), 0, (hipStream_t)s, logits, ld, time, censoring,
                       dt_c, N, ties == MH_COX_EFRON, loss_rows, ws);
    MH_LAUNCH_CHECK("mh_cox_loss_fwd (pairs)");
    if (out) {
        hipLaunchKernelGGL(cox_fold_kernel, dim3(1), dim3(CX_THREADS), 0, (hipStream_t)s, N, reduction, (const double*)ws, out);
        MH_LAUNCH_CHECK("mh_cox_loss_fwd (fold)");
    }
    return MH_OK;
}

extern "C" int mh_cox_loss_bwd(const float* logits, int64_t ld, const double* time, const void* censoring, int dt_c, int N, int ties,
                               int reduction, const float* g, int g_per_row, const void* workspace, float* dlogits, int64_t ld_d,
                               mh_stream s) {
    int rc = cx_check("mh_cox_loss_bwd", logits, ld, time, censoring, dt_c, N, ties, reduction, workspace);
    if (rc) return rc;
    MH_REQUIRE(g && dlogits && ld_d >= 1, "mh_cox_loss_bwd: g / dlogits must be non-null, ld_d >= 1");
    MH_REQUIRE(!g_per_row || reduction == MH_COX_RED_NONE, "mh_cox_loss_bwd: a per-row upstream gradient needs reduction none");
    hipLaunchKernelGGL(cox_bwd_kernel, dim3(mh_cdiv(N, CX_ROWS)), dim3(CX_THREADS), 0, (hipStream_t)s, time, censoring, dt_c, N,
                       reduction, g, g_per_row, (const double*)workspace, dlogits, ld_d);
    MH_LAUNCH_CHECK("mh_cox_loss_bwd");
    return MH_OK;
}

extern "C" int mh_logrank_stats(const uint8_t* event, const double* time, const uint8_t* group, int64_t n, double* stats, mh_stream s) {
    MH_REQUIRE(event && time && group && stats, "mh_logrank_stats: null pointer");
    MH_REQUIRE(n >= 1 && n <= CX_MAX_N, "mh_logrank_stats: n = %lld outside [1, %d]", (long long)n, CX_MAX_N);
    MH_REQUIRE(((uintptr_t)time & 7) == 0 && ((uintptr_t)stats & 7) == 0, "mh_logrank_stats: time / stats must be 8-byte aligned");
    hipLaunchKernelGGL(logrank_kernel, dim3(1), dim3(CX_THREADS), 0, (hipStream_t)s, event, time, group, (int)n, stats);
    MH_LAUNCH_CHECK("mh_logrank_stats");
    return MH_OK;
}
