// Ridge Cox probe of frozen embeddings (mirror_amd/coxprobe.py): J = (folds + 1) x strengths independent L2-penalised Cox
// proportional-hazards regressions over the SAME prepared rows, sorted once by time (non-increasing).  One full-batch FISTA iteration is
// three launches on the caller's stream: mh_coxprobe_scores, mh_coxprobe_grad and mh_coxprobe_step (linprobe.hip).  Nothing allocated, no
// host wait, no float atomics: every sum has a fixed order, so two runs agree bit for bit.
//
//   mh_coxprobe_scores  the J weight rows are the keys of retrieval_tile.h's exact-f32 128 x 128 product (one key per job, no pad
//                       slots); the tile goes through LDS 64 rows at a time and leaves job-major, V [J x nq]: 64 consecutive floats of
//                       one job per wave, so that a job's scores are contiguous for the scan below and for mh_cindex_counts.
//   mh_coxprobe_grad    one workgroup of 256 threads per job walks its column of V; thread t owns the contiguous rows
//                       [t c, (t + 1) c), c = ceil(n / 256).  On rows in non-increasing time order the risk set of row i is a prefix
//                       and a tie group is a run, so the partial likelihood is scans, not pairs:
//                         0  m = max of the training scores (a NaN among them makes m NaN)
//                         A  forward: w = exp(v - m); P = inclusive prefix sum of w (S of a group = P at its last row); inside a tie
//                            group the running sum De of w and the running count ce over its training events (D, d = their values at
//                            the group's last row, l_i = ce_i - 1)
//                         B  backward, (S, D, d) carried down from each group's last row: den = S - f D, q = 1 / den, the loss term;
//                            Qs = inclusive suffix sum of q, inside a group the running sum QF of q f (both read at the group's FIRST row)
//                         C  forward, (Qs, QF) carried up from each group's first row:
//                            g_k = r (w_k (Qs - e_k QF) - e_k)     [Qs = sum over t_i <= t_k of q_i]
//                       Every pass is the same fixed-order block scan: a thread folds its chunk in row order, thread 0 folds the 256
//                       chunk summaries in thread order through LDS (a segmented sum restarts at a group boundary, a carried value is
//                       replaced there), and the thread walks its chunk again from its carry-in.  Every sum, exp and log is f64; only
//                       the stores to G round to f32.  The scan state (w, two f64 rows, the event counts) lives in the global
//                       workspace: LDS holds the 256 chunk summaries only.  A thread touches the workspace rows of its own chunk and no
//                       other, so the passes need no global fence: what crosses threads crosses through LDS behind a barrier.
#include <math.h>

#include "retrieval_tile.h"

namespace {

constexpr int CP_THREADS = 256;       // the gradient's workgroup: one per job
constexpr int CP_MAXN = 65536;
constexpr int CP_MAXD = 4096;
constexpr int CP_HALF = RT_TILE / 2;  // rows per pass of the scores' epilogue
constexpr int CP_LDT = RT_TILE + 1;   // LDS row stride of the spilled half tile (fewshot.hip says why 129)

// ------------------------------------------------------------------ scores, job-major
__global__ void __launch_bounds__(RT_THREADS, 3) coxprobe_scores_kernel(const float* __restrict__ q, const float* __restrict__ w, int nq,
                                                                        int nk, int D, int vec, float* __restrict__ V) {
    __shared__ float s_stage[4][RT_TILE * RT_LD];         // the product's two double-buffered stages, then the spilled half tile
    static_assert(CP_HALF * CP_LDT <= 4 * RT_TILE * RT_LD, "half a tile must fit the stages");
    float (&s_a)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[0][0]);
    float (&s_b)[2][RT_TILE * RT_LD] = *reinterpret_cast<float (*)[2][RT_TILE * RT_LD]>(&s_stage[2][0]);
    float* s_t = &s_stage[0][0];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE, col0 = blockIdx.y * RT_TILE;

    f32x16 acc[2][2];
    retr_product(acc, q, w, nq, nk, D, row0, col0, vec, s_a, s_b);      // ends with a barrier behind the last read of the stages

#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        s_t[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * CP_LDT + wn * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
        }
        __syncthreads();
        for (int t = tid; t < CP_HALF * RT_TILE; t += RT_THREADS) {     // a wave: 64 consecutive rows of one job
            const int rl = t & (CP_HALF - 1), kl = t >> 6;
            const int row = row0 + pass * CP_HALF + rl, key = col0 + kl;
            if (row < nq && key < nk) V[(int64_t)key * nq + row] = s_t[rl * CP_LDT + kl];
        }
        __syncthreads();                                  // the next pass overwrites the half tile
    }
}

// ------------------------------------------------------------------ partial-likelihood gradient of every job
struct cp_row {
    bool a, e, start, end;            // trains in the job; is a training event; first / last row of its tie group
};

__device__ __forceinline__ cp_row cp_flags(const double* __restrict__ time, const uint8_t* __restrict__ event,
                                           const int32_t* __restrict__ fold, int held, int i, int n) {
    const double t = time[i];
    const uint8_t ev = event[i];
    const int f = fold[i];
    cp_row r;
    r.a = ev <= 1 && t == t && f >= 0 && f != held;
    r.e = r.a && ev == 1;
    r.start = i == 0 || time[i - 1] != t;                 // a NaN time equals nothing: such a row is a group of its own
    r.end = i == n - 1 || time[i + 1] != t;
    return r;
}

__global__ void __launch_bounds__(CP_THREADS) coxprobe_grad_kernel(const float* __restrict__ V, int n, int J, const double* __restrict__ time,
                                                                   const uint8_t* __restrict__ event, const int32_t* __restrict__ fold,
                                                                   const int32_t* __restrict__ heldout, const float* __restrict__ rscale,
                                                                   int efron, float* __restrict__ G, double* __restrict__ loss,
                                                                   double* ws_w, double* ws_a, double* ws_b, int32_t* ws_c) {
    __shared__ double s_x[CP_THREADS], s_y[CP_THREADS], s_z[CP_THREADS];
    __shared__ int s_c[CP_THREADS], s_f[CP_THREADS];

    const int tid = threadIdx.x, job = blockIdx.x;
    const int held = heldout[job];
    const double r = (double)rscale[job];
    const int chunk = (n + CP_THREADS - 1) / CP_THREADS;
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    const float* v = V + (int64_t)job * n;
    double* w = ws_w + (int64_t)job * n;                  // w_i; then unchanged
    double* wa = ws_a + (int64_t)job * n;                 // P_i; then q_i; then Qs at a group's first row
    double* wb = ws_b + (int64_t)job * n;                 // De_i; then q_i f_i; then QF at a group's first row
    int32_t* wc = ws_c + (int64_t)job * n;                // ce_i

    // ---- 0: m
    {
        float mx = -INFINITY;
        int bad = 0;
        for (int i = lo; i < hi; i++) {
            if (cp_flags(time, event, fold, held, i, n).a) {
                const float x = v[i];
                bad |= x != x;
                mx = fmaxf(mx, x);
            }
        }
        s_x[tid] = (double)mx;
        s_f[tid] = bad;
    }
    __syncthreads();
    double m = -INFINITY;
    {
        int bad = 0;
        for (int u = 0; u < CP_THREADS; u++) {
            m = fmax(m, s_x[u]);
            bad |= s_f[u];
        }
        if (bad) m = NAN;
    }
    __syncthreads();

    // ---- A, first walk: w, and the chunk's summary
    {
        double p = 0.0, de = 0.0;
        int ce = 0, hasb = 0;
        for (int i = lo; i < hi; i++) {
            const cp_row fl = cp_flags(time, event, fold, held, i, n);
            if (fl.start) {
                de = 0.0;
                ce = 0;
                hasb = 1;
            }
            const double wi = fl.a ? exp((double)v[i] - m) : 0.0;
            w[i] = wi;
            p += wi;
            if (fl.e) {
                de += wi;
                ce++;
            }
        }
        s_x[tid] = p;
        s_y[tid] = de;
        s_c[tid] = ce;
        s_f[tid] = hasb;
    }
    __syncthreads();
    if (tid == 0) {                                       // the carry into every chunk, in thread order
        double P = 0.0, De = 0.0;
        int Ce = 0;
        for (int u = 0; u < CP_THREADS; u++) {
            const double px = s_x[u], dy = s_y[u];
            const int cc = s_c[u], hb = s_f[u];
            s_x[u] = P;
            s_y[u] = De;
            s_c[u] = Ce;
            P += px;
            De = hb ? dy : De + dy;
            Ce = hb ? cc : Ce + cc;
        }
    }
    __syncthreads();
    // ---- A, second walk: P, De, ce of every row; what the chunk's lowest end row holds
    double gS = 0.0, gD = 0.0;
    int gd = 1;
    {
        double p = s_x[tid], de = s_y[tid];
        int ce = s_c[tid];
        double eP = 0.0, eD = 0.0;
        int eC = 0, hasend = 0;
        for (int i = lo; i < hi; i++) {
            const cp_row fl = cp_flags(time, event, fold, held, i, n);
            if (fl.start) {
                de = 0.0;
                ce = 0;
            }
            p += w[i];
            if (fl.e) {
                de += w[i];
                ce++;
            }
            wa[i] = p;
            wb[i] = de;
            wc[i] = ce;
            if (fl.end && !hasend) {
                hasend = 1;
                eP = p;
                eD = de;
                eC = ce;
            }
        }
        __syncthreads();                                  // every carry-in has been read
        s_x[tid] = eP;
        s_y[tid] = eD;
        s_c[tid] = eC;
        s_f[tid] = hasend;
        __syncthreads();
        for (int u = tid + 1; u < CP_THREADS; u++) {      // (S, D, d) of the group that runs on past this chunk: the nearest end row above
            if (s_f[u]) {
                gS = s_x[u];
                gD = s_y[u];
                gd = s_c[u];
                break;
            }
        }
        __syncthreads();
    }

    // ---- B, first walk (backward): q, q f, the loss terms
    {
        double qs = 0.0, qf = 0.0, ls = 0.0;
        int hasend = 0;
        for (int i = hi - 1; i >= lo; i--) {
            const cp_row fl = cp_flags(time, event, fold, held, i, n);
            if (fl.end) {
                gS = wa[i];
                gD = wb[i];
                gd = wc[i];
                qf = 0.0;
                hasend = 1;
            }
            double qi = 0.0, qfi = 0.0;
            if (fl.e) {
                const double f = efron ? (double)(wc[i] - 1) / (double)gd : 0.0;
                const double den = gS - f * gD;
                qi = 1.0 / den;
                qfi = qi * f;
                ls += log(den) + m - (double)v[i];
            }
            wa[i] = qi;
            wb[i] = qfi;
            qs += qi;
            qf += qfi;
        }
        s_x[tid] = qs;
        s_y[tid] = qf;
        s_z[tid] = ls;
        s_f[tid] = hasend;
    }
    __syncthreads();
    if (tid == 0) {                                       // the carry into every chunk from above, in descending thread order
        double Q = 0.0, QF = 0.0, L = 0.0;
        for (int u = CP_THREADS - 1; u >= 0; u--) {
            const double qx = s_x[u], fy = s_y[u];
            const int hb = s_f[u];
            L += s_z[u];
            s_x[u] = Q;
            s_y[u] = QF;
            Q += qx;
            QF = hb ? fy : QF + fy;
        }
        loss[job] = r * L;
    }
    __syncthreads();
    // ---- B, second walk (backward): Qs, QF at every group's first row; what the chunk's highest start row holds
    double cQ = 0.0, cB = 0.0;
    {
        double qs = s_x[tid], qf = s_y[tid];
        double sQ = 0.0, sB = 0.0;
        int hasst = 0;
        for (int i = hi - 1; i >= lo; i--) {
            const cp_row fl = cp_flags(time, event, fold, held, i, n);
            if (fl.end) qf = 0.0;
            qs += wa[i];
            qf += wb[i];
            if (fl.start) {
                wa[i] = qs;
                wb[i] = qf;
                if (!hasst) {
                    hasst = 1;
                    sQ = qs;
                    sB = qf;
                }
            }
        }
        __syncthreads();                                  // every carry-in has been read
        s_x[tid] = sQ;
        s_y[tid] = sB;
        s_f[tid] = hasst;
        __syncthreads();
        for (int u = tid - 1; u >= 0; u--) {              // (Qs, QF) of the group that began before this chunk: the nearest start row below
            if (s_f[u]) {
                cQ = s_x[u];
                cB = s_y[u];
                break;
            }
        }
    }

    // ---- C: the gradient, exactly 0 off the training rows
    for (int i = lo; i < hi; i++) {
        const cp_row fl = cp_flags(time, event, fold, held, i, n);
        if (fl.start) {
            cQ = wa[i];
            cB = wb[i];
        }
        double g = 0.0;
        if (fl.a) g = r * (w[i] * (cQ - (fl.e ? cB : 0.0)) - (fl.e ? 1.0 : 0.0));
        G[(int64_t)i * J + job] = (float)g;
    }
}

}  // namespace

extern "C" int mh_coxprobe_scores(const float* q, int64_t nq, int D, const float* W, int J, float* V, mh_stream s) {
    MH_REQUIRE(D >= 1 && D <= CP_MAXD, "mh_coxprobe_scores: D = %d outside [1, %d]", D, CP_MAXD);
    MH_REQUIRE(nq >= 1 && nq <= (1 << 20), "mh_coxprobe_scores: nq = %lld outside [1, 2^20]", (long long)nq);
    MH_REQUIRE(J >= 1 && J <= (1 << 20), "mh_coxprobe_scores: J = %d jobs outside [1, 2^20]", J);
    MH_REQUIRE(nq * J <= (1ll << 28), "mh_coxprobe_scores: nq J = %lld x %d scores, 2^28 at the most", (long long)nq, J);
    MH_REQUIRE(q && W && V, "mh_coxprobe_scores: null pointer");
    const int vec = D % 4 == 0 && mh_quad_ok(q, 4) && mh_quad_ok(W, 4);
    hipLaunchKernelGGL(coxprobe_scores_kernel, dim3(mh_cdiv(nq, RT_TILE), mh_cdiv(J, RT_TILE)), dim3(RT_THREADS), 0, (hipStream_t)s, q, W,
                       (int)nq, J, D, vec, V);
    MH_LAUNCH_CHECK("mh_coxprobe_scores");
    return MH_OK;
}

extern "C" int64_t mh_coxprobe_workspace_bytes(int64_t n, int J) {
    if (n < 1 || n > CP_MAXN || J < 1 || n * J > (1ll << 24)) return -1;
    return (n * J * 28 + 7) / 8 * 8;                      // three f64 rows and one int32 row per job
}

extern "C" int mh_coxprobe_grad(const float* V, int64_t n, int J, const double* time, const uint8_t* event, const int32_t* fold,
                                const int32_t* heldout, const float* rscale, int ties, float* G, double* loss, void* workspace,
                                mh_stream s) {
    MH_REQUIRE(n >= 1 && n <= CP_MAXN, "mh_coxprobe_grad: n = %lld outside [1, %d]", (long long)n, CP_MAXN);
    MH_REQUIRE(J >= 1 && n * J <= (1ll << 24), "mh_coxprobe_grad: n J = %lld x %d scores outside [1, 2^24]", (long long)n, J);
    MH_REQUIRE(ties == MH_COX_BRESLOW || ties == MH_COX_EFRON, "mh_coxprobe_grad: ties = %d is neither MH_COX_BRESLOW nor MH_COX_EFRON",
               ties);
    MH_REQUIRE(V && time && event && fold && heldout && rscale && G && loss && workspace, "mh_coxprobe_grad: null pointer");
    MH_REQUIRE((((uintptr_t)time | (uintptr_t)loss | (uintptr_t)workspace) & 7) == 0,
               "mh_coxprobe_grad: time, loss and workspace must be 8-byte aligned");
    const int64_t nj = n * J;
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(coxprobe_grad_kernel, dim3(J), dim3(CP_THREADS), 0, (hipStream_t)s, V, (int)n, J, time, event, fold, heldout, rscale,
                       ties == MH_COX_EFRON ? 1 : 0, G, loss, ws, ws + nj, ws + 2 * nj, (int32_t*)(ws + 3 * nj));
    MH_LAUNCH_CHECK("mh_coxprobe_grad");
    return MH_OK;
}
