// Downstream subtyping step (train_subtyping.py): the classification loss of its template (timm's LabelSmoothingCrossEntropy,
// train_subtyping.py:984; nn.CrossEntropyLoss, :986 / :990) and its logit gradient, the confusion counts behind top-1 accuracy and
// torcheval's MulticlassF1Score (:1355-1360, :1390-1392), and the exact pair counts of torcheval's one-vs-rest MulticlassAUROC.
//
// Rows of the logits are handled by groups of G = min(64, next power of two >= C) lanes of one wave: each lane strides over the
// classes, the group combines through shuffles.  Sums over rows are formed in a fixed order by one block (bitwise reproducible, no
// float atomics); counts use integer atomics after a per-wave or per-block sum.  Nothing is allocated and nothing waits on the
// host (graph capturable).
#include <math.h>

#include "common.h"

namespace {

constexpr int CL_THREADS = 256;

__device__ __forceinline__ int64_t cl_label(const void* p, int dt, int64_t r) {
    return dt == MH_SV_I32 ? (int64_t)((const int32_t*)p)[r] : ((const int64_t*)p)[r];
}

// combine over the G lanes of an aligned group (G a power of two <= 64)
__device__ __forceinline__ float grp_max(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float grp_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exact integer sum over the 256 lanes of the block; `red` is >= 4 ints of LDS
__device__ __forceinline__ int block_sum256_int(int v, int* red) {
    v = wave_sum_int(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

int cl_group(int C) {
    int G = 1;
    while (G < C && G < 64) G <<= 1;
    return G;
}

struct CeArgs {
    const float* x; int64_t ld;
    const void* y; int dt_y;
    int N, C, G;
    float s;
    int64_t ignore;
};

// group max m and sum of exp(x - m) of row r (every lane of the group gets them); also the sum of (x - m) when want_sx
__device__ __forceinline__ void ce_row_stats(const CeArgs& a, const float* x, int gl, float& m, float& se, float* sx) {
    m = -INFINITY;
    for (int c = gl; c < a.C; c += a.G) m = fmaxf(m, x[c]);
    m = grp_max(m, a.G);
    float e = 0.f, d = 0.f;
    for (int c = gl; c < a.C; c += a.G) {
        const float t = x[c] - m;
        e += expf(t);
        d += t;
    }
    se = grp_sum(e, a.G);
    if (sx) *sx = grp_sum(d, a.G);
}

// loss_r = (1 - s) (lse - x_y) + s (lse - mean_c x) with lse = m + log(se), formed relative to m; 0 for an ignored row, NaN for a
// label outside [0, C).  One block: lanes of a group share row r, groups take rows gid, gid + 256 / G, ... in order.
__global__ void __launch_bounds__(CL_THREADS) cls_ce_fwd_kernel(CeArgs a, int mode, float* __restrict__ rows, float* __restrict__ out) {
    __shared__ float redf[CL_THREADS / 64];
    __shared__ int redi[CL_THREADS / 64];
    const int gid = threadIdx.x / a.G, gl = threadIdx.x % a.G, ngrp = CL_THREADS / a.G;
    float acc = 0.f;
    int cnt = 0;
    for (int r = gid; r < a.N; r += ngrp) {
        const float* x = a.x + (int64_t)r * a.ld;
        float m, se, sx;
        ce_row_stats(a, x, gl, m, se, &sx);
        const int64_t y = cl_label(a.y, a.dt_y, r);
        float loss;
        if (y == a.ignore) {
            loss = 0.f;
        } else if (y < 0 || y >= a.C) {
            loss = __builtin_nanf("");
        } else {
            const float lse = logf(se);
            const float nll = (m - x[y]) + lse;
            const float smooth = lse - sx / (float)a.C;
            loss = (1.0f - a.s) * nll + a.s * smooth;
        }
        if (gl == 0) {
            if (rows) rows[r] = loss;
            acc += loss;
            cnt += y != a.ignore;
        }
    }
    if (mode == MH_CLS_RED_NONE) return;
    const float tot = block_sum256(acc, redf);
    const int n = block_sum256_int(cnt, redi);
    if (threadIdx.x == 0) out[0] = mode == MH_CLS_RED_MEAN ? tot / (float)n : tot;
}

// dx[r, c] = w_r (softmax(x_r)[c] - (1 - s) [c == y_r] - s / C): w_r = g[r] ("none"), g[0] ("sum") or g[0] / #non-ignored rows
// ("mean": every block counts the labels itself, so no second launch and no saved state).  Ignored rows get 0, rows with a label
// outside [0, C) get NaN.  Grid-stride over row passes of 256 / G rows.
__global__ void __launch_bounds__(CL_THREADS) cls_ce_bwd_kernel(CeArgs a, int mode, const float* __restrict__ g, float* __restrict__ dx) {
    __shared__ int redi[CL_THREADS / 64];
    const int gid = threadIdx.x / a.G, gl = threadIdx.x % a.G, ngrp = CL_THREADS / a.G;
    float scale = mode == MH_CLS_RED_NONE ? 0.f : g[0];
    if (mode == MH_CLS_RED_MEAN) {
        int cnt = 0;
        for (int r = threadIdx.x; r < a.N; r += CL_THREADS) cnt += cl_label(a.y, a.dt_y, r) != a.ignore;
        scale = scale / (float)block_sum256_int(cnt, redi);
    }
    const float sc = a.s / (float)a.C, conf = 1.0f - a.s;
    for (int r = blockIdx.x * ngrp + gid; r < a.N; r += gridDim.x * ngrp) {
        const float* x = a.x + (int64_t)r * a.ld;
        float* d = dx + (int64_t)r * a.C;
        float m, se;
        ce_row_stats(a, x, gl, m, se, nullptr);
        const int64_t y = cl_label(a.y, a.dt_y, r);
        const float w = mode == MH_CLS_RED_NONE ? g[r] : scale;
        if (y == a.ignore) {
            for (int c = gl; c < a.C; c += a.G) d[c] = 0.f;
        } else if (y < 0 || y >= a.C) {
            for (int c = gl; c < a.C; c += a.G) d[c] = __builtin_nanf("");
        } else {
            const float inv = 1.0f / se;
            for (int c = gl; c < a.C; c += a.G) d[c] = w * (expf(x[c] - m) * inv - (c == y ? conf : 0.f) - sc);
        }
    }
}

// (value, index) of the first maximum as torch.argmax picks it: a NaN beats everything, the first NaN / first maximum wins
__device__ __forceinline__ void amax_take(float& bv, int& bi, float v, int i) {
    const bool bn = isnan(bv), vn = isnan(v);
    const bool take = bn ? (vn && i < bi) : (vn || v > bv || (v == bv && i < bi));
    if (take) { bv = v; bi = i; }
}

constexpr int CONF_LDS = 4096;   // int32 LDS copy of the confusion matrix when C * C fits (C <= 64)

// conf[label, prediction] += 1 per row with a label in [0, C) and a prediction in [0, C); every other row adds 1 to bad[0].
// Scores (dt_in = MH_SV_F32): the prediction is the first maximum of the row (first NaN if any), one group of G lanes per row.
// Predictions (MH_SV_I32 / MH_SV_I64): read as given.
__global__ void __launch_bounds__(CL_THREADS) cls_confusion_kernel(const void* __restrict__ in, int64_t ld, int dt_in, const void* __restrict__ lab,
                                                                   int dt_l, int N, int C, int G, unsigned long long* __restrict__ conf,
                                                                   unsigned long long* __restrict__ bad) {
    __shared__ int s_conf[CONF_LDS];
    __shared__ int redi[CL_THREADS / 64];
    const bool use_lds = C * C <= CONF_LDS;
    if (use_lds) {
        for (int k = threadIdx.x; k < C * C; k += CL_THREADS) s_conf[k] = 0;
        __syncthreads();
    }
    const int gid = threadIdx.x / G, gl = threadIdx.x % G, ngrp = CL_THREADS / G;
    int nbad = 0;
    for (int r = blockIdx.x * ngrp + gid; r < N; r += gridDim.x * ngrp) {
        int64_t p;
        if (dt_in == MH_SV_F32) {
            const float* x = (const float*)in + (int64_t)r * ld;
            float bv = -INFINITY;
            int bi = C;
            for (int c = gl; c < C; c += G) amax_take(bv, bi, x[c], c);
            for (int o = G >> 1; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                amax_take(bv, bi, ov, oi);
            }
            p = bi < C ? bi : 0;   // a row of -inf only: torch.argmax answers 0
        } else {
            p = cl_label(in, dt_in, r);
        }
        if (gl != 0) continue;
        const int64_t y = cl_label(lab, dt_l, r);
        if (y < 0 || y >= C || p < 0 || p >= C) {
            nbad++;
        } else if (use_lds) {
            atomicAdd(&s_conf[y * C + p], 1);
        } else {
            atomicAdd(&conf[y * C + p], 1ull);
        }
    }
    const int b = block_sum256_int(nbad, redi);   // also the barrier before the flush
    if (threadIdx.x == 0 && b) atomicAdd(bad, (unsigned long long)b);
    if (use_lds) {
        for (int k = threadIdx.x; k < C * C; k += CL_THREADS)
            if (s_conf[k]) atomicAdd(&conf[k], (unsigned long long)s_conf[k]);
    }
}

// One-vs-rest AUROC pair counts.  blockIdx.z = class c; lane = sample i (a positive of c when labels[i] == c); blockIdx.y strides
// over chunks of AU_CHUNK samples j staged through LDS in tiles of CL_THREADS.  A j that is not a negative of c, and an i that
// is not a positive, carry NaN, so (s_i > s_j) + (s_i >= s_j) adds 2 per pair ranked right, 1 per tie and 0 otherwise.  Per-lane
// counts stay below 2 N <= 2^21; waves sum them exactly and add them with integer atomics (order-free).  The blockIdx.y == 0
// blocks also count P_c, Q_c and the NaN scores of column c.  With several score tables over the same labels (mh_auroc_counts_many)
// blockIdx.z = e C + c: table e starts ld_table floats behind table e - 1 and owns counts [e C + c][4].
constexpr int AU_CHUNK = 1024;
constexpr int AU_MAX_Y = 64;
constexpr int AU_MAX_Z = 65535;       // the grid's z extent

__global__ void __launch_bounds__(CL_THREADS) auroc_counts_kernel(const float* __restrict__ x, int64_t ld, int64_t ld_table,
                                                                  const int64_t* __restrict__ lab, int N, int C,
                                                                  unsigned long long* __restrict__ counts) {
    __shared__ float s_s[CL_THREADS];
    const int e = blockIdx.z / C, c = blockIdx.z - e * C;
    x += e * ld_table;
    counts += (int64_t)e * C * 4;
    const int i = blockIdx.x * CL_THREADS + threadIdx.x;
    const bool in = i < N;
    const float xi = in ? x[(int64_t)i * ld + c] : 0.f;
    const bool pos = in && lab[i] == c;
    const float si = pos ? xi : __builtin_nanf("");
    if (blockIdx.y == 0) {
        const int v[3] = {(int)pos, (int)(in && !pos), (int)(in && isnan(xi))};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int w = wave_sum_int(v[q]);
            if ((threadIdx.x & 63) == 0 && w) atomicAdd(&counts[c * 4 + 1 + q], (unsigned long long)w);
        }
    }
    int u = 0;
    const int nchunks = (N + AU_CHUNK - 1) / AU_CHUNK;
    for (int ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
        const int j0 = ch * AU_CHUNK;
        const int j1 = j0 + AU_CHUNK < N ? j0 + AU_CHUNK : N;
        for (int base = j0; base < j1; base += CL_THREADS) {
            const int j = base + threadIdx.x;
            __syncthreads();
            if (j < j1) s_s[threadIdx.x] = lab[j] != c ? x[(int64_t)j * ld + c] : __builtin_nanf("");
            __syncthreads();
            const int cnt = j1 - base < CL_THREADS ? j1 - base : CL_THREADS;
            for (int k = 0; k < cnt; k++) {
                const float sj = s_s[k];
                u += (si > sj) + (si >= sj);
            }
        }
    }
    const int w = wave_sum_int(u);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&counts[c * 4], (unsigned long long)w);
}

int ce_check(const char* name, const float* x, int64_t ld, const void* y, int dt_y, int N, int C, float s, int mode) {
    MH_REQUIRE(x && y, "%s: logits / labels must be non-null", name);
    MH_REQUIRE(N >= 1 && C >= 1 && ld >= C, "%s: bad shape N=%d C=%d ld=%lld", name, N, C, (long long)ld);
    MH_REQUIRE(dt_y == MH_SV_I32 || dt_y == MH_SV_I64, "%s: labels must be int32 or int64 (code %d)", name, dt_y);
    MH_REQUIRE(s >= 0.f && s <= 1.f, "%s: smoothing %g outside [0, 1]", name, (double)s);
    MH_REQUIRE(mode == MH_CLS_RED_NONE || mode == MH_CLS_RED_MEAN || mode == MH_CLS_RED_SUM, "%s: bad reduction mode %d", name, mode);
    return MH_OK;
}

}  // namespace

extern "C" int mh_cls_ce_fwd(const float* logits, int64_t ld, const void* labels, int dt_l, int N, int C, float smoothing,
                             int64_t ignore_index, float* row_loss, float* out, int mode, mh_stream s) {
    int rc = ce_check("mh_cls_ce_fwd", logits, ld, labels, dt_l, N, C, smoothing, mode);
    if (rc) return rc;
    MH_REQUIRE(mode == MH_CLS_RED_NONE ? row_loss != nullptr : out != nullptr, "mh_cls_ce_fwd: no output for reduction mode %d", mode);
    const CeArgs a = {logits, ld, labels, dt_l, N, C, cl_group(C), smoothing, ignore_index};
    hipLaunchKernelGGL(cls_ce_fwd_kernel, dim3(1), dim3(CL_THREADS), 0, (hipStream_t)s, a, mode, row_loss, out);
    MH_LAUNCH_CHECK("mh_cls_ce_fwd");
    return MH_OK;
}

extern "C" int mh_cls_ce_bwd(const float* logits, int64_t ld, const void* labels, int dt_l, int N, int C, float smoothing,
                             int64_t ignore_index, const float* g, int mode, float* dlogits, mh_stream s) {
    int rc = ce_check("mh_cls_ce_bwd", logits, ld, labels, dt_l, N, C, smoothing, mode);
    if (rc) return rc;
    MH_REQUIRE(g && dlogits, "mh_cls_ce_bwd: g / dlogits must be non-null");
    const CeArgs a = {logits, ld, labels, dt_l, N, C, cl_group(C), smoothing, ignore_index};
    const int grid = mh_cdiv(N, CL_THREADS / a.G) < 256 ? mh_cdiv(N, CL_THREADS / a.G) : 256;
    hipLaunchKernelGGL(cls_ce_bwd_kernel, dim3(grid), dim3(CL_THREADS), 0, (hipStream_t)s, a, mode, g, dlogits);
    MH_LAUNCH_CHECK("mh_cls_ce_bwd");
    return MH_OK;
}

extern "C" int mh_cls_confusion(const void* input, int64_t ld, int dt_in, const void* labels, int dt_l, int N, int C, int64_t* conf,
                                int64_t* bad, mh_stream s) {
    MH_REQUIRE(input && labels && conf && bad, "mh_cls_confusion: null pointer");
    MH_REQUIRE(N >= 1 && C >= 1 && C <= 65536, "mh_cls_confusion: bad shape N=%d C=%d", N, C);
    MH_REQUIRE(dt_in == MH_SV_F32 || dt_in == MH_SV_I32 || dt_in == MH_SV_I64, "mh_cls_confusion: bad input dtype code %d", dt_in);
    MH_REQUIRE(dt_in != MH_SV_F32 || ld >= C, "mh_cls_confusion: row stride %lld < C = %d", (long long)ld, C);
    MH_REQUIRE(dt_l == MH_SV_I32 || dt_l == MH_SV_I64, "mh_cls_confusion: labels must be int32 or int64 (code %d)", dt_l);
    const int G = dt_in == MH_SV_F32 ? cl_group(C) : 1;
    const int rows = CL_THREADS / G;
    const int grid = mh_cdiv(N, rows) < 1024 ? mh_cdiv(N, rows) : 1024;
    hipLaunchKernelGGL(cls_confusion_kernel, dim3(grid), dim3(CL_THREADS), 0, (hipStream_t)s, input, ld, dt_in, labels, dt_l, N, C, G,
                       (unsigned long long*)conf, (unsigned long long*)bad);
    MH_LAUNCH_CHECK("mh_cls_confusion");
    return MH_OK;
}

extern "C" int mh_auroc_counts(const float* scores, int64_t ld, const int64_t* labels, int N, int C, int64_t* counts, mh_stream s) {
    MH_REQUIRE(scores && labels && counts, "mh_auroc_counts: null pointer");
    MH_REQUIRE(N >= 1 && N <= (1 << 20), "mh_auroc_counts: N = %d outside [1, 2^20]", N);
    MH_REQUIRE(C >= 2 && C <= 1024 && ld >= C, "mh_auroc_counts: bad shape C=%d ld=%lld", C, (long long)ld);
    if (hipMemsetAsync(counts, 0, (size_t)C * 4 * sizeof(int64_t), (hipStream_t)s) != hipSuccess) {
        mh_set_error("mh_auroc_counts: hipMemsetAsync failed");
        return MH_EHIP;
    }
    const int nchunks = mh_cdiv(N, AU_CHUNK);
    const dim3 grid(mh_cdiv(N, CL_THREADS), nchunks < AU_MAX_Y ? nchunks : AU_MAX_Y, C);
    hipLaunchKernelGGL(auroc_counts_kernel, grid, dim3(CL_THREADS), 0, (hipStream_t)s, scores, ld, (int64_t)0, labels, N, C,
                       (unsigned long long*)counts);
    MH_LAUNCH_CHECK("mh_auroc_counts");
    return MH_OK;
}

extern "C" int mh_auroc_counts_many(const float* scores, int64_t ld_row, int64_t ld_table, const int64_t* labels, int N, int C, int E,
                                    int64_t* counts, mh_stream s) {
    MH_REQUIRE(N >= 1 && N <= (1 << 20), "mh_auroc_counts_many: N = %d outside [1, 2^20]", N);
    MH_REQUIRE(C >= 2 && C <= 1024 && ld_row >= C, "mh_auroc_counts_many: bad shape C=%d ld_row=%lld", C, (long long)ld_row);
    MH_REQUIRE(E >= 1 && (int64_t)E * C <= AU_MAX_Z, "mh_auroc_counts_many: E = %d tables of C = %d classes, E C <= %d at the most", E, C,
               AU_MAX_Z);
    MH_REQUIRE(E == 1 || ld_table >= (int64_t)N * ld_row, "mh_auroc_counts_many: ld_table = %lld < N ld_row = %d x %lld",
               (long long)ld_table, N, (long long)ld_row);
    MH_REQUIRE(scores && labels && counts, "mh_auroc_counts_many: null pointer");
    if (hipMemsetAsync(counts, 0, (size_t)E * C * 4 * sizeof(int64_t), (hipStream_t)s) != hipSuccess) {
        mh_set_error("mh_auroc_counts_many: hipMemsetAsync failed");
        return MH_EHIP;
    }
    const int nchunks = mh_cdiv(N, AU_CHUNK);
    const dim3 grid(mh_cdiv(N, CL_THREADS), nchunks < AU_MAX_Y ? nchunks : AU_MAX_Y, E * C);
    hipLaunchKernelGGL(auroc_counts_kernel, grid, dim3(CL_THREADS), 0, (hipStream_t)s, scores, ld_row, E == 1 ? (int64_t)0 : ld_table, labels,
                       N, C, (unsigned long long*)counts);
    MH_LAUNCH_CHECK("mh_auroc_counts_many");
    return MH_OK;
}
