// InfoNCE with explicit negative keys (losses/info_nce.py:126-143, with the `F.cross_entropy(logits / temperature, labels)` the
// reference's branch forgets): logits[i] = [q^[i].k^[i] | q^[i].n^[i, j] (paired) or q^[i].n^[j] (unpaired)] / t, label 0 in every row.
//
// q^ and k^ come from mh_l2norm_fwd.  Paired negatives [N, M, D] are the only large operand: the forward reads them ONCE (one pass
// per row gives q^.n and |n|^2; no normalised copy is written), the backward reads them once and writes d negatives once:
//   dn[i, j] = dl[i, j] * inv[i, j] * (q^[i] - cos[i, j] * inv[i, j] * n[i, j]),   dq^[i] = dpos[i] * k^[i] + sum_j dl[i, j] * inv[i, j] * n[i, j]
// (a row below eps in norm has inv = 1 / eps and a vanishing projection term, as mh_l2norm_bwd treats it).  Unpaired negatives are a
// GEMM against the normalised bank (mh_gemm + mh_l2norm_*); both modes share the label-0 cross-entropy over [pos | neg] rows below.
//
// Every sum is formed in a fixed order (wave shuffles, LDS, per-chunk partials folded by a second launch): results are bitwise
// reproducible, there are no atomics.  Nothing is allocated and nothing waits on the host (graph capturable).
#include "common.h"

namespace {

constexpr int NCE_THREADS = 256;
constexpr int NCE_QP = 4;             // column units a lane owns in the paired backward (one column tile = G * VEC * NCE_QP columns)

template <typename T, int VEC> struct NceVec;
template <typename T> struct NceVec<T, 4> {
    static __device__ __forceinline__ f4_t ld(const T* p) { return ld4<T>(p); }
    static __device__ __forceinline__ void st(T* p, f4_t v) { st4<T>(p, v); }
};
template <typename T> struct NceVec<T, 1> {
    static __device__ __forceinline__ f4_t ld(const T* p) { const f4_t r = {ldf<T>(p), 0.f, 0.f, 0.f}; return r; }
    static __device__ __forceinline__ void st(T* p, f4_t v) { stf<T>(p, v[0]); }
};

// ---- paired forward: G lanes (a power of two <= 64) walk one row n[i, j, :]; a wave takes 64 / G rows per pass.
// grid = (row blocks, N).  cos[i, j] = q^[i].n[i, j] / max(|n[i, j]|, eps), inv[i, j] = 1 / max(|n[i, j]|, eps).
template <typename T, int VEC>
__global__ void __launch_bounds__(NCE_THREADS) nce_paired_fwd_kernel(const float* __restrict__ qn, const T* __restrict__ neg,
                                                                     float* __restrict__ cosv, float* __restrict__ inv, int M, int D,
                                                                     int G, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int RW = 64 / G, sub = lane / G, cl = lane & (G - 1);
    const int i = blockIdx.y;
    const float* qr = qn + (int64_t)i * D;
    const int step = G * VEC;
    for (int jb = (blockIdx.x * 4 + wave) * RW; jb < M; jb += gridDim.x * 4 * RW) {      // wave-uniform bounds
        const int j = jb + sub;
        float dot = 0.f, ss = 0.f;
        if (j < M) {
            const T* nr = neg + ((int64_t)i * M + j) * D;
            for (int c = cl * VEC; c < D; c += 2 * step) {
                const bool two = c + step < D;
                const f4_t v0 = NceVec<T, VEC>::ld(nr + c);
                f4_t v1 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
                if (two) v1 = NceVec<T, VEC>::ld(nr + c + step);
                const f4_t q0 = NceVec<float, VEC>::ld(qr + c);
                if (two) q1 = NceVec<float, VEC>::ld(qr + c + step);
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    dot += v0[e] * q0[e] + v1[e] * q1[e];
                    ss += v0[e] * v0[e] + v1[e] * v1[e];
                }
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            dot += __shfl_xor(dot, o, 64);
            ss += __shfl_xor(ss, o, 64);
        }
        if (j < M && cl == 0) {
            const float iv = 1.0f / fmaxf(sqrtf(ss), eps);
            const int64_t r = (int64_t)i * M + j;
            cosv[r] = dot * iv;
            inv[r] = iv;
        }
    }
}

// ---- paired backward: grid = (chunks of jc rows j, N, column tiles).  A lane owns NCE_QP column units of its tile: it keeps q^[i]
// there and the running sum of a * n[i, j] over the rows its group walks.  The block's sums over its chunk go to
// part[i, chunk, :] (folded by nce_fold_kernel), summed over sub-rows, then over the four waves, in a fixed order.
template <typename T, int VEC>
__global__ void __launch_bounds__(NCE_THREADS) nce_paired_bwd_kernel(const float* __restrict__ qn, const T* __restrict__ neg,
                                                                     const float* __restrict__ cosv, const float* __restrict__ inv,
                                                                     const float* __restrict__ dl, T* __restrict__ dneg,
                                                                     float* __restrict__ part, int M, int D, int G, int jc) {
    __shared__ float red[4][NCE_QP * VEC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int RW = 64 / G, sub = lane / G, cl = lane & (G - 1);
    const int i = blockIdx.y, ch = blockIdx.x;
    const int c0 = blockIdx.z * (G * VEC * NCE_QP);
    int col[NCE_QP];
    f4_t q[NCE_QP], acc[NCE_QP];
#pragma unroll
    for (int t = 0; t < NCE_QP; t++) {
        col[t] = c0 + (cl + G * t) * VEC;
        const f4_t z = {0.f, 0.f, 0.f, 0.f};
        acc[t] = z;
        q[t] = col[t] < D ? NceVec<float, VEC>::ld(qn + (int64_t)i * D + col[t]) : z;
    }
    const int j1 = min(ch * jc + jc, M);
    for (int j = ch * jc + wave * RW + sub; j < j1; j += 4 * RW) {
        const int64_t r = (int64_t)i * M + j;
        const float iv = inv[r];
        const float a = dl[r] * iv, b = a * cosv[r] * iv;
        const T* nr = neg + r * D;
        f4_t v[NCE_QP];
#pragma unroll
        for (int t = 0; t < NCE_QP; t++)
            if (col[t] < D) v[t] = NceVec<T, VEC>::ld(nr + col[t]);
#pragma unroll
        for (int t = 0; t < NCE_QP; t++) {
            if (col[t] < D) {
                f4_t o;
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    acc[t][e] += a * v[t][e];
                    o[e] = a * q[t][e] - b * v[t][e];
                }
                if (dneg) NceVec<T, VEC>::st(dneg + r * D + col[t], o);
            }
        }
    }
    if (!part) return;
#pragma unroll
    for (int t = 0; t < NCE_QP; t++)
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            float s = acc[t][e];
            for (int o = 32; o >= G; o >>= 1) s += __shfl_xor(s, o, 64);
            red[wave][t * VEC + e][lane] = s;
        }
    __syncthreads();
    if (wave == 0 && sub == 0) {
        float* pr = part + ((int64_t)i * gridDim.x + ch) * D;
#pragma unroll
        for (int t = 0; t < NCE_QP; t++) {
            if (col[t] < D) {
                f4_t o;
#pragma unroll
                for (int e = 0; e < VEC; e++)
                    o[e] = (red[0][t * VEC + e][lane] + red[1][t * VEC + e][lane]) + (red[2][t * VEC + e][lane] + red[3][t * VEC + e][lane]);
                NceVec<float, VEC>::st(pr + col[t], o);
            }
        }
    }
}

// ---- label-0 cross-entropy over [pos | neg] rows: one block per row i.  With x0 = q^[i].k^[i] / t and x_j = neg[i, j] / t:
// lse[i] = logsumexp([x0 | x]), rows[i] = lse[i] - x0, pneg[i] = 1 - softmax[i, 0] = sum_j exp(x_j - lse[i]).
// The sum over the negatives is kept apart from the positive's term: a row whose positive dominates (loss near 0, the trained
// regime) gets its loss as log1p(sum) and its 1 - p0 as sum / (1 + sum), not as differences of numbers near 1.
__global__ void __launch_bounds__(NCE_THREADS) nce_rows_fwd_kernel(const float* __restrict__ qn, const float* __restrict__ kn,
                                                                   const float* __restrict__ neg, int64_t ld, int M, int D, float inv_t,
                                                                   float* __restrict__ pneg, float* __restrict__ lse,
                                                                   float* __restrict__ rows) {
    __shared__ float red[4];
    const int i = blockIdx.x;
    float p = 0.f;
    for (int c = threadIdx.x; c < D; c += NCE_THREADS) p += qn[(int64_t)i * D + c] * kn[(int64_t)i * D + c];
    p = block_sum256(p, red);
    const float x0 = p * inv_t;
    const float* nr = neg + (int64_t)i * ld;
    float m = x0;
    for (int j = threadIdx.x; j < M; j += NCE_THREADS) m = fmaxf(m, nr[j] * inv_t);
    m = block_max256(m, red);
    float sn = 0.f;
    for (int j = threadIdx.x; j < M; j += NCE_THREADS) sn += expf(nr[j] * inv_t - m);
    sn = block_sum256(sn, red);
    if (threadIdx.x == 0) {
        const float sp = expf(x0 - m);                      // 1 when the positive is the row's maximum
        const float loss = x0 == m ? log1pf(sn) : (m - x0) + logf(sp + sn);
        pneg[i] = sn / (sp + sn);
        lse[i] = x0 + loss;
        rows[i] = loss;
    }
}

// out[0] = coef * sum_r rows[r]: one block, fixed order
__global__ void __launch_bounds__(NCE_THREADS) nce_reduce_kernel(const float* __restrict__ rows, int N, float coef, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int r = threadIdx.x; r < N; r += NCE_THREADS) acc += rows[r];
    const float tot = block_sum256(acc, red);
    if (threadIdx.x == 0) out[0] = coef * tot;
}

// dneg[i, j] = u_i * exp(neg[i, j] / t - lse[i]),   dpos[i] = -u_i * pneg[i] (= u_i * (softmax[i, 0] - 1)),   u_i = gcoef * g[0 or i] / t
__global__ void __launch_bounds__(NCE_THREADS) nce_rows_bwd_kernel(const float* __restrict__ neg, int64_t ld, const float* __restrict__ pneg,
                                                                   const float* __restrict__ lse, const float* __restrict__ g,
                                                                   int g_per_row, float gcoef, float inv_t, int M,
                                                                   float* __restrict__ dneg, float* __restrict__ dpos) {
    const int i = blockIdx.y;
    const float u = gcoef * g[g_per_row ? i : 0] * inv_t;
    const float l = lse[i];
    const float* nr = neg + (int64_t)i * ld;
    float* dr = dneg + (int64_t)i * M;
    for (int j = blockIdx.x * NCE_THREADS + threadIdx.x; j < M; j += gridDim.x * NCE_THREADS) dr[j] = u * expf(nr[j] * inv_t - l);
    if (blockIdx.x == 0 && threadIdx.x == 0) dpos[i] = -u * pneg[i];
}

// dq[i, c] = dpos[i] * k^[i, c] + sum_p part[i, p, c] (p ascending),   dk[i, c] = dpos[i] * q^[i, c]
__global__ void __launch_bounds__(NCE_THREADS) nce_fold_kernel(const float* __restrict__ dpos, const float* __restrict__ qn,
                                                               const float* __restrict__ kn, const float* __restrict__ part, int nparts,
                                                               float* __restrict__ dq, float* __restrict__ dk, int N, int D) {
    const int64_t e = (int64_t)blockIdx.x * NCE_THREADS + threadIdx.x;
    if (e >= (int64_t)N * D) return;
    const int i = (int)(e / D), c = (int)(e - (int64_t)i * D);
    const float dp = dpos[i];
    if (dk) dk[e] = dp * qn[e];
    if (dq) {
        float s = 0.f;
        for (int p = 0; p < nparts; p++) s += part[((int64_t)i * nparts + p) * D + c];
        dq[e] = dp * kn[e] + s;
    }
}

int nce_group(int D, int vec) {
    const int units = mh_cdiv(D, vec);
    int G = 1;
    while (G < units && G < 64) G <<= 1;
    return G;
}

int nce_paired_check(const char* name, int N, int M, int D, int dt_neg) {
    MH_REQUIRE(N >= 1 && M >= 1 && D >= 1, "%s: bad shape N=%d M=%d D=%d", name, N, M, D);
    MH_REQUIRE(N <= 65535, "%s: N=%d exceeds 65535 rows", name, N);
    MH_REQUIRE((int64_t)N * M <= 0x7fffffffLL, "%s: N * M = %lld exceeds 2^31 - 1", name, (long long)N * M);
    MH_REQUIRE(dt_neg == MH_F32 || dt_neg == MH_BF16, "%s: negative_keys must be f32 or bf16 (code %d)", name, dt_neg);
    return MH_OK;
}

}  // namespace

extern "C" int mh_infonce_paired_fwd(const float* qn, const void* neg, float* cosv, float* inv, int N, int M, int D, float eps,
                                     int dt_neg, mh_stream s) {
    int rc = nce_paired_check("mh_infonce_paired_fwd", N, M, D, dt_neg);
    if (rc) return rc;
    MH_REQUIRE(qn && neg && cosv && inv, "mh_infonce_paired_fwd: null pointer");
    const int vec = (D % 4 == 0 && mh_quad_ok(qn, 4) && mh_quad_ok(neg, mh_dt_size(dt_neg))) ? 4 : 1;
    const int G = nce_group(D, vec);
    const int per_block = 4 * (64 / G);
    int gx = mh_cdiv(M, per_block);
    const int cap = mh_cdiv(4096, N);
    if (gx > cap) gx = cap;
    const dim3 grid(gx, N);
#define NCE_F(T, V) hipLaunchKernelGGL((nce_paired_fwd_kernel<T, V>), grid, dim3(NCE_THREADS), 0, (hipStream_t)s, qn, (const T*)neg, cosv, inv, M, D, G, eps)
    if (dt_neg == MH_F32) { if (vec == 4) NCE_F(float, 4); else NCE_F(float, 1); }
    else { if (vec == 4) NCE_F(bf16_t, 4); else NCE_F(bf16_t, 1); }
#undef NCE_F
    MH_LAUNCH_CHECK("mh_infonce_paired_fwd");
    return MH_OK;
}

extern "C" int mh_infonce_paired_bwd(const float* qn, const void* neg, const float* cosv, const float* inv, const float* dl, void* dneg,
                                     float* dq_part, int N, int M, int D, int jc, int dt_neg, mh_stream s) {
    int rc = nce_paired_check("mh_infonce_paired_bwd", N, M, D, dt_neg);
    if (rc) return rc;
    MH_REQUIRE(qn && neg && cosv && inv && dl, "mh_infonce_paired_bwd: null pointer");
    MH_REQUIRE(dneg || dq_part, "mh_infonce_paired_bwd: neither dneg nor dq_part wanted");
    MH_REQUIRE(jc >= 1, "mh_infonce_paired_bwd: chunk of %d rows", jc);
    const int esz = mh_dt_size(dt_neg);
    const int vec = (D % 4 == 0 && mh_quad_ok(qn, 4) && mh_quad_ok(neg, esz) && mh_quad_ok(dneg, esz) && mh_quad_ok(dq_part, 4)) ? 4 : 1;
    const int G = nce_group(D, vec);
    const int tiles = mh_cdiv(D, G * vec * NCE_QP);
    MH_REQUIRE(tiles <= 65535, "mh_infonce_paired_bwd: D=%d needs %d column tiles", D, tiles);
    const dim3 grid(mh_cdiv(M, jc), N, tiles);
#define NCE_B(T, V) hipLaunchKernelGGL((nce_paired_bwd_kernel<T, V>), grid, dim3(NCE_THREADS), 0, (hipStream_t)s, qn, (const T*)neg, cosv, inv, dl, (T*)dneg, dq_part, M, D, G, jc)
    if (dt_neg == MH_F32) { if (vec == 4) NCE_B(float, 4); else NCE_B(float, 1); }
    else { if (vec == 4) NCE_B(bf16_t, 4); else NCE_B(bf16_t, 1); }
#undef NCE_B
    MH_LAUNCH_CHECK("mh_infonce_paired_bwd");
    return MH_OK;
}

extern "C" int mh_infonce_rows_fwd(const float* qn, const float* kn, const float* neg, int64_t ld, int N, int M, int D, float inv_t,
                                   float coef, float* pneg, float* lse, float* loss_rows, float* out, mh_stream s) {
    MH_REQUIRE(qn && kn && neg && pneg && lse && loss_rows, "mh_infonce_rows_fwd: null pointer");
    MH_REQUIRE(N >= 1 && M >= 1 && D >= 1 && ld >= M, "mh_infonce_rows_fwd: bad shape N=%d M=%d D=%d ld=%lld", N, M, D, (long long)ld);
    hipLaunchKernelGGL(nce_rows_fwd_kernel, dim3(N), dim3(NCE_THREADS), 0, (hipStream_t)s, qn, kn, neg, ld, M, D, inv_t, pneg, lse, loss_rows);
    if (out) hipLaunchKernelGGL(nce_reduce_kernel, dim3(1), dim3(NCE_THREADS), 0, (hipStream_t)s, (const float*)loss_rows, N, coef, out);
    MH_LAUNCH_CHECK("mh_infonce_rows_fwd");
    return MH_OK;
}

extern "C" int mh_infonce_rows_bwd(const float* neg, int64_t ld, const float* pneg, const float* lse, const float* g, int g_per_row,
                                   float gcoef, float inv_t, int N, int M, float* dneg, float* dpos, mh_stream s) {
    MH_REQUIRE(neg && pneg && lse && g && dneg && dpos, "mh_infonce_rows_bwd: null pointer");
    MH_REQUIRE(N >= 1 && N <= 65535 && M >= 1 && ld >= M, "mh_infonce_rows_bwd: bad shape N=%d M=%d ld=%lld", N, M, (long long)ld);
    int gx = mh_cdiv(M, NCE_THREADS);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(nce_rows_bwd_kernel, dim3(gx, N), dim3(NCE_THREADS), 0, (hipStream_t)s, neg, ld, pneg, lse, g, g_per_row, gcoef, inv_t, M,
                       dneg, dpos);
    MH_LAUNCH_CHECK("mh_infonce_rows_bwd");
    return MH_OK;
}

extern "C" int mh_infonce_fold(const float* dpos, const float* qn, const float* kn, const float* part, int nparts, float* dq, float* dk,
                               int N, int D, mh_stream s) {
    MH_REQUIRE(dpos && qn && kn, "mh_infonce_fold: null pointer");
    MH_REQUIRE(dq || dk, "mh_infonce_fold: neither dq nor dk wanted");
    MH_REQUIRE(N >= 1 && D >= 1 && nparts >= 0 && (nparts == 0 || part), "mh_infonce_fold: bad arguments N=%d D=%d nparts=%d", N, D, nparts);
    hipLaunchKernelGGL(nce_fold_kernel, dim3(mh_cdiv((int64_t)N * D, NCE_THREADS)), dim3(NCE_THREADS), 0, (hipStream_t)s, dpos, qn, kn, part,
                       nparts, dq, dk, N, D);
    MH_LAUNCH_CHECK("mh_infonce_fold");
    return MH_OK;
}
