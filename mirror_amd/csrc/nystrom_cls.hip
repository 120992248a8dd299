// One row of the Nystrom attention matrix ([3P] NystromAttention.forward(..., return_attn=True), called at models/mirror.py:312):
//   attn = attn1 @ pinv(attn2) @ attn3,   row = attn[cls_row, :]   — the slide attention map of TransMIL's CLS token.
// The [n_p x n_p] matrix is never formed (9.7 GB in f32 at 4352 tokens, 8 heads, B = 16); one row of it factors:
//   p1[j]  = softmax_j(scale q[cls_row] . k_l[j])                          (m values)
//   u[j]   = sum_i p1[i] Z[i, j]                                            (Z = pinv(attn2), the iteration's output)
//   row[n] = sum_j u[j] exp(scale q_l[j] . k[n] - lse3[j])                  (n over the n_p padded positions)
// grid (walkers, B h), 4 waves.  Every workgroup stages the head's q_l rows in LDS once and forms p1 and u itself (m dot products and
// an m x m mat-vec: ~0.1 MFLOP); after that every wave walks its own 32-key blocks of the sequence (block = first + i * 4 * walkers)
// with the k fragments read straight from HBM — no LDS writes and no barriers in the loop, as in nys_a1_fwd_kernel.  A block is
// S[landmark][key] = q_l k^T (landmarks in the accumulator registers, the key on the lane), 32 landmarks at a time, on
// v_mfma_f32_32x32x16_bf16 (bf16 operands) or v_mfma_f32_32x32x2_f32 (f32 operands: the exact-f32 policy); u and -lse3 are per-register
// values read from LDS, the weighted column sum stays in the lane and its two halves meet once per block.  row[n] has exactly one
// writer (plain vector stores, no atomics).
// lse3 == NULL: the workgroup first takes the row log-sum-exp over ALL n_p keys itself (same products in the other orientation —
// key in the registers, landmark on the lane — with an online max / sum per lane).  That pass cannot be shared between workgroups, so
// the launch then uses ONE walker per (b, h): twice the products, B h workgroups (the composed core of the fp32 policy, inference only).
// Key-padding mask (mrow / mlm as in nystrom_fused.hip): an invalid landmark gets p1 = 0 and its attn3 row is uniform (1 / n_p, the
// package's fully masked row), a valid landmark's row is zero on invalid keys; row[n] of an invalid key n is written as exactly 0.
// Bound: the q_l k^T product, 2 n_p m dh flops per (b, h) — what nys_a3_fwd_kernel spends on its first product (its second, P v, has no
// counterpart here) — under the same exponential per logit.  Bytes per (b, h): k once (n_p dh elements), q_l | k_l (2 m dh) and Z (m^2)
// once PER WALKER, n_p floats out.  At n_p = 4352, dh = 64, m = 256, bf16, 4 walkers: 557 KB of k + 4 x (64 KB + 128 KB) = 1.3 MB read,
// 17 KB written, against 143 MFLOP.
#include "gemm_kernel.h"

namespace {

constexpr int CT = 256;   // threads per workgroup (4 waves)
constexpr float C_LOG2E = 1.4426950408889634f;
constexpr float C_NEG_BIG = -1e30f;

// operand fragments of one 32 x 32 MFMA step, row `lane & 31` of a [rows][dh] image, lane half hl = lane >> 5.
//   bf16: k-step of 16, elements 16 ks + 8 hl + {0..7};  f32: k-step of 2, element hl * dh / 2 + ks (each lane half owns a contiguous
//   half of the row: both operands use the same order, which is all a contraction needs)
template <typename T, int DH> struct Op;
template <int DH> struct Op<bf16_t, DH> {
    static constexpr int KSTEPS = DH / 16, PAD = 8;
    typedef bf16x8 frag;
    static __device__ __forceinline__ frag ld(const bf16_t* row, int ks, int hl) { return *reinterpret_cast<const bf16x8*>(row + 16 * ks + 8 * hl); }
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <int DH> struct Op<float, DH> {
    static constexpr int KSTEPS = DH / 2, PAD = 4;
    typedef float frag;
    static __device__ __forceinline__ frag ld(const float* row, int ks, int hl) { return row[hl * (DH / 2) + ks]; }
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};

__device__ __forceinline__ f32x16 c_zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0.f;
    return z;
}
// accumulator registers <-> rows 8 (r >> 2) + 4 hl + (r & 3): the 16 per-row values of `src` for this lane
__device__ __forceinline__ f32x16 c_rowvals16(const float* src, int hl) {
    f32x16 v;
#pragma unroll
    for (int gq = 0; gq < 4; gq++) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src + 8 * gq + 4 * hl);
        v[4 * gq] = x[0]; v[4 * gq + 1] = x[1]; v[4 * gq + 2] = x[2]; v[4 * gq + 3] = x[3];
    }
    return v;
}

struct ClsGeo {
    int h, n_p, cls_row;
    float scale, scale2;    // scale2 = scale * log2(e)
    long lm_ld;             // row stride of lm in elements
    const float* mrow;      // [B, n_p] valid rows (NULL: no mask)
    const float* mlm;       // [B, m] valid landmarks
    int z_colmajor;         // Z: 1 = bf16 column-major (the pinv chain's zfT), 0 = f32 row-major
};

template <typename T, int DH, int M, bool MASKED>
__global__ __launch_bounds__(CT) void nys_cls_kernel(const T* __restrict__ qkv, const T* __restrict__ lm, const void* __restrict__ Z,
                                                     const float* __restrict__ lse3, float* __restrict__ row, ClsGeo g) {
    using O = Op<T, DH>;
    constexpr int P = DH + O::PAD, KSTEPS = O::KSTEPS, LB = M / 32;
    __shared__ __attribute__((aligned(16))) T s_ql_[M * P];
    __shared__ __attribute__((aligned(16))) float s_u_[M];      // u (pass 1: the running sums)
    __shared__ __attribute__((aligned(16))) float s_nl_[M];     // -lse3 log2(e) (pass 1: the running maxima)
    __shared__ __attribute__((aligned(16))) float s_p1[M];
    __shared__ __attribute__((aligned(16))) float s_q[DH];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, hl = lane >> 5;
    const int bh = blockIdx.y, b = bh / g.h, hd = bh % g.h, D = g.h * DH;
    const long LD = g.lm_ld;
    const int nblk = g.n_p / 32;
    const T* lmb = lm + (long)b * M * LD + hd * DH;                        // q_l rows of this head; k_l rows at + D
    const T* qb = qkv + (long)b * g.n_p * 3 * D + hd * DH;                 // q rows; k rows at + D
    const T* kb = qb + D;
    const float* mrb = MASKED ? g.mrow + (long)b * g.n_p : nullptr;
    const float* mlb = MASKED ? g.mlm + (long)b * M : nullptr;
    // ---- q_l -> LDS image, q[cls_row] -> f32
    constexpr int VE = 16 / sizeof(T), CPR = DH / VE;                      // elements per 16-byte piece, pieces per row
    for (int cid = tid; cid < M * CPR; cid += CT) {
        const int r = cid / CPR, cc = cid % CPR;
        *reinterpret_cast<u32x4*>(s_ql_ + r * P + cc * VE) = *reinterpret_cast<const u32x4*>(lmb + (long)r * LD + cc * VE);
    }
    if (tid < DH) s_q[tid] = ldf<T>(qb + (long)g.cls_row * 3 * D + tid);
    __syncthreads();
    // ---- pass 1 (no lse3 given): row log-sum-exp of sim3 over all keys.  S^T[key][landmark]: the landmark on the lane
    if (lse3 == nullptr) {
        float mrun[LB], lrun[LB];
#pragma unroll
        for (int lb = 0; lb < LB; lb++) { mrun[lb] = C_NEG_BIG; lrun[lb] = 0.f; }
#pragma unroll 1
        for (int rb = wave; rb < nblk; rb += 4) {
            int opq = 0;
            asm volatile("" : "+v"(opq));       // the q_l fragments do not depend on the block: keep their LDS reads inside the loop
            const T* s_ql = s_ql_ + opq;
            typename O::frag kf[KSTEPS];
            const T* krow = kb + (long)(32 * rb + c) * 3 * D;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) kf[ks] = O::ld(krow, ks, hl);
            f32x16 vr = c_zero16();
            if (MASKED) vr = c_rowvals16(mrb + 32 * rb, hl);
#pragma unroll
            for (int lb = 0; lb < LB; lb++) {
                f32x16 s = c_zero16();
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ks++) s = O::mma(kf[ks], O::ld(s_ql + (32 * lb + c) * P, ks, hl), s);
                s = s * g.scale2;
                if (MASKED) {
#pragma unroll
                    for (int e = 0; e < 16; e++) s[e] = vr[e] != 0.f ? s[e] : C_NEG_BIG;
                }
                float mx = s[0];
#pragma unroll
                for (int e = 1; e < 16; e++) mx = fmaxf(mx, s[e]);
                const float mnew = fmaxf(mrun[lb], mx);
                float sum = 0.f;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const float ex = __builtin_amdgcn_exp2f(s[e] - mnew);
                    sum += (!MASKED || vr[e] != 0.f) ? ex : 0.f;
                }
                lrun[lb] = lrun[lb] * __builtin_amdgcn_exp2f(mrun[lb] - mnew) + sum;
                mrun[lb] = mnew;
            }
        }
        // the two lane halves, then the four waves one after the other through s_nl_ (maxima) / s_u_ (sums)
#pragma unroll
        for (int lb = 0; lb < LB; lb++) {
            const float m2 = __shfl_xor(mrun[lb], 32, 64), l2 = __shfl_xor(lrun[lb], 32, 64);
            const float mm = fmaxf(mrun[lb], m2);
            lrun[lb] = lrun[lb] * __builtin_amdgcn_exp2f(mrun[lb] - mm) + l2 * __builtin_amdgcn_exp2f(m2 - mm);
            mrun[lb] = mm;
        }
        for (int w = 0; w < 4; w++) {
            if (wave == w && hl == 0) {
#pragma unroll
                for (int lb = 0; lb < LB; lb++) {
                    const int j = 32 * lb + c;
                    if (w == 0) { s_nl_[j] = mrun[lb]; s_u_[j] = lrun[lb]; }
                    else {
                        const float m0 = s_nl_[j], l0 = s_u_[j], mm = fmaxf(m0, mrun[lb]);
                        s_nl_[j] = mm;
                        s_u_[j] = l0 * __builtin_amdgcn_exp2f(m0 - mm) + lrun[lb] * __builtin_amdgcn_exp2f(mrun[lb] - mm);
                    }
                }
            }
            __syncthreads();
        }
        for (int j = tid; j < M; j += CT) s_nl_[j] = -(s_nl_[j] + __log2f(s_u_[j]));
    } else {
        for (int j = tid; j < M; j += CT) s_nl_[j] = -lse3[(long)bh * M + j] * C_LOG2E;
    }
    __syncthreads();
    // ---- p1 = softmax_j(scale q[cls_row] . k_l[j]); an invalid pair is filled before the softmax, a fully masked row is uniform
    const bool cls_ok = !MASKED || mrb[g.cls_row] != 0.f;
    constexpr int JT = (M + CT - 1) / CT;
    float lg[JT], mx = C_NEG_BIG;
#pragma unroll
    for (int t = 0; t < JT; t++) {
        const int j = tid + t * CT;
        lg[t] = C_NEG_BIG;
        if (j < M) {
            const T* kl = lmb + (long)j * LD + D;
            float acc = 0.f;
#pragma unroll 4
            for (int d = 0; d < DH; d += 4) {
                const f4_t x = ld4<T>(kl + d);
                const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + d);
                acc += x[0] * qv[0] + x[1] * qv[1] + x[2] * qv[2] + x[3] * qv[3];
            }
            const bool ok = cls_ok && (!MASKED || mlb[j] != 0.f);
            lg[t] = ok ? acc * g.scale2 : C_NEG_BIG;
            mx = fmaxf(mx, lg[t]);
        }
    }
    mx = block_max256(mx, s_red);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < JT; t++) {
        const int j = tid + t * CT;
        if (j < M) {
            lg[t] = mx <= C_NEG_BIG ? 1.f : __builtin_amdgcn_exp2f(lg[t] - mx);      // (an invalid logit beside a valid one: exp2(-1e30) = 0)
            sum += lg[t];
        }
    }
    sum = block_sum256(sum, s_red);
    const float inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < JT; t++) {
        const int j = tid + t * CT;
        if (j < M) s_p1[j] = lg[t] * inv;
    }
    __syncthreads();
    // ---- u = p1 Z
    if (g.z_colmajor) {      // zfT[j][i] = Z[i][j], bf16: a wave per output, the lanes along i
        const bf16_t* zb = reinterpret_cast<const bf16_t*>(Z) + (long)bh * M * M;
        for (int j = wave; j < M; j += 4) {
            const bf16_t* zr = zb + (long)j * M;
            float acc = 0.f;
#pragma unroll
            for (int i = 2 * lane; i < M; i += 128) {
                const unsigned w = *reinterpret_cast<const unsigned*>(zr + i);
                acc += __uint_as_float(w << 16) * s_p1[i] + __uint_as_float(w & 0xffff0000u) * s_p1[i + 1];
            }
            acc = wave_sum(acc);
            if (lane == 0) s_u_[j] = acc;
        }
    } else {                 // Z[i][j] f32: a thread per output, coalesced along j
        const float* zb = reinterpret_cast<const float*>(Z) + (long)bh * M * M;
        for (int j = tid; j < M; j += CT) {
            float acc = 0.f;
#pragma unroll 8
            for (int i = 0; i < M; i++) acc += s_p1[i] * zb[(long)i * M + j];
            s_u_[j] = acc;
        }
    }
    __syncthreads();
    // an invalid landmark's attn3 row is uniform: its u goes to every position as one constant and leaves the walk
    float unif = 0.f;
    if (MASKED) {
        float part = 0.f;
        for (int j = tid; j < M; j += CT) {
            if (mlb[j] == 0.f) {
                part += s_u_[j];
                s_u_[j] = 0.f;
                s_nl_[j] = C_NEG_BIG;
            }
        }
        unif = block_sum256(part, s_red) / (float)g.n_p;
        __syncthreads();
    }
    // ---- the walk: S[landmark][key], the key on the lane
    float* rowb = row + (long)bh * g.n_p;
#pragma unroll 1
    for (int rb = 4 * blockIdx.x + wave; rb < nblk; rb += 4 * gridDim.x) {
        int opq = 0;
        asm volatile("" : "+v"(opq));
        const T* s_ql = s_ql_ + opq;
        const float* s_u = s_u_ + opq;
        const float* s_nl = s_nl_ + opq;
        const int n = 32 * rb + c;
        typename O::frag kf[KSTEPS];
        const T* krow = kb + (long)n * 3 * D;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) kf[ks] = O::ld(krow, ks, hl);
        const float mr = MASKED ? mrb[n] : 1.f;
        float acc = 0.f;
#pragma unroll 2
        for (int lb = 0; lb < LB; lb++) {
            f32x16 s = c_zero16();
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) s = O::mma(O::ld(s_ql + (32 * lb + c) * P, ks, hl), kf[ks], s);
            const f32x16 uv = c_rowvals16(s_u + 32 * lb, hl), nl = c_rowvals16(s_nl + 32 * lb, hl);
            s = s * g.scale2 + nl;
            float part = 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) part += uv[e] * __builtin_amdgcn_exp2f(s[e]);
            acc += part;
        }
        acc += __shfl_xor(acc, 32, 64);
        acc += unif;
        if (MASKED) acc = mr != 0.f ? acc : 0.f;
        if (hl == 0) rowb[n] = acc;
    }
}

int cls_walkers(int BH, int n_p) {
    int w = 1;
    while (BH * w < 512 && 4 * w * 2 <= n_p / 32) w *= 2;
    return w;
}

template <typename T, int DH, int M>
void cls_launch(const void* qkv, const void* lm, const void* z, const float* lse3, float* row, const ClsGeo& g, int B, hipStream_t s) {
    const dim3 grid(lse3 ? cls_walkers(B * g.h, g.n_p) : 1, B * g.h);      // (no lse3: the first pass is per workgroup, see the header)
    if (g.mrow) hipLaunchKernelGGL((nys_cls_kernel<T, DH, M, true>), grid, dim3(CT), 0, s, (const T*)qkv, (const T*)lm, z, lse3, row, g);
    else hipLaunchKernelGGL((nys_cls_kernel<T, DH, M, false>), grid, dim3(CT), 0, s, (const T*)qkv, (const T*)lm, z, lse3, row, g);
}

}  // namespace

extern "C" int mh_nys_cls_attn(const void* qkv, const void* lm, const void* z, const float* lse3, float* row, const float* mrow,
                               const float* mlm, int B, int h, int n_p, int m, int dh, int cls_row, float scale, int64_t lm_ld,
                               int z_colmajor, int dt, mh_stream s) {
    MH_REQUIRE(dt == MH_F32 || dt == MH_BF16, "mh_nys_cls_attn: dt must be MH_F32 or MH_BF16 (got %d)", dt);
    MH_REQUIRE((dh == 64 && m == 256) || (dh == 96 && m == 384),
               "mh_nys_cls_attn: built for (dh, m) = (64, 256) and (96, 384), bf16 or f32 (got dh=%d m=%d)", dh, m);
    MH_REQUIRE(B >= 0 && h >= 1 && n_p >= m && n_p % m == 0, "mh_nys_cls_attn: n_p=%d must be a positive multiple of m=%d", n_p, m);
    MH_REQUIRE(cls_row >= 0 && cls_row < n_p, "mh_nys_cls_attn: cls_row=%d outside [0, %d)", cls_row, n_p);
    MH_REQUIRE((mrow == nullptr) == (mlm == nullptr), "mh_nys_cls_attn: mrow and mlm go together");
    MH_REQUIRE(lm_ld == 0 || (lm_ld >= 2L * h * dh && lm_ld % 8 == 0), "mh_nys_cls_attn: lm_ld must be 0 or a multiple of 8 >= 2 D");
    MH_REQUIRE(z_colmajor == 0 || z_colmajor == 1, "mh_nys_cls_attn: z_colmajor is 0 (f32 row-major Z) or 1 (bf16 column-major Z)");
    if (B == 0) return MH_OK;
    MH_REQUIRE(qkv && lm && z && row, "mh_nys_cls_attn: qkv, lm, z and row are needed");
    MH_REQUIRE(((((uintptr_t)qkv) | ((uintptr_t)lm) | ((uintptr_t)z) | ((uintptr_t)mrow)) & 15) == 0,
               "mh_nys_cls_attn: qkv, lm, z and mrow must be 16-byte aligned");
    const ClsGeo g{h, n_p, cls_row, scale, scale * C_LOG2E, lm_ld > 0 ? (long)lm_ld : 2L * h * dh, mrow, mlm, z_colmajor};
    const hipStream_t st = (hipStream_t)s;
    if (dt == MH_BF16) {
        if (dh == 64) cls_launch<bf16_t, 64, 256>(qkv, lm, z, lse3, row, g, B, st);
        else cls_launch<bf16_t, 96, 384>(qkv, lm, z, lse3, row, g, B, st);
    } else {
        if (dh == 64) cls_launch<float, 64, 256>(qkv, lm, z, lse3, row, g, B, st);
        else cls_launch<float, 96, 384>(qkv, lm, z, lse3, row, g, B, st);
    }
    MH_LAUNCH_CHECK("mh_nys_cls_attn");
    return MH_OK;
}
