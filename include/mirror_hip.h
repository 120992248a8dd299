/* libmirror_hip.so — C ABI of the MI355X (gfx950) kernels behind the MIRROR pre-training hot path.
 *
 * The reference (TianyiFranklinWang/MIRROR) contains no native code: every entry point below
 * replaces the ATen ops that one reference call site dispatches (file:line are relative to the
 * reference tree; [3P] = arithmetic that lives in the pip packages nystrom_attention~=0.0.14 /
 * timm~=1.0.15, called from the cited line).  The Python host (mirror_amd/) binds these with
 * ctypes and wraps them in torch.autograd.Function; INTEGRATION.md shows the binding.
 *
 * Contract: plain device pointers + sizes, explicit dtypes, caller-owned memory
 * and workspaces, a hipStream_t per call, int status return (0 ok, <0 error, text via
 * mh_last_error()); no allocation, no synchronisation, no exceptions; re-entrant across streams.
 */
#ifndef MIRROR_HIP_H
#define MIRROR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_OK 0
#define MH_EINVAL (-1)
#define MH_EUNSUP (-2)
#define MH_EHIP (-3)

#define MH_F32 0
#define MH_BF16 1

#define MH_ACT_NONE 0
#define MH_ACT_RELU 1
#define MH_ACT_GELU 2

typedef void* mh_stream; /* hipStream_t */

const char* mh_last_error(void);
int mh_version(void);       /* 123 */
int mh_exp_build(void);      /* 1: built with -DMH_EXP (timing-experiment switches compiled in); the shipped build returns 0 */
/* number of visible HIP devices whose arch is gfx950; <=0 means the library cannot run here */
int mh_device_ok(void);
/* Which of its kernels the calling thread's last elementwise / row-kernel entry point launched: "<entry>:<form>", e.g. "add:quad",
 * "softmax_fwd:block,scalar", "layernorm_bwd:ws", "colsum:bf16oct", or "<entry>:none" for a call that returned before any launch.
 * The kernels that walk the token sequence note theirs the same way: "ppeg_fwd:pair" / ":strip", "ppeg_wgrad:strip", "ppeg_bwd:one" /
 * ":one,drop", "resconv_fwd:mfma" / ":vec" / ":scalar", "resconv_wgrad:mfma" / ":vec8" / ":scalar", "resconv_bwd:mfma" / ":two_pass"
 * (written after the two entry points it forwards to), "landmark_fwd:quad" / ":scalar", "landmark_bwd:oct" / ":scalar"; a call that
 * was refused (MH_EINVAL) has noted "<entry>:none" as well.
 * The fused loss notes the branches its kernels take: "loss_terms_fwd:<align>,<cluster>" with <align> = "ext" (no rank-local alignment
 * term), "quad" (D % 4 == 0) or "scalar" staging of the embeddings and <cluster> = "regs" (P <= 4096: the score row in registers) or
 * "global"; "loss_terms_bwd:<align>,<cluster>" with <align> = "ext", "bm16" (B <= 16) or "bm32"; ":none" when the call was refused.
 * mh_note_form is what the entry points call beside the launch they pick: it keeps the POINTER (string literals only), one store. */
void mh_note_form(const char* literal);
const char* mh_last_form(void);

/* ---------------------------------------------------------------- MFMA GEMM (all contractions)
 * C[z] (+)= act(alpha * op(A[z]) x op(B[z]) + diag*I + bias + rcoef*R[z])   z = (b1, b2) two-level batch
 *   A(m,k) at A[m*lda + k] if a_kc else A[k*lda + m];  B(k,n) at B[n*ldb + k] if b_kc else B[k*ldb + n]
 *   mma = MH_F32  -> v_mfma_f32_32x32x2_f32 (exact fp32, parity mode; dtA=dtB=dtC=f32)
 *   mma = MH_BF16 -> v_mfma_f32_32x32x16_bf16, fp32 accumulate; f32 operands are rounded to bf16
 *                    while being staged into LDS (dtA must equal dtB)
 * Replaces: nn.Linear fwd/bwd (models/mirror.py:346, :70-74, :470-495, :594-605, :823-827),
 * [3P] NystromAttention's to_qkv / einsum similarities / attn@v / pinv matmuls / to_out
 * (models/mirror.py:312), ClipLoss logits (losses/mirror_loss.py:39-40).                      */
/* Fused epilogues of the 256 x 256-tile projection GEMM (mh_gemm_desc.epi; NULL = none).  Each replaces an elementwise pass
 * (and its HBM round trip) that the reference runs as a separate op behind an nn.Linear; the call fails with MH_EINVAL when
 * the shape is not on that kernel (bf16 operands, N % 256 == 0, K % 64 == 0, M > 256, no split-K / accumulate / R / diag), and
 * the host then runs the composed ops.  The Linear's result is rounded to bf16 (the activation dtype autocast gives it)
 * before the fused op, so fused == composed bit for bit.
 *   MH_EPI_DROPADD: C[f32] = resid + Dropout_p(A W^T + bias)         [3P] to_out = Sequential(Linear, Dropout) and the residual
 *                   add of TransLayer.forward, models/mirror.py:312-313.  The mask is mh_dropout_lite's: element i of C (flat,
 *                   C contiguous: ldc == N) uses 16-bit field i & 7 of the Philox4x32-7 block with counter (offset + i) >> 3.
 *   MH_EPI_MASKPOS: C[f32] = (t >= first && mask[b, t - first] ? token : A W^T + bias) + pos[t]      retention_embed followed by
 *                   random_masking's mask-token select and `+ retention_gene_embed`, models/mirror.py:636-643, :691-693;
 *                   flat row r of C is (b, t) = (r / rows_per_batch, r % rows_per_batch).
 *   MH_EPI_SQERR:   C[bf16] = A W^T + bias as usual, and sq[0] += sum over rows with mask[b, t] != 0 of mean_D (C - tgt)^2,
 *                   sq[1] += the number of such rows: mh_mse_masked_fwd's accumulator, filled by the projection that produces the
 *                   prediction (tgt f32 at tgt + b * tgt_bs + t * D + col; rows_per_batch % 256 == 0)
 *                   retention_head + the masked MSE of MIRRORLoss.forward, losses/mirror_loss.py:98-103. */
#define MH_EPI_NONE 0
#define MH_EPI_DROPADD 1
#define MH_EPI_MASKPOS 2
#define MH_EPI_SQERR 3
typedef struct {
    int32_t kind;
    const float* resid;           /* DROPADD: residual stream, C's shape and layout */
    float p; uint64_t seed, offset; const uint64_t* dev_base;      /* DROPADD: as mh_dropout_lite */
    const float* mask;            /* MASKPOS: [batches, rows_per_batch - first]; SQERR: [batches, rows_per_batch] (f32, != 0 = masked) */
    const float* token;           /* MASKPOS: [N] */
    const float* pos;             /* MASKPOS: [rows_per_batch, N] */
    int32_t rows_per_batch, first;
    const float* tgt; int64_t tgt_bs;      /* SQERR */
    float* sq;                    /* SQERR: 2 f32, accumulated with atomics (caller zeroes) */
} mh_gemm_epi;

typedef struct {
    const void* A; const void* B; void* C;
    const float* bias;            /* [N] f32 or NULL */
    int32_t M, N, K;
    int64_t lda, ldb, ldc;
    int32_t a_kc, b_kc;
    int32_t dtA, dtB, dtC, mma;
    int32_t batch1, batch2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2;   /* element strides of the two batch levels */
    float alpha, diag;
    int32_t act;                  /* MH_ACT_* (needs split_k == 1) */
    int32_t accumulate;           /* 0: C = r, 1: C += r */
    int32_t split_k;              /* >1: K split over workgroups, f32 atomics into C (needs accumulate=1, dtC=f32).
                                     A batch whose sC1 = sC2 = 0 with accumulate=1 also reduces into C with atomics. */
    const void* R; float rcoef;   /* optional addend: C (+)= ... + rcoef * R; R has C's dtype, ldc and batch strides
                                     (lets the pinv polynomial 15I - 7P + P.P come out of one launch) */
    float* workspace;             /* optional scratch for reductions into one C (split-K, batch broadcast): with at least
                                     mh_gemm_workspace_bytes(d) BYTES = parts * M * N * 2 (parts = splits * batch) the large-tile kernel
                                     writes plain partial tiles there and a fold pass adds them to C in f32.  The partial tiles are
                                     **bf16**: every K-slice's f32 accumulator is rounded ONCE on its way to the workspace, so an element
                                     of C carries an extra error <= parts * 2^-9 * max_slice |partial| (relative to the largest partial,
                                     not to the final sum: slices that cancel keep their rounding).  NULL / too small: f32 atomics (exact
                                     f32 partial sums, summation order not reproducible) — the caller's precision policy chooses
                                     (mirror_amd: kernels.SPLITK_PARTIALS, env MIRROR_SPLITK_PARTIALS=f32) */
    int64_t workspace_floats;     /* size of `workspace` in 4-byte units (the buffer is typed float* for alignment only) */
    void* C2;                     /* optional bf16 copy of the final C (C's ldc and batch strides), written by the same epilogue:
                                     the next product's operand without a cast launch.  192 x 384 tile kernel only (bf16
                                     operands, M % 192 == 0, N % 384 == 0, K % 64 == 0, no bias / activation / split-K) */
    int32_t r_bf16;               /* 1: R is bf16 although C is f32; 2 (v118): R is f32 although C is bf16 — a sum kept in f32 whose
                                   * next consumer reads bf16 leaves as bf16 without the f32 read-modify-write (same tile kernel only) */
    int32_t k_segments;           /* > 1: C = sum_s A_s B_s over k_segments operand pairs of K each, A_s = A + s * sA_seg, B_s = B + s * sB_seg
                                     (elements): a sum of products in one accumulator, e.g. dX = sum_k dP_k z_k^T of the pinv reverse
                                     mode without an f32 read-modify-write of C per term.  Same tile kernel only; 0 / 1: one pair */
    int64_t sA_seg, sB_seg;
    int32_t row_softmax;          /* 1: C = softmax over each row of alpha * A B, written as bf16 (N == 384 = one tile row of the same
                                     tile kernel; no R / accumulate / diag / C2): sim1 = q k_l^T of the template geometry (m = 384
                                     landmarks, models/mirror.py:312 [3P] `attn1 = sim1.softmax(dim=-1)`) without the f32 logits round trip;
                                     2: its backward, C = P o (alpha A B - rowsum(P o alpha A B)) with the probabilities P given as R (bf16) */
    const mh_gemm_epi* epi;       /* optional fused epilogue (above); NULL: none */
    int32_t a_rows_per_batch, a_row_skip;   /* > 0: A's M rows are `a_rows_per_batch`-row windows of larger batches: flat row r lives at
                                     A row r + (r / a_rows_per_batch) * a_row_skip (a_kc = 1 only).  Lets `to_out(out)[:, -n:]` and
                                     `retention_head(x)[:, 1:]` run as ONE flat problem instead of a batched one with a ragged tile per slide */
    int32_t shared_chip;          /* hint: != 0 when another stream's kernel shares the chip with this launch (the half-chip pinv chain):
                                     the persistent kernel (one workgroup per CU for the whole launch) would keep the other kernel's
                                     workgroups from being scheduled until it ends, so the one-workgroup-per-tile kernel is used */
    int32_t c_rows_per_batch, c_row_skip;   /* > 0 (bf16 C, with or without a_rows_per_batch, no `epi`): flat row r of the result is written to
                                     C row r + (r / c_rows_per_batch) * c_row_skip.  [3P] NystromAttention pads the sequence in FRONT
                                     (`F.pad(x, (0, 0, padding, 0))`, called at models/mirror.py:312): to_qkv of the pad rows is zero (no
                                     bias), so only the B x n real rows are multiplied, as one flat problem from and into the padded buffers
                                     (its data gradient likewise) */
    int32_t window_batches;       /* > 0: the row windows above cover `window_batches` batches only; flat rows past them follow the last
                                     window without a gap (row r lives at r + min(r / rows_per_batch, window_batches - 1) * row_skip).
                                     The landmark rows of a Nystrom layer sit behind the padded sequences of all slides in to_qkv's
                                     operand / result buffers and are multiplied by the same launch.  0: every flat row is window row */
} mh_gemm_desc;
int mh_gemm(const mh_gemm_desc* d, mh_stream s);
/* The kernel instance the calling thread's last mh_gemm call launched (e.g. "gemm_pq_kernel<float,false,false,part>",
 * "gemm_kernel<1,bf16,bf16,float,true,false,2,2,1>"): lets a profiler name launches without restating the dispatch rules. */
const char* mh_gemm_variant_name(void);
/* Bytes of `workspace` with which this call reduces through plain **bf16** partial tiles (parts * M * N * 2) + an f32 fold pass
 * instead of f32 atomics (0: the call has no use for one — no split-K / batch broadcast, fewer than 8 parts, or the shape is not
 * on the large-tile kernel). */
int64_t mh_gemm_workspace_bytes(const mh_gemm_desc* d);

/* ---------------------------------------------------------------- skinny-M linears (RNA encoder / style heads: every
 * tensor is [B, D], models/mirror.py:77-102, :217-224, :845-857): weight-streaming kernels, bf16 operands.
 * y[M<=32, N] = act(x[M,K] W[N,K]^T + bias + addend); K % 32 == 0 with 16-byte aligned rows streams 16-byte fragments, any other K / row
 * stride (the template's 10234 genes and 1975-wide MLP, configs/pretrain/mirror.template.yaml:27-46) the same kernel element-wise
 * (v116+); the data gradient is the same call on the W^T shadow, and
 * `addend` (nullable f32 [M, N], row stride ldadd) is how the data gradients of two linears that read the same x are summed
 * without a launch of their own (style_mu / style_logstd, models/mirror.py:845-857). */
int mh_skinny_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, const float* addend, int64_t ldadd,
                  void* y, int64_t ldy, int M, int N, int K, int act, int dt_x, int dt_y, mh_stream s);      /* x bf16, or f32 rounded to bf16 on load */
/* dW[N,K] (+)= dy[M,N]^T x[M,K]  (f32, plain read-modify-write: one block owns each output tile) */
int mh_skinny_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, float* db, int M, int N,
                    int K, int accumulate, int dt_dy, int dt_x, mh_stream s);   /* db (optional, [N] f32): db += column sums of dy (the bias gradient) */
/* Up to MH_SKINNY_MANY_MAX of those weight gradients in ONE launch (always accumulating: dW += dy^T x, db += column sums of dy):
 * the backward of the [B, D]-row linears queues its (dy, x) pairs and one grid covers the tiles of all of them. */
#define MH_SKINNY_MANY_MAX 32
typedef struct {
    const void* dy; int64_t lddy;     /* [M, N] bf16 (or f32, rounded to bf16 on load: dt_dy) */
    const void* x; int64_t ldx;       /* [M, K] bf16 (or f32: dt_x) */
    float* dw; int64_t lddw;          /* [N, K] f32, 16-byte aligned */
    float* db;                        /* [N] f32 or NULL */
    int32_t M, N, K;
    int32_t dt_dy, dt_x;              /* MH_BF16 / MH_F32 */
} mh_skinny_wgrad_item;
int mh_skinny_wgrad_many(const mh_skinny_wgrad_item* items, int n, mh_stream s);
/* bf16 [R,C] -> [C,R]; the batched form walks table[i] = {src_off, dst_off, R, C} (int64 element offsets).
 * vec_ok != 0: every entry has R % 8 == 0, C % 8 == 0 and offsets that are multiples of 8 (16-byte accesses) */
int mh_transpose_bf16(const void* in, void* out, int R, int C, mh_stream s);
int mh_transpose_bf16_many(const void* src, void* dst, const int64_t* table, int n, int max_r, int max_c, int vec_ok,
                           mh_stream s);

/* ---------------------------------------------------------------- LayerNorm (models/mirror.py:298, :350, :604, :210)
 * rows are addressed as (b, i): x + b*x_bs + i*D, y + b*y_bs + i*D, i < rows_per_batch (lets the
 * output land inside the front-zero-padded Nystrom buffer, or skip the square-pad rows :679). */
int mh_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     int batches, int rows_per_batch, int D, int64_t x_bs, int64_t y_bs, float eps,
                     int dt_x, int dt_y, mh_stream s);
/* f32 output y plus a bf16 copy y_bf16 (same row addressing) in one pass: the encoder's final norm (models/mirror.py:679) feeds
 * f32 consumers (retention target :699, cls row :684) and the bf16 operand of retention_embed (:690).  D % 4 == 0, D <= 2048. */
int mh_layernorm_fwd_dual(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16, float* mean, float* rstd,
                          int batches, int rows_per_batch, int D, int64_t x_bs, int64_t y_bs, float eps, mh_stream s);
/* the same with an e4m3 copy of the output beside the bf16 one (x f32, y bf16; q8 has y's row addressing, one byte per element):
 * delayed per-tensor scaling as in mh_quant_fp8_delayed (ring: 3 uint32 of this call site, tick: device step counter), scale[0] =
 * the dequantisation factor.  Config 5: the fp8 forward of [3P] to_qkv reads q8, its weight gradient the bf16 copy. */
int mh_layernorm_fwd_q8(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                        int batches, int rows_per_batch, int D, int64_t x_bs, int64_t y_bs, float eps, void* q8, unsigned* ring,
                        const float* tick, float margin, float* scale, mh_stream s);
/* LayerNorm backward: ONE entry point, described by a zero-initialised mh_ln_bwd.  dx = d loss / d x; dgamma / dbeta are accumulated
 * (+=, f32; the caller zeroes them); dy uses y's addressing.  Beside the base block the descriptor holds four optional riders, work
 * of a neighbouring op done while this launch holds the operands.  A rider is present exactly when its lead pointer is non-NULL; an
 * all-zero rider block means absent (l == 0 beside gadd == NULL is l = 1).  Accepted combinations: none; landmark; landmark + ReLU;
 * fan; drop; drop + fan.  Anything else, or a rider whose conditions below do not hold, is refused with MH_EINVAL before the first
 * launch: a refused call has touched nothing.
 * Every rider needs the WORKSPACE FORM: D % 4 == 0, x_bs % 4 == y_bs % 4 == 0, dy / x / dx / gamma 16-byte aligned, >= 64 rows and
 * a workspace of >= 2 D floats (3 D where said).  A call without a rider that is off that form runs on the same-address-atomics forms. */
int64_t mh_layernorm_bwd_workspace_bytes(int64_t rows, int D);      /* full-speed size of mh_ln_bwd.workspace */
typedef struct {
    /* ---- base */
    const void* dy;               /* dt_dy */
    const void* x;                /* dt_x */
    const float *gamma, *mean, *rstd;
    void* dx;                     /* dt_dx == dt_x */
    float *dgamma, *dbeta;        /* [D] f32, += */
    int32_t batches, rows_per_batch, D;
    int64_t x_bs, y_bs;           /* elements per batch of x / dx and of dy */
    int32_t dt_x, dt_dy, dt_dx;   /* MH_F32 / MH_BF16 */
    int32_t accumulate_dx;        /* dx += instead of dx = */
    float* workspace;             /* optional, f32: per-block dgamma / dbeta partials are written there and folded by a second small */
    int64_t ws_floats;            /* launch instead of thousands of same-address atomics; 2 D min(rows / 16, 1024) floats for full speed */
    /* ---- landmark rider: the backward of mh_layernorm_fwd_lm.  dy row i of batch b also receives gadd[b, (i + pad) / l] / l, where
     * gadd [batches, (pad + rows_per_batch) / l, D] in dy's dtype, 16-byte aligned, = d loss / d xpm; l >= 1, pad >= 0,
     * (pad + rows_per_batch) % l == 0.  row_mask / lm_scale (nullable, need gadd): the forward's mask and scale (see there) */
    const void* gadd;
    int32_t pad, l;
    const float* row_mask;        /* f32 [batches, pad + rows_per_batch]: a masked row's total dy is zero */
    const float* lm_scale;        /* f32 [batches, (pad + rows_per_batch) / l]: multiplies the group's gadd */
    /* ---- ReLU rider (needs gadd; f32 x, bf16 dy, D % 4 == 0): x rows [relu_first, relu_first + relu_rows) of every batch, a range
     * inside the batch, are the output of a ReLU (`_fc1 = Linear + ReLU`, models/mirror.py:346, :652-654, feeds layer 1's norm):
     * their total gradient is written to relu_out (bf16 [batches, relu_rows, D], 8-byte aligned) as x > 0 ? dx : 0, the operand of
     * _fc1's weight gradient, and NOT as f32 dx (no separate ReLU-backward pass); the other rows (cls) keep their f32 dx */
    void* relu_out;
    int32_t relu_first, relu_rows;
    float* relu_db;               /* nullable, f32 [D], needs relu_out and a 16-byte aligned workspace of >= 3 D floats: += the column
                                     sums of relu_out as stored, _fc1's bias gradient, a third partial row (no mh_colsum pass) */
    /* ---- fan rider (excludes gadd; f32 x / dx, dy f32 or bf16, rows_per_batch >= 2, D % 4 == 0): the LayerNorm output fans out (the
     * WSI encoder's final norm: decoder input, retention target = rows 1.., cls row; models/mirror.py:684-700, :833).  dy row i >= 1
     * of batch b also receives fan_alpha * fan_bf16[b, i - 1] (bf16 [batches, rows_per_batch - 1, D], 8-byte aligned: the masked MSE
     * hands its target gradient over as -dpred) and row 0 fan_cls[b] — the three-way sum mh_fanout_bwd writes is formed while this
     * launch reads its operands */
    const void* fan_bf16;
    float fan_alpha;
    const float* fan_cls;         /* nullable, f32 [batches, D], 16-byte aligned */
    /* ---- drop rider (excludes gadd, may carry the fan rider; f32 x / dx, dy f32 or bf16, D % 8 == 0, D <= 1024, a 16-byte aligned
     * workspace of >= 3 D floats): x is the output of `resid + Dropout_p(Linear(core))` ([3P] to_out = Sequential(Linear, Dropout)
     * and TransLayer's residual add, models/mirror.py:312), so this launch's dx is that Dropout's upstream gradient: drop_out
     * (bf16 [batches, drop_rows_per_batch, D], 8-byte aligned) receives mask * dx / (1 - p) on the lite Philox stream (the masks
     * mh_gemm_epi DROPADD drew for (seed, offset + *dev_base, element)), the operand of to_out's two gradient products, and drop_db
     * its column sums: mh_dropout_lite_colsum's pass over dx is not launched */
    void* drop_out;
    float drop_p;                 /* in [0, 1) */
    uint64_t drop_seed, drop_offset;        /* drop_offset % 8 == 0 */
    const uint64_t* drop_base;    /* nullable device-side base added to drop_offset */
    float* drop_db;               /* required, f32 [D]: += to_out's bias gradient */
    int32_t drop_rows_per_batch;  /* >= rows_per_batch: rows per batch of the Dropout's tensor; a norm over the first rows of a
                                     square-padded sequence leaves the rows behind them to the caller (zeros) */
} mh_ln_bwd;
int mh_layernorm_bwd(const mh_ln_bwd* d, mh_stream s);

/* LayerNorm of a Nystrom layer that also leaves the landmark means of its output (models/mirror.py:298 + [3P] NystromAttention's
 * front padding and `q_landmarks = reduce(q, '... (n l) d -> ... n d', 'sum') / l`): x f32 [batches, >= rows, D] (x_bs elements per
 * batch) -> y bf16 [batches, pad + rows, D] (pad zero rows first, written here) and xpm f32 [batches, (pad + rows) / l, D] =
 * the mean of each group of l consecutive rows of y.  to_qkv is linear and bias-free, so the landmarks are to_qkv(xpm)[:, :2D].
 * Its backward is mh_layernorm_bwd with the landmark rider (gadd = d loss / d xpm).
 * xpm (f32) may be NULL when only the bf16 means are wanted (they are the landmark rows behind the sequence in to_qkv's operand). */
int mh_layernorm_fwd_lm(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* xpm,
                        void* xpm_bf16, int batches, int rows, int D, int64_t x_bs, int pad, int l, float eps, const float* row_mask,
                        const float* lm_scale, mh_stream s);
                        /* row_mask (nullable, f32 [batches, pad + rows]; BASELINE config 4): the key-padding mask, front-padded like the
                           sequence — rows with a zero entry leave as zero rows ([3P] `q, k, v = t * mask[..., None]` through the bias-free
                           to_qkv) and stay out of their group's sum: the landmark rows are masked sums / l (the caller scales them by
                           l / valid count — or passes those factors as lm_scale, f32 [batches, (pad + rows) / l], nullable: the landmark rows then leave as
                           the masked MEANS); mh_layernorm_bwd's landmark rider takes the same mask and scale */
                        /* xpm_bf16 (optional): the bf16 rounding of xpm, the B operand of the landmark projection's weight gradient */

/* ---------------------------------------------------------------- fp8 forward projections (BASELINE config 5)
 * mh_quant_fp8: q[i] = e4m3(x[i] * 448 / max|x|) for a whole tensor (x f32 / bf16, n % 4 == 0), scale[0] = max|x| / 448
 *               (amax_scratch: one uint32 of device scratch).
 * mh_gemm_fp8 : C[z] = act(scale_a * scale_b * A[z] B^T + bias), v_mfma_f32_32x32x16_fp8_fp8, f32 accumulate.  A [batch][M, K] and
 *               B [N, K] are e4m3 bytes with K contiguous (lda, ldb, a_bs in bytes); C f32 / bf16 (ldc, c_bs in elements);
 *               K % 64 == 0, N % 128 == 0, M ragged.  Replaces the forward of nn.Linear at models/mirror.py:346 (`_fc1`), [3P]
 *               to_qkv / to_out and the retention embed / head (:595-607) under the `fp8` precision policy. */
int mh_quant_fp8(const void* x, int64_t n, void* q, float* scale, unsigned* amax_scratch, int dt, mh_stream s);
/* Delayed scaling, ONE pass: the scale is `margin` x this tensor's max |x| of the PREVIOUS step (ring: 3 uint32 of device state
 * per call site, zero-initialised; tick: device f32 holding the step counter, e.g. TrainEngine's Adam state), this step's
 * max is gathered for the next step.  Values past the e4m3 range saturate.  The first two steps of a call site (ring still
 * empty) must go through mh_quant_fp8. */
int mh_quant_fp8_delayed(const void* x, int64_t n, void* q, float* scale, unsigned* ring, const float* tick, float margin,
                         int dt, mh_stream s);
int mh_gemm_fp8(const void* A, int64_t lda, int64_t a_bs, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t c_bs, int batch,
                const float* scale_a, const float* scale_b, const float* bias, int act, int M, int N, int K, int dt_c, mh_stream s);

/* ---------------------------------------------------------------- row softmax ([3P] sim.softmax(-1); Attention :95)
 * x/y: rows x cols, row stride ld (elements). In place allowed when dtypes match. */
int mh_softmax_fwd(const void* x, void* y, int64_t rows, int cols, int64_t ldx, int64_t ldy,
                   int dt_x, int dt_y, mh_stream s);
/* dx = y * (dy - sum(dy*y)) ; in place on dy allowed */
int mh_softmax_bwd(const void* y, const void* dy, void* dx, int64_t rows, int cols, int64_t ldy, int64_t lddy,
                   int64_t lddx, int dt_y, int dt_dy, int dt_dx, mh_stream s);

/* Key-padding-mask variants ([3P] NystromAttention.forward(x, mask=...): `sim.masked_fill_(~(rowmask & colmask), -finfo.max)`
 * before each of the three softmaxes; BASELINE config 4).  x, y: contiguous [batches, h, R, cols]; rowmask [batches, R] and
 * colmask [batches, cols] hold 0 / 1 floats.  A fully masked row comes out uniform, as in the package.  bwd: dx = 0 at
 * filled entries, y (dy - sum y dy) elsewhere; in place on dy allowed. */
int mh_softmax_masked_fwd(const void* x, void* y, const float* rowmask, const float* colmask, int64_t batches, int h, int R,
                          int cols, int dt_x, int dt_y, mh_stream s);
int mh_softmax_masked_bwd(const void* y, const void* dy, void* dx, const float* rowmask, const float* colmask, int64_t batches,
                          int h, int R, int cols, int dt_y, int dt_d, mh_stream s);
/* y[r, :] = x[r, :] * scale[r] (masked rows zeroed before the bias-free to_qkv; masked-mean landmarks = sum / (count + 1e-8)) */
int mh_row_scale(const void* x, const float* scale, void* y, int64_t rows, int D, int dt, mh_stream s);
/* Key-padding plan of one Nystrom layer in one launch (BASELINE config 4; the `mask` argument of [3P] NystromAttention.forward).
 * mask: [B, n_src] bool bytes (non-zero = real patch).  The layer's sequence is [pad zeros | lead ones (cls) | mask |
 * mask[:, :wrap] (the square-pad rows of models/mirror.py:357-360)], pad + lead + n_src + wrap = m * l.  Out, all f32:
 * mrow [B, m*l] row mask, mlm [B, m] = (valid rows of the group > 0), lscale [B, m] = l * (1 / (count + 1e-8)). */
int mh_keymask_plan(const unsigned char* mask, float* mrow, float* mlm, float* lscale, int64_t B, int64_t n_src, int lead, int wrap,
                    int pad, int l, mh_stream s);

/* ---------------------------------------------------------------- Nystrom pieces ([3P], called at models/mirror.py:312)
 * qkv: [B, n_p, 3D] (q | k | v column blocks, heads are dh-wide column slices).
 * landmarks: lm[b, j, c] = mean_{t<l} qkv[b, j*l+t, c], c < 2D  -> lm [B, m, 2D]            */
int mh_landmark_fwd(const void* qkv, void* lm, int B, int n_p, int D, int l, int dt, mh_stream s);
/* dqkv[b, r, c] += dlm[b, r/l, c] / l for c < 2D */
int mh_landmark_bwd(const void* dlm, void* dqkv, int B, int n_p, int D, int l, int dt, mh_stream s);
/* out[b,t,h*dh+d] += sum_j w[h][j] * v[b, t+j-K/2, h*dh+d]; v = qkv[..., 2D:3D] (ldv = 3D), out ld = ldo.
 * transpose=1 applies the adjoint (data gradient).                                           */
int mh_resconv_fwd(const void* v, int64_t ldv, int64_t v_bs, const float* w, void* out, int64_t ldo, int64_t o_bs,
                   int B, int n_p, int heads, int dh, int taps, int transpose, int accumulate,
                   int dt_v, int dt_o, mh_stream s);
/* dw[h][j] += sum_{b,t,d} dout[b,t,h,d] * v[b,t+j-K/2,h,d]  (f32 atomics) */
int mh_resconv_wgrad(const void* v, int64_t ldv, int64_t v_bs, const void* dout, int64_t ldo, int64_t o_bs,
                     float* dw, int B, int n_p, int heads, int dh, int taps, int dt_v, int dt_o, mh_stream s);
/* Both gradients of res_conv in ONE pass over dout ([3P] `out += self.res_conv(v)`, called at models/mirror.py:312):
 *   dv[b,t,h*dh+d] += sum_j w[h][j] * dout[b, t-j+K/2, h*dh+d]      (= mh_resconv_fwd(dout -> dv, transpose=1, accumulate=1))
 *   dw[h][j]       += sum_{b,t,d} dout[b,t,h,d] * v[b,t+j-K/2,h,d]   (= mh_resconv_wgrad)
 * bf16 operands with dh = 64, 33 taps and `workspace` of mh_resconv_bwd_workspace_bytes(..) bytes: one launch over 128-row tiles
 * (the dout tile of a head sits in LDS for the adjoint conv; the tap gradient is 8 more MFMAs per 32 rows against v rows read
 * beside it, its per-tile sums go through `workspace`) + a fold launch; anything else runs the two passes above. */
int64_t mh_resconv_bwd_workspace_bytes(int B, int n_p, int heads, int dh, int taps);
int mh_resconv_bwd(const void* dout, int64_t ldo, int64_t o_bs, const void* v, int64_t ldv, int64_t v_bs, const float* w, void* dv,
                   int64_t lddv, int64_t dv_bs, float* dw, float* workspace, int64_t ws_floats, int B, int n_p, int heads, int dh,
                   int taps, int dt_v, int dt_o, mh_stream s);
/* moore_penrose_iter_pinv initial scaling: stats[0]=max_i sum_j|x|, stats[1]=max_j sum_i|x| over the
 * WHOLE [BH,m,m] tensor (couples the batch), with arg positions packed in stats64. */
int mh_pinv_absmax(const float* x, uint64_t* stats64, int BH, int m, mh_stream s);
/* z0[bh,i,j] = x[bh,j,i] / (c*r) */
int mh_pinv_z0(const float* x, const uint64_t* stats64, float* z0, int BH, int m, mh_stream s);
/* dx += dz0^T/(c r) + sub-gradients through the two max(); z0 may be NULL (m % 64 == 0): z0 = x^T / (c r) is then formed on the fly.
 * scratch1 = one device float the kernels reduce into; scratch_zeroed != 0: the caller hands it over holding 0 (no memset here) */
int mh_pinv_z0_bwd(const float* x, const float* z0, const float* dz0, const uint64_t* stats64, float* dx,
                   float* scratch1, int scratch_zeroed, int BH, int m, mh_stream s);
/* attn2's backward tail in one pass (m = 256, x = p = the softmax output of [3P] sim2, no key-padding mask): on entry dx holds the
 * chain's d loss / d x; on exit dx = d loss / d sim2-logits = softmax_bwd(p, dx + dz0^T / (c r) + max sub-gradients).  Equals
 * mh_pinv_z0_bwd(x = p, z0 = NULL) followed by mh_softmax_bwd up to the rounding of the row sums (the row maximum's constant cancels
 * in a softmax backward; the column maximum's is applied as a rank-one correction of the one matrix that holds it). */
int mh_pinv_s2_bwd(const float* p, const float* dz0, const uint64_t* stats64, float* dx, float* scratch1, int scratch_zeroed, int BH,
                   int m, const float* mlm, int heads, mh_stream s);
                   /* mlm (nullable, f32 [BH / heads, m]; BASELINE config 4): p came out of masked_fill + softmax (mh_nys_sim2(mlm) /
                      mh_softmax_masked_fwd); entries of an invalid row or column landmark receive no gradient (dx = 0 there) */
/* The whole iteration as ONE launch per pass (bf16 policy, m = 256; other sizes return MH_EINVAL and the caller
 * composes mh_gemm): one 256-thread workgroup per (b,h) walks the chain of m x m products; a wave owns 64 columns of
 * every product, its B operand never leaves the register file, A is one LDS image (pinv_panel.hip).
 * Chain-private matrices are "panel native" (PN): PN(M)[jblk][T][lane][e] = M[16T + 4hl + (e&3) + 8(e>>2)][32 jblk + c],
 * c = lane & 31, hl = lane >> 5 — the 16 bytes one lane feeds to one MFMA k-step, lanes consecutive (coalesced).
 *   prep : x [BH,m,m] f32 (attn2) + stats64 -> z0 = x^T/(c r) f32 row-major (as mh_pinv_z0), xp = PN(x),
 *          z0p = PN(z0) (the caller places it at saved[0][0])
 *   pack : dz [BH,m,m] f32 row-major (d z_iters) -> up = PN(dz^T), the backward's input
 *   fwd  : XP = xp; saved [iters][4][BH][m][m] bf16 = PN{z_k, P_k, T2_k, T3_k}; zfT[j][i] = z_iters[i][j] (column-major,
 *          i.e. the row-major transpose of the pseudo-inverse)
 *   bwd  : dzf = up; work like saved (scratch); dX (f32, row-major) = sum_k dP_k z_k^T, dz0 (f32, row-major) = d z_0 */
int mh_pinv_chain_prep(const float* x, const uint64_t* stats64, float* z0, void* xp, void* z0p, int BH, int m, mh_stream s);
int mh_pinv_chain_pack(const float* dz, void* up, int BH, int m, mh_stream s);
int mh_pinv_chain_fwd(const void* XP, void* saved, void* zfT, int BH, int m, int iters, const float* z0f, const uint64_t* stats64,
                      int z0_rowmajor, mh_stream s);     /* z0f != NULL: z_0 = z0f / (c r) (mh_nys_sim2's unscaled panel-native attn2^T, stats64 = its maxima),
                                           rounded to bf16 and written to saved[0] here; NULL: saved[0] is pre-filled (mh_pinv_chain_prep) */
/* attn2 = softmax(scale q_l k_l^T) of [3P] NystromAttention (m = 256 landmarks, dh = 64) and what moore_penrose_iter_pinv's start
 * needs from it, one launch: lm bf16 [B, m, 2 D] (q | k landmarks) -> a2 f32 [B h, m, m] row-major, xp = panel-native bf16 a2 (the
 * chain's X), z0f = panel-native f32 a2^T (unscaled z_0), stats64[0 / 1] = packed (value << 32 | flat index) maxima of the row /
 * column abs sums as mh_pinv_absmax leaves them (caller zeroes stats64).  Replaces mh_gemm + mh_softmax_fwd + mh_pinv_absmax +
 * mh_pinv_chain_prep on the fused path. */
int mh_nys_sim2(const void* lm, float* a2, void* xp, float* z0f, uint64_t* stats64, int B, int m, int D, int heads, float scale,
                int64_t lm_ld, const float* mlm, mh_stream s);
                /* lm_ld: row stride of lm in elements; 0 = contiguous [B, m, 2D] (see mh_nys_attn1_fwd).  mlm (nullable, f32 [B, m]; BASELINE
                   config 4): valid-landmark flags of the key-padding mask — entries of an invalid row or column are filled with -FLT_MAX in
                   front of the softmax ([3P] sim2.masked_fill_), z0f must then be NULL (mh_pinv_chain_fwd(z0_rowmajor) forms z_0) */
/* The two small products that open NystromAttention's backward around the chain, one launch (m = 256, dh = 64; dw2, av f32
 * [BH, m, dh], zfT bf16 [BH, m, m] = the chain's column-major output): up = PN((dw2 av^T)^T) bf16, the input of mh_pinv_chain_bwd
 * (what mh_gemm + mh_pinv_chain_pack produce), dav = Z^T dw2 bf16 [BH, m, dh].  delta3 (f32 [BH, m], may be NULL) receives
 * sum_d dav[., d] av[., d] of the rounded dav: hand it to mh_nys_attn3_bwd with av = NULL and that call skips its first launch. */
int mh_nys_dz_dav(const float* dw2, const float* av, const void* zfT, void* up, void* dav, float* delta3, int BH, int m, int dh,
                  mh_stream s);
int mh_pinv_chain_bwd(const void* XP, const void* saved, const void* dzf, void* work, float* dX, float* dz0, int BH, int m,
                      int iters, mh_stream s);
/* Bytes of the chain's caller-allocated buffers: which = 0: `saved` (forward output, backward input: [iters, 4, BH, m, m]
 * bf16 = the iterates z_k, P_k, T2_k, T3_k); which = 1: `work` (backward scratch: [iters + 4, BH, m, m] bf16 = W_k of every
 * iteration for dX, and four slots of per-iteration temporaries). */
int64_t mh_pinv_chain_workspace_bytes(int BH, int m, int iters, int which);
/* Fused attention sides of the Nystrom core (bf16 policy, dh = 64, m = 256 landmarks; anything else returns
 * MH_EINVAL and the caller composes mh_gemm + mh_softmax).  The [n_p x m] / [m x n_p] similarity matrices stay in MFMA
 * accumulators; only row statistics reach HBM.  Replaces, in [3P] NystromAttention.forward (called at
 * models/mirror.py:312): sim1/sim3 einsum + softmax + the two products with them, and their autograd.
 *   qkv [B,n_p,3D] bf16 (D = 64 h, heads are 64-wide column slices), lm [B,m,2D] bf16 = q_l | k_l,
 *   w2 [B,h,m,64] bf16, out/dout [B,n_p,D] bf16, av [B,h,m,64] f32, dav [B,h,m,64] bf16,
 *   lse1/delta1 [B,h,n_p] f32, lse3 [B,h,m] f32, dqkv like qkv, dw2 [B,h,m,64] f32, dlm [B,m,2D] f32.
 * attn1_fwd: out[:, :, head] (+)= softmax_m(scale q k_l^T) w2 (accumulate = 1 adds to what is there, e.g. the res_conv
 *            term computed while the pinv chain was running), lse1 = row logsumexp.
 * attn3_fwd: av = softmax_n(scale q_l k^T) v, lse3.
 * attn1_bwd: ONE kernel that walks the rows once (S, dP and the exponentials computed once, q / dO / o1 read once; needs every buffer).
 *   ADDS (f32 atomics) dw2 = P1^T dO and dk_l = dS1^T q into dw2 and the k_l half of dlm, WRITES delta1[b, h, n] = sum_l P1 dP1 =
 *   sum_d dO[n, d] o1[n, d] — o1 = attn1's own output rows as mh_nys_attn1_fwd(o1 = ..) saved them (the flash-attention identity) —
 *   and writes the q block of dqkv = dS1 k_l.
 * attn3_bwd: writes the k and v blocks of dqkv and delta3 [B,h,m] f32 (scratch); ADDS into the q_l half of dlm. */
/* mrow [B, n_p] / mlm [B, m] (f32 0 / 1, both or neither): the package's key-padding mask — valid sequence rows and landmark
 * groups that contain a valid row.  A logit whose row or landmark is invalid is masked_fill'ed before the softmax (a fully
 * masked row comes out uniform, as in the package) and gets no gradient.  NULL: no mask. */
/* lm_ld (all mh_nys_attn*): row stride of `lm` in elements, 0 = 2 D (a contiguous [B, m, 2D]).  3 D when the landmarks are rows of
 * to_qkv's output buffer behind the sequence (landmarks = to_qkv(group means): [3P] landmarks are means over l consecutive
 * positions of q and k, and to_qkv is linear and bias-free); batch b's landmarks start at lm + b * m * lm_ld. */
/* o1 (nullable, bf16 [B, n_p, D]): attn1's own rows softmax(scale q k_l^T) w2, WITHOUT whatever `out` held under accumulate = 1
 * (res_conv(v)): what mh_nys_attn1_bwd takes delta1 from. */
int mh_nys_attn1_fwd(const void* qkv, const void* lm, const void* w2, void* out, float* lse1, const float* mrow, const float* mlm,
                     int B, int h, int n_p, int m, int dh, float scale, int accumulate, int64_t lm_ld, void* o1, mh_stream s);
/* unmasked mh_nys_attn1_fwd that also writes the e4m3 copy q8 [B, n_p, D] bytes of `out` (delayed scaling: ring / tick / margin as
 * in mh_quant_fp8_delayed, q8_scale[0] = dequantisation factor): the fp8 forward of [3P] to_out needs no quantisation pass */
int mh_nys_attn1_fwd_q8(const void* qkv, const void* lm, const void* w2, void* out, float* lse1, int B, int h, int n_p, int m, int dh,
                        float scale, int accumulate, void* q8, unsigned* ring, const float* tick, float margin, float* q8_scale, void* o1,
                        mh_stream s);
/* attn3_fwd cuts the sequence into ranges (one workgroup each) when B*h alone would not fill the chip; the partial results
 * live in `workspace` (mh_nys_attn3_ws_floats(B, h, n_p) floats; NULL / too small: one workgroup per (b, h)). */
int64_t mh_nys_attn3_ws_floats(int B, int h, int n_p);
int64_t mh_nys_attn3_workspace_bytes(int B, int h, int n_p);         /* the same in bytes */
/* rc_w / rc_out (both or neither): [3P] `out += self.res_conv(v)` computed by the same launch — rc_w = the 33-tap filters [h][33]
 * (Conv2d(h, h, (33, 1), groups=h, bias=False), models/mirror.py:299-309), rc_out [B, n_p, D] bf16 receives res_conv(v) (every row
 * written; mh_nys_attn1_fwd(accumulate=1) then adds its product): the conv reads the v tile this kernel stages anyway. */
int mh_nys_attn3_fwd(const void* qkv, const void* lm, float* av, float* lse3, float* workspace, int64_t ws_floats,
                     const float* mrow, const float* mlm, int B, int h, int n_p, int m, int dh, float scale, int64_t lm_ld,
                     const float* rc_w, void* rc_out, mh_stream s);
int mh_nys_attn1_bwd(const void* qkv, const void* lm, const void* w2, const void* dout, const float* lse1, const void* o1, float* delta1,
                     void* dqkv, float* dw2, float* dlm, const float* mrow, const float* mlm, int B, int h, int n_p, int m, int dh,
                     float scale, int64_t lm_ld, mh_stream s);
/* av == NULL: delta3 already holds sum_d dav av (mh_nys_dz_dav wrote it); otherwise it is scratch this call fills first */
/* dk, dv and dq_l from ONE kernel (every logit / dP / exponential computed once, k and v read once: the landmark-owning waves hand P
 * and dS to the key-owning role through two LDS images) */
int mh_nys_attn3_bwd(const void* qkv, const void* lm, const float* av, const void* dav, const float* lse3, float* delta3,
                     void* dqkv, float* dlm, const float* mrow, const float* mlm, int B, int h, int n_p, int m, int dh,
                     float scale, int64_t lm_ld, mh_stream s);
/* One row of the Nystrom attention matrix: row[b, h, :] = (attn1 @ pinv(attn2) @ attn3)[cls_row, :], f32 [B, h, n_p] — what [3P]
 * NystromAttention.forward(..., return_attn=True) returns, for the one query position whose map is drawn (TransMIL's CLS token);
 * the n_p x n_p matrix is never formed:  p1 = softmax_j(scale q[cls_row] . k_l[j]),  u = p1 Z,
 * row[n] = sum_j u[j] exp(scale q_l[j] . k[n] - lse3[j]).
 *   qkv [B,n_p,3D] and lm [B,m,2D] (row stride lm_ld as above) of element type dt (MH_BF16 or MH_F32), D = h dh;
 *   z = pinv(attn2) per (b, h): z_colmajor = 1: bf16, column-major (mh_pinv_chain_fwd's zfT); 0: f32, row-major [B,h,m,m];
 *   lse3 [B,h,m] f32 = row logsumexp of scale q_l k^T (mh_nys_attn3_fwd's), or NULL: the kernel takes it in a first pass over k;
 *   mrow / mlm as for mh_nys_attn*: an invalid landmark has p1 = 0 and a uniform attn3 row (the package's fully masked row), a valid
 *   landmark's row is zero on invalid keys, and row[n] of an invalid key n is written as exactly 0.
 * Supported: (dh, m) = (64, 256) and (96, 384), n_p a multiple of m, 0 <= cls_row < n_p; anything else returns MH_EINVAL.
 * Every row[b, h, n] has one writer (no atomics).  Entries may be slightly negative and rows need not sum to 1 (z is a pseudo-inverse). */
int mh_nys_cls_attn(const void* qkv, const void* lm, const void* z, const float* lse3, float* row, const float* mrow, const float* mlm,
                    int B, int h, int n_p, int m, int dh, int cls_row, float scale, int64_t lm_ld, int z_colmajor, int dt,
                    mh_stream s);
/* out[r, 0:cols] = bf16(a[r] + b[r]) (f32 [rows, cols], b may be NULL) at row stride out_ld, out[r, cols:cols + zero_cols] = 0: the
 * landmark gradient (q_l | k_l halves from the attention kernels + sim2's products) written as rows [dq_l | dk_l | 0] of to_qkv's
 * output gradient, where its data / weight gradient products pick it up together with the sequence rows. */
int mh_lm_merge(const float* a, const float* b, void* out, int64_t rows, int cols, int64_t out_ld, int zero_cols, mh_stream s);
/* T = d*I - P  (batched [BH,m,m] f32) */
int mh_eye_minus(const float* P, float* T, float d, int BH, int m, mh_stream s);

/* ---------------------------------------------------------------- TransMIL glue (models/mirror.py:657-665, :317-331)
 * seq [B, n, D]: row 0 <- cls, rows 1+N.. <- copies of rows 1..add (square pad). */
int mh_seq_finish(void* seq, const float* cls, int B, int N, int add, int D, int dt, mh_stream s);
/* dseq[b,1+i] += dseq[b,1+N+i] (i<add); dcls[c] += sum_b dseq[b,0,c] */
int mh_seq_finish_bwd(void* dseq, float* dcls, int B, int N, int add, int D, int dt, mh_stream s);
/* merged[49][D] = w7 + embed(w5) + embed(w3) + centre 1 ; bsum[D] = b7+b5+b3 */
int mh_ppeg_merge(const float* w7, const float* w5, const float* w3, const float* b7, const float* b5,
                  const float* b3, float* merged, float* bsum, int D, mh_stream s);
/* depthwise 7x7 on tokens 1..S*S of seq [B, 1+S*S, D]; cls row copied. flip=1 -> adjoint (no bias). */
int mh_ppeg_fwd(const void* x, void* y, const float* merged, const float* bsum, int B, int S, int D,
                int flip, int dt_x, int dt_y, mh_stream s);
/* dmerged[tap][c] += sum dout*x(shifted); dbsum[c] += sum dout  (f32 atomics) */
int mh_ppeg_wgrad(const void* x, const void* dout, float* dmerged, float* dbsum, int B, int S, int D,
                  int dt_x, int dt_o, mh_stream s);
/* PPEG's whole backward in one pass over dy and x (f32, [B, 1+S*S, D]): dx = the adjoint filter over dy (cls row copied), dmerged / dbsum
 * += as mh_ppeg_wgrad.  drop_out != NULL: x came out of a Dropout on the lite stream (p, seed, offset, dev_base as mh_dropout_lite, D % 8
 * == 0) — drop_out (bf16, same shape) = that Dropout's backward of dx and drop_db [D] += its column sums, as mh_dropout_lite_colsum. */
int mh_ppeg_bwd(const float* x, const float* dy, const float* merged, float* dx, float* dmerged, float* dbsum, int B, int S,
                int D, void* drop_out, float* drop_db, float p, uint64_t seed, uint64_t offset, const uint64_t* dev_base,
                mh_stream s);
/* dw7 [D,1,7,7] += dmerged^T, dw5 [D,1,5,5] += its centre 5x5, dw3 [D,1,3,3] += its centre 3x3, db7 / db5 / db3 [D] += dbsum:
 * the gradients of the three depthwise kernels PPEG sums (models/mirror.py:324-331) from the merged kernel's gradient
 * (dmerged is tap-major [49, D] as mh_ppeg_wgrad writes it).  Accumulates: the caller owns the zeroing. */
int mh_ppeg_grad_scatter(const float* dmerged, const float* dbsum, float* dw7, float* dw5, float* dw3, float* db7,
                         float* db5, float* db3, int D, mh_stream s);

/* ---------------------------------------------------------------- masking (models/mirror.py:624-649, :510-533)
 * mask[b,i] = 1 if rank(noise[b,i]) >= len_keep (rank by ascending noise, ties by index) */
int mh_rank_mask(const float* noise, float* mask, int B, int N, int len_keep, mh_stream s);
/* y [B, T, D] (dt_y): rows t>=first take `token` where mask[b,t-first] != 0, else x (dt_x); then + pos[t]  (pos [T,D]) */
int mh_mask_apply_fwd(const void* x, void* y, const float* mask, const float* token, const float* pos, int B, int T, int D,
                      int first, int token_scalar, int dt_x, int dt_y, mh_stream s);   /* y may be x (in place, same dtype) */
/* dx (dt_dx) = dy*(1-mask) (dx may be dy when the dtypes agree); dtoken += sum mask*dy ; dpos[t] += sum_b dy.
 * dbias [D] f32 (may be NULL; only where mh_mask_apply_bwd_dbias_ok): += the column sums of dx, i.e. the bias gradient of the Linear
 * whose output the forward masked (retention_embed, models/mirror.py:636-643) — the pass already holds both sums it is the
 * difference of, so mh_colsum over dx is not launched. */
int mh_mask_apply_bwd_dbias_ok(const void* dy, const void* dx, const float* dpos, int D, int dt_dy, int dt_dx);
int mh_mask_apply_bwd(const void* dy, void* dx, const float* mask, float* dtoken, float* dpos, int B, int T, int D,
                      int first, int token_scalar, int dt_dy, int dt_dx, float* dbias, mh_stream s);

/* Compact retention embed: the projection in front of the mask-token select (retention_embed, models/mirror.py:690-693) is only needed
 * at the `first` unmasked prefix rows and the `keep` kept tokens of every batch.  mh_rank_mask_keep = mh_rank_mask (the same mask, bit
 * for bit) that also leaves keep_idx [B, len_keep] int32 (the token of rank j < len_keep) and slot [B, N] int32 (the rank of a kept
 * token, -1 for a masked one).  Compact layout [B, first + keep, .]: row b * (first + keep) + t (t < first) = prefix row t, row
 * b * (first + keep) + first + j = token keep_idx[b, j]. */
int mh_rank_mask_keep(const float* noise, float* mask, int* keep_idx, int* slot, int B, int N, int len_keep, mh_stream s);
/* out [B, first + keep, K] bf16 = the compact rows of x [B, T, K] bf16 (K % 8 == 0, 16-byte aligned) */
int mh_rows_gather(const void* x, const int* keep_idx, void* out, int B, int T, int K, int first, int keep, mh_stream s);
/* y [B, T, D] f32 = (slot < 0 ? token : rc[compact row]) + pos[t] for the compact bf16 projection rc [B, first + keep, D]: bit-identical
 * to mh_mask_apply_fwd on the dense bf16 projection (D % 4 == 0; slot [B, T - first]) */
int mh_mask_expand_fwd(const void* rc, float* y, const int* slot, const float* token, const float* pos, int B, int T, int D, int first,
                       int keep, mh_stream s);
/* mh_mask_apply_bwd's quad form (f32 dy, bf16 dx, per-channel token: the same arithmetic and summation order for dtoken, dpos and
 * dbias) whose dx is the COMPACT tensor drc [B, first + keep, D] bf16: nothing is stored for a masked row */
int mh_mask_apply_bwd_keep(const float* dy, void* drc, const int* slot, float* dtoken, float* dpos, int B, int T, int D, int first,
                           int keep, float* dbias, mh_stream s);
/* dh [B, T, K] f32 = dhc [B, first + keep, K] f32 at the prefix and kept rows, exact zeros at the masked rows (K % 4 == 0) */
int mh_rows_expand_zero(const float* dhc, const int* slot, float* dh, int B, int T, int K, int first, int keep, mh_stream s);

/* ---------------------------------------------------------------- RNA encoder pieces (models/mirror.py:77-102)
 * qkv [B, 3D] -> softmax over the HEADS axis -> out[b, d*H + h]; attn [B,H,H] saved for backward */
/* One pre-norm Block of the RNA transformer (reference: Block.forward models/mirror.py:149-152, Attention.forward :77-102,
 * [3P] timm Mlp fc1 -> GELU -> drop -> fc2 -> drop) on [B <= 32, D] rows, forward and backward, ONE call per direction:
 *   x1 = x + drop(proj(headattn(qkv(LN1(x)))));  y = x1 + drop(fc2(drop(gelu(fc1(LN2(x1))))))
 * LayerNorm, bias, GELU, the three dropouts (Philox, regenerated in the backward) and the residual adds ride in the
 * prologues / epilogues of the weight-streaming GEMM kernels (5 launches forward, 6 backward; csrc/rna_block.hip).
 * Needs D % 32 == 0, Hh % 32 == 0, D % H == 0.  Weights are bf16 [N, K] row-major; wt_* are their transposes [K, N] (the
 * data gradients stream them like forward weights).  Saved tensors are caller-allocated in the forward and handed back
 * unchanged in the backward; gradients ACCUMULATE into the f32 d* buffers. */
typedef struct {
    int32_t B, D, Hh, H;          /* rows, model width, MLP hidden width, attention heads */
    float eps, p_drop;            /* LayerNorm eps; dropout probability (0 = eval mode) */
    uint64_t seed, offset;        /* Philox streams: proj output at `offset`, fc1 activation at + q4(B D), fc2 output at + q4(B Hh) more (q4 = round up to 4) */
    const uint64_t* dev_base;     /* optional device-side base added to `offset` (per-step base of a replayed HIP graph) */
    const void *w_qkv, *w_proj, *w_fc1, *w_fc2;         /* bf16 [3D, D], [D, D], [Hh, D], [D, Hh] */
    const void *wt_qkv, *wt_proj, *wt_fc1, *wt_fc2;     /* bf16 transposes (backward only) */
    const float *b_qkv, *b_proj, *b_fc1, *b_fc2;        /* biases (b_qkv may be NULL) */
    const float *g1, *be1, *g2, *be2;                   /* LayerNorm 1 / 2 weight and bias */
    const float* x;               /* [B, D] f32 block input */
    float* y;                     /* [B, D] f32 block output (forward) */
    float* stats;                 /* saved: [4, B] mean1, rstd1, mean2, rstd2 */
    void* qkv;                    /* saved: bf16 [B, 3D] */
    float* attn;                  /* saved: f32 [B, H, H] attention probabilities */
    void* o;                      /* saved: bf16 [B, D] attention output */
    float* x1;                    /* saved: f32 [B, D] stream after the attention half */
    void* u;                      /* saved: bf16 [B, Hh] fc1 output before GELU */
    void* f;                      /* saved: bf16 [B, Hh] fc2 input */
    const float* dy;              /* backward: [B, D] f32 gradient of y */
    float* dx;                    /* backward: [B, D] f32 gradient of x (written) */
    float *dw_qkv, *dw_proj, *dw_fc1, *dw_fc2, *db_qkv, *db_proj, *db_fc1, *db_fc2, *dg1, *dbe1, *dg2, *dbe2;
    void* scratch;                /* backward: mh_rna_block_workspace_bytes(B, D, Hh) bytes */
} mh_rna_block;
int mh_rna_block_fwd(const mh_rna_block* blk, mh_stream s);
int mh_rna_block_bwd(const mh_rna_block* blk, mh_stream s);
int64_t mh_rna_block_workspace_bytes(int B, int D, int Hh);
/* Host only.  LDS bytes of the largest of the nine GEMM launches of both directions (forward contractions D, D, D, Hh; data
 * gradients over D, Hh, D, 3 D; the weight-gradient tile), and the admission rule built on it: 1 when mh_rna_block_fwd AND
 * mh_rna_block_bwd accept the geometry (every launch fits the LDS budget and the limits above hold), else 0.  Both entry
 * points refuse a geometry that does not fit before they launch anything. */
int64_t mh_rna_block_lds_bytes(int B, int D, int Hh);
int mh_rna_block_fits(int B, int D, int Hh, int H);

/* Attention over the heads axis of qkv [B, 3 H hd] (f32 or bf16): out [B, H hd], attn [B, H, H] f32.  Both directions admit the same
 * shapes, H <= 64 and H hd <= 4096, and opt in to the backward's dynamic LDS (16 H hd + 8 H^2 bytes, up to 96 KiB; the forward asks
 * for 12 H hd + 4 H^2): where the device declines that, the forward refuses too, so no forward succeeds whose backward cannot run. */
int mh_headattn_fwd(const void* qkv, void* out, float* attn, int B, int H, int hd, int dt, mh_stream s);
int mh_headattn_bwd(const void* qkv, const float* attn, const void* dout, void* dqkv, int B, int H, int hd,
                    int dt, mh_stream s);

/* ---------------------------------------------------------------- elementwise / reductions */
int mh_add(const void* a, const void* b, void* y, int64_t n, int dt_a, int dt_b, int dt_y, mh_stream s);
int mh_cast(const void* x, void* y, int64_t n, int dt_x, int dt_y, mh_stream s);
int mh_gelu_fwd(const void* x, void* y, int64_t n, int dt_x, int dt_y, mh_stream s);
int mh_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dt_x, int dt_dy, int dt_dx, mh_stream s);
/* dx = dy * (y > 0); `batches` blocks of n_per_batch contiguous elements at the given batch strides */
int mh_relu_bwd(const void* y, const void* dy, void* dx, int64_t n_per_batch, int batches, int64_t y_bs, int64_t dy_bs,
                int64_t dx_bs, int dt_y, int dt_dy, int dt_dx, mh_stream s);
/* The four random draws of a training step in one launch (models/mirror.py:630 `torch.rand(B, N)`, :516 `torch.rand(B, D)`, :832-833
 * `torch.randn_like` twice): out[0, n_uniform) uniform in [0, 1) on 24 random bits, out[n_uniform, n_uniform + n_normal) standard normal
 * (Box-Muller); Philox4x32-10 on the dropout stream: element i = word (i & 3) of block (offset + *dev_base + i) >> 2 under `seed`.
 * n_uniform and offset are multiples of 4.  The VALUES differ from torch's generator (as any seed change would); callers that pin the
 * draws (parity tests) pass them in instead. */
int mh_noise_draws(float* out, int64_t n_uniform, int64_t n_normal, uint64_t seed, uint64_t offset, const uint64_t* dev_base, mh_stream s);
/* y = x * keep/(1-p); keep from Philox4x32-10(seed, offset + *dev_base + i)  ([3P] nn.Dropout in to_out; :75, :142).
 * dev_base (nullable, device memory): per-step base offset, so that a captured graph draws fresh masks at every replay */
int mh_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset, const uint64_t* dev_base,
               int dt_x, int dt_y, mh_stream s);
/* y = a + dropout(x): the residual add behind the Dropout of [3P] NystromAttention.to_out (models/mirror.py:312), one pass.
 * Same mask as mh_dropout for the same (seed, offset [+ *dev_base]).  n % 4 == 0, quad-aligned buffers; a, y f32. */
int mh_dropout_add(const float* a, const void* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset,
                   const uint64_t* dev_base, int dt_x, mh_stream s);
/* The "lite" dropout stream of the [B, n, D]-sized WSI dropouts ([3P] to_out[1], models/mirror.py:312): Philox4x32-7, 16 random
 * bits per element (8 elements per block: element i = 16-bit field i & 7 of the block with counter (offset + i) >> 3), kept when
 * field >= round(p * 65536), scaled by the exact 1 / P(keep).  y = dropout(x) (a NULL) or a + dropout(x) (y f32);
 * n % 8 == 0, offset % 8 == 0.  The DROPADD projection epilogue (mh_gemm_epi) draws the same stream. */
int mh_dropout_lite(const float* a, const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset,
                    const uint64_t* dev_base, int dt_x, int dt_y, mh_stream s);
/* Timeline probe: *dst = the device's constant-rate wall clock (100 MHz ticks) when this one-thread launch runs on stream s.
 * Profiling aid (tools/exp/probe_timeline.py: where the branches of a replayed step really start and end, without a tracer
 * attached); nothing on the product path calls it. */
int mh_timestamp(uint64_t* dst, mh_stream s);
/* mh_dropout_lite's backward use on a [rows, N] f32 gradient -> bf16, which also adds the column sums of what it wrote to db [N]:
 * the bias gradient of [3P] to_out[0] (models/mirror.py:312) without mh_colsum's pass over the bf16 gradient. */
int mh_dropout_lite_colsum(const float* x, void* y, int64_t rows, int N, float p, uint64_t seed, uint64_t offset,
                           const uint64_t* dev_base, float* db, mh_stream s);
/* out[c] += sum_r x[r*ld + c]  (bias gradients; f32 atomics) */
int mh_colsum(const void* x, float* out, int64_t rows, int cols, int64_t ld, int dt, mh_stream s);
/* y[r] = x[r*x_rs .. +D] / max(||.||, eps) (F.normalize, models/mirror.py:540, :683); norm[r] saved */
int mh_l2norm_fwd(const void* x, void* y, float* nrm, int rows, int D, int64_t x_rs, float eps, int dt_x, int dt_y,
                  mh_stream s);
int mh_l2norm_bwd(const void* y, const float* nrm, const void* dy, void* dx, int rows, int D, int64_t dx_rs,
                  float eps, int dt_y, int dt_dy, int dt_dx, int accumulate, mh_stream s);
/* y = exp(x) on a small f32 tensor (`logit_scale.exp()`, models/mirror.py:911); backward dx (+)= dy * y (accumulate != 0: summed
   into dx, the parameter's gradient slot) */
int mh_exp_fwd(const float* x, float* y, int64_t n, mh_stream s);
int mh_exp_bwd(const float* dy, const float* y, float* dx, int64_t n, int accumulate, mh_stream s);
/* z = mu + eps*exp(0.5*logstd) (models/mirror.py:830-833); backward: dmu = dz + add_mu, dlogstd = dz*eps*0.5*exp(0.5*logstd) +
   add_logstd (add_* nullable: what reached mu / logstd from their other consumer, the KL term of losses/mirror_loss.py:112-117) */
int mh_reparam_fwd(const float* mu, const float* logstd, const float* eps, float* z, int64_t n, mh_stream s);
int mh_reparam_bwd(const float* logstd, const float* eps, const float* dz, const float* add_mu, const float* add_logstd,
                   float* dmu, float* dlogstd, int64_t n, mh_stream s);

/* ---------------------------------------------------------------- losses (losses/mirror_loss.py, losses/info_nce.py)
 * cross-entropy of rows of scale*G against label (label_off + row); G [R x C] f32.
 * out[0] += coef * sum_r (lse_r - scale*G[r,label]) ; loss_rows[r] = coef * (...) ; lse [R] saved.
 * scale is read from device memory (no host sync). */
int mh_ce_rows_fwd(const float* G, int64_t ldg, const float* scale, float scale_mul, int R, int C, int label_off,
                   float coef, float* loss_rows, float* lse, float* out, mh_stream s);
/* dG[r,c] = gcoef * g[0 or r] * scale * (softmax - onehot); dscale += sum dG_unscaled*G  */
int mh_ce_rows_bwd(const float* G, int64_t ldg, const float* scale, float scale_mul, const float* lse, const float* g,
                   int g_per_row, float gcoef, float* dG, float* dscale, int R, int C, int label_off, mh_stream s);
/* acc[0] += sum_r mask[r] * mean_D (p-t)^2 ; acc[1] += sum_r mask[r]   (losses/mirror_loss.py:98-103)
 * pred [rows, D] contiguous; target row r at tgt + (r / rows_per_batch) * tgt_bs + (r % rows_per_batch) * D elements
 * (a row window of a larger buffer: the WSI target is encoder_output[:, 1:], models/mirror.py:700) */
int mh_mse_masked_fwd(const void* pred, const void* tgt, const float* mask, float* acc, int64_t rows, int D,
                      int64_t rows_per_batch, int64_t tgt_bs, int dt_p, int dt_t, mh_stream s);
/* The same sums in an order that does not depend on the run: mh_mse_masked_fwd adds its blocks' partial sums with float atomics
 * in whatever order the blocks arrive, so acc[0] of the same inputs moves by an ulp between launches (a validation loss that is
 * not bit-reproducible).  Here every block leaves its pair in workspace (MH_MSE_FWD_WS_FLOATS f32, 4-byte aligned, nothing to
 * zero) and a second launch of one wave adds them in block order onto acc.  Two launches, nothing allocated, no host wait. */
#define MH_MSE_FWD_WS_FLOATS 2048
int mh_mse_masked_fwd_ordered(const void* pred, const void* tgt, const float* mask, float* acc, int64_t rows, int D,
                              int64_t rows_per_batch, int64_t tgt_bs, int dt_p, int dt_t, float* workspace, mh_stream s);
/* dpred[rows, D] (dt_dp) = g[0] * gmul * 2*mask*(p-t)/(D*acc[1]) (gmul: the term's loss weight, host constant); dtgt[rows, D] (dt_t) = -dpred, not written when NULL.
 * colsum_ws [cs_blocks, D] f32 (may be NULL; bf16 pred / f32 target / bf16 dpred, D a multiple of 256 up to 1024): the launch runs cs_blocks blocks and block i
 * leaves the column sums of the dpred rows it wrote in row i (every row is written, nothing to zero): mh_colsum over that table is the
 * bias gradient of the Linear that produced pred (retention_head, models/mirror.py:698-699) without a second pass over dpred. */
int mh_mse_masked_bwd(const void* pred, const void* tgt, const float* mask, const float* acc, const float* g, float gmul,
                      void* dpred, void* dtgt, int64_t rows, int D, int64_t rows_per_batch, int64_t tgt_bs, int dt_p, int dt_t,
                      int dt_dp, float* colsum_ws, int cs_blocks, mh_stream s);
/* Data feed (datasets/dataset_pretrain.py:150-167, `wsi_feature[sampled_indices]`): out[r, :] = src[row[r], :] for R rows of F
 * elements; src is the bank of all slides' patch features back to back ([src_rows, F]); row holds GLOBAL row indices
 * (slide offset + sampled index; clamped to the bank). */
int mh_gather_rows(const void* src, const int64_t* row, void* out, int64_t R, int64_t F, int64_t src_rows, int dt, mh_stream s);
/* Data feed draws (csrc/datafeed.hip): the token draw `np.random.choice(n_i, N, replace=n_i < N)` of dataset_pretrain.py:157-161,
 * dataset_subtyping.py:187-200 and dataset_survival.py:293-314 for a whole batch, and the slide-id draw of utils/loader.py:15-26
 * (`WeightedRandomSampler(weights, len(weights))`), one launch each, no host round trip, capturable in a graph.
 *
 * The stream: Philox4x32-10 under key = (lo32(seed), hi32(seed)) like mh_dropout / mh_noise_draws, whose counters have c2 = c3 = 0;
 * a draw sets bit 31 of c3 and so never shares a block with them under the same seed:
 *     counter = (lo32(blk), kind, lo32(draw), 0x80000000 | hi32(draw))     kind = 0 for token draws, 1 for slide-id draws; draw < 2^63
 * Element e of a draw is word e & 3 of block blk = e >> 2.
 *
 * mh_sample_rows: rows [B, N] int64.  Batch slot b holds slide sl = slot_slide[b] of n = length[sl] rows that begin at bank row
 * start[sl], and uses draw = offset + *dev_base + b (*dev_base counts as 0 when the pointer is NULL; it is device memory, so a captured
 * graph that bumps it draws fresh rows at every replay, and two slots that hold the same slide get different rows).  The result
 * depends on (seed, draw, n, N) only.  With w_e = element e of the draw:
 *   n <  N (with replacement):     rows[b, i] = start[sl] + ((w_i * n) >> 32); the multiply-shift favours some rows by at most
 *                                  n / 2^32 (relative), against a uniform draw.
 *   n >= N (without replacement):  row j of the slide gets the 64-bit key K_j = (w_j << 32) | j; rows[b, :] = start[sl] + the N
 *                                  indices j with the smallest keys, in ascending key order — a uniformly random ORDERED subset, what
 *                                  np.random.choice(n, N, replace=False) returns.  Equal 32-bit words are ordered by index: a relative
 *                                  bias of order 2^-32.
 * All four tables are device memory.  A slot whose slide id lies outside [0, S) gets -1 in every row (mh_gather_rows clamps to the
 * bank); a slot whose slide has length <= 0 or >= 2^31 gets start[sl] in every row: the lengths live on the device, so the launch
 * cannot refuse them without a read-back (DeviceSlideBank refuses such slides when it is built).  MH_EINVAL for N > 8192, N < 0, B < 0
 * or offset + B >= 2^63.
 * The kernel: one workgroup per slot sorts keys in LDS (at most 16384).  It keeps the keys whose word lies below a threshold chosen
 * for an expected N + slack * sqrt(N) candidates, compacts them into LDS and sorts those; a slide whose n keys all fit a sort of that
 * size (the next power of two, at least 128) skips the threshold and sorts them all.  When fewer than N or more than 16384 keys pass,
 * the threshold moves and the pass repeats — any threshold that lets between N and 16384 keys through gives the same rows bit for
 * bit, so `slack` (>= 0; 8: a retry about once in 1e15 slots, 0: about every other slot, 1e3 on a slide above 16384 rows: always too
 * many at first) changes the time, never the result. */
int mh_sample_rows(const int64_t* slot_slide, const int64_t* length, const int64_t* start, int64_t* rows, int B, int N, int64_t S,
                   uint64_t seed, uint64_t offset, const uint64_t* dev_base, float slack, mh_stream s);
/* out [count] int64 = slide ids drawn with replacement from the distribution whose cumulative sums are cdf [S] (f64, device,
 * non-decreasing, cdf[S - 1] = 1), on the stream above with kind = 1 and draw = offset + *dev_base.  Output i uses elements 2 i and 2 i + 1:
 *     u = (((w_{2i} >> 5) << 26) | (w_{2i+1} >> 6)) * 2^-53        (53 random bits, u in [0, 1), exact in f64)
 *     out[i] = min(#{k : cdf[k] <= u}, S - 1)                      (a binary search, no other arithmetic)
 * An entry of weight 0 (cdf[k] == cdf[k - 1], or cdf[0] == 0) is never drawn.  By distribution this is torch's
 * WeightedRandomSampler(weights, count, replacement=True); the values differ, as under any change of generator.  count <= 2^32. */
int mh_sample_weighted(const double* cdf, int64_t S, int64_t* out, int64_t count, uint64_t seed, uint64_t offset,
                       const uint64_t* dev_base, mh_stream s);
/* Gradient of the WSI encoder output E [B, T, D] (f32), which three consumers read (models/mirror.py:684, :690, :700, :833):
 *   dE[b, t] = gfull[b, t] + alpha * x[b, t - 1] (t >= 1) + (t == 0 ? c[b] : 0)
 * gfull f32 [B, T, D], x [B, T-1, D] in dt_x, c f32 [B, D]; each may be NULL (taken as zero). */
int mh_fanout_bwd(const float* gfull, const void* x, float alpha, const float* c, float* dE, int B, int T, int D, int dt_x,
                  mh_stream s);
/* total = sum_i w_i * term_i over up to 6 separate f32 scalars (losses/mirror_loss.py:121-127); bwd: dterms[i] = w_i * g[0] */
int mh_weighted_sum(const float* t0, const float* t1, const float* t2, const float* t3, const float* t4, const float* t5,
                    float w0, float w1, float w2, float w3, float w4, float w5, int n, float* out, mh_stream s);
int mh_weighted_sum_bwd(const float* g, float w0, float w1, float w2, float w3, float w4, float w5, int n, float* dterms,
                        mh_stream s);
/* out[0] += coef * sum (exp(ls) + mu^2 - 1 - ls)   (losses/mirror_loss.py:105-112) */
int mh_kl_fwd(const float* mu, const float* ls, float* out, int64_t n, float coef, mh_stream s);
int mh_kl_bwd(const float* mu, const float* ls, const float* g, float* dmu, float* dls, int64_t n, float coef,
              mh_stream s);
/* out[0] += coef * sum_b sum_k (p_r - p_w)(log p_r - log p_w)  (losses/mirror_loss.py:114-119) */
int mh_symkl_fwd(const float* w, const float* r, float* out, int B, int P, float coef, mh_stream s);
int mh_symkl_bwd(const float* w, const float* r, const float* g, float* dw, float* dr, int B, int P, float coef,
                 mh_stream s);

/* MIRRORLoss's small terms in one launch each way (losses/mirror_loss.py:74-135, everything but the WSI retention MSE):
 * the rank-local CLIP alignment term (:37-52: logits s W R^T, both cross-entropies, and in the backward the gradient
 * products d W = P R, d R = P^T W and d s), the RNA retention MSE (:98-103), both style KLs (:105-112), the cluster KL
 * (:114-119) and the weighted total (:121-127).  All tensors f32, contiguous.  weight[] = {alignment, wsi retention,
 * rna retention, style (wsi), style (rna), cluster}.
 *   forward : out[8] = {total, alignment, wsi retention, rna retention, style_w + style_r, cluster, style_w, style_r};
 *             wsi_acc = the {num, den} pair mh_mse_masked_fwd accumulated on the same stream BEFORE this call (NULL: 0);
 *             scratch = 8 + Bc + 64 floats, the first 8 zeroed by the caller (kept for the backward; behind the 8 words every
 *             block of a shared term keeps its partial sum, added in a fixed order: the same operands give the same bits on
 *             every launch), save = B*B + 2B floats (kept as well).
 *   backward: the upstream of term i is weight[i] * g_total[0] + (g_terms ? g_terms[i] : 0); every d_* of a term that is
 *             present is overwritten.  The WSI retention gradient stays mh_mse_masked_bwd(g = g_total, gmul = weight[1]).
 * has_align = 0: the alignment term was computed by the caller over the gathered batch (align_ext, one float, may be
 * NULL = 0) and the backward writes its upstream to d_align_ext.  Alignment in here needs B <= 32 and
 * 2 B (D + 1) + B (B + 1) floats of LDS <= 150 KiB. */
typedef struct {
    const float* wsi_emb;      /* [B, D] L2-normalised alignment embeddings */
    const float* rna_emb;      /* [B, D] */
    const float* logit_scale;  /* one float: exp(logit_scale parameter) */
    const float* align_ext;
    int32_t B, D, has_align;
    const float* rna_pred;     /* [n_rna] reconstructed expression, target, mask (1 = masked gene) */
    const float* rna_tgt;
    const float* rna_mask;
    int64_t n_rna;
    const float* w_mu;         /* style posteriors: [rows, latent] each */
    const float* w_logstd;
    const float* r_mu;
    const float* r_logstd;
    int64_t n_wstyle, n_rstyle;
    int32_t rows_wstyle, rows_rstyle;
    const float* w_score;      /* prototype scores [Bc, P] (logits; the kernel takes the softmax) */
    const float* r_score;
    int32_t Bc, P;
    const float* wsi_acc;
    float weight[6];
    float* scratch;
    float* save;
    float* out;
    const float* g_total;      /* backward only from here */
    const float* g_terms;
    float* d_wsi_emb;
    float* d_rna_emb;
    float* d_logit_scale;
    float* d_align_ext;
    float* d_rna_pred;
    float* d_rna_tgt;          /* = -d_rna_pred; NULL: not written (the target is data) */
    float* d_w_mu;
    float* d_w_logstd;
    float* d_r_mu;
    float* d_r_logstd;
    float* d_w_score;
    float* d_r_score;
} mh_loss_terms;
int mh_loss_terms_fwd(const mh_loss_terms* d, mh_stream s);
int mh_loss_terms_bwd(const mh_loss_terms* d, mh_stream s);

/* ---------------------------------------------------------------- step glue (train_mirror.py:1133-1136, :1230, :1254-1255) */
/* w[r] /= max(||w[r]||, eps) in place (the prototype renormalisation, train_mirror.py:1133-1136); shadow_bf16 (nullable, [rows, D]
 * contiguous) receives the bf16 copy of the result in the same pass */
int mh_rownorm_(float* w, void* shadow_bf16, int rows, int D, float eps, mh_stream s);
/* x = min(max(x, lo), hi) in place as torch.clamp_ has it: the bounds apply to +-inf, a NaN stays a NaN (the optimizers' clamped
 * element below follows the same rule) */
int mh_clamp_(float* x, int64_t n, float lo, float hi, mh_stream s);
/* torch.optim.Adam (wd=0): flat f32 params/grads/moments; optional bf16 shadow copy of the params.  This is mh_optim_step's rule
 * MH_OPT_ADAM without a group map behind an older argument list: one device body (optim.hip) serves both, bit for bit.
 * dev_state (nullable, 6 device floats {t, 1-b1^t, 1-b2^t, lr, clip, |g|}): when given, t is advanced and the bias
 * corrections are refreshed ON THE DEVICE before the update, lr / bias_c1 / bias_c2 arguments are ignored and the
 * gradient is additionally scaled by dev_state[4] (1, or the factor mh_grad_clip left there) — nothing step-dependent
 * is a launch argument, so the whole step can be captured in a HIP graph (train_mirror.py:1254 optimizer.step()).
 * Step glue that rides along instead of costing launches of its own: clamp_index >= 0 clamps that one parameter to
 * [clamp_lo, clamp_hi] right behind its update, master and shadow (`logit_scale.clamp_(0, ln 100)`, train_mirror.py:1255; -1 =
 * none); counter (nullable) += counter_add on the device (the dropout streams' per-step base).
 * One optimizer step as TWO launches (round 5: the RNA encoder's parameters, 80 % of the arena, have their gradients 2 ms before the
 * step's last one): tick = 0 reads dev_state without advancing it (the other launch of the step did), and elements [hole_lo, hole_hi)
 * (quad-aligned, not holding clamp_index) are left untouched — the range the other launch updates.  tick = 1, hole_lo = hole_hi = 0:
 * the whole arena in one launch, as before.  tick = 2: like 1, for the EARLY launch of such a pair (it runs as `adam_range_kernel`, so that
 * profiling tools that cut a kernel trace into steps at `adam_kernel` keep working).
 * The kernel's name follows what is launched, not the entry point: rule Adam with no group map and no EMA runs as `adam_kernel` /
 * `adam_range_kernel` from mh_optim_step too; every other launch runs as an `optim_kernel<rule, EMA, momentum>` instance.
 * With dev_state == NULL (this entry point only) lr / bias_c1 / bias_c2 are the arguments and no clip factor is applied. */
int mh_adam(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1,
            float beta2, float eps, float bias_c1, float bias_c2, float grad_scale, float* dev_state, int64_t clamp_index,
            float clamp_lo, float clamp_hi, int64_t* counter, int64_t counter_add, int tick, int64_t hole_lo, int64_t hole_hi,
            mh_stream s);

/* ---------------------------------------------------------------- model EMA (timm ModelEmaV3; added to v120)
 * train_mirror.py:787-799 (ModelEmaV3(model, decay, use_warmup)), :1283-1284 (model_ema.update(model, step=num_updates)); the same in
 * train_subtyping.py:867-879, :1293 and train_survival.py:879-891, :1322.  The decay of step t is timm's get_decay(t), computed on the
 * device in double: s = max(0, t - update_after_step - 1); s == 0 -> 0 (the update copies); use_warmup -> max(min(1 - (1 + s /
 * warmup_gamma)^-warmup_power, decay), min_decay); else decay.  The lerp weight 1 - decay is rounded to f32 once and applied in
 * torch.lerp's form (w < 0.5 ? e + w (p - e) : p - (p - e)(1 - w)); w = 1 is an exact copy.
 * mh_adam_ema: mh_adam (every argument keeps its meaning) plus ema (f32, laid out like p, 16-B aligned): each updated element's
 * final value (after the clamp) is lerped into ema in the same pass (+8 B per parameter), with t = dev_state[0] after the tick
 * (dev_state is required).  It is mh_optim_step's rule MH_OPT_ADAM with ema set and no group map; both launches of a two-launch step
 * run as `optim_kernel<MH_OPT_ADAM, true, true>`, so tools that cut a trace at `adam_kernel` see no EMA step.
 * The settings travel as a host struct, read at launch (kernel arguments: a captured graph keeps them). */
typedef struct {
    double decay, min_decay, warmup_gamma, warmup_power;   /* timm's ModelEmaV3 settings (warmup_gamma > 0) */
    int64_t update_after_step;
    int use_warmup;
} mh_ema_cfg;
int mh_adam_ema(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1, float beta2,
                float eps, float bias_c1, float bias_c2, float grad_scale, float* dev_state, int64_t clamp_index, float clamp_lo,
                float clamp_hi, int64_t* counter, int64_t counter_add, int tick, int64_t hole_lo, int64_t hole_hi, float* ema,
                const mh_ema_cfg* cfg, mh_stream s);
/* ema[off_i + j] = lerp(ema[off_i + j], src_i[j], w) for j < n_i, for the nseg rows {off_i, (int64) src_i, n_i} of the device
 * table (int64 [nseg, 3]; src_i: f32 device pointers; the ranges must not overlap).  One workgroup per row: split long tensors
 * into rows of a few 10^4 elements (a multiple of 4) for balance.  w = weight (in [0, 1]) when dev_state is NULL (cfg unused,
 * may be NULL), else the decay rule of cfg applied to t = dev_state[0] (graph-capturable). */
int mh_ema_update_many(float* ema, const int64_t* table, int nseg, float weight, const float* dev_state, const mh_ema_cfg* cfg,
                       mh_stream s);

/* ---------------------------------------------------------------- the arena optimizer (optim.hip; added to v121)
 * TrainEngine's update for every rule; mh_adam and mh_adam_ema above are its rule MH_OPT_ADAM without decay.
 * train_mirror.py:742-746 `create_optimizer_v2(model, **optimizer_kwargs(cfg=args))` (the same in train_subtyping.py and
 * train_survival.py) for --opt adam / adamw / sgd / nesterov / momentum with --weight-decay, --momentum, --opt-eps, --opt-betas.
 * Each rule follows torch's single-tensor path; grad_scale * dev_state[4] scales the gradient BEFORE any weight decay:
 *   MH_OPT_ADAM   g' = gs g + wd p, then Adam on g'                                   torch.optim.Adam(weight_decay=wd)
 *   MH_OPT_ADAMW  p *= 1 - lr wd, then Adam on gs g                                   torch.optim.AdamW
 *   MH_OPT_SGD    g' = gs g + wd p; buf = momentum buf + g'; p -= lr (nesterov ? g' + momentum buf : buf)
 *                 torch.optim.SGD(momentum, dampening=0, nesterov); a zero buffer gives torch's first-step buf = g'.
 *                 momentum == 0: p -= lr g', m is not read (may be NULL).  v is never read by SGD (may be NULL).
 * m: exp_avg / momentum_buffer, v: exp_avg_sq.  Weight decay is per parameter: group_map (nullable = no decay anywhere) holds one
 * byte per 8-element block of the arena, (n + 7) / 8 bytes — every parameter starts on such a block — naming the block's decay
 * group, and group_wd[n_groups <= 256] (device f32) that group's weight decay (timm's param_groups_weight_decay: 1-D and `.bias`
 * parameters in a weight_decay = 0 group).  For a sub-range launch pass the map from the range's first block.
 * dev_state (required), clamp_index / clamp_lo / clamp_hi, counter / counter_add, tick (0, 1, 2) and hole_lo / hole_hi are mh_adam's;
 * lr is dev_state[3]; the tick advances t for SGD too (the EMA decay and fp8 delayed scaling read it) and leaves dev_state[1..2]
 * alone there.  ema (nullable) + ema_cfg: mh_adam_ema's lerp of each element's final value, in the same pass.
 * Kernel names: see mh_adam.
 * Deterministic (no atomics), graph capturable; the settings travel as host structs read at launch. */
#define MH_OPT_ADAM 0
#define MH_OPT_ADAMW 1
#define MH_OPT_SGD 2
typedef struct {
    int rule;                 /* MH_OPT_* */
    float beta1, beta2, eps;  /* the Adam rules */
    float momentum;           /* MH_OPT_SGD */
    int nesterov;
} mh_optim_cfg;
int mh_optim_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, const mh_optim_cfg* opt,
                  const uint8_t* group_map, const float* group_wd, int n_groups, float grad_scale, float* dev_state,
                  int64_t clamp_index, float clamp_lo, float clamp_hi, int64_t* counter, int64_t counter_add, int tick,
                  int64_t hole_lo, int64_t hole_hi, float* ema, const mh_ema_cfg* ema_cfg, mh_stream s);

/* mh_optim_step with one learning rate per parameter group (torch.optim's param_groups[i]["lr"], which lr schedulers write): the
 * update of mirror_amd.optim.ArenaOptimizer.  group_map is required here; group_lr[n_groups] (device f32) stands beside group_wd, and
 * group_lr[g] takes the place of dev_state[3] for the elements of group g.  The step size lr / (1 - b1^t) is formed per group by the
 * same division as mh_optim_step's, so a table that holds one value everywhere gives mh_optim_step's bits with that value in
 * dev_state[3].  Both tables live in device memory: a captured graph replays with whatever they hold at the replay.
 * The group byte MH_OPT_SKIP_GROUP (255) marks blocks the launch leaves untouched — p, m, v, shadow and ema keep their bits: torch.optim's
 * treatment of a parameter whose .grad is None.  It has no table entry, so n_groups <= 255 here.
 * Every other argument keeps mh_optim_step's meaning.  Runs as `optim_groups_kernel<rule, EMA, momentum>`. */
#define MH_OPT_SKIP_GROUP 255
int mh_optim_groups(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, const mh_optim_cfg* opt,
                    const uint8_t* group_map, const float* group_wd, const float* group_lr, int n_groups, float grad_scale,
                    float* dev_state, int64_t clamp_index, float clamp_lo, float clamp_hi, int64_t* counter, int64_t counter_add,
                    int tick, int64_t hole_lo, int64_t hole_hi, float* ema, const mh_ema_cfg* ema_cfg, mh_stream s);

/* arena[off_i + j] = (float) src_i[j] for j < n_i, for the nrows rows {off_i, (int64) src_i, n_i, dtype_i} of the device table (int64
 * [nrows, 4]; dtype_i = MH_F32 or MH_BF16, a bf16 source is widened; src_i aligned to its element size; the destination ranges must
 * not overlap): the write-side twin of mh_ema_update_many, one launch for gradients that were left outside the gradient arena and for
 * loading optimizer state.  One workgroup per row: split long tensors into rows of a few 10^4 elements (a multiple of 8).  16-byte
 * accesses where source and destination reach a 16-byte boundary at the same element (a scalar head up to it, a scalar tail), scalar
 * otherwise.  HBM-bound: 8 B per f32 element, 6 B per bf16 element.  Deterministic, graph capturable. */
int mh_gather_many(float* arena, const int64_t* table, int nrows, mh_stream s);

/* clip-grad "norm" mode (train_mirror.py:1206-1230): dev_state[5] = ||grad_scale * g||_2, dev_state[4] =
 * min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0); scratch1 = one device float. */
int mh_grad_clip(const float* g, int64_t n, float grad_scale, float max_norm, float* scratch1, float* dev_state, mh_stream s);

/* ---------------------------------------------------------------- downstream survival step (train_survival.py, v119)
 * logits [N x M] f32, row stride ld; event_times [N] int32 / int64 (dt_t = MH_SV_I32 / MH_SV_I64: the dataset's disc_label is
 * torch.int, datasets/dataset_survival.py:307); censoring [N] read through dt_c (bool / uint8, int32, int64 or f32), compared as
 * the reference does (`censoring == 1`, `== 0`).  lo / hi: the hazard clamp bounds eps, 1 - eps rounded to f32 as torch rounds a
 * clamp scalar; lo is also the CE clamp of p_sum and of the chosen probability.  One lane per row, the M bins in the reference's
 * order; every entry point is deterministic (no float atomics) and graph capturable. */
#define MH_SV_U8 0
#define MH_SV_I32 1
#define MH_SV_I64 2
#define MH_SV_F32 3
#define MH_SURV_NLL 0   /* losses/nll_surv.py:17-94 (NLLSurvLoss.forward) */
#define MH_SURV_CE 1    /* losses/cross_entropy_surv.py:25-105 (CrossEntropySurvLoss.forward) */
/* per-row losses into loss_rows [N] (nullable) and out[0] = coef * sum_r loss_r (nullable; STORED, not accumulated; the rows are
 * summed in a fixed order by one block).  NLL: loss_r = w_all * nll_r + w_unc * [censoring_r == 1] * nll_r with w_all = 1 - alpha,
 * w_unc = alpha (losses/nll_surv.py:84-87); rows with censoring outside {0, 1} are 0; T >= M and T < 0 follow the reference's masks.
 * CE: the target is T when censoring == 1, else class M; an uncensored T outside [0, M] (where the reference's gather raises) gives
 * NaN in that row.  w_all / w_unc are ignored for CE. */
int mh_surv_loss_fwd(const float* logits, int64_t ld, const void* event_times, int dt_t, const void* censoring, int dt_c, int N, int M,
                     int kind, float lo, float hi, float w_all, float w_unc, float coef, float* loss_rows, float* out, mh_stream s);
/* dlogits [N x M] contiguous = d(sum_r gcoef * g[0 or r] * loss_r) / d logits, recomputed from logits (nothing saved by the forward):
 * the derivative of the reference's expression as written (zero where the sigmoid clamp is active; CE through p / clamp(p_sum) and
 * the clamp of the chosen probability).  A NaN CE row (see above) gives a NaN dlogits row. */
int mh_surv_loss_bwd(const float* logits, int64_t ld, const void* event_times, int dt_t, const void* censoring, int dt_c, int N, int M,
                     int kind, float lo, float hi, float w_all, float w_unc, const float* g, int g_per_row, float gcoef, float* dlogits,
                     mh_stream s);
/* risk[r] = -sum_j prod_{i <= j} (1 - sigmoid(logits[r, i]))   (train_survival.py:1431-1433; no clamp) */
int mh_surv_risk(const float* logits, int64_t ld, int N, int M, float* risk, mh_stream s);
/* pair counts of the censored concordance index (sksurv.metrics.concordance_index_censored, train_survival.py:1460-1465):
 * counts[5] int64 = {concordant, discordant, tied_risk, tied_time, comparable}, zeroed on s by this call.  Pair (i, j) is comparable
 * when event[i] and (time[j] > time[i] or (time[j] == time[i] and !event[j])); tied when |est[j] - est[i]| <= tied_tol in f32,
 * concordant when not tied and est[j] < est[i], discordant otherwise; tied_time counts the comparable pairs at equal time.
 * O(n^2) pairs through LDS, integer atomics (deterministic); n <= 2^26. */
int mh_cindex_counts(const uint8_t* event, const double* time, const float* estimate, int64_t n, float tied_tol, int64_t* counts,
                     mh_stream s);

/* ---------------------------------------------------------------- continuous-time survival: Cox loss and log-rank test (added in v122)
 * The Cox proportional-hazards partial likelihood of a one-logit head (MCAT / PORPOISE `CoxSurvLoss`, DeepSurv, pycox) on the
 * follow-up time itself, no bins.  scores r [N] f32 read through the row stride ld (a [N] vector, or one column of a matrix);
 * time [N] f64, 8-byte aligned; e_i = (censoring_i == 1) read through dt_c (MH_SV_*), anything else is censored.
 *   m = max_j r_j,  w_j = exp(r_j - m) in f64
 *   S_i = sum_j [t_j >= t_i] w_j     D_i = sum_j [t_j == t_i][e_j] w_j     d_i = sum_j [t_j == t_i][e_j]
 *   l_i = sum_{j < i} [t_j == t_i][e_j]
 *   f_i = 0 (MH_COX_BRESLOW);  l_i / d_i on event rows, else 0 (MH_COX_EFRON);   den_i = S_i - f_i D_i  (> 0 whenever w_i > 0)
 *   loss_i = e_i (log den_i + m - r_i)
 * which, summed over a tie group in index order, is the textbook Breslow / Efron partial likelihood.  Reductions: none (rows only),
 * sum, mean = sum / max(n_events, 1) (DeepSurv / pycox), batch = sum / N (MCAT); no events: loss 0, gradient 0.  n_events and the
 * divisor stay on the device.  A NaN time gives NaN in that row's loss and gradient and the row is in no other row's risk set; a NaN
 * logit makes m, and with it every row, NaN.  Domain: max r - min r <= 700 (beyond it w underflows in f64); 1 <= N <= 65536.
 * Every sum is f64 in a fixed order (per row four partial sums over ascending j, added in order; rows folded by one block): bitwise
 * reproducible, no atomics, nothing allocated, no host wait, graph capturable.  Only the stores to loss_rows / out / dlogits round to
 * f32. */
#define MH_COX_BRESLOW 0
#define MH_COX_EFRON 1
#define MH_COX_RED_NONE 0
#define MH_COX_RED_SUM 1
#define MH_COX_RED_MEAN 2
#define MH_COX_RED_BATCH 3
/* bytes of the workspace the forward fills and the backward reads (m, n_events, w, den, f and the f64 rows: 8 (4 N + 2)); -1 for a
 * bad N */
int64_t mh_cox_workspace_bytes(int N);
/* loss_rows [N] f32 (nullable) = loss_i; out[0] (nullable, needs a reduction other than none; STORED, not accumulated) = the reduced
 * loss.  Three launches: m / w / n_events, the pair pass (64 rows per block, one per lane; the block's four waves split each LDS
 * tile of 256 j), the fold. */
int mh_cox_loss_fwd(const float* logits, int64_t ld, const double* time, const void* censoring, int dt_c, int N, int ties,
                    int reduction, float* loss_rows, float* out, void* workspace, mh_stream s);
/* dlogits[k * ld_d] = d(sum_i g_i loss_i) / d r_k = w_k sum_i q_i ([t_k > t_i] + [t_k == t_i](1 - e_k f_i)) - g_k e_k with
 * q_i = g_i e_i / den_i, where g_i = g[i] (g_per_row, reduction none only) or the reduction's coefficient times g[0].  workspace: as
 * the forward with the same inputs, ties and N left it (ties is already folded into f there; the scores enter through w). */
int mh_cox_loss_bwd(const float* logits, int64_t ld, const double* time, const void* censoring, int dt_c, int N, int ties,
                    int reduction, const float* g, int g_per_row, const void* workspace, float* dlogits, int64_t ld_d, mh_stream s);
/* Two-group log-rank statistics: event [n] (nonzero = event), time [n] f64, group [n] (nonzero = group 1), 1 <= n <= 65536.
 * For every distinct event time tau: n(tau) = #{t_j >= tau}, n1(tau) the same within group 1, d(tau) = #{t_j == tau, event_j},
 * d1(tau); stats f64 [4] = {O1 = sum d1, E1 = sum d n1 / n, V = sum n1 (n - n1) d (n - d) / (n^2 (n - 1)) over n > 1, n_events}.
 * The first event row (smallest index) at a time owns its term; counts are integers, the terms f64, added in index order by one
 * block.  Rows with a NaN time are ignored.  chi2 = (O1 - E1)^2 / V and p = erfc(sqrt(chi2 / 2)) are the caller's. */
int mh_logrank_stats(const uint8_t* event, const double* time, const uint8_t* group, int64_t n, double* stats, mh_stream s);

/* ---------------------------------------------------------------- downstream subtyping step (train_subtyping.py, v120)
 * logits / scores [N x C] f32, row stride ld (the f32 output of mirror_classifier, models/mirror.py:667-707); labels [N] int32 /
 * int64 read through dt_l (MH_SV_I32 / MH_SV_I64 of the survival block).  Every entry point is deterministic (no float atomics:
 * fixed-order sums in one block, integer atomics for counts) and graph capturable; nothing is allocated. */
#define MH_CLS_RED_NONE 0   /* torch's Reduction enum: "none" */
#define MH_CLS_RED_MEAN 1   /* "mean" */
#define MH_CLS_RED_SUM 2    /* "sum" */
/* Cross-entropy with label smoothing s, per row: loss_r = (1 - s) (lse_r - x[r, y_r]) + s (lse_r - mean_c x[r, c]), lse_r =
 * logsumexp(x[r, :]) (timm's LabelSmoothingCrossEntropy, train_subtyping.py:984; nn.CrossEntropyLoss(label_smoothing=s,
 * ignore_index, reduction), :986 / :990).  A row whose label equals ignore_index has loss 0 and is not counted; a row whose label
 * is otherwise outside [0, C) has loss NaN (torch raises / device-asserts there).  row_loss [N]: the per-row losses (nullable
 * unless mode = MH_CLS_RED_NONE); out[0] (mean / sum; STORED, not accumulated) = the sum of the rows in a fixed order, divided
 * by the number of non-ignored rows for MH_CLS_RED_MEAN (NaN when every row is ignored, as torch).  One block, one launch. */
int mh_cls_ce_fwd(const float* logits, int64_t ld, const void* labels, int dt_l, int N, int C, float smoothing, int64_t ignore_index,
                  float* row_loss, float* out, int mode, mh_stream s);
/* dlogits [N x C] contiguous: dx[r, c] = w_r (softmax(x_r)[c] - (1 - s) [c == y_r] - s / C), recomputed from the logits; w_r =
 * g[r] (MH_CLS_RED_NONE), g[0] (SUM) or g[0] / #non-ignored rows (MEAN); 0 for ignored rows, NaN for out-of-range labels. */
int mh_cls_ce_bwd(const float* logits, int64_t ld, const void* labels, int dt_l, int N, int C, float smoothing, int64_t ignore_index,
                  const float* g, int mode, float* dlogits, mh_stream s);
/* Confusion counts behind top-1 accuracy (timm.utils.accuracy, train_subtyping.py:1390) and MulticlassF1Score (:1358-1360, :1392):
 * conf [C x C] int64, indexed [label, prediction], ACCUMULATED (the caller zeroes it).  input: f32 scores [N x C] with row stride
 * ld (dt_in = MH_SV_F32; the prediction is the first maximum of the row, or its first NaN, as torch.argmax) or predicted labels
 * [N] (dt_in = MH_SV_I32 / MH_SV_I64; ld ignored).  A row whose label or prediction lies outside [0, C) leaves conf alone and adds
 * 1 to bad[0] (int64, accumulated).  An int32 LDS copy of conf per block when C * C <= 4096, integer atomics. */
int mh_cls_confusion(const void* input, int64_t ld, int dt_in, const void* labels, int dt_l, int N, int C, int64_t* conf, int64_t* bad,
                     mh_stream s);
/* One-vs-rest AUROC of torcheval's MulticlassAUROC (train_subtyping.py:1355-1357, :1391, :1419-1422) as exact integer pair counts:
 * counts [C x 4] int64 = {U2_c, P_c, Q_c, NaN_c}, zeroed on s by this call.  For class c the positives are the rows with
 * labels == c, the negatives all others (out-of-range labels included) and the score is the raw column scores[:, c];
 * U2_c = 2 #{(i pos, j neg): s_i > s_j} + #{s_i == s_j}, so AUROC_c = U2_c / (2 P_c Q_c); NaN_c = the NaN scores in column c
 * (their pairs add nothing).  labels int64 [N].  O(N^2 C) pairs through LDS; 1 <= N <= 2^20, 2 <= C <= 1024. */
int mh_auroc_counts(const float* scores, int64_t ld, const int64_t* labels, int N, int C, int64_t* counts, mh_stream s);
/* The same pair counts for E score tables that share ONE label vector, in one launch (the S strengths of a held-out fold of
 * LinearProbe.evaluate): table e is scores + e ld_table, its rows ld_row floats apart; counts [E x C x 4] int64, zeroed on s by this
 * call, and counts[e] is, integer for integer, what mh_auroc_counts(scores + e ld_table, ld_row, ..) answers: the same kernel with
 * the (table, class) pair e C + c in the grid's z, the negatives staged through LDS and integer atomics as there.  1 <= N <= 2^20,
 * 2 <= C <= 1024, ld_row >= C, E >= 1, E C <= 65535 (the grid's z extent), ld_table >= N ld_row when E > 1.
 * O(E N^2 C) pairs; per (table, class) N 4 bytes of scores and N 8 of labels per block row of 256 positives. */
int mh_auroc_counts_many(const float* scores, int64_t ld_row, int64_t ld_table, const int64_t* labels, int N, int C, int E,
                         int64_t* counts, mh_stream s);

/* ---------------------------------------------------------------- InfoNCE with explicit negative keys (losses/info_nce.py:126-143;
 * the reference builds these logits and labels and forgets `F.cross_entropy(logits / temperature, labels)`).
 * logits[i] = [q^[i].k^[i] | neg[i, :]] / t with label 0; q^, k^ [N x D] f32 are the normalised query / positive key (mh_l2norm_fwd).
 * Every entry point is deterministic (fixed summation order, no atomics), allocates nothing and never waits on the host.
 *
 * Paired negatives n [N x M x D] (f32 / bf16 by dt_neg, contiguous, read in place: no normalised copy exists).
 *   fwd: ONE read of n:  inv[i, j] = 1 / max(|n[i, j]|, eps),  cosv[i, j] = q^[i].n[i, j] * inv[i, j]   (both f32 [N x M]).
 *   bwd: ONE read of n (+ ONE write of dneg): dl f32 [N x M] is d loss / d cosv (mh_infonce_rows_bwd);
 *        dneg[i, j] = dl inv (q^[i] - cosv inv n[i, j]) in n's dtype (NULL: not written);
 *        dq_part f32 [N x ceil(M / jc) x D] = per-chunk sums of dl inv n[i, j] over jc consecutive j (NULL: not formed), folded by
 *        mh_infonce_fold.  N <= 65535, N * M < 2^31. */
int mh_infonce_paired_fwd(const float* qn, const void* neg, float* cosv, float* inv, int N, int M, int D, float eps, int dt_neg,
                          mh_stream s);
int mh_infonce_paired_bwd(const float* qn, const void* neg, const float* cosv, const float* inv, const float* dl, void* dneg,
                          float* dq_part, int N, int M, int D, int jc, int dt_neg, mh_stream s);
/* The label-0 cross-entropy both modes share; neg f32 [N x M] with row stride ld holds the cosines (paired: cosv; unpaired: q^ n^T of
 * mh_gemm).  fwd, with x0 = q^[i].k^[i] * inv_t: lse[i] = logsumexp([x0 | neg[i, :] * inv_t]), loss_rows[i] = lse[i] - x0,
 * pneg[i] = 1 - softmax[i, 0] = sum_j exp(neg[i, j] inv_t - lse[i]) (all f32 [N], all written; a row whose positive dominates gets its
 * loss as log1p of the negatives' sum, not as a difference of numbers near 1), out[0] = coef * sum_i loss_rows[i] (NULL: not formed).
 * bwd: with u_i = gcoef * g[g_per_row ? i : 0] * inv_t:  dneg[i, j] = u_i exp(neg[i, j] inv_t - lse[i]) (f32 [N x M] contiguous),
 * dpos[i] = -u_i pneg[i]. */
int mh_infonce_rows_fwd(const float* qn, const float* kn, const float* neg, int64_t ld, int N, int M, int D, float inv_t, float coef,
                        float* pneg, float* lse, float* loss_rows, float* out, mh_stream s);
int mh_infonce_rows_bwd(const float* neg, int64_t ld, const float* pneg, const float* lse, const float* g, int g_per_row, float gcoef,
                        float inv_t, int N, int M, float* dneg, float* dpos, mh_stream s);
/* dq[i] = dpos[i] k^[i] + sum_p part[i, p, :] (p ascending; part f32 [N x nparts x D]: mh_infonce_paired_bwd's dq_part, or the
 * unpaired dl n^ product with nparts = 1),  dk[i] = dpos[i] q^[i];  dq / dk NULL: not written. */
int mh_infonce_fold(const float* dpos, const float* qn, const float* kn, const float* part, int nparts, float* dq, float* dk, int N,
                    int D, mh_stream s);

/* ---------------------------------------------------------------- cross-modal retrieval (the zero-shot check of the alignment
 * heads: recall@k and median rank, train_mirror.py:1382-1526)
 * rank of each query's positive key among nk keys, by dot-product similarity:
 * ranks[i] = 1 + #{ j != target[i] : !(dot(q_i, k_j) < dot(q_i, k_target[i])) }      (int32 [nq], initialised on s by this call)
 * q [nq x D], k [nk x D] f32 contiguous; target int64 [nq] in [0, nk), or NULL = identity (needs nq == nk).
 * Pessimistic on ties and NaN: a key that ties with the positive, or whose similarity (or the positive's) is NaN, counts
 * against the query, so a collapsed encoder (all embeddings equal) scores rank nk everywhere, never rank 1.
 * Every dot product, the positive's included, is the same k-ordered f32 fmaf chain (v_mfma_f32_32x32x2_f32, no split-K): a key row
 * bit-identical to the positive's ties with it at every D.  Only the column j == target[i] is excluded, not its duplicates.
 * A target outside [0, nk) is not clamped: no key is read for it and the query gets rank nk + 1.
 * 1 <= nq, nk <= 2^20, 1 <= D <= 4096.  The nq x nk matrix is never written.  Deterministic (integer atomics only).
 * workspace: mh_retrieval_workspace_bytes(nq, nk, D) bytes (O(nq): the positives' similarities), 4-byte aligned. */
int mh_retrieval_ranks(const float* q, const float* k, int64_t nq, int64_t nk, int D, const int64_t* target, int32_t* ranks,
                       void* workspace, mh_stream s);
int64_t mh_retrieval_workspace_bytes(int64_t nq, int64_t nk, int D);
/* The same rank with SEVERAL positives per query (a sample with several slides: every slide of it is paired with the same RNA row).
 * Group ids are arbitrary int64 values compared for equality only, all 64 bits.  With s_ij = dot(q_i, k_j) (the same fmaf chain) and
 * P_i = { j : kgroup[j] == qgroup[i] }:
 *   d_i      = max_{j in P_i} s_ij, the best positive; NaN if P_i is empty or any s_ij, j in P_i, is NaN
 *   ranks[i] = 1 + #{ j not in P_i, kcount[j] != 0 : !(s_ij < d_i) }                  (int32 [nq], initialised on s by this call)
 * kcount: uint8 [nk] or NULL (every key counts).  It never removes a positive from P_i, it only says which non-positives can count
 * (e.g. one row per group: a gallery of distinct samples).  A key of ANOTHER group that is a bit-identical copy of the best positive
 * ties and counts; a copy inside the own group never counts.  An empty P_i gives 1 + the number of counted keys.
 * kgroup_sorted int64 [nk]: kgroup in ascending order; kperm int64 [nk]: the key row each sorted position came from (what a sort of
 * kgroup returns).  An entry of kperm outside [0, nk) reads no key and makes its group's d_i NaN.
 * Same limits, the same two launches, nothing allocated, no host wait, deterministic; workspace: mh_retrieval_workspace_bytes(nq, nk, D)
 * bytes as above.  With all-distinct ids on a square problem and kcount NULL the ranks equal mh_retrieval_ranks' with target NULL. */
int mh_retrieval_ranks_grouped(const float* q, const float* k, int64_t nq, int64_t nk, int D, const int64_t* qgroup,
                               const int64_t* kgroup, const int64_t* kgroup_sorted, const int64_t* kperm, const uint8_t* kcount,
                               int32_t* ranks, void* workspace, mh_stream s);
/* The neighbours themselves: for every query the kk eligible keys with the largest s_ij = dot(q_i, k_j), the same fmaf chain as above
 * (val is that chain bit for bit, so top-k and ranks are decided by the same numbers whatever the tiling or `parts`).
 *   idx int32 [nq x kk], val f32 [nq x kk]; slot 0 is the best.  The order is total: the larger s_ij first, equal s_ij by the SMALLER j.
 *   Key j is eligible for query i unless s_ij is NaN, or (with group ids) kgroup[j] == qgroup[i], compared on all 64 bits.
 *   Slots beyond the number of eligible keys hold idx = -1, val = -inf (kk > nk is allowed; a NaN query gets all -1).
 * qgroup int64 [nq], kgroup int64 [nk]: both or neither (NULL), 8-byte aligned.  Leave-one-out over one set: the ids 0 .. n - 1.
 * 1 <= kk <= 64; nq, nk, D as above.  The nq x nk matrix is never written; nothing is allocated, no host wait, no atomics: deterministic.
 * The keys are walked in `parts` strips of 128-key tiles, each keeping a list per query, merged by the same order in a second launch.
 * parts = 0: chosen from nq, nk and the CU count; parts > 0: as given, at most the number of key tiles.  The result does not depend on it.
 * workspace: mh_retrieval_topk_workspace_bytes(nq, nk, D, kk, parts) bytes (the strips' lists, 8 nq parts kk), 8-byte aligned. */
int mh_retrieval_topk(const float* q, const float* k, int64_t nq, int64_t nk, int D, int kk, const int64_t* qgroup, const int64_t* kgroup,
                      int parts, int32_t* idx, float* val, void* workspace, mh_stream s);
int64_t mh_retrieval_topk_workspace_bytes(int64_t nq, int64_t nk, int D, int kk, int parts);
/* The kNN vote on a top-k result: idx / val [nq x kk] as above, labels int64 [nk] (8-byte aligned) of the bank, scores f32 [nq x C]:
 *   w_is        = exp((val[i, s] - val[i, 0]) * inv_temperature)        (val[i, 0] is the row's maximum: exp stays in (0, 1])
 *   score[i, c] = sum_s [labels[idx[i, s]] == c] w_is / sum_s' w_is'    (both sums in slot order, s' over the contributing slots)
 * Empty slots (idx < 0; idx >= nk is not read) and labels outside [0, C) contribute nothing; a row without contribution is all zeros,
 * every other row sums to 1.  inv_temperature = 0 is the unweighted vote.  1 <= kk <= 64, 1 <= C <= 1024, 0 <= inv_temperature < inf.
 * One wave per query, a fixed order of additions, no atomics. */
int mh_knn_scores(const int32_t* idx, const float* val, const int64_t* labels, int64_t nq, int64_t nk, int kk, int C,
                  float inv_temperature, float* scores, mh_stream s);

/* ---------------------------------------------------------------- few-shot prototype probe of frozen embeddings (csrc/fewshot.hip;
 * the reference has the protocol only: tools/gen_few_shot_files.py draws `shots` training slides per class with random.choices,
 * tools/downstream_tasks_evaluator.py evaluates on the fold's validation slides).  The classifier is SimpleShot's nearest centroid
 * (Wang et al. 2019): centre, L2-normalise, average the support, take the nearest prototype, over E support draws ("episodes") at once.
 * Every entry point is deterministic (fixed summation order, no float atomics), allocates nothing and never waits on the host.
 *
 * mu [D] f32 = the column means of x [n x D] f32 contiguous: up to 128 strips of rows, each summed in row order in f64, the strips
 * added in strip order, divided by n and rounded to f32 once (an error of half an ulp of mu[d], whatever n).  Two launches.
 * 1 <= n <= 2^20, 1 <= D <= 4096.  workspace: mh_colmean_workspace_bytes(n, D) bytes (the strips' sums, 8 D per strip), 8-byte aligned,
 * nothing to zero.  (mh_colsum adds with float atomics and in no fixed order.) */
int mh_colmean(const float* x, int64_t n, int D, float* mu, void* workspace, mh_stream s);
int64_t mh_colmean_workspace_bytes(int64_t n, int D);
/* y[r] = (x[r] - mu) / max(||x[r] - mu||, eps), x, y [n x D] f32 contiguous (y may be x), mu [D]: mh_l2norm_fwd behind a centring.
 * One wave per row: a lane adds the squares of its columns d = lane, lane + 64, .. in that order, the lanes are added by a fixed
 * butterfly.  Same limits; eps > 0.  2 n D 4 bytes read (the second pass from cache at D <= 4096), n D 4 written. */
int mh_center_l2norm(const float* x, const float* mu, float* y, int64_t n, int D, float eps, mh_stream s);
#define MH_FEWSHOT_EUCLIDEAN 0   /* SimpleShot: nearest prototype by distance, as the argmax of q.p - |p|^2 / 2 */
#define MH_FEWSHOT_COSINE 1      /* the prototype is normalised again; no bias */
/* Prototypes of E episodes x C classes from K support rows each: rows int64 [E x C x K] indexes the prepared pool y [n x D] f32,
 * through perm int64 [n] when that is not NULL (row = perm[rows[..]]: the class-sorted order mh_sample_rows drew in).
 *   p[e, c] = (sum_k y[row(e, c, k)]) * (1 / K)       summed in k order in f32 from 0, one multiply by the f32 reciprocal of K
 *   euclidean: bias[e, c] = -0.5 |p|^2 (f32; argmax_c of q.p + bias = argmin_c |q - p|);  cosine: p / max(|p|, 1e-12), bias must be NULL.
 * protos f32 [E x Cp x D], bias f32 [E x Cp], Cp = the next power of two >= C: slots c >= C are pads, 0 with bias -inf, so that an
 * episode's keys never straddle a 128-key tile of mh_fewshot_predict.  An index outside [0, n) (in rows, or in perm where rows points)
 * reads nothing and makes that one prototype and its bias NaN.  |p|^2: per thread in column order, a fixed butterfly, the four waves in
 * order.  2 <= C <= 64, 1 <= K <= 1024, 1 <= D <= 4096, 1 <= n <= 2^20, E Cp <= 2^20.  One workgroup per (e, slot);
 * E C K D 4 bytes read, E Cp D 4 written. */
int mh_fewshot_protos(const float* y, int64_t n, const int64_t* rows, const int64_t* perm, int E, int C, int Cp, int K, int D, int metric,
                      float* protos, float* bias, mh_stream s);
/* pred int32 [E x nq]: the class of the largest score[e, i, c] = dot(q_i, p[e, c]) + bias[e, c], where the dot product is the k-ordered
 * f32 fmaf chain from 0 of the retrieval kernels (v_mfma_f32_32x32x2_f32 over the E Cp prototypes as keys, no split-K) and the bias is
 * ONE f32 add (bias NULL, the cosine metric: no add).  A NaN score is not eligible, equal scores go to the SMALLER class, pad slots are
 * never looked at; pred = -1 when no class is eligible (a NaN query row).  q [nq x D] f32 contiguous (prepared like the pool).
 * Grid ceil(nq / 128) x ceil(E Cp / 128); the 128 x 128 tile goes through LDS in two halves behind the product and one thread scans
 * each (row, episode) in ascending class order: no [nq x E Cp] matrix is written, no atomics.  Limits as above, 1 <= nq <= 2^20.
 * (nq + E Cp) D 4 bytes read per tile row / column, E nq 4 written. */
int mh_fewshot_predict(const float* q, const float* protos, const float* bias, int64_t nq, int E, int C, int Cp, int D, int32_t* pred,
                       mh_stream s);
/* Per-episode confusion counts and summary of pred [E x nq] against labels int64 [nq] (8-byte aligned):
 *   conf int32 [E x C x C], indexed [label, prediction], STORED (nothing to zero).  A row whose label lies outside [0, C) or whose
 *   prediction is -1 enters no cell and adds 1 to bad[e] (int32 [E], stored).
 *   summary f64 [E x 3], with tp_c = conf[c, c], n_c = the rows of label c (a prediction of -1 included), m_c = sum_y conf[y, c]:
 *     [0] accuracy, percent            100 sum_c tp_c / sum_c n_c
 *     [1] balanced accuracy, percent   100 mean of tp_c / n_c over the classes with n_c > 0
 *     [2] macro F1 in [0, 1]           mean of 2 tp_c / (n_c + m_c) over the classes with n_c + m_c > 0 (sklearn's f1_score "macro")
 *   each formed in f64 from the integer counts in class order; NaN when no class qualifies.
 * One workgroup per episode, integer LDS atomics only.  2 <= C <= 64, 1 <= E, nq <= 2^20. */
int mh_fewshot_tally(const int32_t* pred, const int64_t* labels, int64_t nq, int E, int C, int32_t* conf, int32_t* bad, double* summary,
                     mh_stream s);

/* ---------------------------------------------------------------- k-means of frozen embeddings, scored against labels (csrc/kmeans.hip;
 * mirror_amd/cluster.py).  The label-free question of a self-supervised encoder: do the slide embeddings fall into the cohort's
 * subtypes on their own?  Lloyd's iteration over R restarts at once (the restarts in the role of the few-shot episodes), then NMI, ARI
 * and purity of the clusters against the labels.  Every entry point is deterministic (fixed summation order, no float atomics),
 * allocates nothing and never waits on the host.  Shared limits: 1 <= K <= 1024 clusters, 1 <= D <= 4096, 1 <= n <= 2^20 rows,
 * 1 <= R <= 65535 restarts (one grid row each) with R K <= 2^20.  x [n x D] f32 contiguous is the prepared pool (mh_colmean,
 * mh_center_l2norm), cent [R x K x D] f32 the centroids, assign int32 [R x n].
 *
 * assign[r, i] = the k with the largest score dot(x_i, cent[r, k]) + bias[r, k]: the dot product is the k-ordered f32 fmaf chain from 0
 * of the retrieval kernels (v_mfma_f32_32x32x2_f32, no split-K), the bias (f32 [R x K], or NULL: no add) is ONE f32 add.  A NaN score is
 * not eligible, equal scores go to the SMALLER k, assign = -1 when nothing is eligible (a NaN row).  score f32 [R x n] or NULL: the
 * winning value (NaN beside -1).  prev int32 [R x n] or NULL, and it may be assign itself: with it, changed[r] (int32 [R], ZEROED BY THE
 * CALLER, NULL exactly when prev is) grows by the number of rows of restart r whose assignment differs from prev: one integer atomic per
 * workgroup.  Grid ceil(n / 128) x R: a workgroup walks the ceil(K / 128) key tiles of its restart in ascending order and carries every
 * row's best across them; no [n x R K] matrix is written, columns >= K are never looked at, cent needs no padding.
 * A workgroup loads its 128 rows again for every key tile and all K centroids of its restart once: R (n ceil(K / 128) + ceil(n / 128) K) D 4
 * bytes read, 2 n R K D flop. */
int mh_kmeans_assign(const float* x, const float* cent, const float* bias, int64_t n, int R, int K, int D, const int32_t* prev,
                     int32_t* assign, float* score, int32_t* changed, mh_stream s);
#define MH_KMEANS_EUCLIDEAN 0    /* nearest centroid by distance, as the argmax of x.c - |c|^2 / 2 */
#define MH_KMEANS_COSINE 1       /* spherical k-means: the centroid is normalised; no bias */
/* The centroid update.  For every (r, k) with at least one row i of assign[r, i] = k:
 *   cent[r, k, d] = (sum of x[i, d] over those rows IN ASCENDING ROW ORDER IN F64) / their number, in f64, rounded to f32 ONCE
 *   euclidean: bias[r, k] = -0.5 |c|^2 of the ROUNDED centroid, |c|^2 in f64, rounded to f32 once
 *   cosine: c / max(|c|, 1e-12) afterwards, the quotient in f64 from the rounded mean and rounded once more; bias must be NULL.
 * |c|^2: per thread in column order, a fixed butterfly, the four waves in order.  count int32 [R x K]: the members, stored.  An empty
 * cluster KEEPS its centroid and its bias and reports 0; rows with assign outside [0, K) belong to no cluster.  The same assign gives
 * the same centroids bit for bit, so a converged restart is a fixed point of assign + update.  One workgroup per (r, k) scans
 * assign[r, :] 256 rows at a time and compacts the members in row order: R K n 4 bytes of assign (from cache) and R n D 4 bytes of x
 * read.  workspace: mh_kmeans_update_workspace_bytes(n, R, K, D) bytes, which is 0 for this form (NULL is fine). */
int mh_kmeans_update(const float* x, const int32_t* assign, int64_t n, int R, int K, int D, int metric, float* cent, float* bias,
                     int32_t* count, void* workspace, mh_stream s);
int64_t mh_kmeans_update_workspace_bytes(int64_t n, int R, int K, int D);
/* bias[r, k] = -0.5 |cent[r, k]|^2 for centroids that did not come out of the update (the rows a restart starts from, a caller's own
 * centroids): |c|^2 in f64 in the update's order of additions, rounded to f32 once, so on an updated centroid it repeats the update's
 * bias bit for bit.  One workgroup per (r, k). */
int mh_kmeans_bias(const float* cent, int R, int K, int D, float* bias, mh_stream s);
/* inertia f64 [R]: the sum over the rows with assign in [0, K) of |x_i - cent[r, assign[r, i]]|^2, each row's term in f64 over ascending
 * d (one fma per column), the rows of a strip added in row order, the strips (mh_colmean's: up to 128 of at least 64 rows) in strip
 * order.  Two launches.  workspace: mh_kmeans_inertia_workspace_bytes(n, R) bytes (8 per strip and restart), 8-byte aligned, nothing to
 * zero.  2 R n D 4 bytes read. */
int mh_kmeans_inertia(const float* x, const float* cent, const int32_t* assign, int64_t n, int R, int K, int D, double* inertia,
                      void* workspace, mh_stream s);
int64_t mh_kmeans_inertia_workspace_bytes(int64_t n, int R);
/* Per-restart contingency counts and agreement scores of assign [R x n] against labels int64 [n] (8-byte aligned):
 *   cont int32 [R x K x C], indexed [cluster, label], STORED (nothing to zero).  A row whose label lies outside [0, C) or whose
 *   assignment lies outside [0, K) enters no cell and adds 1 to bad[r] (int32 [R], stored); N below is the number of the other rows.
 *   summary f64 [R x 3], with a_k and b_c the row and column sums of cont:
 *     [0] NMI      I / ((H(a) + H(b)) / 2), natural log, I = sum over the cells n_kc > 0 of (n_kc / N) (log n_kc - log a_k - log b_c + log N)
 *                  (a term below 2^-52 counts as 0, a negative sum as 0), H(a) = -sum_k (a_k / N) (log a_k - log N)
 *     [1] ARI      2 (tp tn - fn fp) / ((tp + fn) (fn + tn) + (tp + fp) (fp + tn)) from the exact integer pair counts
 *     [2] purity   sum_k max_c n_kc / N
 *   each formed in f64 from the integer counts: a cluster's cells in label order, the clusters in cluster order.  The degenerate cases
 *   are sklearn's (normalized_mutual_info_score, adjusted_rand_score): NMI = 1 when neither side splits the rows, 0 when exactly one
 *   does not or I = 0; ARI = 1 when fn = fp = 0; N = 0 gives NMI = ARI = 1 and purity NaN.
 * One workgroup per restart; integer atomics only, on the workgroup's own slice of cont and in LDS.  1 <= K, C <= 1024, K C <= 65536,
 * 1 <= R, n <= 2^20. */
int mh_kmeans_tally(const int32_t* assign, const int64_t* labels, int64_t n, int R, int K, int C, int32_t* cont, int32_t* bad,
                    double* summary, mh_stream s);

/* ---------------------------------------------------------------- cluster probe: seeding, silhouette, matched accuracy
 * (csrc/cluster_ext.hip; mirror_amd/cluster.py).  As the k-means section: deterministic (fixed orders of addition, no float atomics),
 * nothing allocated, no host wait, every launch on the caller's stream (graph-capturable).  Limits: 1 <= n <= 2^20, 1 <= D <= 4096,
 * 1 <= K <= 1024, 1 <= R <= 65535.
 *
 * Silhouette of R label rows lab int32 [R x n] over the prepared rows y [n x D] f32 contiguous.  Per label row, with
 *   s_ij  = dot(y_i, y_j): the k-ordered f32 fmaf chain from 0 of the retrieval kernels (v_mfma_f32_32x32x2_f32, no split-K)
 *   q_i   = the SAME chain of row i with itself, so that identical rows are at distance exactly 0
 *   d_ij  = sqrt(max(fma(-2, s_ij, q_i + q_j), 0)) in f64 from the f32 values   (MH_KMEANS_EUCLIDEAN)
 *           1 - s_ij in f64   (MH_KMEANS_COSINE: on unit rows, which the probe prepares, sklearn's metric="cosine")
 *   S_i[k] = sum of d_ij over j != i with lab_j = k; the pair i = j is left out BY INDEX, not by value
 *   a_i = S_i[l_i] / (n_l_i - 1),  b_i = min over the non-empty k != l_i of S_i[k] / n_k,  s_i = (b_i - a_i) / max(a_i, b_i)
 *   s_i = 0 when the row's cluster is a singleton or max(a_i, b_i) = 0 (sklearn's silhouette_samples); NaN when fewer than two clusters
 *   are non-empty.
 * A row with lab outside [0, K) takes no part, as sample or as neighbour: it adds 1 to bad[r] (int32 [R], stored) and its sil is NaN.
 * sil f64 [R x n] or NULL; mean f64 [R]: the mean of s_i over the rows that take part, each of mh_colmean's strips (up to 128 of at
 * least 64 rows) added in row order, the strips in strip order, divided by their number; NaN when fewer than two clusters are non-empty
 * or no row takes part.  A NaN anywhere in y may make every sample, and the mean, NaN.
 * Order of additions of S_i[k]: the rows are sorted by cluster id (stable: row order inside a cluster, the rows outside last) and
 * the sorted sequence is cut into key tiles of 128 and those into quarters of 32; the T = ceil(n' / 128) key tiles (n' the rows that
 * take part) form P contiguous groups, group p the tiles [p T / P, (p + 1) T / P), with P = min(16, ceil(n / 128), ceil(1024 /
 * ceil(n / 128)), 1 + floor(2^26 / (8 n K))): a workgroup per (row tile, group), so that a few thousand rows fill the chip, while the
 * slices of S beyond the first stay within 64 MiB; P = 1 from n = 2^17 on and wherever n K >= 2^23.  A (tile,
 * quarter)'s distances to cluster k are added in ascending sorted order from 0; of one tile, the quarters' sums for the same k that
 * reach an end of their quarter are added to each other in ascending order first; the results are added to the group's sum in
 * ascending order, and the P groups' sums in group order.  Every sample therefore carries a relative error of a few 2^-53 on top of
 * the f32 products'.
 * Five launches per label row; the n x n products are formed once per label row and never stored: no [n x n] matrix, the only state
 * that grows with K is S f64 [P x n x K] in the workspace: [n x K] and at most 64 MiB more (one form for every K).  Rows are loaded again for
 * every key tile: 2 n ceil(n / 128) D 4 bytes read, 2 n^2 D flop per label row.
 * workspace: mh_silhouette_workspace_bytes(n, K, D) bytes (the sorted copy of y, S, the samples in row order, q, the order, the sorted
 * ids, the cluster sizes: about n (4 D + 8 P K + 20)), 16-byte aligned, nothing to zero, shared by the label rows. */
int mh_silhouette(const float* y, const int32_t* lab, int64_t n, int R, int K, int D, int metric, double* sil, double* mean, int32_t* bad,
                  void* workspace, mh_stream s);
int64_t mh_silhouette_workspace_bytes(int64_t n, int K, int D);
/* k-means++ seeding (Arthur and Vassilvitskii 2007: D^2 sampling, ONE draw per centre; NOT sklearn's greedy variant with local
 * trials) of R restarts at once from the prepared rows y [n x D]: rows int64 [R x K] (8-byte aligned) the chosen rows, cent f32
 * [R x K x D] bit copies of them.  R K <= 2^20.  Restart r uses draw id offset + r of the data feed's Philox stream under kind = 2
 * (counter = (lo32(blk), 2, lo32(draw), 0x80000000 | hi32(draw)), key = seed; draw ids stay below 2^63); u_j comes from elements 2 j and
 * 2 j + 1 by mh_sample_weighted's rule, (((w >> 5) << 26) | (w' >> 6)) 2^-53.
 *   centre 0    row floor(u_0 n), one f64 product
 *   centre j    m_i = min over the chosen centres c of |y_i - c|^2: f64, ascending d, one fma per column (mh_kmeans_inertia's term);
 *               a NaN distance counts as 0.  P_p = the sum of m_i over strip p of mh_colmean's partition in row order from 0,
 *               T = the sum of P_p in strip order from 0, t = u_j T.  The pick is the first strip p with (P_0 + .. + P_p) > t, and in it
 *               the first row i with (P_0 + .. + P_(p-1)) + (the strip's own running sum up to and including i) > t: such a row has
 *               m_i > 0.  If rounding leaves no strip (t = T), the pick is the last row with m_i > 0.  If T = 0 (fewer distinct rows
 *               than centres) or T is NaN, the pick is row floor(u_j n).
 * The distance is Euclidean in the prepared space for both metrics (on unit rows it is monotone in the cosine).  Two launches per
 * centre (one for centre 0): m is updated against the newest centre only.  workspace: mh_kmeanspp_workspace_bytes(n, R) bytes
 * (m f64 [R x n] and 8 per strip and restart), 8-byte aligned, nothing to zero.  R K n D 4 bytes read. */
int mh_kmeanspp_init(const float* y, int64_t n, int R, int K, int D, uint64_t seed, uint64_t offset, int64_t* rows, float* cent,
                     void* workspace, mh_stream s);
int64_t mh_kmeanspp_workspace_bytes(int64_t n, int R);
/* Matched accuracy from the contingency counts cont int32 [R x K x C] of mh_kmeans_tally ([cluster, label], non-negative): per
 * restart a one-to-one assignment of clusters to classes with min(K, C) pairs and the largest sum of cont[k, match[k]].
 *   match int32 [R x K]: the class of cluster k, or -1 (K > C: K - C clusters stay without);  hits int64 [R] (8-byte aligned): that sum.
 * All arithmetic is integer (int64 potentials), so hits is the exact optimum; among assignments of equal sum the choice is
 * deterministic (the smaller column of equal minima) but otherwise free.  One workgroup per restart: shortest augmenting paths
 * (Jonker-Volgenant), the smaller side as rows, a serial outer loop with the minimum over the columns workgroup-parallel; the cells
 * are read from LDS when K C <= 4096 and from cont in place otherwise: no workspace.  The tally's limits: 1 <= K, C <= 1024,
 * K C <= 65536, 1 <= R <= 2^20. */
int mh_cluster_match(const int32_t* cont, int R, int K, int C, int32_t* match, int64_t* hits, mh_stream s);

/* ---------------------------------------------------------------- linear probe of frozen embeddings (csrc/linprobe.hip;
 * mirror_amd/linprobe.py; the reference's train_subtyping.py --linear_probe over the folds of tools/gen_splits.py, with the frozen
 * encoder taken out of the loop).  J independent L2-regularised softmax regressions over the SAME prepared rows y [n x D] f32
 * contiguous (the folds x strengths in the role of the few-shot episodes); per job j
 *   F_j(W, b) = r_j sum_{i in train_j} CE(softmax(W y_i + b), label_i) + (lambda_j / 2) |W|^2     (the bias is not penalised)
 *   train_j   = { i : label_i in [0, C), fold_i >= 0, fold_i != heldout_j }                        (heldout_j = -1: every valid row)
 * and one FISTA iteration is the two launches below.  Layout as mh_fewshot_protos: Cp = the next power of two >= C, weights f32
 * [J x Cp x D], bias f32 [J x Cp], pad slots c >= C hold weight 0 and bias -inf (the caller sets them; neither entry point writes
 * them), so that a job's keys never straddle a 128-key tile.  Both are deterministic (fixed summation order, no float atomics),
 * allocate nothing and never wait on the host.  Shared limits: 2 <= C <= 64, 1 <= D <= 4096, 1 <= n <= 2^20, J Cp <= 2^20,
 * n J Cp <= 2^28.
 *
 * G f32 [n x J Cp], STORED (nothing to zero): G[i, j Cp + c] = r_j (p_c - [c = label_i]) for i in train_j and c < C, p = softmax of
 * v_c = dot(y_i, Wz[j, c]) + bz[j, c]; 0 for every other row and for pad columns.  The dot product is the k-ordered f32 fmaf chain
 * from 0 of the retrieval kernels (v_mfma_f32_32x32x2_f32 over the J Cp weight rows as keys), the bias ONE f32 add; then in class
 * order in f32: m = max_c v_c, lse = m + logf(sum_c expf(v_c - m)), p_c = expf(v_c - lse).  labels int64 [n] (8-byte aligned), fold
 * int32 [n], heldout int32 [J], rscale f32 [J] (r_j).  loss_part f64 [ceil(n / 128) x J] (8-byte aligned) or NULL:
 * loss_part[t, j] = r_j sum of CE_i = lse - v_label (f32) over the training rows of row tile t, added in row order in f64; their sum
 * over t is the data term of F_j at (Wz, bz), without the regulariser.  A NaN in a row makes the G rows and the loss of every job that
 * trains on it NaN (and, through the step, that job's weights): nothing is filtered.  Grid ceil(n / 128) x ceil(J Cp / 128); the tile
 * goes through LDS in two halves behind the product and one thread owns each (row, job).
 * (n + J Cp) D 4 bytes read per tile row / column, n J Cp 4 written. */
int mh_linprobe_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* labels, const int32_t* fold,
                     const int32_t* heldout, const float* rscale, int J, int C, int Cp, float* G, double* loss_part, mh_stream s);
/* The weight gradient at the look-ahead point and the FISTA update, in place:
 *   dW[j, c, d] = sum_i G[i, j Cp + c] y[i, d] + lambda_j Wz[j, c, d]          db[j, c] = sum_i G[i, j Cp + c]
 *   X' = Z - eta_j g,   Z' = X' + beta (X' - X)          over Wx, Wz f32 [J x Cp x D] and bx, bz f32 [J x Cp]
 * The sums over i are ONE f32 fmaf chain from 0 per element in ascending row order i = 0 .. n - 1 (v_mfma_f32_32x32x2_f32 contracting
 * over the rows; rows past n enter as fmaf(0, 0, acc) = acc); db is column D of the same product against a column of ones formed in
 * the load.  Then g = fmaf(lambda_j, Z, sum) (bias: g = sum), X' = fmaf(-eta_j, g, Z), Z' = fmaf(beta, X' - X, X'), each rounded
 * once.  One workgroup owns a 128 (key) x 128 (column) tile of [J Cp x (D + 1)] and walks all n rows: no split over n, every
 * element has exactly one owner.  Pad slots are skipped outright: they are neither read nor written.  lam, eta f32 [J];
 * 0 <= beta <= 1.  gmax_part f32 [ceil((D + 1) / 128) x J], STORED, or NULL: gmax_part[t, j] = max |g| over job j's weights in
 * column tile t (the bias belongs to the tile of column D); the maximum over t is job j's gradient in the max norm, NaN if any of
 * its elements is NaN.  Grid ceil(J Cp / 128) x ceil((D + 1) / 128).
 * n (J Cp + D) 4 bytes read per tile, 4 J C (D + 1) 4 bytes read and written. */
int mh_linprobe_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* bx, float* Wz, float* bz, const float* lam,
                     const float* eta, float beta, int J, int C, int Cp, float* gmax_part, mh_stream s);
/* Class probabilities of nq query rows q [nq x D] f32 contiguous under E jobs (weights W f32 [E x Cp x D], bias b f32 [E x Cp], the
 * layout above; pad slots are never read into P or written): P f32 [E x nq x C] (C columns, not Cp), STORED (nothing to zero):
 * P[e, i, c] = expf(v_c - lse) with v_c, m and lse formed by the SAME arithmetic sequence as in mh_linprobe_grad (one device function
 * serves both kernels): the k-ordered f32 fmaf chain of the tile product over the E Cp weight rows as keys, ONE f32 add of the bias,
 * then in class order in f32 m = max_c v_c, lse = m + logf(sum_c expf(v_c - m)).  So, with rscale = 1, P[e, i, c] equals
 * G[i, e Cp + c] bit for bit at every c != label_i of a training row.  A NaN query row gives a NaN probability row under every job:
 * nothing is filtered.  labels int64 [nq] (8-byte aligned) or NULL; nll_part f64 [ceil(nq / 128) x E] (8-byte aligned) or NULL, and it
 * requires labels: nll_part[t, e] = the sum of lse - v_label (f32) over the rows of row tile t whose label lies in [0, C), added in
 * row order in f64 as loss_part is (without a scale); rows with any other label add nothing; the sum over t is job e's log-loss over
 * the labelled rows.  Limits: those above with nq for n and E for J.  Deterministic, allocates nothing, never waits on the host.
 * Grid ceil(nq / 128) x ceil(E Cp / 128); one thread owns each (row, job); the half tile leaves LDS job by job, 64 C consecutive floats.
 * (nq + E Cp) D 4 bytes read per tile row / column, E nq C 4 written. */
int mh_linprobe_proba(const float* q, int64_t nq, int D, const float* W, const float* b, int E, int C, int Cp, const int64_t* labels,
                      float* P, double* nll_part, mh_stream s);

/* ---------------------------------------------------------------- survival linear probe of frozen embeddings (csrc/survprobe.hip;
 * mirror_amd/survprobe.py; the reference's train_survival.py --linear_probe: one linear layer of num_bins hazard logits under
 * NLLSurvLoss, losses/nll_surv.py:17-94, scored by the risk of train_survival.py:1431-1433, with the frozen encoder taken out of the
 * loop).  J independent L2-regularised hazard regressions over the SAME prepared rows y [n x D] f32 contiguous; per job j, with
 * v = W y_i + b in R^M, bin T_i and event indicator e_i,
 *   nll_i     = sum_{t < T_i} softplus(v_t) + softplus(v_T) - e_i v_T                (no term for t > T_i)
 *   F_j(W, b) = r_j sum_{i in train_j} w_i nll_i + (lambda_j / 2) |W|^2,   w_i = 1 if e_i = 1 else w_cens     (the bias unpenalised)
 *   train_j   = { i : T_i in [0, M), e_i in {0, 1}, fold_i >= 0, fold_i != heldout_j }
 * which is NLLSurvLoss(alpha = 1 - w_cens, reduction "mean") without its clamp of the hazards to [eps, 1 - eps]: the two agree
 * wherever every |v_t| <= log((1 - eps) / eps) (16.1 at eps = 1e-7).  One FISTA iteration is mh_survprobe_grad followed by
 * mh_linprobe_step with C = M, Cp = Mp.  Layout as mh_linprobe_*: Mp = the next power of two >= M, weights f32 [J x Mp x D], bias f32
 * [J x Mp]; neither entry point reads what a pad slot t >= M holds.  Both are deterministic (fixed summation order, no float atomics),
 * allocate nothing and never wait on the host.  Shared limits: 2 <= M <= 64, 1 <= D <= 4096, 1 <= n <= 2^20, J Mp <= 2^20.
 *
 * G f32 [n x J Mp] (n J Mp <= 2^28), STORED (nothing to zero): G[i, j Mp + t] = r_j w_i (sigmoid(v_t) - [t = T_i] e_i) for i in
 * train_j and t <= T_i; exactly 0 for t > T_i, for pad columns and for every other row.  v_t = dot(y_i, Wz[j, t]) + bz[j, t]: the
 * k-ordered f32 fmaf chain from 0 of the retrieval kernels and ONE f32 add; then e = expf(-|v|), sigmoid(v) = (v >= 0 ? 1 : e) /
 * (1 + e), softplus(v) = max(v, 0) + log1pf(e), nll_i added in bin order in f32.  bins int64 [n] (8-byte aligned), event uint8 [n],
 * fold int32 [n], heldout int32 [J], rscale f32 [J] (r_j), 0 <= w_cens <= 1.  loss_part f64 [ceil(n / 128) x J] (8-byte aligned) or
 * NULL: loss_part[t, j] = r_j sum of w_i nll_i (f32) over the training rows of row tile t, added in row order in f64; their sum over
 * t is the data term of F_j at (Wz, bz).  A NaN in a row makes the G rows and the loss of every job that trains on it NaN.  Grid
 * ceil(n / 128) x ceil(J Mp / 128); one thread owns each (row, job). */
int mh_survprobe_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* bins, const uint8_t* event,
                      const int32_t* fold, const int32_t* heldout, const float* rscale, float w_cens, int J, int M, int Mp, float* G,
                      double* loss_part, mh_stream s);
/* risk f32 [S x nq], STORED: risk[s, i] = -sum_{t < M} prod_{u <= t} sigmoid(-v_u), v = W[s] q_i + b[s], the product and the sum in
 * bin order in f32 (mh_surv_risk's definition with 1 - sigmoid(v) formed as sigmoid(-v); no clamp).  The S Mp weight rows of one
 * fold's jobs are the keys of the same tile product; the [nq x S Mp] logits are never stored.  1 <= nq <= 2^20, S Mp <= 2^20.
 * Grid ceil(nq / 128) x ceil(S Mp / 128). */
int mh_survprobe_risk(const float* q, int64_t nq, int D, const float* W, const float* b, int S, int M, int Mp, float* risk, mh_stream s);

/* ---------------------------------------------------------------- ridge Cox probe of frozen embeddings (csrc/coxprobe.hip, the step in
 * csrc/linprobe.hip; mirror_amd/coxprobe.py: the L2-penalised Cox proportional-hazards model on the frozen slide embedding that
 * slide-encoder benchmarks report, strength chosen over folds, scored by the c-index).  J independent regressions over the SAME prepared
 * rows y [n x D] f32 contiguous, SORTED by time, non-increasing (NaN times last); job j has one weight row w_j in R^D and no intercept
 * (the partial likelihood does not see one).  With scores v_i = dot(y_i, w_j), the definitions are those of the Cox block above
 * restricted to the job's training rows train_j = { i : event_i in {0, 1}, time_i not NaN, fold_i >= 0, fold_i != heldout_j }
 * (a_ij = [i in train_j], e_i = [event_i = 1]):
 *   m_j = max_{train_j} v,   w_k = a_kj exp(v_k - m_j) in f64
 *   S_i = sum_{t_k >= t_i} w_k     D_i = sum_k [t_k = t_i] a_kj e_k w_k     d_i = sum_k [t_k = t_i] a_kj e_k
 *   l_i = sum_{k < i} [t_k = t_i] a_kj e_k     f_i = 0 (MH_COX_BRESLOW), l_i / d_i (MH_COX_EFRON)     den_i = S_i - f_i D_i
 *   F_j(w) = r_j sum_i a_ij e_i (log den_i + m_j - v_i) + (lambda_j / 2) |w|^2
 *   g_k = dF_j / dv_k = r_j a_kj [ w_k sum_i q_i ([t_k > t_i] + [t_k = t_i](1 - e_k f_i)) - e_k ],   q_i = a_ij e_i / den_i
 * With r_j = 1 / |train_j| this has the minimiser of sksurv's CoxPHSurvivalAnalysis(alpha = lambda_j |train_j|).  One FISTA iteration
 * is mh_coxprobe_scores, mh_coxprobe_grad, mh_coxprobe_step.  All three are deterministic (fixed summation order, no float atomics),
 * allocate nothing and never wait on the host.
 *
 * V f32 [J x nq], job-major, STORED: V[j, i] = dot(q_i, W[j]), the k-ordered f32 fmaf chain from 0 of the retrieval kernels' exact-f32
 * 128 x 128 tile product with the J weight rows W f32 [J x D] as the keys (no pad slots).  1 <= D <= 4096, 1 <= nq <= 2^20,
 * 1 <= J <= 2^20, nq J <= 2^28.  Grid ceil(nq / 128) x ceil(J / 128); (nq + J) D 4 bytes read per tile row / column, nq J 4 written. */
int mh_coxprobe_scores(const float* q, int64_t nq, int D, const float* W, int J, float* V, mh_stream s);
/* G f32 [n x J] row-major (the layout mh_coxprobe_step reads), STORED: G[k, j] = g_k of job j; exactly 0 on every row outside train_j,
 * whatever V holds there; NaN on the rows of train_j when a score of train_j is NaN (no other job is touched).  loss f64 [J], STORED:
 * the data term r_j sum_i ..., 0 for a job without training events.  V f32 [J x n] as mh_coxprobe_scores leaves it.  Input contract:
 * the rows are in non-increasing time order and rows with a NaN time come last; time f64 [n], tie groups are runs of equal times (a
 * NaN time is a group of its own and trains nowhere); event uint8 [n] (0 censored, 1 event, anything else: the row trains nowhere);
 * fold int32 [n]; heldout int32 [J]; rscale f32 [J] (r_j); ties MH_COX_BRESLOW / MH_COX_EFRON.  On sorted rows S_i is a prefix sum
 * read at the last row of i's tie group and sum_{t_i <= t_k} q_i a suffix sum read at the first row of k's: one workgroup of 256
 * threads per job walks its column of V in three fixed-order block scans (thread t owns the contiguous rows [t c, (t + 1) c),
 * c = ceil(n / 256); the 256 chunk summaries are folded in thread order by one thread).  Every sum, exp and log is f64, only the
 * stores to G round to f32.  Limits: 1 <= n <= 65536, n J <= 2^24, max - min of a job's training scores <= 700 (the Cox block's
 * domain).  time, loss and workspace 8-byte aligned; workspace: mh_coxprobe_workspace_bytes(n, J) bytes (28 per score: w, two scan
 * rows and the event counts), nothing to zero; -1 outside the limits.  Grid J. */
int mh_coxprobe_grad(const float* V, int64_t n, int J, const double* time, const uint8_t* event, const int32_t* fold,
                     const int32_t* heldout, const float* rscale, int ties, float* G, double* loss, void* workspace, mh_stream s);
int64_t mh_coxprobe_workspace_bytes(int64_t n, int J);
/* mh_linprobe_step's kernel with one key per job (C = Cp = 1) and no bias column: g = G^T y + lambda_j Wz (ONE row-ordered f32 fmaf
 * chain from 0 per element, then fmaf(lambda_j, Wz, .)), X' = fmaf(-eta_j, g, Wz), Z' = fmaf(beta, X' - X, X'), stored over Wx / Wz
 * f32 [J x D] in place.  With a second, zero key per job, a mask of ones and fit_intercept = 0, mh_gsel_step at C = 2 forms the same
 * bits.  gmax_part f32 [ceil((D + 1) / 128) x J], STORED, or NULL: max |g| per column tile and job (0 from a tile that holds the
 * unused bias column alone).  1 <= D <= 4096, 1 <= n <= 65536, n J <= 2^24, 0 <= beta <= 1.  Grid ceil(J / 128) x ceil((D + 1) / 128). */
int mh_coxprobe_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* Wz, const float* lam, const float* eta,
                     float beta, int J, float* gmax_part, mh_stream s);

/* ---------------------------------------------------------------- cross-validated recursive gene elimination (csrc/geneselect.hip,
 * the step in csrc/linprobe.hip; mirror_amd/geneselect.py; the reference's tools/distill_rna_feature.py:121-132:
 * RFECV(LinearSVC(), step=0.05, cv=StratifiedKFold(5), scoring="accuracy") over the cohort's transcripts).  J = folds + 1 jobs over the
 * SAME prepared rows y [n x D] f32 contiguous, each C one-vs-rest squared-hinge machines (also for C = 2) with a per-job mask
 * uint8 [J x D] of the features still in play; per job j
 *   F_j(W, b) = r_j sum_{i in train_j} sum_{c < C} max(0, 1 - t_ic v_ic)^2 + (lambda_j / 2) |W o mask_j|^2      (the bias is not penalised)
 *   t_ic = +1 if label_i = c else -1,   v = W y_i + b,   train_j = { i : label_i in [0, C), fold_i >= 0, fold_i != heldout_j }
 * With lambda_j = 1 / (svm_c n_train_j) this has the minimiser of LinearSVC(C = svm_c) up to the bias: liblinear penalises it, and
 * fit_intercept = 0 (the bias pinned to 0) is the setting under which the two agree exactly.  One FISTA iteration is mh_gsel_grad then
 * mh_gsel_step; a round ends with mh_gsel_eliminate.  Layout as mh_linprobe_*: Cp = the next power of two >= C, weights f32
 * [J x Cp x D], bias f32 [J x Cp]; no entry point reads what a pad slot c >= C holds, and the weights of an eliminated feature are
 * exactly 0 and stay 0.  Every entry point is deterministic (fixed summation order, no float atomics), allocates nothing and never
 * waits on the host.  Shared limits: 2 <= C <= 64, 1 <= D <= 2^18, 1 <= n <= 2^20, J Cp <= 2^20, n J Cp <= 2^28.
 *
 * mu, rstd f32 [D] of x [n x D] f32 contiguous: the column sums as mh_colmean forms them (up to 128 strips of at least 64 rows, each
 * summed in row order in f64, the strips added in strip order), mu = sum / n rounded to f32 once; then a second pass in the same
 * order over the squares of the centred values (double)x - (double)mu: var = sum / n (population, ddof = 0), rstd = 1 / sqrt(var) rounded
 * to f32 once, and 0 where var is not positive (a constant column: mu is exact and var is exactly 0).  Four launches, grids
 * ceil(D / 256) x strips and ceil(D / 256).  workspace: mh_colstats_workspace_bytes(n, D) bytes (8 D per strip), 8-byte aligned, nothing
 * to zero.  2 n D 4 bytes read. */
int mh_colstats(const float* x, int64_t n, int D, float* mu, float* rstd, void* workspace, mh_stream s);
int64_t mh_colstats_workspace_bytes(int64_t n, int D);
/* y[i, d] = (x[i, d] - mu[d]) * rstd[d], a subtraction and a multiplication in f32; y may be x.  Grid ceil(D / 256) x min(n, 4096);
 * n D 4 bytes read and written. */
int mh_standardize(const float* x, const float* mu, const float* rstd, float* y, int64_t n, int D, mh_stream s);
/* out f32 [J x n], STORED: out[j, i] = the sum of y[i, d]^2 over the d with mask[j, d] != 0.  One wave per row: a lane adds the squares
 * of its active columns d = lane, lane + 64, .. in that order (fmaf from 0), the lanes are added by the fixed butterfly of
 * mh_center_l2norm.  J <= 2^19, n J <= 2^28.  Grid ceil(n / 4) x min(J, 1024); J n D 4 bytes read (a row's later jobs from cache). */
int mh_gsel_rowsq(const float* y, int64_t n, int D, const uint8_t* mask, int J, float* out, mh_stream s);
/* G f32 [n x J Cp], STORED (nothing to zero): G[i, j Cp + c] = -2 r_j t_ic max(0, 1 - t_ic v_ic) for i in train_j and c < C; exactly 0
 * for every other row, for pad columns and where the hinge is inactive.  v_ic = dot(y_i, Wz[j, c]) + bz[j, c], formed in two
 * launches.  First: the J Cp weight rows are the keys of the retrieval kernels' exact-f32 128 x 128 tile product
 * (v_mfma_f32_32x32x2_f32) with the contraction cut into Z = mh_gsel_slices(n, J Cp, D) slices of ks columns; slice z is ONE k-ordered
 * f32 fmaf chain from 0 over the columns [z ks, min(D, (z + 1) ks)) and is stored to workspace [Z x n x J Cp]; grid ceil(n / 128) x
 * ceil(J Cp / 128) x Z.  The slicing depends on the shape alone, never on the device: with T = ceil(n / 128) ceil(J Cp / 128) tiles,
 * z0 = min(ceil(D / 256), clamp(floor(768 / T), 1, 128)), ks = ceil(D / z0) rounded up to a multiple of 16, Z = ceil(D / ks)
 * (768 = 256 CUs x 3 resident workgroups of 35 KB of LDS; a slice is at least 16 stages of the product; Z = 1 for D <= 256).
 * Second: one thread per (row, job) adds the slices in slice order from slice 0 (f32), then ONE f32 add of the bias; m = 1 - v for the
 * row's class and 1 + v for the others, exact roundings of 1 - t v; the hinge h = m where m > 0 or m is NaN, else 0;
 * G = -(2 r_j h) / +(2 r_j h), one rounding.  labels int64 [n] (8-byte aligned), fold int32 [n], heldout int32 [J], rscale f32 [J] (r_j).
 * loss_part f64 [ceil(n / 128) x J] (8-byte aligned) or NULL: loss_part[t, j] = r_j sum over the training rows of row tile t, added
 * in row order in f64, of sum_c h^2 (an f32 fmaf chain from 0 in class order); the sum over t is the data term of F_j at (Wz, bz).
 * pred int32 [J x n] or NULL, STORED for EVERY row, in train or not: the class of the largest v_c under mh_fewshot_predict's rule (a
 * NaN is not eligible, equal values go to the smaller class, -1 when none is eligible).  A NaN in a row makes pred -1 and the G rows
 * and the loss NaN for exactly the jobs that train on it.  workspace: mh_gsel_grad_workspace_bytes(n, J, Cp, D) bytes, 4-byte aligned,
 * nothing to zero.  Second grid ceil(n / 128) x ceil(J / 16).
 * Z (n + J Cp) ks 4 bytes read per tile row / column, Z n J Cp 4 written and read back, n J Cp 4 written. */
int mh_gsel_grad(const float* y, int64_t n, int D, const float* Wz, const float* bz, const int64_t* labels, const int32_t* fold,
                 const int32_t* heldout, const float* rscale, int J, int C, int Cp, float* G, double* loss_part, int32_t* pred,
                 void* workspace, mh_stream s);
int64_t mh_gsel_grad_workspace_bytes(int64_t n, int J, int Cp, int D);
/* Z above for nk = J Cp keys; 0 outside the limits.  No stream, nothing launched. */
int mh_gsel_slices(int64_t n, int nk, int D);
/* mh_linprobe_step (the same kernel, the mask a template parameter: with a mask of ones and fit_intercept = 1 the two agree bit for
 * bit) with mask uint8 [J x D], shared by a job's classes, and fit_intercept in {0, 1}.  A (job, column) with mask = 0 is neither read
 * for the update nor written (Wx, Wz keep what they hold) and takes no part in gmax_part; with fit_intercept = 0 the same holds for bx /
 * bz and the bias gradient.  The contraction over the rows still walks every column tile: the active columns are not compacted.
 * D up to 2^18.  gmax_part f32 [ceil((D + 1) / 128) x J], STORED, or NULL.  Grid ceil(J Cp / 128) x ceil((D + 1) / 128).
 * n (J Cp + D) 4 bytes read per tile, 4 J C (D + 1) 4 bytes read and written at the most, J D mask bytes read. */
int mh_gsel_step(const float* y, int64_t n, int D, const float* G, float* Wx, float* bx, float* Wz, float* bz, const float* lam,
                 const float* eta, float beta, const uint8_t* mask, int fit_intercept, int J, int C, int Cp, float* gmax_part,
                 mh_stream s);
/* Drop the k least important active features of every job.  imp[j, d] = the f32 fmaf chain from 0 of Wx[j, c, d]^2 in class order
 * c < C, over the d with mask[j, d] != 0.  The k active features with the smallest key (bits of imp as uint32, then d) are removed:
 * equal importances go by the smaller index first, +inf sorts above every number and a NaN above +inf.  For a removed feature
 * mask[j, d] = 0, elim_round[j, d] = round (int32 [J x D]; the caller starts it at -1; round >= 0) and Wx, Wz[j, c < C, d] = 0; nothing
 * else is written.  k = 0 removes nothing; k >= the job's active count removes every active feature.  importance f32 [J x D] or NULL,
 * STORED: imp as formed, 0 for inactive features (the state BEFORE the removal).  Integer decisions only: one workgroup of 1024
 * threads per job finds the k-th smallest key by a radix select over the key bits (four passes of 8 bits, LDS histograms with integer
 * atomics) and then walks the features in index order, breaking the tie at the threshold by prefix counts (ballots, wave counts in
 * LDS); no sort, no workspace.  Grid J; 6 J C D 4 bytes read at the most (imp is formed again in every pass), J D 9 written at the most. */
int mh_gsel_eliminate(float* Wx, float* Wz, uint8_t* mask, int32_t* elim_round, int J, int C, int Cp, int D, int k, int round,
                      float* importance, mh_stream s);

#ifdef __cplusplus
}
#endif
#endif
