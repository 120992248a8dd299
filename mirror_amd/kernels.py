"""Tensor-level launchers for the C-ABI kernels (no autograd here; see functional.py).

Every function takes HIP tensors, checks shapes on the host (a faulting kernel can take the whole
node down) and launches on torch's current stream.  There is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
from typing import Optional


import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, MH_BF16, MH_F32, GemmDesc, MirrorHipError

_DT = {torch.float32: MH_F32, torch.bfloat16: MH_BF16}


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise MirrorHipError(f"unsupported dtype {t.dtype} (f32 / bf16 only)") from None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """hipStream_t of torch's current stream.  `torch.cuda.current_stream()` builds a Stream object (~9 us: ~4 ms of host
    time per step over ~450 launches); the raw accessor is ~0.3 us."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise MirrorHipError("mirror_amd kernels need HIP device tensors: there is no CPU fallback path")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _contig(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_contiguous():
        raise MirrorHipError(f"{name} must be contiguous, got strides {t.stride()} for shape {tuple(t.shape)}")
    return t


# ----------------------------------------------------------------------------- GEMM
def _mat(t: torch.Tensor):
    """[.., R, C] view (<= 2 batch dims) -> (t4, rowmajor, ld, s1, s2)."""
    if t.dim() < 2 or t.dim() > 4:
        raise MirrorHipError(f"gemm operand must have 2..4 dims, got {tuple(t.shape)}")
    while t.dim() < 4:
        t = t.unsqueeze(0)
    b1, b2, r, c = t.shape
    st = t.stride()
    if st[3] == 1 or c == 1:
        rowmajor, ld = True, (st[2] if r > 1 else max(c, 1))
    elif st[2] == 1 or r == 1:
        rowmajor, ld = False, (st[3] if c > 1 else max(r, 1))
    else:
        raise MirrorHipError(f"gemm operand needs a unit stride in one of its last two dims: {st}")
    return t, rowmajor, ld, (st[0] if b1 > 1 else 0), (st[1] if b2 > 1 else 0)


def _launch_gemm(d: GemmDesc) -> None:
    """mh_gemm on the current stream, through the profiler when one is installed."""
    prof = gemm_profiler
    if prof is None:
        _lib.call("mh_gemm", C.byref(d), stream=_stream())
    else:
        prof.launch(d, lambda: _lib.call("mh_gemm", C.byref(d), stream=_stream()))


def gemm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, *, alpha: float = 1.0,
         diag: float = 0.0, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, accumulate: bool = False,
         split_k: int = 1, mma: int = MH_F32, out_dtype: Optional[torch.dtype] = None,
         R: Optional[torch.Tensor] = None, rcoef: float = 0.0, c2: Optional[torch.Tensor] = None,
         kseg: Optional[tuple] = None, softmax: bool = False,
         softmax_bwd_of: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[..] (+)= act(alpha * a @ b + diag*I + bias + rcoef*R) with a [..,M,K], b [..,K,N] given as (possibly
    transposed / strided / broadcast) views; <= 2 leading batch dims.  c2: optional bf16 tensor shaped and strided like `out`
    that receives a copy of the final result (192 x 384 tile kernel only, see gemm_tile_ok).  kseg = (S, a_stride, b_stride):
    the product becomes sum_s a_s @ b_s over S operand pairs that start a_stride / b_stride elements apart (gemm_ksum).
    softmax=True: out = softmax(alpha * a @ b, dim=-1) as bf16, the rows normalised in the epilogue (gemm_softmax_ok shapes);
    softmax_bwd_of=P (bf16 probabilities, shaped and strided like out): out = P * (dP - sum(P * dP, -1)) with dP = alpha * a @ b."""
    _chk(a, b, out, bias)
    nd = max(a.dim(), b.dim())
    a4, a_rm, lda, sa1, sa2 = _mat(a)
    b4, b_rm, ldb, sb1, sb2 = _mat(b)
    M, K = a4.shape[2], a4.shape[3]
    K2, N = b4.shape[2], b4.shape[3]
    if K != K2:
        raise MirrorHipError(f"gemm: inner dims differ: {tuple(a.shape)} @ {tuple(b.shape)}")
    B1 = max(a4.shape[0], b4.shape[0])
    B2 = max(a4.shape[1], b4.shape[1])
    for t4 in (a4, b4):
        if t4.shape[0] not in (1, B1) or t4.shape[1] not in (1, B2):
            raise MirrorHipError(f"gemm: batch dims do not broadcast: {tuple(a.shape)} @ {tuple(b.shape)}")
    if a4.dtype != b4.dtype and mma == MH_F32:
        raise MirrorHipError(f"gemm: f32 MMA needs f32 operands, got {a4.dtype} x {b4.dtype}")
    if out is None:
        if accumulate:
            raise MirrorHipError("gemm: accumulate needs an explicit output")
        out = torch.empty((B1, B2, M, N), device=a.device, dtype=out_dtype or a.dtype)
        o4 = out
        out = out.reshape(out.shape[4 - nd:])
    else:
        o4 = out
        while o4.dim() < 4:
            o4 = o4.unsqueeze(0)
        if tuple(o4.shape) != (B1, B2, M, N):
            raise MirrorHipError(f"gemm: output shape {tuple(out.shape)} != {(B1, B2, M, N)}")
    so = o4.stride()
    if not (so[3] == 1 or N == 1):
        raise MirrorHipError("gemm: output must have unit stride in its last dim")
    if mma == MH_F32 and (a4.dtype != torch.float32 or b4.dtype != torch.float32 or o4.dtype != torch.float32):
        raise MirrorHipError("gemm: f32 MMA needs f32 operands and output")
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous():
            raise MirrorHipError("gemm: bias must be contiguous f32 [N]")
    d = GemmDesc()
    d.A, d.B, d.C, d.bias = a4.data_ptr(), b4.data_ptr(), o4.data_ptr(), _p(bias)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, (so[2] if M > 1 else max(N, 1))
    d.a_kc, d.b_kc = int(a_rm), int(not b_rm)
    d.dtA, d.dtB, d.dtC, d.mma = dt(a4), dt(b4), dt(o4), mma
    d.batch1, d.batch2 = B1, B2
    d.sA1, d.sA2, d.sB1, d.sB2 = sa1, sa2, sb1, sb2
    d.sC1, d.sC2 = (so[0] if B1 > 1 else 0), (so[1] if B2 > 1 else 0)
    d.alpha, d.diag, d.act, d.accumulate, d.split_k = alpha, diag, act, int(accumulate), max(1, int(split_k))
    if R is not None:
        _chk(R)
        tile = gemm_tile_ok(M, N, K, a4.dtype, b4.dtype) and bias is None and act == ACT_NONE and d.split_k == 1
        if R.numel() != o4.numel() or tuple(R.stride()) != tuple(out.stride()) or not (
                R.dtype == o4.dtype or (tile and R.dtype in (torch.bfloat16, torch.float32))):
            raise MirrorHipError("gemm: R must have the output's dtype (or bf16 / f32 on the 192 x 384 tile kernel), shape and strides")
        d.R, d.rcoef = R.data_ptr(), rcoef
        d.r_bf16 = 0 if R.dtype == o4.dtype else (1 if R.dtype == torch.bfloat16 else 2)
    if c2 is not None:
        _chk(c2)
        if c2.dtype != torch.bfloat16 or c2.numel() != o4.numel() or tuple(c2.stride()) != tuple(out.stride()):
            raise MirrorHipError("gemm: c2 must be a bf16 tensor with the output's shape and strides")
        d.C2 = c2.data_ptr()
    if softmax:
        if not (gemm_softmax_ok(M, N, K, a4.dtype, b4.dtype) and o4.dtype == torch.bfloat16 and bias is None and act == ACT_NONE
                and d.split_k == 1 and not accumulate and R is None and c2 is None and diag == 0.0):
            raise MirrorHipError("gemm: softmax=True needs bf16 operands and output, M % 192 == 0, N == 384, K % 8 == 0 and a plain product")
        d.row_softmax = 1
    if softmax_bwd_of is not None:
        P_ = softmax_bwd_of
        _chk(P_)
        if not (gemm_softmax_ok(M, N, K, a4.dtype, b4.dtype) and o4.dtype == torch.bfloat16 and P_.dtype == torch.bfloat16 and bias is None
                and act == ACT_NONE and d.split_k == 1 and not accumulate and R is None and c2 is None and diag == 0.0 and not softmax
                and P_.numel() == o4.numel() and tuple(P_.stride()) == tuple(out.stride())):
            raise MirrorHipError("gemm: softmax_bwd_of needs bf16 operands / output / probabilities (same layout as out), M % 192 == 0, N == 384")
        d.row_softmax, d.R = 2, P_.data_ptr()
    if kseg is not None and int(kseg[0]) > 1:
        if not (gemm_tile_ok(M, N, K, a4.dtype, b4.dtype) and bias is None and act == ACT_NONE and d.split_k == 1):
            raise MirrorHipError("gemm: a sum over operand pairs (kseg) needs the 192 x 384 tile kernel (see gemm_tile_ok)")
        d.k_segments, d.sA_seg, d.sB_seg = int(kseg[0]), int(kseg[1]), int(kseg[2])
    # reductions into one f32 C (split-K / a batch that broadcasts into C) on the large-tile kernel: give it room for plain
    # partial tiles + a fold pass (f32 atomics of a 64-way split cost more than the K loop).  `ws` stays alive until the call
    # is enqueued; the caching allocator keeps the block valid for stream-ordered use.
    wsb = int(_lib.load().mh_gemm_workspace_bytes(C.byref(d))) if (accumulate and SPLITK_PARTIALS == "bf16") else 0
    if 0 < wsb <= (1 << 29):
        ws = torch.empty((wsb // 4,), device=a.device, dtype=torch.float32)
        d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()
    d.shared_chip = int(shared_chip)
    _launch_gemm(d)
    return out


# set (by functional.NystromCoreFn, through chip_shared) while the half-chip pinv chain runs on its side stream: launches issued
# meanwhile must not use the persistent GEMM kernel (mh_gemm_desc.shared_chip)
shared_chip = False


@contextlib.contextmanager
def chip_shared(on: bool = True):
    """shared_chip = on inside the block; on every way out of it (an exception included) the value it had before."""
    global shared_chip
    prev, shared_chip = shared_chip, on
    try:
        yield
    finally:
        shared_chip = prev


EPI_DROPADD, EPI_MASKPOS, EPI_SQERR = 1, 2, 3
_EPI_ON = True       # the fused projection epilogues (mh_gemm_epi); test hook: False = composed projection + elementwise passes


def linear_fused_ok(x: torch.Tensor, w: torch.Tensor, window: Optional[tuple] = None) -> bool:
    """Shapes mh_gemm's fused epilogues take: bf16 activations x [B, T, K] (contiguous; optionally the row window
    [r0, r0 + R) of every batch), bf16 weight [N, K] contiguous, N % 256 == 0, K % 64 == 0, more than 256 rows in all."""
    if not (_EPI_ON and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 3 and x.is_contiguous() and w.dim() == 2
            and w.is_contiguous() and x.is_cuda):
        return False
    Bn, T, Kd = x.shape
    R = T if window is None else window[1]
    return (w.shape[1] == Kd and Kd % 64 == 0 and w.shape[0] % 256 == 0 and Bn * R > 256 and (window is None or R >= 256 or Bn == 1)
            and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def linear_fused_tail(rows: int) -> int:
    """Flat rows that a fused launch leaves to the caller: a few rows past whole 256-row tiles (B x 4097 = 256 tiles + 16 rows) would
    cost every launch a third round of workgroups on 256 CUs for two almost empty tiles; the caller runs them through the composed
    ops (a [16, K] product and a 16-row elementwise launch)."""
    rem = rows % 256
    return rem if (rows > 512 and 0 < rem <= 64) else 0


def linear_fused(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epi: "_lib.GemmEpi",
                 window: Optional[tuple] = None, m_rows: Optional[int] = None) -> torch.Tensor:
    """out [B * R, N] (flat rows, contiguous) = epilogue(x[:, r0:r0 + R] @ w^T + bias) on the 256 x 256-tile kernel with one of the
    fused epilogues of include/mirror_hip.h (mh_gemm_epi).  window = (r0, R) or None (all T rows).  The row windows of all batches
    are ONE flat problem (mh_gemm_desc.a_rows_per_batch): no ragged tile per slide, no tail launch."""
    _chk(x, w, out, bias)
    Bn, T, Kd = x.shape
    r0, R = (0, T) if window is None else window
    N = w.shape[0]
    if not out.is_contiguous() or out.numel() != Bn * R * N:
        raise MirrorHipError("linear_fused: out must be contiguous [B * R, N]")
    d = GemmDesc()
    d.A, d.B, d.C, d.bias = x.data_ptr() + r0 * Kd * 2, w.data_ptr(), out.data_ptr(), _p(bias)
    d.M, d.N, d.K = (Bn * R if m_rows is None else int(m_rows)), N, Kd      # m_rows: only the first m_rows flat rows (see linear_fused_tail)
    d.lda, d.ldb, d.ldc = Kd, Kd, N
    d.a_kc, d.b_kc = 1, 1
    d.dtA, d.dtB, d.dtC, d.mma = MH_BF16, MH_BF16, dt(out), MH_BF16
    d.batch1 = d.batch2 = 1
    d.alpha, d.split_k = 1.0, 1
    if R != T and Bn > 1:
        d.a_rows_per_batch, d.a_row_skip = R, T - R
    d.epi = C.pointer(epi)
    _launch_gemm(d)
    return out


def _weight_view_ld(b2: torch.Tensor, who: str) -> tuple:
    """(ldb, b_kc) of a 2-D weight view [K, N]."""
    if b2.stride(0) == 1:            # W^T of a row-major [N, K] weight: contraction index contiguous
        return b2.stride(1), 1
    if b2.stride(1) == 1:            # row-major [K, N]
        return b2.stride(0), 0
    raise MirrorHipError(f"{who}: the weight view must have a unit stride")


def gemm_rows_window(a3: torch.Tensor, b2: torch.Tensor, out3: torch.Tensor, r0: int, R: int, m_rows: Optional[int] = None,
                     a_r0: Optional[int] = None) -> None:
    """out3[:, r0:r0 + R] = a3[:, a_r0:a_r0 + R] @ b2 as ONE flat problem over the B * R real rows of buffers that hold T >= R rows per batch
    (mh_gemm_desc.a_rows_per_batch / c_rows_per_batch): [3P] NystromAttention's front-padded sequence — the pad rows are never multiplied.
    a3 [B, Ta, K] bf16 (rows K-contiguous; a_r0 defaults to r0, Ta == R: a plain contiguous operand), b2 a 2-D weight view [K, N] (W^T of
    an [N, K] row-major weight, or a row-major [K, N]), out3 [B, T, N] bf16 (may be a column slice of a wider buffer).  m_rows: only the
    first m_rows flat rows (whole 256-row tiles)."""
    _chk(a3, b2, out3)
    Bn, Ta, Kd = a3.shape
    T = out3.shape[1]
    N = b2.shape[1]
    bf = torch.bfloat16
    a_r0 = r0 if a_r0 is None else a_r0
    if not (a3.dtype == b2.dtype == out3.dtype == bf and a3.stride(2) == 1 and out3.stride(2) == 1 and a3.stride(0) == Ta * a3.stride(1)
            and out3.stride(0) == T * out3.stride(1) and tuple(out3.shape) == (Bn, T, N) and b2.shape[0] == Kd and 0 <= r0 and r0 + R <= T
            and 0 <= a_r0 and a_r0 + R <= Ta):
        raise MirrorHipError("gemm_rows_window: bad operands")
    d = GemmDesc()
    d.A, d.B, d.C, d.bias = a3.data_ptr() + a_r0 * a3.stride(1) * 2, b2.data_ptr(), out3.data_ptr() + r0 * out3.stride(1) * 2, None
    d.M, d.N, d.K = (Bn * R if m_rows is None else int(m_rows)), N, Kd
    d.lda, d.ldc = a3.stride(1), out3.stride(1)
    d.ldb, d.b_kc = _weight_view_ld(b2, "gemm_rows_window")
    d.a_kc = 1
    d.dtA, d.dtB, d.dtC, d.mma = MH_BF16, MH_BF16, MH_BF16, MH_BF16
    d.batch1 = d.batch2 = 1
    d.alpha, d.split_k = 1.0, 1
    if Bn > 1:
        if R != Ta:
            d.a_rows_per_batch, d.a_row_skip = R, Ta - R
        if R != T:
            d.c_rows_per_batch, d.c_row_skip = R, T - R
    d.shared_chip = 1 if shared_chip else 0
    _launch_gemm(d)


def gemm_rows_ext_ok(Bn: int, T: int, r0: int, R: int, extra: int, Kd: int, N: int, a2: torch.Tensor, out2: torch.Tensor) -> bool:
    """shapes for which gemm_rows_ext runs on the direct-to-LDS 256 x 256 kernels."""
    bf = torch.bfloat16
    M = Bn * R + extra
    return (a2.dim() == 2 and out2.dim() == 2 and a2.dtype == bf and out2.dtype == bf and a2.is_cuda and R >= 256 and M > 512 and 0 <= extra < R
            and r0 + R == T and M % 256 <= extra
            and N % 256 == 0 and Kd % 64 == 0 and a2.stride(1) == 1 and out2.stride(1) == 1 and a2.stride(0) % 8 == 0 and out2.stride(0) % 8 == 0
            and a2.data_ptr() % 16 == 0 and out2.data_ptr() % 16 == 0 and a2.shape[0] == Bn * T + extra and out2.shape[0] == Bn * T + extra)


def gemm_rows_ext(a2: torch.Tensor, b2: torch.Tensor, out2: torch.Tensor, Bn: int, T: int, r0: int, R: int, extra: int) -> int:
    """The row-window product of gemm_rows_window over buffers that hold `extra` more rows behind the Bn batches of T rows (the landmark
    rows of a Nystrom layer: a2 [Bn * T + extra, K], out2 [Bn * T + extra, N], 2-D views with unit column stride): ONE flat problem over
    the Bn * R real rows (r0 + R == T: the window ends with the batch) followed by the extra rows, M = Bn * R + extra.  The kernels'
    row remap r -> r + min(r / R, Bn - 1) * (T - R) (mh_gemm_desc.window_batches) lands the extra rows right behind the last batch.
    Only whole 256-row tiles are computed; returns the number of flat rows left over at the end (< 256, all of them extra rows) for the
    caller to finish (a2[-tail:] @ b2 -> out2[-tail:])."""
    _chk(a2, b2, out2)
    Kd, N = a2.shape[1], b2.shape[1]
    if not gemm_rows_ext_ok(Bn, T, r0, R, extra, Kd, N, a2, out2) or b2.shape[0] != Kd or b2.dtype != torch.bfloat16:
        raise MirrorHipError("gemm_rows_ext: bad operands")
    M = Bn * R + extra
    tail = M % 256
    d = GemmDesc()
    d.A, d.B, d.C, d.bias = a2.data_ptr() + r0 * a2.stride(0) * 2, b2.data_ptr(), out2.data_ptr() + r0 * out2.stride(0) * 2, None
    d.M, d.N, d.K = M - tail, N, Kd
    d.lda, d.ldc = a2.stride(0), out2.stride(0)
    d.ldb, d.b_kc = _weight_view_ld(b2, "gemm_rows_ext")
    d.a_kc = 1
    d.dtA, d.dtB, d.dtC, d.mma = MH_BF16, MH_BF16, MH_BF16, MH_BF16
    d.batch1 = d.batch2 = 1
    d.alpha, d.split_k = 1.0, 1
    if R != T:
        d.a_rows_per_batch, d.a_row_skip = R, T - R
        d.c_rows_per_batch, d.c_row_skip = R, T - R
        d.window_batches = Bn          # the extra rows follow the last batch's window without a gap
    d.shared_chip = 1 if shared_chip else 0
    _launch_gemm(d)
    return tail


def gemm_rows_window_ok(a3: torch.Tensor, out3: torch.Tensor, r0: int, R: int, N: int) -> bool:
    """shapes for which gemm_rows_window runs (the direct-to-LDS 256 x 256 kernels)."""
    bf = torch.bfloat16
    return (a3.dim() == 3 and out3.dim() == 3 and a3.dtype == bf and out3.dtype == bf and a3.is_cuda and R >= 256 and a3.shape[0] * R > 512
            and N % 256 == 0 and a3.shape[2] % 64 == 0 and a3.stride(2) == 1 and out3.stride(2) == 1 and a3.stride(1) % 8 == 0
            and out3.stride(1) % 8 == 0 and a3.data_ptr() % 16 == 0 and out3.data_ptr() % 16 == 0
            and a3.stride(0) == a3.shape[1] * a3.stride(1) and out3.stride(0) == out3.shape[1] * out3.stride(1))


def epi_dropadd(resid: torch.Tensor, p: float, seed: int, offset: int, dev_base) -> "_lib.GemmEpi":
    _chk(resid)
    e = _lib.GemmEpi()
    e.kind, e.resid, e.p, e.seed, e.offset, e.dev_base = EPI_DROPADD, resid.data_ptr(), float(p), int(seed), int(offset), _p(dev_base)
    return e


def epi_maskpos(mask: torch.Tensor, token: torch.Tensor, pos: torch.Tensor, rows_per_batch: int, first: int) -> "_lib.GemmEpi":
    _chk(mask, token, pos)
    e = _lib.GemmEpi()
    e.kind, e.mask, e.token, e.pos, e.rows_per_batch, e.first = EPI_MASKPOS, mask.data_ptr(), token.data_ptr(), pos.data_ptr(), int(rows_per_batch), int(first)
    return e


def epi_sqerr(mask: torch.Tensor, tgt: torch.Tensor, tgt_bs: int, sq: torch.Tensor, rows_per_batch: int) -> "_lib.GemmEpi":
    _chk(mask, tgt, sq)
    e = _lib.GemmEpi()
    e.kind, e.mask, e.tgt, e.tgt_bs, e.sq, e.rows_per_batch = EPI_SQERR, mask.data_ptr(), tgt.data_ptr(), int(tgt_bs), sq.data_ptr(), int(rows_per_batch)
    return e


def gemm_softmax_ok(M: int, N: int, Kd: int, dta=torch.bfloat16, dtb=torch.bfloat16) -> bool:
    """Shapes whose row softmax the 192 x 384 tile kernel computes in its epilogue (a whole row of length N = 384 in one tile)."""
    return M % 192 == 0 and N == 384 and Kd % 8 == 0 and dta == torch.bfloat16 and dtb == torch.bfloat16


def gemm_ksum(a_stack: torch.Tensor, b_stack: torch.Tensor, out: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """sum_s a_stack[s] @ b_stack[s] in ONE launch and one accumulator (192 x 384 tile kernel): the operand pairs sit a constant
    stride apart (the leading dim of the two stacks; a transpose of the trailing dims or a strided slice of a longer stack
    is fine), so the K loop simply walks from one pair to the next and the f32 sum never takes a read-modify-write through HBM."""
    if a_stack.shape[0] != b_stack.shape[0] or a_stack.shape[0] < 1:
        raise MirrorHipError("gemm_ksum: the stacks need the same, non-zero leading length")
    return gemm(a_stack[0], b_stack[0], out, kseg=(a_stack.shape[0], a_stack.stride(0), b_stack.stride(0)), **kw)


def gemm_tile_ok(M: int, N: int, Kd: int, dta=torch.bfloat16, dtb=torch.bfloat16) -> bool:
    """Shapes the 192 x 384 tile kernel (csrc/gemm_tile.hip) takes: the batched 384-cubed products of the template's pinv."""
    return M % 192 == 0 and N % 384 == 0 and Kd % 64 == 0 and dta == torch.bfloat16 and dtb == torch.bfloat16


# Precision policy of the split-K weight-gradient reductions.  "bf16": every K-slice's f32 accumulator is rounded to bf16 on
# its way to the workspace and the fold sums in f32 (half the partial traffic: -0.77 % step time); the
# extra error of an element is bounded by parts * 2^-9 * max |partial| — relative to the largest partial, not to the final sum
# (tests/test_kernels_gpu.py::test_split_k_bf16_partials_error_bound_under_cancellation).  "f32": no workspace, f32 atomics into C
# (exact f32 partial sums, order not reproducible).  The bf16 form is the bf16 training policy's default; MIRROR_SPLITK_PARTIALS=f32
# selects the other for a run, and the fp32 parity policy never splits into bf16 (mh_gemm_workspace_bytes is 0 for f32 operands).
import os as _os
SPLITK_PARTIALS = _os.environ.get("MIRROR_SPLITK_PARTIALS", "bf16")
if SPLITK_PARTIALS not in ("bf16", "f32"):
    raise MirrorHipError(f"MIRROR_SPLITK_PARTIALS={SPLITK_PARTIALS!r}: 'bf16' or 'f32'")


class GemmProfiler:
    """Times GEMM (and named fused-kernel) launches with HIP events on the launch stream (bench.py's roofline leg).  A GEMM launch is
    named by the LIBRARY after the fact (mh_gemm_variant_name: the template instance mh_gemm dispatched to, as rocprofv3 reports
    it), so nothing here restates the dispatch rules.  only=<variant>: summary() keeps just that instance."""

    def __init__(self, only: Optional[str] = None):
        self.only = only
        self.records = []   # (variant, flops, start_event, end_event)

    def launch(self, d: GemmDesc, fn) -> None:
        if torch.cuda.is_current_stream_capturing():
            fn()                 # events recorded inside a capture (the RNA branch graph) are not timing events
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()          # recorded on the stream the kernel is launched on (torch's current stream)
        fn()
        e1.record()
        name = (_lib.load().mh_gemm_variant_name() or b"").decode()
        if d.epi and not name.endswith(f",epi{d.epi.contents.kind}>"):
            name = name[:-1] + f",epi{d.epi.contents.kind}>"
        self.records.append((name, 2.0 * d.M * d.N * d.K * d.batch1 * d.batch2, e0, e1))

    def launch_named(self, v: str, flops: float, fn) -> None:
        if (self.only is not None and v != self.only) or torch.cuda.is_current_stream_capturing():
            fn()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.records.append((v, flops, e0, e1))

    def summary(self):
        """variant -> dict(launches, total_ms, flops); call after a device synchronise."""
        out = {}
        for v, fl, e0, e1 in self.records:
            if self.only is not None and v != self.only:
                continue
            s = out.setdefault(v, {"launches": 0, "total_ms": 0.0, "flops": 0.0})
            s["launches"] += 1
            s["total_ms"] += e0.elapsed_time(e1)
            s["flops"] += fl
        return out


gemm_profiler: Optional[GemmProfiler] = None


# ----------------------------------------------------------------------------- fp8 forward projections (config 5)
def quant_fp8(x: torch.Tensor):
    """Per-tensor e4m3 quantisation: (q uint8 like x, scale f32[1]) with x ~= q * scale."""
    _chk(x)
    _contig(x, "quant_fp8 input")
    if x.numel() % 4:
        raise MirrorHipError("quant_fp8: numel must be a multiple of 4")
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    scale = torch.empty((1,), device=x.device, dtype=torch.float32)
    scratch = torch.empty((1,), device=x.device, dtype=torch.int32)
    _lib.call("mh_quant_fp8", _p(x), x.numel(), _p(q), _p(scale), _p(scratch), dt(x), stream=_stream())
    return q, scale


def quant_fp8_delayed(x: torch.Tensor, ring: torch.Tensor, tick: torch.Tensor, margin: float = 1.25):
    """One-pass e4m3 quantisation with the previous step's scale (ring: int32[3] device state of this call site, tick: device f32
    step counter).  Returns (q, scale) like quant_fp8."""
    _chk(x, ring, tick)
    _contig(x, "quant_fp8_delayed input")
    if x.numel() % 4 or ring.numel() != 3 or ring.dtype != torch.int32 or tick.dtype != torch.float32:
        raise MirrorHipError("quant_fp8_delayed: bad operands")
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    scale = torch.empty((1,), device=x.device, dtype=torch.float32)
    _lib.call("mh_quant_fp8_delayed", _p(x), x.numel(), _p(q), _p(scale), _p(ring), _p(tick), float(margin), dt(x), stream=_stream())
    return q, scale


def gemm_fp8_ok(a: torch.Tensor, n_out: int) -> bool:
    """a [..., R, K] as e4m3 bytes: K % 64 == 0, N % 128 == 0, rows K-contiguous, <= one batch dim with 16-byte strides."""
    Kd = a.shape[-1]
    if Kd % 64 or n_out % 128 or a.stride(-1) != 1 or a.dim() not in (2, 3) or a.stride(-2) % 16:
        return False
    return a.dim() == 2 or a.stride(0) % 16 == 0


def gemm_fp8(aq: torch.Tensor, sa: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, out: torch.Tensor,
             bias: Optional[torch.Tensor] = None, act: int = ACT_NONE) -> torch.Tensor:
    """out[..., R, N] = act(sa * sw * aq @ wq^T + bias); aq uint8 [R, K] or [B, R, K] (a row window is fine), wq uint8 [N, K]
    contiguous, out f32 / bf16 with unit column stride (a row window of a larger buffer is fine)."""
    _chk(aq, wq, out, sa, sw, bias)
    N, Kd = wq.shape
    assert aq.dtype == torch.uint8 and wq.dtype == torch.uint8 and wq.is_contiguous() and aq.shape[-1] == Kd
    assert out.stride(-1) == 1 and out.shape[-1] == N and out.shape[:-1] == aq.shape[:-1]
    if aq.dim() == 3:
        batch, M, a_bs, c_bs = aq.shape[0], aq.shape[1], aq.stride(0), out.stride(0)
    else:
        batch, M, a_bs, c_bs = 1, aq.shape[0], 0, 0
    _lib.call("mh_gemm_fp8", _p(aq), aq.stride(-2), a_bs, _p(wq), Kd, _p(out), out.stride(-2), c_bs, batch, _p(sa), _p(sw), _p(bias),
              act, M, N, Kd, dt(out), stream=_stream())
    return out


# ----------------------------------------------------------------------------- skinny-M linears
def skinny_ok(x2d: torch.Tensor, w: torch.Tensor) -> bool:
    """bf16 or f32 x [M<=32, K] (row-strided ok; f32 is rounded to bf16 on load: no cast launch) against bf16 W [N, K] contiguous.
    K % 32 == 0 with 16-byte aligned rows runs on 16-byte fragments, anything else (10234 genes, a 1975-wide MLP) on the element-wise
    instance of the same kernel (skinny_vec_ok says which)."""
    return (x2d.dim() == 2 and w.dim() == 2 and x2d.dtype in (torch.bfloat16, torch.float32) and w.dtype == torch.bfloat16
            and 1 <= x2d.shape[0] <= 32 and x2d.shape[1] == w.shape[1] and w.shape[1] >= 1 and w.is_contiguous() and x2d.stride(1) == 1)


def skinny_vec_ok(x2d: torch.Tensor, w: torch.Tensor) -> bool:
    """The 16-byte-fragment instance of mh_skinny_fwd applies (what mh_skinny_fwd itself checks)."""
    return (skinny_ok(x2d, w) and w.shape[1] % 32 == 0 and x2d.stride(0) % 8 == 0 and x2d.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def skinny_fwd(x2d: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int, out_dtype, out: Optional[torch.Tensor] = None,
               addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out: optional [M, N] destination rows (any row stride that keeps rows 16-byte aligned, e.g. rows of a larger buffer);
    addend: optional f32 [M, N] summed in front of the activation (two data gradients of one x in two launches, no add)."""
    _chk(x2d, w, bias, out, addend)
    if addend is not None and (addend.dtype != torch.float32 or tuple(addend.shape) != (x2d.shape[0], w.shape[0]) or addend.stride(1) != 1):
        raise MirrorHipError("skinny_fwd: the addend is f32 [M, N] with unit inner stride")
    M, Kd = x2d.shape
    N = w.shape[0]
    y = torch.empty((M, N), device=x2d.device, dtype=out_dtype) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or x2d.stride(1) != 1 or w.stride(1) != 1:
        raise MirrorHipError("skinny_fwd: bad operands")
    _lib.call("mh_skinny_fwd", _p(x2d), x2d.stride(0), _p(w), w.stride(0), _p(bias), _p(addend), 0 if addend is None else addend.stride(0),
              _p(y), y.stride(0), M, N, Kd, act, dt(x2d), dt(y), stream=_stream())
    return y


def skinny_rows_ok(x2d: torch.Tensor, w: torch.Tensor, y2d: torch.Tensor) -> bool:
    """mh_skinny_fwd's limits for rows of larger buffers (x2d [M <= 32, K], w [N, K], y2d [M, N]; unit inner strides)."""
    ok_dt = (torch.bfloat16, torch.float32)
    return (x2d.dim() == 2 and w.dim() == 2 and y2d.dim() == 2 and 1 <= x2d.shape[0] <= 32 and x2d.shape[1] % 32 == 0
            and x2d.shape[1] == w.shape[1] and tuple(y2d.shape) == (x2d.shape[0], w.shape[0])
            and x2d.stride(1) == 1 and w.stride(1) == 1 and y2d.stride(1) == 1
            and x2d.stride(0) % 8 == 0 and w.stride(0) % 8 == 0 and y2d.stride(0) % 8 == 0
            and x2d.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and y2d.data_ptr() % 16 == 0
            and x2d.dtype in ok_dt and y2d.dtype in ok_dt and w.dtype == torch.bfloat16)


def skinny_wgrad(dy2d: torch.Tensor, x2d: torch.Tensor, dw: torch.Tensor, accumulate: bool, db: Optional[torch.Tensor] = None) -> None:
    """dW (+)= dy^T x; with `db` ([N] f32) also db += column sums of dy (the bias gradient) in the same launch."""
    _chk(dy2d, x2d, dw, db)
    assert db is None or (db.dtype == torch.float32 and db.numel() == dy2d.shape[1] and db.is_contiguous())
    M, N = dy2d.shape
    Kd = x2d.shape[1]
    ok_dt = (torch.bfloat16, torch.float32)
    if (dy2d.dtype not in ok_dt or x2d.dtype not in ok_dt or dw.dtype != torch.float32 or x2d.shape[0] != M
            or tuple(dw.shape) != (N, Kd) or dy2d.stride(1) != 1 or x2d.stride(1) != 1 or dw.stride(1) != 1):
        raise MirrorHipError("skinny_wgrad: bad operands")
    _lib.call("mh_skinny_wgrad", _p(dy2d), dy2d.stride(0), _p(x2d), x2d.stride(0), _p(dw), dw.stride(0), _p(db), M, N, Kd,
              int(accumulate), dt(dy2d), dt(x2d), stream=_stream())


SKINNY_MANY_MAX = 32


def skinny_wgrad_many(items) -> None:
    """items: list of (dy2d, x2d, dw, db or None) as skinny_wgrad takes them (always accumulating); ONE launch per 32 items."""
    for i0 in range(0, len(items), SKINNY_MANY_MAX):
        chunk = items[i0:i0 + SKINNY_MANY_MAX]
        arr = (_lib.SkinnyWgradItem * len(chunk))()
        for e, (dy2d, x2d, dw, db) in zip(arr, chunk):
            _chk(dy2d, x2d, dw, db)
            M, N = dy2d.shape
            Kd = x2d.shape[1]
            if (dy2d.dtype not in (torch.bfloat16, torch.float32) or x2d.dtype not in (torch.bfloat16, torch.float32) or dw.dtype != torch.float32 or x2d.shape[0] != M
                    or tuple(dw.shape) != (N, Kd) or dy2d.stride(1) != 1 or x2d.stride(1) != 1 or dw.stride(1) != 1
                    or (db is not None and (db.dtype != torch.float32 or db.numel() != N or not db.is_contiguous()))):
                raise MirrorHipError("skinny_wgrad_many: bad operands")
            e.dy, e.lddy, e.x, e.ldx, e.dw, e.lddw, e.db = dy2d.data_ptr(), dy2d.stride(0), x2d.data_ptr(), x2d.stride(0), dw.data_ptr(), dw.stride(0), _p(db)
            e.M, e.N, e.K, e.dt_dy, e.dt_x = M, N, Kd, dt(dy2d), dt(x2d)
        _lib.call("mh_skinny_wgrad_many", arr, len(chunk), stream=_stream())


def transpose_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, out)
    _contig(x, "transpose input")
    R, Cc = x.shape
    y = out if out is not None else torch.empty((Cc, R), device=x.device, dtype=torch.bfloat16)
    _lib.call("mh_transpose_bf16", _p(x), _p(y), R, Cc, stream=_stream())
    return y


def transpose_bf16_many(src: torch.Tensor, dst: torch.Tensor, table: torch.Tensor, n: int, max_r: int, max_c: int,
                        vec_ok: bool = False) -> None:
    """vec_ok: the caller checked that every table entry has R % 8 == C % 8 == 0 and offsets that are multiples of 8."""
    _chk(src, dst, table)
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() == 4 * n
    _lib.call("mh_transpose_bf16_many", _p(src), _p(dst), _p(table), n, max_r, max_c, int(vec_ok), stream=_stream())


# ----------------------------------------------------------------------------- row kernels
def layernorm_fwd(x, gamma, beta, y, mean, rstd, batches, rpb, D, x_bs, y_bs, eps):
    _chk(x, gamma, beta, y, mean, rstd)
    _lib.call("mh_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), batches, rpb, D, x_bs, y_bs,
              eps, dt(x), dt(y), stream=_stream())


def layernorm_fwd_dual(x, gamma, beta, y, y16, mean, rstd, batches, rpb, D, x_bs, y_bs, eps):
    """layernorm_fwd (f32 in, f32 out) that also writes the bf16 copy y16 (same row addressing as y)."""
    _chk(x, gamma, beta, y, y16, mean, rstd)
    if not (x.dtype == torch.float32 and y.dtype == torch.float32 and y16.dtype == torch.bfloat16):
        raise MirrorHipError("layernorm_fwd_dual: f32 input, f32 + bf16 outputs")
    _lib.call("mh_layernorm_fwd_dual", _p(x), _p(gamma), _p(beta), _p(y), _p(y16), _p(mean), _p(rstd), batches, rpb, D, x_bs, y_bs,
              eps, stream=_stream())


def layernorm_fwd_q8(x, gamma, beta, y, mean, rstd, batches, rpb, D, x_bs, y_bs, eps, q8, ring, tick, margin: float = 1.25):
    """layernorm_fwd (f32 in, bf16 out) that also writes the e4m3 copy q8 (uint8, y's row addressing) with the delayed scale of
    `ring` (int32[3] device state of the call site) / `tick`; returns the dequantisation factor (f32[1])."""
    _chk(x, gamma, beta, y, mean, rstd, q8, ring, tick)
    if not (x.dtype == torch.float32 and y.dtype == torch.bfloat16 and q8.dtype == torch.uint8 and ring.numel() == 3
            and ring.dtype == torch.int32 and tick.dtype == torch.float32):
        raise MirrorHipError("layernorm_fwd_q8: f32 input, bf16 + uint8 outputs, int32[3] ring, f32 tick")
    scale = torch.empty((1,), device=x.device, dtype=torch.float32)
    _lib.call("mh_layernorm_fwd_q8", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), batches, rpb, D, x_bs, y_bs, eps,
              _p(q8), _p(ring), _p(tick), float(margin), _p(scale), stream=_stream())
    return scale


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, batches, rpb, D, x_bs, y_bs, accumulate_dx=False, gadd=None,
                  pad: int = 0, l: int = 1, relu_out=None, relu_first: int = 0, relu_db=None, fan=None, drop=None, row_mask=None, lm_scale=None):
    """mh_layernorm_bwd: one descriptor (mh_ln_bwd) carrying every rider given here; the library refuses the combinations it has no
    kernel for (the landmark riders beside fan or drop) before it launches anything.
    gadd ([batches, (pad + rpb) / l, D], dy's dtype): the gradient of the landmark means layernorm_fwd_lm produced; every dy row also
    receives gadd[b, (i + pad) / l] / l.  relu_out (bf16 [batches, R, D], with gadd only): rows [relu_first,
    relu_first + R) of x are a ReLU's output — their gradient leaves as bf16 (x > 0 ? dx : 0) in relu_out instead of f32 dx;
    relu_db (f32 [D], with relu_out): += the column sums of relu_out (the bias gradient of the Linear in front of the ReLU).
    fan = (src bf16 [batches, rpb - 1, D], alpha, cls f32 [batches, D] or None), without gadd: dy rows 1.. also receive alpha * src, row 0
    cls (layernorm_bwd_fan_ok says whether the shapes are on that form).
    drop = (out bf16 [batches, >= rpb, D] (the Dropout's tensor; rows past rpb are the caller's), p, seed, offset, dev_base, db f32 [D]), without gadd: x is the output of resid + Dropout_p(Linear),
    so out receives the lite-stream dropout backward of this launch's dx and db its column sums (fan may ride along)."""
    _chk(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, gadd, relu_out, relu_db, row_mask, lm_scale)
    d = _lib.LnBwdDesc()
    d.dy, d.x, d.gamma, d.mean, d.rstd, d.dx, d.dgamma, d.dbeta = _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta)
    d.batches, d.rows_per_batch, d.D, d.x_bs, d.y_bs = batches, rpb, D, x_bs, y_bs
    d.dt_x, d.dt_dy, d.dt_dx, d.accumulate_dx = dt(x), dt(dy), dt(dx), int(accumulate_dx)
    ws = None
    nbytes = int(_lib.load().mh_layernorm_bwd_workspace_bytes(batches * rpb, D))
    if nbytes:          # per-block dgamma / dbeta partials (folded by a second launch) instead of same-address atomics
        ws = torch.empty((nbytes // 4,), device=x.device, dtype=torch.float32)
        d.workspace, d.ws_floats = ws.data_ptr(), ws.numel()
    if gadd is not None:
        if gadd.dtype != dy.dtype or not gadd.is_contiguous() or gadd.numel() != batches * ((pad + rpb) // l) * D:
            raise MirrorHipError("layernorm_bwd: gadd must be contiguous [batches, (pad + rows) / l, D] in dy's dtype")
        d.gadd, d.pad, d.l = _p(gadd), int(pad), int(l)
    if lm_scale is not None:
        if lm_scale.dtype != torch.float32 or not lm_scale.is_contiguous() or lm_scale.numel() != batches * ((pad + rpb) // l):
            raise MirrorHipError("layernorm_bwd: lm_scale is a contiguous f32 [batches, (pad + rows) / l]")
        d.lm_scale = _p(lm_scale)
    if row_mask is not None:
        if row_mask.dtype != torch.float32 or not row_mask.is_contiguous() or row_mask.numel() != batches * (pad + rpb):
            raise MirrorHipError("layernorm_bwd: row_mask is a contiguous f32 [batches, pad + rows]")
        d.row_mask = _p(row_mask)
    if relu_out is not None:
        if (relu_out.dtype != torch.bfloat16 or not relu_out.is_contiguous() or relu_out.dim() != 3
                or relu_out.shape[0] != batches or relu_out.shape[2] != D or relu_first + relu_out.shape[1] > rpb):
            raise MirrorHipError("layernorm_bwd: relu_out must be contiguous bf16 [batches, R, D] with relu_first + R <= rows")
        d.relu_out, d.relu_first, d.relu_rows = _p(relu_out), int(relu_first), int(relu_out.shape[1])
    if relu_db is not None:
        if relu_db.dtype != torch.float32 or relu_db.numel() != D or not relu_db.is_contiguous():
            raise MirrorHipError("layernorm_bwd: relu_db is a contiguous f32 [D]")
        d.relu_db = _p(relu_db)
    if fan is not None:
        src, alpha, cls = fan
        _chk(src, cls)
        if not layernorm_bwd_fan_ok(dy, x, dx, src, cls, batches, rpb, D) or ws is None:
            raise MirrorHipError("layernorm_bwd: fan needs f32 x / dx, a contiguous bf16 [batches, rows - 1, D] source and >= 64 rows")
        d.fan_bf16, d.fan_alpha, d.fan_cls = _p(src), float(alpha), _p(cls)
    if drop is not None:
        dout, p_, seed_, off_, base_, ddb = drop
        _chk(dout, base_, ddb)
        if ws is None or not layernorm_bwd_drop_ok(dy, x, dx, dout, ddb, batches, rpb, D, off_):
            raise MirrorHipError("layernorm_bwd: drop needs f32 x / dx, a contiguous bf16 [batches, rows, D] output, D % 8 == 0, D <= 1024, offset % 8 == 0, >= 64 rows")
        d.drop_out, d.drop_p, d.drop_seed, d.drop_offset, d.drop_base, d.drop_db = _p(dout), float(p_), int(seed_), int(off_), _p(base_), _p(ddb)
        d.drop_rows_per_batch = int(dout.shape[1])
    _lib.call("mh_layernorm_bwd", C.byref(d), stream=_stream())


def layernorm_bwd_drop_ok(dy, x, dx, dout, ddb, batches: int, rpb: int, D: int, offset: int) -> bool:
    f = torch.float32
    return (x.dtype == f and dx.dtype == f and dy.dtype in (f, torch.bfloat16) and dout.dtype == torch.bfloat16 and dout.is_contiguous()
            and dout.dim() == 3 and dout.shape[0] == batches and dout.shape[1] >= rpb and dout.shape[2] == D and ddb.dtype == f and ddb.is_contiguous() and ddb.numel() == D and D % 8 == 0 and D <= 1024
            and offset % 8 == 0 and batches * rpb >= 64 and all(t.data_ptr() % 16 == 0 for t in (dy, x, dx, dout)))


def layernorm_bwd_fan_ok(dy, x, dx, src, cls, batches: int, rpb: int, D: int) -> bool:
    f = torch.float32
    return (dy.dtype in (f, torch.bfloat16) and x.dtype == f and dx.dtype == f and src.dtype == torch.bfloat16 and src.is_contiguous()
            and src.numel() == batches * (rpb - 1) * D and rpb >= 2 and batches * rpb >= 64 and D % 4 == 0
            and (cls is None or (cls.dtype == f and cls.is_contiguous() and cls.numel() == batches * D and cls.data_ptr() % 16 == 0))
            and all(t.data_ptr() % 16 == 0 for t in (dy, x, dx)) and src.data_ptr() % 8 == 0)


def layernorm_fwd_lm(x, gamma, beta, y, mean, rstd, xpm, batches, rows, D, x_bs, pad, l, eps, xpm_bf16=None, row_mask=None, lm_scale=None):
    """LayerNorm (f32 in, bf16 out behind `pad` zero rows, which this launch writes) + the landmark means xpm [batches, (pad + rows) / l, D]
    (f32) of its output rows (mh_layernorm_fwd_lm)."""
    _chk(x, gamma, beta, y, mean, rstd, xpm, xpm_bf16, row_mask, lm_scale)
    if lm_scale is not None and not (lm_scale.dtype == torch.float32 and lm_scale.is_contiguous() and lm_scale.numel() == batches * ((pad + rows) // l)):
        raise MirrorHipError("layernorm_fwd_lm: lm_scale is a contiguous f32 [batches, (pad + rows) / l]")
    if row_mask is not None and not (row_mask.dtype == torch.float32 and row_mask.is_contiguous() and row_mask.numel() == batches * (pad + rows)):
        raise MirrorHipError("layernorm_fwd_lm: row_mask is a contiguous f32 [batches, pad + rows]")
    if not (x.dtype == torch.float32 and y.dtype == torch.bfloat16 and y.is_contiguous() and (xpm is not None or xpm_bf16 is not None)
            and (xpm is None or (xpm.dtype == torch.float32 and xpm.is_contiguous()))):
        raise MirrorHipError("layernorm_fwd_lm: f32 input, contiguous bf16 rows and f32 (and / or bf16) landmark means")
    n_lm = batches * ((pad + rows) // l) * D
    if xpm_bf16 is not None and not (xpm_bf16.dtype == torch.bfloat16 and xpm_bf16.is_contiguous() and xpm_bf16.numel() == n_lm):
        raise MirrorHipError("layernorm_fwd_lm: xpm_bf16 must be a contiguous bf16 tensor of batches * (pad + rows) / l * D elements")
    _lib.call("mh_layernorm_fwd_lm", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(xpm), _p(xpm_bf16), batches, rows, D, x_bs, int(pad),
              int(l), eps, _p(row_mask), _p(lm_scale), stream=_stream())


def softmax_fwd(x: torch.Tensor, y: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
    """softmax over the last dim of a contiguous tensor (in place when y is x)."""
    _chk(x, y)
    _contig(x, "softmax input")
    cols = x.shape[-1]
    if y is None:
        y = torch.empty_like(x, dtype=out_dtype or x.dtype)
    _contig(y, "softmax output")
    _lib.call("mh_softmax_fwd", _p(x), _p(y), x.numel() // max(cols, 1), cols, cols, cols, dt(x), dt(y), stream=_stream())
    return y


def softmax_bwd(y: torch.Tensor, dy: torch.Tensor, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(y, dy, dx)
    _contig(y, "softmax y"), _contig(dy, "softmax dy")
    cols = y.shape[-1]
    if dx is None:
        dx = dy
    _lib.call("mh_softmax_bwd", _p(y), _p(dy), _p(dx), y.numel() // max(cols, 1), cols, cols, cols, cols, dt(y), dt(dy),
              dt(dx), stream=_stream())
    return dx


def softmax_masked_fwd(x: torch.Tensor, rowmask: torch.Tensor, colmask: torch.Tensor, y: Optional[torch.Tensor] = None,
                       out_dtype=None) -> torch.Tensor:
    """softmax(masked_fill(x, ~(rowmask[b, i] & colmask[b, j]), -max)) over the last dim of x [B, h, R, C]."""
    _chk(x, y, rowmask, colmask)
    _contig(x, "softmax input")
    Bn, h, R, Cc = x.shape
    assert rowmask.shape == (Bn, R) and colmask.shape == (Bn, Cc) and rowmask.dtype == colmask.dtype == torch.float32
    if y is None:
        y = torch.empty_like(x, dtype=out_dtype or x.dtype)
    _contig(y, "softmax output")
    _lib.call("mh_softmax_masked_fwd", _p(x), _p(y), _p(rowmask.contiguous()), _p(colmask.contiguous()), Bn, h, R, Cc, dt(x), dt(y),
              stream=_stream())
    return y


def softmax_masked_bwd(y: torch.Tensor, dy: torch.Tensor, rowmask: torch.Tensor, colmask: torch.Tensor) -> torch.Tensor:
    """In place on dy."""
    _chk(y, dy, rowmask, colmask)
    _contig(y, "softmax y"), _contig(dy, "softmax dy")
    Bn, h, R, Cc = y.shape
    _lib.call("mh_softmax_masked_bwd", _p(y), _p(dy), _p(dy), _p(rowmask.contiguous()), _p(colmask.contiguous()), Bn, h, R, Cc, dt(y),
              dt(dy), stream=_stream())
    return dy


def row_scale(x: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[..., r, :] = x[..., r, :] * scale[..., r] (x contiguous, scale f32 with one entry per row)."""
    _chk(x, scale, out)
    _contig(x, "row_scale input")
    D = x.shape[-1]
    rows = x.numel() // max(D, 1)
    assert scale.numel() == rows and scale.dtype == torch.float32
    if out is None:
        out = torch.empty_like(x)
    _lib.call("mh_row_scale", _p(x), _p(scale.contiguous()), _p(out), rows, D, dt(x), stream=_stream())
    return out


def keymask_plan(mask: torch.Tensor, lead: int, wrap: int, pad: int, l: int):  # noqa: E741
    """(mrow [B, m*l], mlm [B, m], lscale [B, m]) f32 for the sequence [pad zeros | lead ones | mask | mask[:, :wrap]] (mh_keymask_plan)."""
    _chk(mask)
    _contig(mask, "key-padding mask")
    assert mask.dtype == torch.bool and mask.dim() == 2
    B, n_src = mask.shape
    n_tot = pad + lead + n_src + wrap
    assert l > 0 and n_tot % l == 0 and 0 <= wrap <= n_src, "the padded sequence must be m groups of l rows"
    m = n_tot // l
    mrow = torch.empty((B, n_tot), device=mask.device, dtype=torch.float32)
    mlm = torch.empty((B, m), device=mask.device, dtype=torch.float32)
    lsc = torch.empty((B, m), device=mask.device, dtype=torch.float32)
    _lib.call("mh_keymask_plan", _p(mask), _p(mrow), _p(mlm), _p(lsc), B, n_src, lead, wrap, pad, l, stream=_stream())
    return mrow, mlm, lsc


def l2norm_fwd(x2d_rows: torch.Tensor, rows: int, D: int, x_rs: int, eps: float, out_dtype):
    _chk(x2d_rows)
    y = torch.empty((rows, D), device=x2d_rows.device, dtype=out_dtype)
    nrm = torch.empty((rows,), device=x2d_rows.device, dtype=torch.float32)
    _lib.call("mh_l2norm_fwd", _p(x2d_rows), _p(y), _p(nrm), rows, D, x_rs, eps, dt(x2d_rows), dt(y), stream=_stream())
    return y, nrm


def l2norm_bwd(y, nrm, dy, dx, rows, D, dx_rs, accumulate):
    _chk(y, nrm, dy, dx)
    _lib.call("mh_l2norm_bwd", _p(y), _p(nrm), _p(dy), _p(dx), rows, D, dx_rs, 0.0, dt(y), dt(dy), dt(dx),
              int(accumulate), stream=_stream())


# ----------------------------------------------------------------------------- Nystrom pieces
def landmark_fwd(qkv: torch.Tensor, l: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(qkv, out)
    _contig(qkv, "qkv")
    B, n_p, D3 = qkv.shape
    D = D3 // 3
    if out is not None and (tuple(out.shape) != (B, n_p // l, 2 * D) or out.dtype != qkv.dtype or not out.is_contiguous()):
        raise MirrorHipError("landmark_fwd: out must be a contiguous [B, n_p / l, 2 D] tensor of qkv's dtype")
    lm = out if out is not None else torch.empty((B, n_p // l, 2 * D), device=qkv.device, dtype=qkv.dtype)
    _lib.call("mh_landmark_fwd", _p(qkv), _p(lm), B, n_p, D, l, dt(qkv), stream=_stream())
    return lm


def landmark_bwd(dlm: torch.Tensor, dqkv: torch.Tensor, l: int) -> None:
    _chk(dlm, dqkv)
    _contig(dlm, "dlm"), _contig(dqkv, "dqkv")
    B, n_p, D3 = dqkv.shape
    if dlm.dtype != dqkv.dtype or tuple(dlm.shape) != (B, n_p // l, 2 * (D3 // 3)):
        raise MirrorHipError("landmark_bwd: shape/dtype mismatch")
    _lib.call("mh_landmark_bwd", _p(dlm), _p(dqkv), B, n_p, D3 // 3, l, dt(dqkv), stream=_stream())


def resconv(v_src: torch.Tensor, w: torch.Tensor, out: torch.Tensor, heads: int, transpose: bool, accumulate: bool) -> None:
    """v_src / out: [B, n_p, C] views with unit last stride (e.g. the v column block of qkv)."""
    _chk(v_src, w, out)
    B, n_p, Cc = v_src.shape
    if tuple(out.shape) != (B, n_p, Cc) or v_src.stride(2) != 1 or out.stride(2) != 1:
        raise MirrorHipError("resconv: bad views")
    taps = w.numel() // heads
    _lib.call("mh_resconv_fwd", _p(v_src), v_src.stride(1), v_src.stride(0), _p(_contig(w, "res_conv weight")), _p(out),
              out.stride(1), out.stride(0), B, n_p, heads, Cc // heads, taps, int(transpose), int(accumulate), dt(v_src),
              dt(out), stream=_stream())


def resconv_wgrad(v_src: torch.Tensor, dout: torch.Tensor, dw: torch.Tensor, heads: int) -> None:
    _chk(v_src, dout, dw)
    B, n_p, Cc = v_src.shape
    if tuple(dout.shape) != (B, n_p, Cc) or v_src.stride(2) != 1 or dout.stride(2) != 1 or dw.dtype != torch.float32:
        raise MirrorHipError("resconv_wgrad: bad views")
    taps = dw.numel() // heads
    _lib.call("mh_resconv_wgrad", _p(v_src), v_src.stride(1), v_src.stride(0), _p(dout), dout.stride(1), dout.stride(0),
              _p(dw), B, n_p, heads, Cc // heads, taps, dt(v_src), dt(dout), stream=_stream())


def resconv_bwd(dout: torch.Tensor, v_src: torch.Tensor, w: torch.Tensor, dv: torch.Tensor, dw: torch.Tensor, heads: int) -> None:
    """Both gradients of res_conv in one pass over dout (mh_resconv_bwd): dv += conv^T(dout), dw += the tap gradient.  dout / v_src /
    dv: [B, n_p, C] views with unit last stride (v_src, dv: the v column blocks of qkv / d qkv); dw f32 [heads * taps]."""
    _chk(dout, v_src, w, dv, dw)
    B, n_p, Cc = v_src.shape
    if (tuple(dout.shape) != (B, n_p, Cc) or tuple(dv.shape) != (B, n_p, Cc) or v_src.stride(2) != 1 or dout.stride(2) != 1 or dv.stride(2) != 1
            or dw.dtype != torch.float32 or dv.dtype != v_src.dtype):
        raise MirrorHipError("resconv_bwd: bad views")
    taps = dw.numel() // heads
    nbytes = int(_lib.load().mh_resconv_bwd_workspace_bytes(B, n_p, heads, Cc // heads, taps))
    ws = torch.empty((max(nbytes // 4, 1),), device=dout.device, dtype=torch.float32)
    _lib.call("mh_resconv_bwd", _p(dout), dout.stride(1), dout.stride(0), _p(v_src), v_src.stride(1), v_src.stride(0),
              _p(_contig(w, "res_conv weight")), _p(dv), dv.stride(1), dv.stride(0), _p(dw), _p(ws), nbytes // 4, B, n_p, heads, Cc // heads, taps,
              dt(v_src), dt(dout), stream=_stream())


def pinv_absmax(x: torch.Tensor, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stats: optional zeroed int64[2] (the caller's pre-zeroed arena saves the fill launch)."""
    _chk(x)
    _contig(x, "pinv input")
    m = x.shape[-1]
    if stats is None:
        stats = torch.zeros(2, device=x.device, dtype=torch.int64)
    _lib.call("mh_pinv_absmax", _p(x), _p(stats), x.numel() // (m * m), m, stream=_stream())
    return stats


def pinv_z0(x: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    m = x.shape[-1]
    z0 = torch.empty_like(x)
    _lib.call("mh_pinv_z0", _p(x), _p(stats), _p(z0), x.numel() // (m * m), m, stream=_stream())
    return z0


def _scratch1(scratch, like):
    """(one-float scratch, zeroed flag): a caller-provided f32[1] that already holds 0 (a slice of the step's zero arena), else a
    fresh one the entry point clears itself."""
    if scratch is None:
        return torch.empty(1, device=like.device, dtype=torch.float32), 0
    if scratch.dtype != torch.float32 or scratch.numel() != 1 or scratch.device != like.device:
        raise MirrorHipError("scratch: one f32 on the operands' device")
    return scratch, 1


def pinv_z0_bwd(x, z0, dz0, stats, dx, zeroed_scratch=None) -> None:
    """z0 None: formed on the fly from x and the maxima (nys_sim2 path: no stored f32 z_0)."""
    _chk(x, z0, dz0, stats, dx, zeroed_scratch)
    m = x.shape[-1]
    scratch, zf = _scratch1(zeroed_scratch, x)
    _lib.call("mh_pinv_z0_bwd", _p(x), _p(z0), _p(_contig(dz0, "dz0")), _p(stats), _p(dx), _p(scratch), zf,
              x.numel() // (m * m), m, stream=_stream())


def pinv_s2_bwd(p, dz0, stats, dx, zeroed_scratch=None, mlm=None, heads: int = 1) -> None:
    """dx (the chain's gradient wrt attn2 on entry) -> gradient wrt sim2's logits, one pass (mh_pinv_s2_bwd: m = 256).  mlm (f32 [B, m]) +
    heads: the valid-landmark flags of a key-padding mask (p [B, heads, m, m]): filled entries get no gradient."""
    _chk(p, dz0, stats, dx, zeroed_scratch, mlm)
    if mlm is not None and not (mlm.dtype == torch.float32 and mlm.is_contiguous() and mlm.numel() * heads * p.shape[-1] == p.numel()):
        raise MirrorHipError("pinv_s2_bwd: mlm is a contiguous f32 [B, m] with p [B, heads, m, m]")
    m = p.shape[-1]
    if not (p.dtype == dz0.dtype == dx.dtype == torch.float32 and p.is_contiguous() and dz0.is_contiguous() and dx.is_contiguous()
            and p.shape == dz0.shape == dx.shape and p.shape[-2] == m):
        raise MirrorHipError("pinv_s2_bwd: contiguous f32 [.., m, m] tensors of one shape")
    scratch, zf = _scratch1(zeroed_scratch, p)
    _lib.call("mh_pinv_s2_bwd", _p(p), _p(dz0), _p(stats), _p(dx), _p(scratch), zf, p.numel() // (m * m), m, _p(mlm), int(heads), stream=_stream())


PINV_CHAIN_M = 256


def pinv_chain_saved_alloc(iters: int, BH: int, m: int, device) -> torch.Tensor:
    """The chain's saved-iterate buffer (what mh_pinv_chain_fwd writes for mh_pinv_chain_bwd): [iters, 4, BH, m, m] bf16,
    slot k = (z_k, P_k, T2_k, T3_k), panel native."""
    nbytes = int(_lib.load().mh_pinv_chain_workspace_bytes(BH, m, iters, 0))
    if nbytes != iters * 4 * BH * m * m * 2:
        raise MirrorHipError(f"pinv chain: m={m} unsupported (mh_pinv_chain_workspace_bytes says {nbytes})")
    return torch.empty((iters, 4, BH, m, m), device=device, dtype=torch.bfloat16)


def pinv_chain_work_alloc(iters: int, BH: int, m: int, device) -> torch.Tensor:
    """The backward's scratch (mh_pinv_chain_workspace_bytes(which=1)): [iters + 4, BH, m, m] bf16."""
    n = int(_lib.load().mh_pinv_chain_workspace_bytes(BH, m, iters, 1)) // 2
    return torch.empty((n,), device=device, dtype=torch.bfloat16)


def pinv_chain_z0_slot(saved: torch.Tensor) -> torch.Tensor:
    """Where mh_pinv_chain_prep has to put the panel-native z_0."""
    return saved[0, 0]


def pinv_chain_prep(x: torch.Tensor, stats: torch.Tensor, z0cm_out: torch.Tensor):
    """attn2 (f32 [.., m, m]) -> (z0 f32 = x^T/(c r) row-major, XP = panel-native bf16 x); writes the panel-native z_0 into
    `z0cm_out` (normally saved[0, 0] of the chain).  Panel-native layout: include/mirror_hip.h."""
    _chk(x, stats, z0cm_out)
    _contig(x, "pinv_chain_prep input")
    m = x.shape[-1]
    BH = x.numel() // (m * m)
    if x.dtype != torch.float32 or z0cm_out.dtype != torch.bfloat16 or not z0cm_out.is_contiguous() or z0cm_out.numel() != x.numel():
        raise MirrorHipError("pinv_chain_prep: bad operands")
    z0 = torch.empty_like(x)
    xt = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _lib.call("mh_pinv_chain_prep", _p(x), _p(stats), _p(z0), _p(xt), _p(z0cm_out), BH, m, stream=_stream())
    return z0, xt


def pinv_chain_pack(dz: torch.Tensor) -> torch.Tensor:
    """d z_iters (f32 row-major [.., m, m]) -> the panel-native bf16 input of pinv_chain_bwd."""
    _chk(dz)
    _contig(dz, "pinv_chain_pack input")
    m = dz.shape[-1]
    if dz.dtype != torch.float32:
        raise MirrorHipError("pinv_chain_pack: f32 input expected")
    up = torch.empty(dz.shape, device=dz.device, dtype=torch.bfloat16)
    _lib.call("mh_pinv_chain_pack", _p(dz), _p(up), dz.numel() // (m * m), m, stream=_stream())
    return up


def nys_dz_dav(dw2: torch.Tensor, av: torch.Tensor, zfT: torch.Tensor, want_delta3: bool = False, out=None):
    """(PN((dw2 av^T)^T) bf16 [.., m, m] for mh_pinv_chain_bwd, dAV = Z^T dw2 bf16 [.., m, dh]) in one launch (mh_nys_dz_dav);
    want_delta3: a third result, sum_d dAV av f32 [.., m], for nys_attn3_bwd(delta3=...).  out: the two bf16 result buffers, for a
    caller that launches on another stream than the one that owns the memory."""
    _chk(dw2, av, zfT)
    m, dh = dw2.shape[-2], dw2.shape[-1]
    BH = dw2.numel() // (m * dh)
    if not (dw2.dtype == av.dtype == torch.float32 and zfT.dtype == torch.bfloat16 and dw2.is_contiguous() and av.is_contiguous()
            and zfT.is_contiguous() and av.shape == dw2.shape and zfT.numel() == BH * m * m):
        raise MirrorHipError("nys_dz_dav: contiguous f32 [.., m, dh] gradients / products and the bf16 column-major chain output")
    if out is None:
        up = torch.empty(zfT.shape, device=dw2.device, dtype=torch.bfloat16)
        dav = torch.empty(dw2.shape, device=dw2.device, dtype=torch.bfloat16)
    else:
        up, dav = out
        _chk(up, dav)
        if not (up.dtype == dav.dtype == torch.bfloat16 and up.is_contiguous() and dav.is_contiguous() and up.numel() == zfT.numel()
                and dav.shape == dw2.shape):
            raise MirrorHipError("nys_dz_dav: out must be contiguous bf16 buffers shaped like zfT and dw2")
    delta3 = torch.empty(dw2.shape[:-1], device=dw2.device, dtype=torch.float32) if want_delta3 else None
    _lib.call("mh_nys_dz_dav", _p(dw2), _p(av), _p(zfT), _p(up), _p(dav), _p(delta3), BH, m, dh, stream=_stream())
    return (up, dav, delta3) if want_delta3 else (up, dav)


_NYS_SIM2 = True       # test hook: False = sim2 as GEMM + softmax + absmax + operand packing (tests/test_fused_epilogue_gpu.py)


def nys_sim2_ok(lm: torch.Tensor, heads: int) -> bool:
    """mh_nys_sim2's geometry: bf16 landmarks [B, 256, 2 D] with D = heads * 64."""
    return (_NYS_SIM2 and lm.dim() == 3 and lm.dtype == torch.bfloat16 and _lm_ld(lm) > 0 and lm.shape[1] == PINV_CHAIN_M
            and lm.shape[2] == 2 * heads * 64)


def nys_sim2_alloc(lm: torch.Tensor, heads: int):
    """(attn2, xt) buffers of nys_sim2, for a caller that launches it on another stream than the one that owns the memory."""
    Bn, m, _ = lm.shape
    return (torch.empty((Bn, heads, m, m), device=lm.device, dtype=torch.float32),
            torch.empty((Bn, heads, m, m), device=lm.device, dtype=torch.bfloat16))


def nys_sim2(lm: torch.Tensor, heads: int, scale: float, stats: Optional[torch.Tensor] = None, want_z0f: bool = False, out=None, mlm=None):
    """(attn2 f32 [B, h, m, m], xt = panel-native bf16 attn2, z0f, stats) in one launch.  z0f (want_z0f) = panel-native f32 attn2^T, the
    unscaled z_0; by default None: the chain forward forms z_0 from the ROWS of attn2 (pinv_chain_fwd(z0f=a2, z0_rowmajor=True)) and the
    launch skips its second pass.  out: (attn2, xt) from nys_sim2_alloc.  mlm (f32 [B, m]): valid-landmark flags of a key-padding mask
    (masked_fill in front of the softmax; no z0f then)."""
    _chk(lm, stats, mlm)
    if mlm is not None and (want_z0f or mlm.dtype != torch.float32 or not mlm.is_contiguous() or mlm.numel() != lm.shape[0] * lm.shape[1]):
        raise MirrorHipError("nys_sim2: mlm is a contiguous f32 [B, m] and excludes want_z0f")
    Bn, m, D2 = lm.shape
    D = D2 // 2
    if stats is None:
        stats = torch.zeros(2, device=lm.device, dtype=torch.int64)
    a2, xt = out if out is not None else nys_sim2_alloc(lm, heads)
    _chk(a2, xt)
    if not (a2.shape == xt.shape == (Bn, heads, m, m) and a2.dtype == torch.float32 and xt.dtype == torch.bfloat16
            and a2.is_contiguous() and xt.is_contiguous()):
        raise MirrorHipError("nys_sim2: out must be the contiguous (f32, bf16) [B, h, m, m] pair of nys_sim2_alloc")
    z0f = torch.empty((Bn, heads, m, m), device=lm.device, dtype=torch.float32) if want_z0f else None
    _lib.call("mh_nys_sim2", _p(lm), _p(a2), _p(xt), _p(z0f), _p(stats), Bn, m, D, heads, float(scale), _lm_ld(lm), _p(mlm), stream=_stream())
    return a2, xt, z0f, stats


def pinv_chain_fwd(XT: torch.Tensor, saved: torch.Tensor, zfT: torch.Tensor, iters: int, z0f: Optional[torch.Tensor] = None,
                   stats: Optional[torch.Tensor] = None, z0_rowmajor: bool = False) -> None:
    """XT = panel-native x, saved[0, 0] = panel-native z_0 (or z0f / stats from nys_sim2: the kernel then forms z_0 itself and
    writes saved[0, 0]); zfT receives the column-major z_iters (= pinv^T row-major)."""
    _chk(XT, saved, zfT, z0f, stats)
    m = XT.shape[-1]
    BH = XT.numel() // (m * m)
    bf = torch.bfloat16
    if not (XT.dtype == bf and saved.dtype == bf and zfT.dtype == bf and XT.is_contiguous() and saved.is_contiguous()
            and zfT.is_contiguous() and saved.numel() == iters * 4 * BH * m * m and zfT.numel() == BH * m * m):
        raise MirrorHipError("pinv_chain_fwd: bad operands")
    if z0f is not None and not (z0f.dtype == torch.float32 and z0f.is_contiguous() and z0f.numel() == BH * m * m and stats is not None):
        raise MirrorHipError("pinv_chain_fwd: bad z0f / stats")
    fn = lambda: _lib.call("mh_pinv_chain_fwd", _p(XT), _p(saved), _p(zfT), BH, m, iters, _p(z0f), _p(stats), int(z0_rowmajor), stream=_stream())  # noqa: E731
    if gemm_profiler is None:
        fn()
    else:
        gemm_profiler.launch_named("pinv_panel_fwd_kernel", iters * 4 * 2.0 * m ** 3 * BH, fn)


def pinv_chain_bwd(XT, saved, dzf, work, dX, dz0, iters: int) -> None:
    """dzf = pinv_chain_pack(d z_iters).  dX / dz0: row-major f32 outputs."""
    _chk(XT, saved, dzf, work, dX, dz0)
    m = XT.shape[-1]
    BH = XT.numel() // (m * m)
    bf = torch.bfloat16
    if not (all(t.dtype == bf and t.is_contiguous() for t in (XT, saved, dzf, work))
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == BH * m * m for t in (dX, dz0))
            and saved.numel() == iters * 4 * BH * m * m and work.numel() >= (iters + 4) * BH * m * m and dzf.numel() == BH * m * m):
        raise MirrorHipError("pinv_chain_bwd: bad operands")
    fn = lambda: _lib.call("mh_pinv_chain_bwd", _p(XT), _p(saved), _p(dzf), _p(work), _p(dX), _p(dz0), BH, m, iters,  # noqa: E731
                           stream=_stream())
    if gemm_profiler is None:
        fn()
    else:
        gemm_profiler.launch_named("pinv_panel_bwd2_kernel", iters * 8 * 2.0 * m ** 3 * BH, fn)


# ------------------------------------------------------------------ fused Nystrom attention sides (nystrom_fused.hip)
NYS_FUSED_M, NYS_FUSED_DH = 256, 64


def nys_fused_ok(qkv: torch.Tensor, heads: int, m: int) -> bool:
    """The fused kernels cover the TransMIL geometry: bf16 qkv, 64-wide heads, 256 landmarks."""
    D = qkv.shape[-1] // 3
    return qkv.dtype == torch.bfloat16 and D == heads * NYS_FUSED_DH and m == NYS_FUSED_M and qkv.shape[1] % m == 0


def _nys_check(name: str, B: int, h: int, n_p: int, **tensors) -> None:
    D = h * NYS_FUSED_DH
    want = {"qkv": ((B, n_p, 3 * D), torch.bfloat16), "dqkv": ((B, n_p, 3 * D), torch.bfloat16),
            "lm": ((B, NYS_FUSED_M, 2 * D), torch.bfloat16), "dlm": ((B, NYS_FUSED_M, 2 * D), torch.float32),
            "w2": ((B, h, NYS_FUSED_M, NYS_FUSED_DH), torch.bfloat16), "dw2": ((B, h, NYS_FUSED_M, NYS_FUSED_DH), torch.float32),
            "av": ((B, h, NYS_FUSED_M, NYS_FUSED_DH), torch.float32), "dav": ((B, h, NYS_FUSED_M, NYS_FUSED_DH), torch.bfloat16),
            "out": ((B, n_p, D), torch.bfloat16), "dout": ((B, n_p, D), torch.bfloat16), "o1": ((B, n_p, D), torch.bfloat16),
            "lse1": ((B, h, n_p), torch.float32), "delta1": ((B, h, n_p), torch.float32),
            "lse3": ((B, h, NYS_FUSED_M), torch.float32)}
    for k, t in tensors.items():
        shape, dtype = want[k]
        if k == "lm" and tuple(t.shape) == shape and t.dtype == dtype and _lm_ld(t) > 0:
            continue                       # landmark rows may sit in a wider buffer (row stride lm_ld, see _lm_ld)
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise MirrorHipError(f"{name}: {k} must be contiguous {dtype} {shape}, got {t.dtype} {tuple(t.shape)} "
                                 f"contiguous={t.is_contiguous()}")


def _lm_ld(lm: torch.Tensor) -> int:
    """Row stride (elements) of a landmark tensor [B, m, 2D] whose rows are unit-stride, evenly spaced and batch-contiguous
    (a contiguous tensor, or the landmark rows behind the sequence in to_qkv's [rows, 3D] output); 0 if it is neither."""
    if lm.dim() != 3 or lm.stride(2) != 1 or lm.stride(0) != lm.shape[1] * lm.stride(1) or lm.stride(1) < lm.shape[2] or lm.stride(1) % 8:
        return 0
    return int(lm.stride(1))


def _nys_launch(name: str, flops: float, fn) -> None:
    if gemm_profiler is None:
        fn()
    else:
        gemm_profiler.launch_named(name, flops, fn)


def _nys_masks(kmask, B: int, n_p: int):
    """(mrow ptr, mlm ptr) of the key-padding mask pair prepared by TransLayer, or (None, None)."""
    if kmask is None:
        return None, None
    mrow, mlm = kmask[0], kmask[1]
    _chk(mrow, mlm)
    assert mrow.shape == (B, n_p) and mlm.shape == (B, NYS_FUSED_M) and mrow.dtype == mlm.dtype == torch.float32
    assert mrow.is_contiguous() and mlm.is_contiguous()
    return _p(mrow), _p(mlm)


def nys_attn1_fwd(qkv, lm, w2, out, heads: int, scale: float, accumulate: bool = False, kmask=None, o1=None) -> torch.Tensor:
    """out[:, :, head] (+)= softmax_m(scale q k_l^T) w2; returns the row logsumexp [B, h, n_p].  kmask: key-padding mask.
    o1: optional bf16 buffer shaped like out that receives the product alone (what nys_attn1_bwd takes delta1 from)."""
    _chk(qkv, lm, w2, out, o1)
    B, n_p, _ = qkv.shape
    lse1 = torch.empty((B, heads, n_p), device=qkv.device, dtype=torch.float32)
    _nys_check("nys_attn1_fwd", B, heads, n_p, qkv=qkv, lm=lm, w2=w2, out=out, **({} if o1 is None else {"o1": o1}))
    _nys_launch("nys_a1_fwd_kernel", 2 * 2.0 * n_p * NYS_FUSED_M * NYS_FUSED_DH * B * heads,
                lambda: _lib.call("mh_nys_attn1_fwd", _p(qkv), _p(lm), _p(w2), _p(out), _p(lse1), *_nys_masks(kmask, B, n_p), B, heads,
                                  n_p, NYS_FUSED_M, NYS_FUSED_DH, scale, int(accumulate), _lm_ld(lm), _p(o1), stream=_stream()))
    return lse1


def nys_attn1_fwd_q8(qkv, lm, w2, out, heads: int, scale: float, accumulate: bool, q8, ring, tick, margin: float = 1.25, o1=None):
    """nys_attn1_fwd (no mask) that also writes the e4m3 copy of `out` into q8 (uint8, out's shape) with the delayed scale of
    `ring` / `tick`; returns (lse1, dequantisation factor)."""
    _chk(qkv, lm, w2, out, q8, ring, tick)
    B, n_p, _ = qkv.shape
    if not (q8.dtype == torch.uint8 and q8.shape == out.shape and q8.is_contiguous() and ring.dtype == torch.int32 and ring.numel() == 3
            and tick.dtype == torch.float32):
        raise MirrorHipError("nys_attn1_fwd_q8: q8 uint8 shaped like out, int32[3] ring, f32 tick")
    lse1 = torch.empty((B, heads, n_p), device=qkv.device, dtype=torch.float32)
    sc = torch.empty((1,), device=qkv.device, dtype=torch.float32)
    _chk(o1)
    _nys_check("nys_attn1_fwd", B, heads, n_p, qkv=qkv, lm=lm.contiguous(), w2=w2, out=out, **({} if o1 is None else {"o1": o1}))
    lm = lm.contiguous()
    _nys_launch("nys_a1_fwd_kernel", 2 * 2.0 * n_p * NYS_FUSED_M * NYS_FUSED_DH * B * heads,
                lambda: _lib.call("mh_nys_attn1_fwd_q8", _p(qkv), _p(lm), _p(w2), _p(out), _p(lse1), B, heads, n_p, NYS_FUSED_M,
                                  NYS_FUSED_DH, scale, int(accumulate), _p(q8), _p(ring), _p(tick), float(margin), _p(sc), _p(o1),
                                  stream=_stream()))
    return lse1, sc


def nys_attn3_fwd(qkv, lm, heads: int, scale: float, kmask=None, rc=None):
    """av = softmax_n(scale q_l k^T) v as [B, h, m, dh] f32, and the row logsumexp [B, h, m].
    rc = (res_w f32 [h * 33] contiguous, out bf16 [B, n_p, D] contiguous): the same launch also writes out = res_conv(v)."""
    _chk(qkv, lm)
    B, n_p, _ = qkv.shape
    rc_w = rc_out = None
    if rc is not None:
        rc_w, rc_out = rc
        _chk(rc_w, rc_out)
        if (rc_w.dtype != torch.float32 or rc_w.numel() != heads * 33 or not rc_w.is_contiguous() or rc_out.dtype != torch.bfloat16
                or tuple(rc_out.shape) != (B, n_p, heads * NYS_FUSED_DH) or not rc_out.is_contiguous()):
            raise MirrorHipError("nys_attn3_fwd: rc = (f32 [h * 33] filters, contiguous bf16 [B, n_p, D] output)")
    av = torch.empty((B, heads, NYS_FUSED_M, NYS_FUSED_DH), device=qkv.device, dtype=torch.float32)
    lse3 = torch.empty((B, heads, NYS_FUSED_M), device=qkv.device, dtype=torch.float32)
    _nys_check("nys_attn3_fwd", B, heads, n_p, qkv=qkv, lm=lm)
    nws = int(_lib.load().mh_nys_attn3_ws_floats(B, heads, n_p))     # partial results of the sequence ranges
    ws = torch.empty((nws,), device=qkv.device, dtype=torch.float32) if nws else None
    _nys_launch("nys_a3_fwd_kernel", 2 * 2.0 * n_p * NYS_FUSED_M * NYS_FUSED_DH * B * heads,
                lambda: _lib.call("mh_nys_attn3_fwd", _p(qkv), _p(lm), _p(av), _p(lse3), _p(ws), nws, *_nys_masks(kmask, B, n_p), B,
                                  heads, n_p, NYS_FUSED_M, NYS_FUSED_DH, scale, _lm_ld(lm), _p(rc_w), _p(rc_out), stream=_stream()))
    return av, lse3


NYS_CLS_GEOMETRIES = ((64, 256), (96, 384))      # (dh, m) pairs csrc/nystrom_cls.hip is built for


def nys_cls_attn(qkv, lm, z, heads: int, scale: float, cls_row: int, lse3=None, mrow=None, mlm=None, z_colmajor: bool = False):
    """row [B, h, n_p] f32 = (attn1 @ pinv(attn2) @ attn3)[cls_row, :] of [3P] NystromAttention (its return_attn=True), without
    the n_p x n_p matrix (csrc/nystrom_cls.hip).  qkv [B, n_p, 3D] and lm [B, m, 2D] bf16 or f32 (same dtype; lm may be rows of a
    wider buffer, see _lm_ld); z [B, h, m, m] = pinv(attn2): f32 row-major, or with z_colmajor the pinv chain's bf16 zfT;
    lse3 [B, h, m] f32 from nys_attn3_fwd, or None (the kernel takes it in a pass of its own); mrow [B, n_p] / mlm [B, m]: the
    key-padding plan (both or neither).  Entries of an invalid key are exactly 0."""
    if qkv.dim() != 3 or lm.dim() != 3 or qkv.shape[2] % (3 * heads) or qkv.dtype != lm.dtype:
        raise MirrorHipError(f"nys_cls_attn: qkv [B, n_p, 3D] and lm [B, m, 2D] of one dtype, D a multiple of heads={heads}; got "
                             f"{tuple(qkv.shape)} {qkv.dtype}, {tuple(lm.shape)} {lm.dtype}")
    B, n_p, D3 = qkv.shape
    D, m = D3 // 3, lm.shape[1]
    dh = D // heads
    if (dh, m) not in NYS_CLS_GEOMETRIES:
        raise MirrorHipError(f"nys_cls_attn: built for (dh, m) in {NYS_CLS_GEOMETRIES}, got ({dh}, {m})")
    if tuple(lm.shape) != (B, m, 2 * D) or n_p < m or n_p % m:
        raise MirrorHipError(f"nys_cls_attn: lm must be [{B}, m, {2 * D}] and n_p={n_p} a multiple of m={m}; lm is {tuple(lm.shape)}")
    if not 0 <= int(cls_row) < n_p:
        raise MirrorHipError(f"nys_cls_attn: cls_row={cls_row} outside [0, {n_p})")
    if (mrow is None) != (mlm is None):
        raise MirrorHipError("nys_cls_attn: mrow and mlm go together (both or neither)")
    _contig(qkv, "nys_cls_attn: qkv")
    if not lm.is_contiguous() and _lm_ld(lm) == 0:
        raise MirrorHipError(f"nys_cls_attn: lm rows must be unit-stride and evenly spaced, got strides {lm.stride()}")
    zdt = torch.bfloat16 if z_colmajor else torch.float32
    if tuple(z.shape) != (B, heads, m, m) or z.dtype != zdt or not z.is_contiguous():
        raise MirrorHipError(f"nys_cls_attn: z must be contiguous {zdt} [{B}, {heads}, {m}, {m}] (z_colmajor={z_colmajor}), got "
                             f"{z.dtype} {tuple(z.shape)} contiguous={z.is_contiguous()}")
    if lse3 is not None and not (tuple(lse3.shape) == (B, heads, m) and lse3.dtype == torch.float32 and lse3.is_contiguous()):
        raise MirrorHipError(f"nys_cls_attn: lse3 must be contiguous f32 [{B}, {heads}, {m}]")
    if mrow is not None and not (tuple(mrow.shape) == (B, n_p) and tuple(mlm.shape) == (B, m) and mrow.dtype == mlm.dtype == torch.float32
                                 and mrow.is_contiguous() and mlm.is_contiguous()):
        raise MirrorHipError(f"nys_cls_attn: mrow / mlm must be contiguous f32 [{B}, {n_p}] / [{B}, {m}]")
    _chk(qkv, lm, z, lse3, mrow, mlm)        # (behind the argument checks: those read no data and give their message on any device)
    row = torch.empty((B, heads, n_p), device=qkv.device, dtype=torch.float32)
    _nys_launch("nys_cls_kernel", (1 if lse3 is not None else 2) * 2.0 * n_p * m * dh * B * heads,
                lambda: _lib.call("mh_nys_cls_attn", _p(qkv), _p(lm), _p(z), _p(lse3), _p(row), _p(mrow), _p(mlm), B, heads, n_p, m, dh,
                                  int(cls_row), float(scale), _lm_ld(lm), int(z_colmajor), dt(qkv), stream=_stream()))
    return row


def nys_attn1_bwd(qkv, lm, w2, dout, lse1, o1, delta1, dqkv, dw2, dlm, heads: int, scale: float, kmask=None) -> None:
    """attn1's backward (mh_nys_attn1_bwd), ONE kernel that walks the rows once (5 products per tile): ADDS into dw2 and into the k_l half
    of dlm (both f32, zeroed by the caller), WRITES delta1 [B, h, n_p] from the forward's saved rows o1 and the q block of dqkv."""
    _chk(qkv, lm, w2, dout, lse1, o1, delta1, dqkv, dw2, dlm)
    B, n_p, _ = qkv.shape
    _nys_check("nys_attn1_bwd", B, heads, n_p, qkv=qkv, lm=lm, w2=w2, dout=dout, lse1=lse1, delta1=delta1, o1=o1, dw2=dw2, dlm=dlm, dqkv=dqkv)
    _nys_launch("nys_a1_bwd_kernels", 5 * 2.0 * n_p * NYS_FUSED_M * NYS_FUSED_DH * B * heads,
                lambda: _lib.call("mh_nys_attn1_bwd", _p(qkv), _p(lm), _p(w2), _p(dout), _p(lse1), _p(o1), _p(delta1), _p(dqkv),
                                  _p(dw2), _p(dlm), *_nys_masks(kmask, B, n_p), B, heads, n_p, NYS_FUSED_M, NYS_FUSED_DH, scale,
                                  _lm_ld(lm), stream=_stream()))


def nys_attn3_bwd(qkv, lm, av, dav, lse3, dqkv, dlm, heads: int, scale: float, kmask=None, delta3=None) -> None:
    """Writes the k and v blocks of dqkv; ADDS into the q_l half of dlm (all from one kernel).  delta3: sum_d dav av from nys_dz_dav
    (skips a launch)."""
    _chk(qkv, lm, av, dav, lse3, dqkv, dlm, delta3)
    B, n_p, _ = qkv.shape
    _nys_check("nys_attn3_bwd", B, heads, n_p, qkv=qkv, lm=lm, av=av, dav=dav, lse3=lse3, dqkv=dqkv, dlm=dlm)
    given = delta3 is not None
    if given and not (delta3.dtype == torch.float32 and delta3.is_contiguous() and delta3.numel() == lse3.numel()):
        raise MirrorHipError("nys_attn3_bwd: delta3 must be contiguous f32 [B, h, m]")
    if not given:
        delta3 = torch.empty_like(lse3)
    _nys_launch("nys_a3_bwd_kernels", 7 * 2.0 * n_p * NYS_FUSED_M * NYS_FUSED_DH * B * heads,
                lambda: _lib.call("mh_nys_attn3_bwd", _p(qkv), _p(lm), None if given else _p(av), _p(dav), _p(lse3), _p(delta3), _p(dqkv), _p(dlm),
                                  *_nys_masks(kmask, B, n_p), B, heads, n_p, NYS_FUSED_M, NYS_FUSED_DH, scale, _lm_ld(lm),
                                  stream=_stream()))


def eye_minus(P: torch.Tensor, d: float) -> torch.Tensor:
    _chk(P)
    _contig(P, "eye_minus input")
    m = P.shape[-1]
    T = torch.empty_like(P)
    _lib.call("mh_eye_minus", _p(P), _p(T), d, P.numel() // (m * m), m, stream=_stream())
    return T


def seq_finish(seq: torch.Tensor, cls: torch.Tensor, N: int, add: int) -> None:
    _chk(seq, cls)
    B, n, D = seq.shape
    assert n == 1 + N + add and seq.is_contiguous() and cls.numel() == D and cls.dtype == torch.float32
    _lib.call("mh_seq_finish", _p(seq), _p(cls), B, N, add, D, dt(seq), stream=_stream())


def seq_finish_bwd(dseq: torch.Tensor, dcls: torch.Tensor, N: int, add: int) -> None:
    _chk(dseq, dcls)
    B, n, D = dseq.shape
    assert n == 1 + N + add and dseq.is_contiguous() and dcls.numel() == D and dcls.dtype == torch.float32
    _lib.call("mh_seq_finish_bwd", _p(dseq), _p(dcls), B, N, add, D, dt(dseq), stream=_stream())


def ppeg_merge(w7, w5, w3, b7, b5, b3):
    _chk(w7, w5, w3, b7, b5, b3)
    D = b7.numel()
    merged = torch.empty((49, D), device=w7.device, dtype=torch.float32)
    bsum = torch.empty((D,), device=w7.device, dtype=torch.float32)
    _lib.call("mh_ppeg_merge", _p(_contig(w7, "w7")), _p(_contig(w5, "w5")), _p(_contig(w3, "w3")), _p(b7), _p(b5), _p(b3),
              _p(merged), _p(bsum), D, stream=_stream())
    return merged, bsum


def ppeg(x: torch.Tensor, merged, bsum, S: int, flip: bool, out_dtype=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, merged, bsum, out)
    B, n, D = x.shape
    assert n == 1 + S * S and x.is_contiguous()
    if out is not None and (out.shape != x.shape or not out.is_contiguous() or out.dtype != (out_dtype or out.dtype)):
        raise MirrorHipError("ppeg: out must be contiguous, of x's shape and of out_dtype")
    y = out if out is not None else torch.empty_like(x, dtype=out_dtype or x.dtype)
    _lib.call("mh_ppeg_fwd", _p(x), _p(y), _p(merged), _p(bsum), B, S, D, int(flip), dt(x), dt(y), stream=_stream())
    return y


def ppeg_wgrad(x, dout, dmerged, dbsum, S: int) -> None:
    _chk(x, dout, dmerged, dbsum)
    B, n, D = x.shape
    assert n == 1 + S * S and x.is_contiguous() and dout.is_contiguous() and dout.shape == x.shape
    _lib.call("mh_ppeg_wgrad", _p(x), _p(dout), _p(dmerged), _p(dbsum), B, S, D, dt(x), dt(dout), stream=_stream())


def ppeg_bwd_ok(x, dy, merged, D: int, drop_offset: Optional[int] = None) -> bool:
    """mh_ppeg_bwd takes contiguous f32 x / dy of one shape; with a Dropout site also a D that mh_dropout_lite_colsum takes."""
    f = torch.float32
    return (x.dtype == f and dy.dtype == f and merged.dtype == f and x.shape == dy.shape and x.is_contiguous() and dy.is_contiguous()
            and all(t.data_ptr() % 16 == 0 for t in (x, dy, merged))
            and (drop_offset is None or (dropout_lite_colsum_ok(D) and drop_offset % 8 == 0)))


def ppeg_bwd(x, dy, merged, dmerged, dbsum, S: int, drop=None) -> torch.Tensor:
    """PPEG's backward in one launch (mh_ppeg_bwd): returns dx (f32, cls row passed through); dmerged [49, D] / dbsum [D] += the merged
    filter's and the summed bias' gradients.  drop = (out bf16 of x's shape, p, seed, offset, dev_base, db [D] f32): x came out of a
    Dropout on the lite stream — out = that Dropout's backward of dx, db += out's column sums (as dropout_lite_colsum of dx)."""
    _chk(x, dy, merged, dmerged, dbsum)
    B, n, D = x.shape
    if n != 1 + S * S or not ppeg_bwd_ok(x, dy, merged, D) or tuple(merged.shape) != (49, D):
        raise MirrorHipError("ppeg_bwd: contiguous 16-byte aligned f32 x / dy [B, 1 + S * S, D] and the merged filter [49, D]")
    for t, m in ((dmerged, 49 * D), (dbsum, D)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != m:
            raise MirrorHipError(f"ppeg_bwd: expected a contiguous f32 accumulator of {m} elements, got {tuple(t.shape)} {t.dtype}")
    dx = torch.empty_like(x)
    out, p, seed, off, base, db = drop if drop is not None else (None, 0.0, 0, 0, None, None)
    if drop is not None:
        _chk(out, base, db)
        if not (ppeg_bwd_ok(x, dy, merged, D, off) and out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == x.shape
                and db.dtype == torch.float32 and db.is_contiguous() and db.numel() == D):
            raise MirrorHipError("ppeg_bwd: the Dropout site needs a contiguous bf16 output of x's shape, an f32 [D] bias gradient, "
                                 "offset % 8 == 0 and a D that dropout_lite_colsum takes")
    _lib.call("mh_ppeg_bwd", _p(x), _p(dy), _p(merged), _p(dx), _p(dmerged), _p(dbsum), B, S, D, _p(out), _p(db), float(p), int(seed),
              int(off), _p(base), stream=_stream())
    return dx


def ppeg_grad_scatter(dmerged, dbsum, dw7, dw5, dw3, db7, db5, db3) -> None:
    """The six PPEG parameter gradients += their share of the merged kernel's gradient (dmerged [49, D], dbsum [D])."""
    D = dbsum.numel()
    outs = (dw7, dw5, dw3, db7, db5, db3)
    _chk(dmerged, dbsum, *outs)
    for t, n in zip((dmerged,) + outs, (49 * D, 49 * D, 25 * D, 9 * D, D, D, D)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise MirrorHipError(f"ppeg_grad_scatter: expected a contiguous f32 tensor of {n} elements, got {tuple(t.shape)} {t.dtype}")
    _lib.call("mh_ppeg_grad_scatter", _p(dmerged), _p(dbsum), *[_p(t) for t in outs], D, stream=_stream())


# ----------------------------------------------------------------------------- data feed
def gather_rows(src: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = src[rows[r]] for a [S, F] bank and int64 row indices of any shape (result: rows.shape + (F,))."""
    _chk(src, rows)
    if src.dim() != 2 or not src.is_contiguous():
        raise MirrorHipError("gather_rows: the bank must be a contiguous [rows, F] tensor")
    if rows.dtype != torch.int64 or not rows.is_contiguous():
        raise MirrorHipError("gather_rows: row indices must be contiguous int64")
    R, Fd = rows.numel(), src.shape[1]
    if out is None:
        out = torch.empty(tuple(rows.shape) + (Fd,), device=src.device, dtype=src.dtype)
    assert out.is_contiguous() and out.numel() == R * Fd and out.dtype == src.dtype
    _lib.call("mh_gather_rows", _p(src), _p(rows), _p(out), R, Fd, src.shape[0], dt(src), stream=_stream())
    return out


def _i64_table(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
        raise MirrorHipError(f"{name} must be a contiguous 1-d int64 tensor, got {tuple(t.shape)} {t.dtype}")
    return t


def _draw_base(dev_base: Optional[torch.Tensor], name: str) -> None:
    if dev_base is not None and (dev_base.dtype not in (torch.int64, torch.uint64) or dev_base.numel() < 1):
        raise MirrorHipError(f"{name}: dev_base is one 64-bit counter in device memory")


def sample_rows(slot_slide: torch.Tensor, lengths: torch.Tensor, starts: torch.Tensor, N: int, seed: int, offset: int,
                dev_base: Optional[torch.Tensor] = None, slack: float = 8.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [B, N] bank rows: slot b draws N rows of slide slot_slide[b] (lengths / starts: the [S] tables of the bank) with draw id
    offset + *dev_base + b under `seed` (mh_sample_rows: without replacement when the slide has >= N rows, with replacement below).
    `slack` moves the kernel's candidate threshold, never the result."""
    _chk(slot_slide, lengths, starts, dev_base, out)
    _i64_table(slot_slide, "sample_rows: slot_slide"), _i64_table(lengths, "sample_rows: lengths"), _i64_table(starts, "sample_rows: starts")
    _draw_base(dev_base, "sample_rows")
    if lengths.numel() != starts.numel():
        raise MirrorHipError("sample_rows: one length and one start per slide")
    B, N = slot_slide.numel(), int(N)
    if out is None:
        out = torch.empty((B, max(N, 0)), device=slot_slide.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, N) or not out.is_contiguous():
        raise MirrorHipError(f"sample_rows: out must be a contiguous int64 [{B}, {N}] tensor")
    _lib.call("mh_sample_rows", _p(slot_slide), _p(lengths), _p(starts), _p(out), B, N, lengths.numel(), int(seed) & (2 ** 64 - 1), int(offset),
              _p(dev_base), float(slack), stream=_stream())
    return out


def sample_weighted(cdf: torch.Tensor, count: int, seed: int, offset: int, dev_base: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [count] ids drawn with replacement from the distribution with cumulative sums cdf [S] (f64), draw id offset + *dev_base
    under `seed` (mh_sample_weighted)."""
    _chk(cdf, dev_base, out)
    if cdf.dtype != torch.float64 or cdf.dim() != 1 or cdf.numel() == 0 or not cdf.is_contiguous():
        raise MirrorHipError(f"sample_weighted: cdf must be a non-empty contiguous 1-d float64 tensor, got {tuple(cdf.shape)} {cdf.dtype}")
    _draw_base(dev_base, "sample_weighted")
    count = int(count)
    if out is None:
        out = torch.empty((max(count, 0),), device=cdf.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.numel() != count or not out.is_contiguous():
        raise MirrorHipError(f"sample_weighted: out must be a contiguous int64 tensor of {count} elements")
    _lib.call("mh_sample_weighted", _p(cdf), cdf.numel(), _p(out), count, int(seed) & (2 ** 64 - 1), int(offset), _p(dev_base), stream=_stream())
    return out


# ----------------------------------------------------------------------------- masking
def rank_mask(noise: torch.Tensor, len_keep: int, keep_map: bool = True) -> torch.Tensor:
    """mask [B, N] f32 (1 = masked): every row keeps the len_keep tokens of lowest noise.  keep_map: the same launch leaves the keep map
    on the returned tensor, `mask._keep = (keep_idx [B, len_keep] int32, slot [B, N] int32, len_keep)` (mh_rank_mask_keep): the rows
    the compact retention embed multiplies (functional.EmbedMaskPosFn)."""
    _chk(noise)
    noise = _contig(noise.float(), "noise")
    B, N = noise.shape
    mask = torch.empty_like(noise)
    len_keep = int(len_keep)
    if not keep_map or not 0 <= len_keep <= N:
        _lib.call("mh_rank_mask", _p(noise), _p(mask), B, N, len_keep, stream=_stream())
        return mask
    keep_idx = torch.empty((B, len_keep), device=noise.device, dtype=torch.int32)
    slot = torch.empty((B, N), device=noise.device, dtype=torch.int32)
    _lib.call("mh_rank_mask_keep", _p(noise), _p(mask), _p(keep_idx), _p(slot), B, N, len_keep, stream=_stream())
    mask._keep = (keep_idx, slot, len_keep)
    return mask


def _keep_geom(slot, keep_idx, B, T, first, keep) -> None:
    for t, shape in ((slot, (B, T - first)), (keep_idx, (B, keep))):
        if t is not None and not (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise MirrorHipError(f"keep map: expected a contiguous int32 {shape}, got {t.dtype} {tuple(t.shape)}")
    if not (0 <= first and 0 <= keep and first + keep <= T):
        raise MirrorHipError(f"keep map: first={first} keep={keep} of T={T}")


def rows_gather(x: torch.Tensor, keep_idx: torch.Tensor, first: int, keep: int) -> torch.Tensor:
    """[B, first + keep, K] bf16: the prefix rows and the kept tokens of x [B, T, K] bf16 (the compact layout of mh_rank_mask_keep)."""
    _chk(x, keep_idx)
    B, T, Kd = x.shape
    _keep_geom(None, keep_idx, B, T, first, keep)
    if x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise MirrorHipError("rows_gather: x must be a contiguous bf16 [B, T, K] tensor")
    out = torch.empty((B, first + keep, Kd), device=x.device, dtype=torch.bfloat16)
    _lib.call("mh_rows_gather", _p(x), _p(keep_idx), _p(out), B, T, Kd, first, keep, stream=_stream())
    return out


def mask_expand_fwd(rc: torch.Tensor, slot: torch.Tensor, token: torch.Tensor, pos: torch.Tensor, T: int, first: int, keep: int,
                    out: torch.Tensor) -> torch.Tensor:
    """out [B, T, D] f32 = (slot < 0 ? token : rc[compact row]) + pos[t] for the compact bf16 projection rc [B, first + keep, D]."""
    _chk(rc, slot, token, pos, out)
    B, Tc, D = rc.shape
    _keep_geom(slot, None, B, T, first, keep)
    if not (rc.dtype == torch.bfloat16 and rc.is_contiguous() and Tc == first + keep and out.dtype == torch.float32 and out.is_contiguous()
            and tuple(out.shape) == (B, T, D) and token.dtype == pos.dtype == torch.float32 and token.is_contiguous() and pos.is_contiguous()
            and token.numel() == D and pos.numel() == T * D):
        raise MirrorHipError("mask_expand_fwd: bad operands")
    _lib.call("mh_mask_expand_fwd", _p(rc), _p(out), _p(slot), _p(token), _p(pos), B, T, D, first, keep, stream=_stream())
    return out


def mask_apply_bwd_keep(dy, slot, dtoken, dpos, B, T, D, first, keep, out, dbias=None) -> None:
    """mask_apply_bwd (f32 dy, the quad form) whose dx is the compact bf16 tensor out [B, first + keep, D]: masked rows are not stored."""
    _chk(dy, slot, dtoken, dpos, out, dbias)
    _keep_geom(slot, None, B, T, first, keep)
    if not (dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == B * T * D and out.dtype == torch.bfloat16 and out.is_contiguous()
            and out.numel() == B * (first + keep) * D and dpos.dtype == dtoken.dtype == torch.float32 and dpos.numel() == T * D
            and dtoken.numel() == D and (dbias is None or (dbias.dtype == torch.float32 and dbias.numel() == D and dbias.is_contiguous()))):
        raise MirrorHipError("mask_apply_bwd_keep: bad operands")
    _lib.call("mh_mask_apply_bwd_keep", _p(dy), _p(out), _p(slot), _p(dtoken), _p(dpos), B, T, D, first, keep, _p(dbias), stream=_stream())


def rows_expand_zero(dhc: torch.Tensor, slot: torch.Tensor, T: int, first: int, keep: int) -> torch.Tensor:
    """[B, T, K] f32: the compact gradient dhc [B, first + keep, K] f32 at the prefix and kept rows, exact zeros at the masked ones."""
    _chk(dhc, slot)
    B, Tc, Kd = dhc.shape
    _keep_geom(slot, None, B, T, first, keep)
    if not (dhc.dtype == torch.float32 and dhc.is_contiguous() and Tc == first + keep):
        raise MirrorHipError("rows_expand_zero: dhc must be a contiguous f32 [B, first + keep, K] tensor")
    dh = torch.empty((B, T, Kd), device=dhc.device, dtype=torch.float32)
    _lib.call("mh_rows_expand_zero", _p(dhc), _p(slot), _p(dh), B, T, Kd, first, keep, stream=_stream())
    return dh


def mask_apply_fwd(x, mask, token, pos, B, T, D, first, token_scalar, out=None) -> None:
    """out (same shape as x, any dtype) receives the result; in place when omitted."""
    out = x if out is None else out
    _chk(x, mask, token, pos, out)
    assert x.is_contiguous() and x.numel() == B * T * D and mask.numel() == B * (T - first) and pos.numel() == T * D
    assert out.is_contiguous() and out.numel() == x.numel()
    _lib.call("mh_mask_apply_fwd", _p(x), _p(out), _p(mask), _p(token), _p(pos), B, T, D, first, int(token_scalar), dt(x), dt(out),
              stream=_stream())


def mask_apply_bwd_dbias_ok(dy, out, dpos, D) -> bool:
    """Can mask_apply_bwd leave the column sums of dx too (the bias gradient of the Linear in front)?"""
    return bool(_lib.load().mh_mask_apply_bwd_dbias_ok(_p(dy), _p(out), _p(dpos), D, dt(dy), dt(out)))


def mask_apply_bwd(dy, mask, dtoken, dpos, B, T, D, first, token_scalar, out=None, dbias=None) -> None:
    """out (same shape as dy, any dtype) receives dx; in place when omitted.  dbias [D] f32: += column sums of dx."""
    out = dy if out is None else out
    _chk(dy, mask, dtoken, dpos, out)
    assert dy.is_contiguous() and dy.numel() == B * T * D and dpos.numel() == T * D
    assert out.is_contiguous() and out.numel() == dy.numel()
    if dbias is not None:
        _chk(dbias)
        assert dbias.dtype == torch.float32 and dbias.numel() == D and dbias.is_contiguous()
    _lib.call("mh_mask_apply_bwd", _p(dy), _p(out), _p(mask), _p(dtoken), _p(dpos), B, T, D, first, int(token_scalar), dt(dy),
              dt(out), _p(dbias), stream=_stream())


# ----------------------------------------------------------------------------- RNA attention
def headattn_fwd(qkv: torch.Tensor, H: int):
    _chk(qkv)
    _contig(qkv, "qkv")
    B, D3 = qkv.shape
    D = D3 // 3
    out = torch.empty((B, D), device=qkv.device, dtype=qkv.dtype)
    attn = torch.empty((B, H, H), device=qkv.device, dtype=torch.float32)
    _lib.call("mh_headattn_fwd", _p(qkv), _p(out), _p(attn), B, H, D // H, dt(qkv), stream=_stream())
    return out, attn


def headattn_bwd(qkv, attn, dout, H: int) -> torch.Tensor:
    _chk(qkv, attn, dout)
    B, D3 = qkv.shape
    dqkv = torch.empty_like(qkv)
    dout = _contig(dout, "dout")
    if dout.dtype != qkv.dtype:
        raise MirrorHipError("headattn_bwd: dtype mismatch")
    _lib.call("mh_headattn_bwd", _p(qkv), _p(attn), _p(dout), _p(dqkv), B, H, D3 // 3 // H, dt(qkv), stream=_stream())
    return dqkv


# ----------------------------------------------------------------------------- fused RNA Block (csrc/rna_block.hip)
@functools.lru_cache(maxsize=None)
def _rna_block_fits(B: int, D: int, Hh: int, H: int) -> bool:
    # the library's own rule (csrc/rna_block.hip mh_rna_block_fits: every launch of both directions fits the LDS budget), the
    # one mh_rna_block_fwd / _bwd check before they launch; cached because it sits on every Block.forward
    return bool(_lib.load().mh_rna_block_fits(B, D, Hh, H))


def rna_block_ok(x: torch.Tensor, D: int, Hh: int, H: int) -> bool:
    """The fused Block covers [B <= 32, D] f32 rows with D, Hh multiples of 32 and H | D (c2: D = 512, Hh = 2048, H = 8), where
    the operand image of every Linear fits LDS in both directions (the qkv data gradient stages [B, 3 D])."""
    if not (x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == D and H >= 1):
        return False
    return _rna_block_fits(int(x.shape[0]), int(D), int(Hh), int(H))


def rna_block_workspace_bytes(B: int, D: int, Hh: int) -> int:
    return int(_lib.load().mh_rna_block_workspace_bytes(B, D, Hh))


def _rna_desc(B, D, Hh, H, eps, p, seed, offset, dev_base, **ptrs) -> "_lib.RnaBlockDesc":
    d = _lib.RnaBlockDesc()
    d.B, d.D, d.Hh, d.H, d.eps, d.p_drop, d.seed, d.offset = B, D, Hh, H, eps, p, seed, offset
    d.dev_base = _p(dev_base)
    for k, v in ptrs.items():
        _chk(v)
        setattr(d, k, _p(v))
    return d


def rna_block_fwd(x, params: dict, H: int, eps: float, p: float, seed: int, offset: int, dev_base):
    """params: bf16 weights w_qkv [3D, D], w_proj [D, D], w_fc1 [Hh, D], w_fc2 [D, Hh]; f32 b_qkv (or None), b_proj, b_fc1,
    b_fc2, g1, be1, g2, be2.  Returns (y, saved) with saved = the tensors mh_rna_block_bwd reads."""
    import ctypes
    B, D = x.shape
    Hh = params["w_fc1"].shape[0]
    dev, bf, f = x.device, torch.bfloat16, torch.float32
    for k in ("w_qkv", "w_proj", "w_fc1", "w_fc2"):
        if params[k].dtype != bf or not params[k].is_contiguous():
            raise MirrorHipError(f"rna_block_fwd: {k} must be a contiguous bf16 matrix")
    saved = {"stats": torch.empty((4, B), device=dev, dtype=f), "qkv": torch.empty((B, 3 * D), device=dev, dtype=bf),
             "attn": torch.empty((B, H, H), device=dev, dtype=f), "o": torch.empty((B, D), device=dev, dtype=bf),
             "x1": torch.empty((B, D), device=dev, dtype=f), "u": torch.empty((B, Hh), device=dev, dtype=bf),
             "f": torch.empty((B, Hh), device=dev, dtype=bf)}
    y = torch.empty((B, D), device=dev, dtype=f)
    d = _rna_desc(B, D, Hh, H, eps, p, seed, offset, dev_base, x=x, y=y, **params, **saved)
    _lib.call("mh_rna_block_fwd", ctypes.byref(d), stream=_stream())
    return y, saved


def rna_block_bwd(x, dy, params: dict, params_t: dict, grads: dict, saved: dict, H: int, eps: float, p: float, seed: int, offset: int,
                  dev_base) -> torch.Tensor:
    """params_t: wt_qkv ... (bf16 transposes); grads: f32 accumulation buffers dw_* / db_* / dg1 / dbe1 / dg2 / dbe2."""
    import ctypes
    B, D = x.shape
    Hh = params["w_fc1"].shape[0]
    if dy.dtype != torch.float32 or not dy.is_contiguous() or dy.shape != x.shape:
        raise MirrorHipError("rna_block_bwd: dy must be a contiguous f32 [B, D] tensor")
    dx = torch.empty_like(x)
    scratch = torch.empty((rna_block_workspace_bytes(B, D, Hh),), device=x.device, dtype=torch.uint8)
    d = _rna_desc(B, D, Hh, H, eps, p, seed, offset, dev_base, x=x, dy=dy, dx=dx, scratch=scratch, **params, **params_t, **grads, **saved)
    _lib.call("mh_rna_block_bwd", ctypes.byref(d), stream=_stream())
    return dx


# ----------------------------------------------------------------------------- elementwise
def add(a: torch.Tensor, b: torch.Tensor, out_dtype=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(a, b, out)
    _contig(a, "add a"), _contig(b, "add b")
    if a.shape != b.shape:
        raise MirrorHipError(f"add: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}")
    y = out if out is not None else torch.empty_like(a, dtype=out_dtype or a.dtype)
    _lib.call("mh_add", _p(a), _p(b), _p(y), a.numel(), dt(a), dt(b), dt(y), stream=_stream())
    return y


def lm_merge(a: torch.Tensor, b: Optional[torch.Tensor], out2: torch.Tensor, zero_cols: int) -> None:
    """out2[:, :cols] = bf16(a + b), out2[:, cols:cols + zero_cols] = 0 for f32 a / b [rows, cols] (b may be None) and a bf16 2-D
    view out2 [rows, cols + zero_cols] with unit column stride (mh_lm_merge): the landmark gradient as rows of to_qkv's gradient buffer."""
    _chk(a, b, out2)
    rows, cols = a.numel() // a.shape[-1], a.shape[-1]
    if not (a.dtype == torch.float32 and a.is_contiguous() and (b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == a.numel()))
            and out2.dim() == 2 and out2.dtype == torch.bfloat16 and out2.stride(1) == 1 and tuple(out2.shape) == (rows, cols + zero_cols)):
        raise MirrorHipError("lm_merge: f32 contiguous a / b, bf16 out2 [rows, cols + zero_cols] with unit column stride")
    _lib.call("mh_lm_merge", _p(a), _p(b), _p(out2), rows, cols, out2.stride(0), int(zero_cols), stream=_stream())


def cast(x: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.dtype == dtype and out is None:
        return x
    _chk(x, out)
    _contig(x, "cast input")
    y = torch.empty_like(x, dtype=dtype) if out is None else _contig(out, "cast output")
    if y.numel() != x.numel():
        raise MirrorHipError("cast: size mismatch")
    _lib.call("mh_cast", _p(x), _p(y), x.numel(), dt(x), dt(y), stream=_stream())
    return y


def last_form() -> str:
    """"<entry>:<form>" of the kernel the calling thread's last elementwise / row-kernel entry point launched (mh_last_form), e.g.
    "add:scalar", "softmax_fwd:wave,quad", "layernorm_bwd:ws"; "<entry>:none" when the call returned before any launch or was refused.
    The sequence kernels note theirs too: ppeg_fwd (pair, strip), ppeg_wgrad (strip), ppeg_bwd (one / one,drop), resconv_fwd (mfma, vec,
    scalar), resconv_wgrad (mfma, vec8, scalar), resconv_bwd (mfma, two_pass: written after the two calls it forwards to), landmark_fwd
    (quad, scalar) and landmark_bwd (oct, scalar).  The fused loss notes "loss_terms_fwd:<align>,<cluster>" (align: ext, quad, scalar;
    cluster: regs, global) and "loss_terms_bwd:<align>,<cluster>" (align: ext, bm16, bm32)."""
    return (_lib.load().mh_last_form() or b"").decode()


def _out_like(out: Optional[torch.Tensor], ref: torch.Tensor, dtype, name: str) -> torch.Tensor:
    """`out` (contiguous, ref's shape) or a fresh tensor of ref's shape."""
    if out is None:
        return torch.empty(ref.shape, device=ref.device, dtype=dtype)
    _chk(out)
    if out.shape != ref.shape or (dtype is not None and out.dtype != dtype):
        raise MirrorHipError(f"{name}: out is {tuple(out.shape)} of {out.dtype}, expected {tuple(ref.shape)} of {dtype}")
    return _contig(out, f"{name} out")


def gelu_fwd(x: torch.Tensor, out_dtype=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x)
    _contig(x, "gelu input")
    y = _out_like(out, x, out_dtype or (x.dtype if out is None else out.dtype), "gelu_fwd")
    _lib.call("mh_gelu_fwd", _p(x), _p(y), x.numel(), dt(x), dt(y), stream=_stream())
    return y


def gelu_bwd(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, dy)
    dy = _contig(dy, "gelu dy")
    _contig(x, "gelu x")           # the launch walks x.numel() elements of all three tensors
    if x.numel() != dy.numel():
        raise MirrorHipError(f"gelu_bwd: x has {x.numel()} elements, dy {dy.numel()}")
    dx = _out_like(out, dy, dy.dtype, "gelu_bwd")
    _lib.call("mh_gelu_bwd", _p(x), _p(dy), _p(dx), x.numel(), dt(x), dt(dy), dt(dx), stream=_stream())
    return dx


def relu_bwd(y: torch.Tensor, dy: torch.Tensor, out_dtype=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = dy * (y > 0).  y / dy: same shape; either contiguous, or 3-D with a contiguous [R, D] block per batch."""
    _chk(y, dy)
    if y.shape != dy.shape:
        raise MirrorHipError("relu_bwd: shape mismatch")
    dx = _out_like(out, y, out_dtype or (dy.dtype if out is None else out.dtype), "relu_bwd")

    def blk(t):
        if t.is_contiguous():
            return 1, t.numel(), 0
        if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]:
            return t.shape[0], t.shape[1] * t.shape[2], t.stride(0)
        raise MirrorHipError(f"relu_bwd: unsupported strides {t.stride()}")

    by, ny, sy = blk(y)
    bd, nd, sd = blk(dy)
    batches = max(by, bd)
    npb = y.numel() // batches
    if by == 1:
        sy = npb
    if bd == 1:
        sd = npb
    _lib.call("mh_relu_bwd", _p(y), _p(dy), _p(dx), npb, batches, sy, sd, npb, dt(y), dt(dy), dt(dx), stream=_stream())
    return dx


def dropout(x: torch.Tensor, p: float, seed: int, offset: int, out: Optional[torch.Tensor] = None,
            dev_base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dev_base: optional int64[1] device tensor added to `offset` on the device (per-step base of a graphed step)."""
    _chk(x, out, dev_base)
    _contig(x, "dropout input")
    y = out if out is not None else torch.empty_like(x)
    _lib.call("mh_dropout", _p(x), _p(y), x.numel(), p, seed, offset, _p(dev_base), dt(x), dt(y), stream=_stream())
    return y


def noise_draws(n_uniform: int, n_normal: int, seed: int, offset: int, dev_base: Optional[torch.Tensor], device) -> torch.Tensor:
    """f32 [n_uniform + n_normal]: uniform [0, 1) then standard normal draws on the dropout stream (mh_noise_draws); n_uniform % 4 == 0."""
    _chk(dev_base)
    assert n_uniform % 4 == 0 and offset % 4 == 0
    out = torch.empty((n_uniform + n_normal,), device=device, dtype=torch.float32)
    _chk(out)
    _lib.call("mh_noise_draws", _p(out), n_uniform, n_normal, seed, offset, _p(dev_base), stream=_stream())
    return out


def dropout_add(a: torch.Tensor, x: torch.Tensor, p: float, seed: int, offset: int, dev_base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a + dropout(x) as f32 (a f32, x f32 / bf16, same shape, numel % 4 == 0)."""
    _chk(a, x, dev_base)
    _contig(a, "dropout_add a"), _contig(x, "dropout_add x")
    assert a.dtype == torch.float32 and a.shape == x.shape and x.numel() % 4 == 0
    y = torch.empty_like(a)
    _lib.call("mh_dropout_add", _p(a), _p(x), _p(y), x.numel(), p, seed, offset, _p(dev_base), dt(x), stream=_stream())
    return y


def dropout_lite_colsum(x: torch.Tensor, p: float, seed: int, offset: int, dev_base, out: torch.Tensor, db: torch.Tensor) -> torch.Tensor:
    """out (bf16) = dropout-backward of the f32 gradient x [.., N] on the lite stream, db [N] += column sums of out (mh_dropout_lite_colsum)."""
    _chk(x, dev_base, out, db)
    N = x.shape[-1]
    if not (x.dtype == torch.float32 and out.dtype == torch.bfloat16 and x.is_contiguous() and out.is_contiguous() and out.shape == x.shape
            and db.dtype == torch.float32 and db.is_contiguous() and db.numel() == N and offset % 8 == 0):
        raise MirrorHipError("dropout_lite_colsum: contiguous f32 gradient, bf16 output of the same shape, f32 [N] bias gradient")
    _lib.call("mh_dropout_lite_colsum", _p(x), _p(out), x.numel() // N, N, p, seed, offset, _p(dev_base), _p(db), stream=_stream())
    return out


def dropout_lite_colsum_ok(N: int) -> bool:
    return N % 8 == 0 and 8 <= N <= 2048 and 256 % (N // 8) == 0


def timestamp(slot: torch.Tensor) -> None:
    """*slot (int64, one element) = the device wall clock when the current stream reaches this point (mh_timestamp: profiling aid)."""
    assert slot.dtype == torch.int64 and slot.numel() == 1 and slot.is_cuda
    _lib.call("mh_timestamp", _p(slot), stream=_stream())


def dropout_lite(x: torch.Tensor, p: float, seed: int, offset: int, dev_base: Optional[torch.Tensor] = None, *, add_to: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dropout(x) (or add_to + dropout(x) as f32) on the lite stream (mh_dropout_lite: Philox4x32-7, 16 bits per element);
    numel % 8 == 0, offset % 8 == 0.  The DROPADD projection epilogue draws the same masks."""
    _chk(x, dev_base, add_to, out)
    _contig(x, "dropout_lite x")
    if x.numel() % 8 or offset % 8:
        raise MirrorHipError("dropout_lite: numel and offset must be multiples of 8")
    if add_to is not None:
        _contig(add_to, "dropout_lite add_to")
        assert add_to.dtype == torch.float32 and add_to.shape == x.shape
        out = torch.empty_like(add_to) if out is None else out
    elif out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.numel() == x.numel()
    _lib.call("mh_dropout_lite", _p(add_to), _p(x), _p(out), x.numel(), p, seed, offset, _p(dev_base), dt(x), dt(out), stream=_stream())
    return out


def colsum(x2d: torch.Tensor, out: torch.Tensor) -> None:
    """out[c] += sum_r x2d[r, c]; x2d may be row-strided."""
    _chk(x2d, out)
    rows, cols = x2d.shape
    if x2d.stride(1) != 1 and cols > 1:
        raise MirrorHipError("colsum: unit column stride required")
    assert out.dtype == torch.float32 and out.numel() == cols
    _lib.call("mh_colsum", _p(x2d), _p(out), rows, cols, x2d.stride(0) if rows > 1 else cols, dt(x2d), stream=_stream())


def exp_fwd(x: torch.Tensor) -> torch.Tensor:
    _chk(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise MirrorHipError("exp_fwd: contiguous f32")
    y = torch.empty_like(x)
    _lib.call("mh_exp_fwd", _p(x), _p(y), x.numel(), stream=_stream())
    return y


def exp_bwd(dy: torch.Tensor, y: torch.Tensor, dx: torch.Tensor, accumulate: bool) -> None:
    _chk(dy, y, dx)
    if not all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == y.numel() for t in (dy, y, dx)):
        raise MirrorHipError("exp_bwd: contiguous f32 tensors of one size")
    _lib.call("mh_exp_bwd", _p(dy), _p(y), _p(dx), y.numel(), int(accumulate), stream=_stream())


def reparam_fwd(mu, logstd, eps) -> torch.Tensor:
    _chk(mu, logstd, eps)
    z = torch.empty_like(mu)
    _lib.call("mh_reparam_fwd", _p(_contig(mu, "mu")), _p(_contig(logstd, "logstd")), _p(_contig(eps, "eps")), _p(z),
              mu.numel(), stream=_stream())
    return z


def reparam_bwd(logstd, eps, dz, add_mu=None, add_ls=None):
    """(dmu, dlogstd) of z = mu + eps * exp(0.5 * logstd); add_mu / add_ls: gradients of mu / logstd from elsewhere, summed in."""
    _chk(logstd, eps, dz, add_mu, add_ls)
    for a in (add_mu, add_ls):
        if a is not None and (a.dtype != torch.float32 or not a.is_contiguous() or a.numel() != logstd.numel()):
            raise MirrorHipError("reparam_bwd: bad addend")
    dmu, dls = torch.empty_like(logstd), torch.empty_like(logstd)
    _lib.call("mh_reparam_bwd", _p(logstd), _p(eps), _p(_contig(dz, "dz")), _p(add_mu), _p(add_ls), _p(dmu), _p(dls), logstd.numel(),
              stream=_stream())
    return dmu, dls


# ----------------------------------------------------------------------------- losses / step glue
def ce_rows_fwd(G, scale, scale_mul, label_off, coef, out, loss_rows=None):
    _chk(G, scale, out, loss_rows)
    R, Cc = G.shape
    assert G.dtype == torch.float32 and G.stride(1) == 1
    lse = torch.empty((R,), device=G.device, dtype=torch.float32)
    _lib.call("mh_ce_rows_fwd", _p(G), G.stride(0), _p(scale), scale_mul, R, Cc, label_off, coef, _p(loss_rows), _p(lse),
              _p(out), stream=_stream())
    return lse


def ce_rows_bwd(G, scale, scale_mul, lse, g, g_per_row, gcoef, dscale, label_off):
    _chk(G, scale, lse, g, dscale)
    R, Cc = G.shape
    dG = torch.empty((R, Cc), device=G.device, dtype=torch.float32)
    _lib.call("mh_ce_rows_bwd", _p(G), G.stride(0), _p(scale), scale_mul, _p(lse), _p(g), int(g_per_row), gcoef, _p(dG),
              _p(dscale), R, Cc, label_off, stream=_stream())
    return dG


def _tgt_rows(tgt: torch.Tensor, rows: int, D: int):
    """(rows_per_batch, batch stride in elements) of a target that is contiguous or a row window [B, R, D] of a larger buffer."""
    if tgt.is_contiguous():
        return rows, rows * D
    if tgt.dim() == 3 and tgt.stride(2) == 1 and tgt.stride(1) == D and tgt.shape[2] == D:
        return tgt.shape[1], tgt.stride(0)
    raise MirrorHipError(f"masked-MSE target must be contiguous or a row window, got strides {tgt.stride()}")


MSE_FWD_WS_FLOATS = 2048      # MH_MSE_FWD_WS_FLOATS of include/mirror_hip.h


def mse_masked_fwd(pred, tgt, mask, acc, rows, D):
    """acc[0] += sum_r mask[r] * mean_D (pred - tgt)^2, acc[1] += sum_r mask[r], the blocks' partial sums added in block order
    (mh_mse_masked_fwd_ordered): the same inputs give the same bits on every launch."""
    _chk(pred, tgt, mask, acc)
    assert pred.is_contiguous() and tgt.numel() == pred.numel()
    rpb, tbs = _tgt_rows(tgt, rows, D)
    ws = torch.empty((MSE_FWD_WS_FLOATS,), device=pred.device, dtype=torch.float32)
    _lib.call("mh_mse_masked_fwd_ordered", _p(pred), _p(tgt), _p(mask), _p(acc), rows, D, rpb, tbs, dt(pred), dt(tgt), _p(ws),
              stream=_stream())


MSE_CS_BLOCKS = 1024      # blocks (= rows of the column-sum table) of mse_masked_bwd(colsum_ws=...)


def mse_masked_bwd_colsum_ok(pred, tgt, dpred, D: int) -> bool:
    return (D in (256, 512, 768, 1024) and pred.dtype == torch.bfloat16 and tgt.dtype == torch.float32 and dpred.dtype == torch.bfloat16
            and tgt.stride(0) % 4 == 0 and tgt.data_ptr() % 16 == 0 and pred.data_ptr() % 8 == 0 and dpred.data_ptr() % 8 == 0)


def mse_masked_bwd(pred, tgt, mask, acc, g, dpred, dtgt, rows, D, gmul: float = 1.0, colsum_ws=None):
    """dtgt None: the target's gradient (-dpred) is not materialised.  The upstream is g[0] * gmul.
    colsum_ws [blocks, D] f32: every block's column sums of dpred (colsum(colsum_ws, db) is then the bias gradient in front of pred)."""
    _chk(pred, tgt, mask, acc, g, dpred, *([] if dtgt is None else [dtgt]))
    assert pred.is_contiguous() and dpred.is_contiguous() and (dtgt is None or (dtgt.is_contiguous() and dtgt.dtype == tgt.dtype))
    rpb, tbs = _tgt_rows(tgt, rows, D)
    nb = 0
    if colsum_ws is not None:
        _chk(colsum_ws)
        assert colsum_ws.dtype == torch.float32 and colsum_ws.is_contiguous() and colsum_ws.dim() == 2 and colsum_ws.shape[1] == D
        nb = colsum_ws.shape[0]
    _lib.call("mh_mse_masked_bwd", _p(pred), _p(tgt), _p(mask), _p(acc), _p(g), float(gmul), _p(dpred), _p(dtgt), rows, D, rpb, tbs, dt(pred),
              dt(tgt), dt(dpred), _p(colsum_ws), nb, stream=_stream())


LOSS_TERMS_BMAX = 32          # alignment block of mh_loss_terms: B <= 32 and 2 B (D + 1) + B (B + 1) floats <= 150 KiB of LDS


def loss_terms_scratch_floats(Bc: int) -> int:
    """Floats of mh_loss_terms.scratch for Bc score rows: 8 words (zeroed by the caller), then one slot per block of the terms that
    several blocks share (Bc cluster rows, 32 + 32 of the RNA MSE; csrc/loss_fused.hip)."""
    return 8 + Bc + 64


def loss_terms_ok(B: int, D: int) -> bool:
    return 1 <= B <= LOSS_TERMS_BMAX and 4 * (2 * B * (D + 1) + B * (B + 1)) <= 150 * 1024


def _loss_terms_desc(weights, t: dict) -> "_lib.LossTermsDesc":
    """t: name -> f32 contiguous device tensor (or None) for the fields of mh_loss_terms; shapes are read off the operands."""
    d = _lib.LossTermsDesc()
    for k, v in t.items():
        if v is not None:
            if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                raise MirrorHipError(f"loss_terms: {k} must be a contiguous f32 device tensor")
            setattr(d, k, v.data_ptr())
    d.has_align = int(t.get("wsi_emb") is not None)
    if d.has_align:
        d.B, d.D = t["wsi_emb"].shape
        if tuple(t["rna_emb"].shape) != (d.B, d.D) or not loss_terms_ok(d.B, d.D):
            raise MirrorHipError(f"loss_terms: alignment embeddings {tuple(t['wsi_emb'].shape)} / {tuple(t['rna_emb'].shape)} not supported")
    d.n_rna = t["rna_pred"].numel()
    if t["rna_tgt"].numel() != d.n_rna or t["rna_mask"].numel() != d.n_rna:
        raise MirrorHipError("loss_terms: rna prediction / target / mask sizes differ")
    d.n_wstyle, d.n_rstyle = t["w_mu"].numel(), t["r_mu"].numel()
    d.rows_wstyle, d.rows_rstyle = t["w_mu"].shape[0], t["r_mu"].shape[0]
    if t["w_logstd"].numel() != d.n_wstyle or t["r_logstd"].numel() != d.n_rstyle:
        raise MirrorHipError("loss_terms: mu / logstd sizes differ")
    d.Bc, d.P = t["w_score"].shape
    if tuple(t["r_score"].shape) != (d.Bc, d.P):
        raise MirrorHipError("loss_terms: prototype score shapes differ")
    if t["scratch"].numel() < loss_terms_scratch_floats(d.Bc):
        raise MirrorHipError(f"loss_terms: scratch holds {t['scratch'].numel()} floats, {loss_terms_scratch_floats(d.Bc)} needed")
    for i, w in enumerate(weights):
        d.weight[i] = float(w)
    return d


def loss_terms_fwd(weights, t: dict) -> None:
    """mh_loss_terms_fwd: t carries the operands plus scratch [loss_terms_scratch_floats(Bc)] (the first 8 zeroed), save [B*B + 2B], out [8], wsi_acc (or None)."""
    _lib.call("mh_loss_terms_fwd", C.byref(_loss_terms_desc(weights, t)), stream=_stream())


def loss_terms_bwd(weights, t: dict) -> None:
    """mh_loss_terms_bwd: t additionally carries g_total (and g_terms) and the d_* outputs."""
    _lib.call("mh_loss_terms_bwd", C.byref(_loss_terms_desc(weights, t)), stream=_stream())


def fanout_bwd(gfull, x, alpha: float, c, B: int, T: int, D: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dE[b,t] = gfull[b,t] + alpha * x[b,t-1] (t >= 1) + (t == 0 ? c[b] : 0); any of the three may be None."""
    ref = next(t for t in (gfull, x, c) if t is not None)
    _chk(*[t for t in (gfull, x, c) if t is not None])
    assert gfull is None or (gfull.is_contiguous() and gfull.dtype == torch.float32 and gfull.numel() == B * T * D)
    assert x is None or (x.is_contiguous() and x.numel() == B * (T - 1) * D)
    assert c is None or (c.is_contiguous() and c.dtype == torch.float32 and c.numel() == B * D)
    if out is None:
        dE = torch.empty((B, T, D), device=ref.device, dtype=torch.float32)
    else:
        _chk(out)
        if out.dtype != torch.float32 or tuple(out.shape) != (B, T, D):
            raise MirrorHipError(f"fanout_bwd: out must be f32 [{B}, {T}, {D}], got {out.dtype} {tuple(out.shape)}")
        dE = _contig(out, "fanout_bwd out")
    _lib.call("mh_fanout_bwd", _p(gfull), _p(x), float(alpha), _p(c), _p(dE), B, T, D, dt(x) if x is not None else _lib.MH_F32,
              stream=_stream())
    return dE


def weighted_sum(terms, weights) -> torch.Tensor:
    """sum_i weights[i] * terms[i] for up to 6 f32 scalars living in separate tensors -> 0-d tensor."""
    n = len(terms)
    assert 1 <= n <= 6 and len(weights) == n
    _chk(*terms)
    ts = [t.reshape(1) for t in terms]
    for t in ts:
        assert t.dtype == torch.float32
    out = torch.empty((1,), device=ts[0].device, dtype=torch.float32)
    ptrs = [_p(t) for t in ts] + [None] * (6 - n)
    ws = [float(w) for w in weights] + [0.0] * (6 - n)
    _lib.call("mh_weighted_sum", *ptrs, *ws, n, _p(out), stream=_stream())
    return out.reshape(())


def weighted_sum_bwd(g: torch.Tensor, weights) -> torch.Tensor:
    n = len(weights)
    _chk(g)
    out = torch.empty((n,), device=g.device, dtype=torch.float32)
    ws = [float(w) for w in weights] + [0.0] * (6 - n)
    _lib.call("mh_weighted_sum_bwd", _p(g), *ws, n, _p(out), stream=_stream())
    return out


def kl_fwd(mu, ls, out, coef):
    _chk(mu, ls, out)
    _lib.call("mh_kl_fwd", _p(mu), _p(ls), _p(out), mu.numel(), coef, stream=_stream())


def kl_bwd(mu, ls, g, coef):
    _chk(mu, ls, g)
    dmu, dls = torch.empty_like(mu), torch.empty_like(ls)
    _lib.call("mh_kl_bwd", _p(mu), _p(ls), _p(g), _p(dmu), _p(dls), mu.numel(), coef, stream=_stream())
    return dmu, dls


def symkl_fwd(w, r, out, coef):
    _chk(w, r, out)
    B, P = w.shape
    _lib.call("mh_symkl_fwd", _p(w), _p(r), _p(out), B, P, coef, stream=_stream())


def symkl_bwd(w, r, g, coef):
    _chk(w, r, g)
    B, P = w.shape
    dw, dr = torch.empty_like(w), torch.empty_like(r)
    _lib.call("mh_symkl_bwd", _p(w), _p(r), _p(g), _p(dw), _p(dr), B, P, coef, stream=_stream())
    return dw, dr


def rownorm_(w: torch.Tensor, eps: float = 1e-12, shadow: Optional[torch.Tensor] = None) -> None:
    """shadow: optional bf16 tensor of w's shape that receives the rounded result in the same launch."""
    _chk(w, shadow)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2
    if shadow is not None and (shadow.dtype != torch.bfloat16 or not shadow.is_contiguous() or tuple(shadow.shape) != tuple(w.shape)):
        raise MirrorHipError("rownorm_: the shadow is a contiguous bf16 tensor of w's shape")
    _lib.call("mh_rownorm_", _p(w), _p(shadow), w.shape[0], w.shape[1], eps, stream=_stream())


def clamp_(x: torch.Tensor, lo: float, hi: float) -> None:
    _chk(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    _lib.call("mh_clamp_", _p(x), x.numel(), lo, hi, stream=_stream())


def grad_clip(g: torch.Tensor, grad_scale: float, max_norm: float, dev_state: torch.Tensor) -> None:
    """Global-L2-norm clipping factor into dev_state[4] (and the norm into dev_state[5]); the optimizer launch applies it."""
    _chk(g, dev_state)
    assert g.dtype == torch.float32 and g.is_contiguous() and dev_state.numel() == 6
    scratch = torch.empty(1, device=g.device, dtype=torch.float32)
    _lib.call("mh_grad_clip", _p(g), g.numel(), grad_scale, max_norm, _p(scratch), _p(dev_state), stream=_stream())


def _step_args(name: str, p, need, shadow, dev_state, clamp, counter, counter_add, tick, hole, ema, ema_cfg):
    """What adam() and optim_step() share.  Checks the arenas (`need`: p, g and the moments the rule reads), the shadow, the device
    step state, the counter and the EMA, and returns the arguments that mh_adam and mh_optim_step have in common behind dev_state:
    (clamp index, lo, hi, counter, counter_add, tick, hole_lo, hole_hi)."""
    n = p.numel()
    for t in need:
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise MirrorHipError(f"{name}: p, g and the moments the rule reads are contiguous f32 tensors of one size")
    if shadow is not None and (shadow.dtype != torch.bfloat16 or not shadow.is_contiguous() or shadow.numel() != n):
        raise MirrorHipError(f"{name}: the shadow is a contiguous bf16 tensor of p's size")
    if dev_state is not None and (dev_state.dtype != torch.float32 or dev_state.numel() != 6 or not dev_state.is_contiguous()):
        raise MirrorHipError(f"{name}: dev_state is the f32[6] device step state")
    if counter is not None and (counter.dtype != torch.int64 or counter.numel() != 1):
        raise MirrorHipError(f"{name}: the counter is one int64")
    ci, clo, chi = (-1, 0.0, 0.0) if clamp is None else (int(clamp[0]), float(clamp[1]), float(clamp[2]))
    if ci >= n:
        raise MirrorHipError(f"{name}: clamp index outside the arena")
    if ema is not None and (ema.dtype != torch.float32 or not ema.is_contiguous() or ema.numel() != n or ema_cfg is None
                            or dev_state is None):
        raise MirrorHipError(f"{name}: the EMA buffer must be a contiguous f32 tensor of p's size, with ema_cfg and dev_state")
    lo, hi = (0, 0) if hole is None else (int(hole[0]), int(hole[1]))
    return ci, clo, chi, _p(counter), int(counter_add), 2 if tick == "early" else int(bool(tick)), lo, hi


def adam(p, g, m, v, shadow, lr, b1, b2, eps, bc1, bc2, grad_scale=1.0, dev_state: Optional[torch.Tensor] = None,
         clamp: Optional[tuple] = None, counter: Optional[torch.Tensor] = None, counter_add: int = 0, tick: bool = True,
         hole: Optional[tuple] = None, ema: Optional[torch.Tensor] = None, ema_cfg=None) -> None:
    """mh_adam: torch.optim.Adam without weight decay over flat f32 arenas (TrainEngine steps through optim_step).
    dev_state: optional f32[6] device tensor {t, 1-b1^t, 1-b2^t, lr, clip, |g|}; when given the step count / bias
    corrections / lr live on the device (advanced by the launch itself), lr, bc1, bc2 are ignored and the gradient is
    also scaled by dev_state[4] (the factor grad_clip left there, else 1).  clamp = (index, lo, hi): that one parameter is clamped
    behind its update (master and shadow); counter (int64[1]) += counter_add in the same launches.  tick=False: dev_state is read,
    not advanced (tick="early": advanced, by the first launch of a two-launch step); hole = (lo, hi): those elements are left alone (the other launch of a two-launch step updates them).
    ema (f32, p's size) + ema_cfg (_lib.EmaCfg, needs dev_state): mh_adam_ema — every updated element's final value is also lerped
    into `ema` with timm's ModelEmaV3 decay of the device step, in the same pass."""
    _chk(p, g, m, v, shadow, dev_state, counter, ema)
    tail = _step_args("adam", p, (p, g, m, v), shadow, dev_state, clamp, counter, counter_add, tick, hole, ema, ema_cfg)
    args = (_p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), lr, b1, b2, eps, bc1, bc2, grad_scale, _p(dev_state), *tail)
    if ema is None:
        _lib.call("mh_adam", *args, stream=_stream())
    else:
        _lib.call("mh_adam_ema", *args, _p(ema), C.addressof(ema_cfg), stream=_stream())


def _optim_args(name: str, p, g, m, v, shadow, opt_cfg, dev_state, group_map, tables, most: int, what: str, optional: bool, **kw):
    """What optim_step() and optim_groups() share in front of the launch: the moments the rule reads, the required dev_state, _step_args
    (kw) and the group map with its tables (`tables`: f32 of one size, 1..`most` entries; `what` ends the refusal; optional: there may
    be no map, and then no groups).  Returns (number of groups, what _step_args returns)."""
    sgd = opt_cfg.rule == _lib.OPT_SGD
    need = [p, g] + ([] if sgd and opt_cfg.momentum == 0.0 else [m]) + ([] if sgd else [v])
    if dev_state is None:
        raise MirrorHipError(f"{name}: dev_state is the f32[6] device step state")
    tail = _step_args(name, p, need, shadow, dev_state, **kw)
    if group_map is None and optional:
        return 0, tail
    ng = 0 if tables[0] is None else tables[0].numel()
    if (group_map is None or group_map.dtype != torch.uint8 or not group_map.is_contiguous() or group_map.numel() < (p.numel() + 7) // 8 or not 1 <= ng <= most
            or any(t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != ng for t in tables)):
        raise MirrorHipError(f"{name}: group_map is uint8 with one entry per 8 elements, {what}")
    return ng, tail


def optim_step(p, g, m, v, shadow, opt_cfg, dev_state: torch.Tensor, grad_scale=1.0, group_map: Optional[torch.Tensor] = None,
               group_wd: Optional[torch.Tensor] = None, clamp: Optional[tuple] = None, counter: Optional[torch.Tensor] = None,
               counter_add: int = 0, tick=True, hole: Optional[tuple] = None, ema: Optional[torch.Tensor] = None, ema_cfg=None) -> None:
    """mh_optim_step: torch.optim.Adam(weight_decay) / AdamW / SGD(momentum, nesterov) over flat f32 arenas, by opt_cfg
    (_lib.OptimCfg); TrainEngine's update.  m: exp_avg / momentum_buffer (None for SGD without momentum), v: exp_avg_sq (None for
    SGD).  group_map (uint8, one entry per 8-element block of p) + group_wd (f32, one weight decay per group): per-parameter decay;
    None = no decay.  dev_state (required here), clamp, counter, tick, hole, ema / ema_cfg: as in adam(); lr is dev_state[3]."""
    _chk(p, g, m, v, shadow, dev_state, counter, ema, group_map, group_wd)
    ng, tail = _optim_args("optim_step", p, g, m, v, shadow, opt_cfg, dev_state, group_map, (group_wd,), 256, "group_wd f32 with 1..256 decays", True,
                           clamp=clamp, counter=counter, counter_add=counter_add, tick=tick, hole=hole, ema=ema, ema_cfg=ema_cfg)
    _lib.call("mh_optim_step", _p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), C.addressof(opt_cfg), _p(group_map),
              _p(group_wd) if group_map is not None else None, ng, grad_scale, _p(dev_state), *tail,
              _p(ema), None if ema is None else C.addressof(ema_cfg), stream=_stream())


def optim_groups(p, g, m, v, shadow, opt_cfg, dev_state: torch.Tensor, group_map: torch.Tensor, group_wd: torch.Tensor,
                 group_lr: torch.Tensor, grad_scale=1.0, clamp: Optional[tuple] = None, counter: Optional[torch.Tensor] = None,
                 counter_add: int = 0, tick=True, hole: Optional[tuple] = None, ema: Optional[torch.Tensor] = None, ema_cfg=None) -> None:
    """mh_optim_groups: optim_step with one learning rate per group — group_lr (f32, one per group, beside group_wd) replaces
    dev_state[3] for the elements of each group — and with the group byte _lib.OPT_SKIP_GROUP for blocks that are left untouched
    (torch.optim's parameter without a gradient).  group_map, group_wd and group_lr are required, at most 255 groups; both tables are
    read from the device at run time, so a captured launch replays with what they hold then."""
    _chk(p, g, m, v, shadow, dev_state, counter, ema, group_map, group_wd, group_lr)
    ng, tail = _optim_args("optim_groups", p, g, m, v, shadow, opt_cfg, dev_state, group_map, (group_wd, group_lr), _lib.OPT_SKIP_GROUP,
                           "group_wd and group_lr f32 with the same 1..255 entries", False,
                           clamp=clamp, counter=counter, counter_add=counter_add, tick=tick, hole=hole, ema=ema, ema_cfg=ema_cfg)
    _lib.call("mh_optim_groups", _p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), C.addressof(opt_cfg), _p(group_map), _p(group_wd),
              _p(group_lr), ng, grad_scale, _p(dev_state), *tail, _p(ema), None if ema is None else C.addressof(ema_cfg),
              stream=_stream())


GATHER_ROW = 1 << 15        # elements per mh_gather_many row: one workgroup copies a row, long tensors are split (a multiple of 8)


def gather_table(arena: torch.Tensor, items) -> torch.Tensor:
    """The device table of gather_many for `items` = [(arena offset, source tensor), ...]: rows {offset, address, n, dtype} of at
    most GATHER_ROW elements.  Sources are contiguous f32 or bf16 tensors on the arena's device; every range is checked against the
    arena here, on the host (the caller keeps the ranges disjoint and the sources alive until the launch has run)."""
    rows = []
    for off, t in items:
        _chk(t)
        if t.device != arena.device or not t.is_contiguous() or off < 0 or off + t.numel() > arena.numel():
            raise MirrorHipError(f"gather_table: a contiguous source on the arena's device inside its {arena.numel()} elements, got "
                                 f"{tuple(t.shape)} at {off}")
        code, size, ptr = dt(t), t.element_size(), t.data_ptr()
        for s in range(0, t.numel(), GATHER_ROW):
            rows += [off + s, ptr + size * s, min(GATHER_ROW, t.numel() - s), code]
    return torch.tensor(rows, dtype=torch.int64).view(-1, 4).to(arena.device)


def gather_many(arena: torch.Tensor, table: torch.Tensor) -> None:
    """arena[o_i : o_i + n_i] = src_i (f32, or bf16 widened) for the rows of `table` (gather_table), in one launch."""
    _chk(arena, table)
    if not (arena.dtype == torch.float32 and arena.is_contiguous() and table.dtype == torch.int64 and table.is_contiguous()
            and table.dim() == 2 and table.shape[1] == 4 and table.device == arena.device):
        raise MirrorHipError("gather_many: f32 contiguous arena, int64 [nrows, 4] table on its device")
    _lib.call("mh_gather_many", _p(arena), _p(table), int(table.shape[0]), stream=_stream())


def ema_update_many(ema: torch.Tensor, table: torch.Tensor, nseg: int, weight: float = 1.0, dev_state: Optional[torch.Tensor] = None,
                    ema_cfg=None) -> None:
    """ema[o_i : o_i + n_i] = lerp(ema[o_i : o_i + n_i], src_i, w) for the rows {o_i, src_i address, n_i} of `table` (int64 [nseg, 3]
    on ema's device; the caller guarantees that every row lies inside `ema` and its f32 source).  w = weight, or timm's decay rule
    of ema_cfg (_lib.EmaCfg) at the device step dev_state[0] (graph-capturable)."""
    _chk(ema, table, dev_state)
    if not (ema.dtype == torch.float32 and ema.is_contiguous() and table.dtype == torch.int64 and table.is_contiguous()
            and table.numel() == 3 * nseg):
        raise MirrorHipError("ema_update_many: f32 contiguous ema, int64 [nseg, 3] table")
    if dev_state is not None and ema_cfg is None:
        raise MirrorHipError("ema_update_many: dev_state needs ema_cfg")
    _lib.call("mh_ema_update_many", _p(ema), _p(table), int(nseg), float(weight), _p(dev_state),
              None if ema_cfg is None else C.addressof(ema_cfg), stream=_stream())


# ----------------------------------------------------------------------------- survival step (train_survival.py)
SURV_NLL, SURV_CE = 0, 1
_SV_T = {torch.int32: 1, torch.int64: 2}
_SV_C = {torch.bool: 0, torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}


def _surv_inputs(logits: torch.Tensor, event_times: torch.Tensor, censoring: torch.Tensor):
    """(logits, event_times, censoring, dt_t, dt_c) checked for mh_surv_loss_*: logits [N, M] f32 with unit column stride,
    event_times / censoring contiguous [N] of a supported dtype."""
    _chk(logits, event_times, censoring)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise MirrorHipError(f"survival logits must be f32 [N, M], got {logits.dtype} {tuple(logits.shape)}")
    if logits.stride(1) != 1 and logits.shape[1] > 1:
        logits = logits.contiguous()
    N = logits.shape[0]
    if event_times.numel() != N or censoring.numel() != N:
        raise MirrorHipError(f"event_times / censoring need {N} elements, got {event_times.numel()} / {censoring.numel()}")
    if event_times.dtype not in _SV_T:
        raise MirrorHipError(f"event_times must be int32 or int64, got {event_times.dtype}")
    if censoring.dtype not in _SV_C:
        raise MirrorHipError(f"censoring must be bool, uint8, int32, int64 or f32, got {censoring.dtype}")
    t, c = event_times.reshape(-1).contiguous(), censoring.reshape(-1).contiguous()
    return logits, t, c, _SV_T[t.dtype], _SV_C[c.dtype]


def _ld(logits: torch.Tensor) -> int:
    return logits.stride(0) if logits.shape[0] > 1 else logits.shape[1]


def surv_loss_fwd(logits, event_times, censoring, kind: int, lo: float, hi: float, w_all: float, w_unc: float, coef: float,
                  out: Optional[torch.Tensor], rows: Optional[torch.Tensor]) -> None:
    """out [1] = coef * sum of the per-row losses (stored); rows [N] (optional) = the per-row losses."""
    logits, t, c, dt_t, dt_c = _surv_inputs(logits, event_times, censoring)
    N, M = logits.shape
    _chk(out, rows)
    assert out is None or (out.dtype == torch.float32 and out.numel() >= 1)
    assert rows is None or (rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() == N)
    _lib.call("mh_surv_loss_fwd", _p(logits), _ld(logits), _p(t), dt_t, _p(c), dt_c, N, M, kind, lo, hi, w_all, w_unc, coef,
              _p(rows), _p(out), stream=_stream())


def surv_loss_bwd(logits, event_times, censoring, kind: int, lo: float, hi: float, w_all: float, w_unc: float, g: torch.Tensor,
                  gcoef: float) -> torch.Tensor:
    """dlogits [N, M] f32 for the upstream gcoef * g (g: one element, or one per row)."""
    logits, t, c, dt_t, dt_c = _surv_inputs(logits, event_times, censoring)
    N, M = logits.shape
    _chk(g)
    g = g.reshape(-1).contiguous().float()
    if g.numel() not in (1, N):
        raise MirrorHipError(f"survival loss upstream gradient must have 1 or {N} elements, got {g.numel()}")
    dx = torch.empty((N, M), device=logits.device, dtype=torch.float32)
    _lib.call("mh_surv_loss_bwd", _p(logits), _ld(logits), _p(t), dt_t, _p(c), dt_c, N, M, kind, lo, hi, w_all, w_unc, _p(g),
              int(g.numel() == N and N > 1), gcoef, _p(dx), stream=_stream())
    return dx


def surv_risk(logits: torch.Tensor) -> torch.Tensor:
    """-sum_j cumprod(1 - sigmoid(logits), 1)[:, j] as f32 [N]."""
    _chk(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise MirrorHipError(f"risk_scores needs f32 [N, M] logits, got {logits.dtype} {tuple(logits.shape)}")
    if logits.stride(1) != 1 and logits.shape[1] > 1:
        logits = logits.contiguous()
    N, M = logits.shape
    risk = torch.empty((N,), device=logits.device, dtype=torch.float32)
    _lib.call("mh_surv_risk", _p(logits), _ld(logits), N, M, _p(risk), stream=_stream())
    return risk


def cindex_counts(event_u8: torch.Tensor, time_f64: torch.Tensor, est_f32: torch.Tensor, tied_tol: float) -> torch.Tensor:
    """int64 [5] {concordant, discordant, tied_risk, tied_time, comparable} on the device (no sync)."""
    _chk(event_u8, time_f64, est_f32)
    n = event_u8.numel()
    assert event_u8.dtype == torch.uint8 and time_f64.dtype == torch.float64 and est_f32.dtype == torch.float32
    assert event_u8.is_contiguous() and time_f64.is_contiguous() and est_f32.is_contiguous()
    if time_f64.numel() != n or est_f32.numel() != n:
        raise MirrorHipError(f"concordance inputs differ in length: {n}, {time_f64.numel()}, {est_f32.numel()}")
    counts = torch.empty((5,), device=event_u8.device, dtype=torch.int64)
    _lib.call("mh_cindex_counts", _p(event_u8), _p(time_f64), _p(est_f32), n, float(tied_tol), _p(counts), stream=_stream())
    return counts


# ----------------------------------------------------------------------------- Cox loss and log-rank test (csrc/cox.hip)
COX_TIES = {"breslow": 0, "efron": 1}
COX_RED = {"none": 0, "sum": 1, "mean": 2, "batch": 3}
COX_MAX_N = 65536


def _cox_inputs(logits: torch.Tensor, time_f64: torch.Tensor, censoring: torch.Tensor):
    """(logits, row stride, time, censoring, dt_c, N) checked for mh_cox_loss_*: logits [N] or [N, 1] f32 read in place through
    their stride, time contiguous f64 [N], censoring [N] of a supported dtype."""
    _chk(logits, time_f64, censoring)
    if logits.dtype != torch.float32 or not (logits.dim() == 1 or (logits.dim() == 2 and logits.shape[1] == 1)):
        raise MirrorHipError(f"Cox logits must be f32 [N] or [N, 1], got {logits.dtype} {tuple(logits.shape)}")
    N = logits.shape[0]
    if N < 1 or N > COX_MAX_N:
        raise MirrorHipError(f"Cox loss needs 1 <= N <= {COX_MAX_N} rows, got {N}")
    ld = logits.stride(0) if N > 1 else 1
    if ld < 1:
        logits, ld = logits.contiguous(), 1
    if time_f64.numel() != N or censoring.numel() != N:
        raise MirrorHipError(f"event_times / censoring need {N} elements, got {time_f64.numel()} / {censoring.numel()}")
    if time_f64.dtype != torch.float64:
        raise MirrorHipError(f"Cox times must be f64 here (CoxLossFn converts them), got {time_f64.dtype}")
    if censoring.dtype not in _SV_C:
        raise MirrorHipError(f"censoring must be bool, uint8, int32, int64 or f32, got {censoring.dtype}")
    t, c = time_f64.reshape(-1).contiguous(), censoring.reshape(-1).contiguous()
    return logits, ld, t, c, _SV_C[c.dtype], N


def cox_workspace(N: int, device) -> torch.Tensor:
    """The f64 workspace the forward fills and the backward reads (mh_cox_workspace_bytes)."""
    nbytes = int(_lib.load().mh_cox_workspace_bytes(int(N)))
    if nbytes < 0:
        raise MirrorHipError(f"Cox loss needs 1 <= N <= {COX_MAX_N} rows, got {N}")
    return torch.empty((nbytes // 8,), device=device, dtype=torch.float64)


def cox_loss_fwd(logits, time_f64, censoring, ties: int, reduction: int, rows: Optional[torch.Tensor], out: Optional[torch.Tensor],
                 ws: torch.Tensor) -> None:
    """rows [N] f32 (optional) = the per-row Cox losses; out [1] (optional) = their reduction (stored); ws = cox_workspace(N)."""
    logits, ld, t, c, dt_c, N = _cox_inputs(logits, time_f64, censoring)
    _chk(rows, out, ws)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= 4 * N + 2
    assert out is None or (out.dtype == torch.float32 and out.numel() >= 1)
    assert rows is None or (rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() == N)
    _lib.call("mh_cox_loss_fwd", _p(logits), ld, _p(t), _p(c), dt_c, N, ties, reduction, _p(rows), _p(out), _p(ws), stream=_stream())


def cox_loss_bwd(logits, time_f64, censoring, ties: int, reduction: int, g: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """dlogits (f32, the logits' shape) for the upstream g: one element, or one per row when reduction is none."""
    logits, ld, t, c, dt_c, N = _cox_inputs(logits, time_f64, censoring)
    _chk(g, ws)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= 4 * N + 2
    g = g.reshape(-1).contiguous().float()
    per_row = reduction == COX_RED["none"]
    if g.numel() != (N if per_row else 1):
        raise MirrorHipError(f"Cox loss upstream gradient must have {N if per_row else 1} elements, got {g.numel()}")
    dx = torch.empty(logits.shape, device=logits.device, dtype=torch.float32)
    _lib.call("mh_cox_loss_bwd", _p(logits), ld, _p(t), _p(c), dt_c, N, ties, reduction, _p(g), int(per_row and N > 1), _p(ws),
              _p(dx), 1, stream=_stream())
    return dx


def logrank_stats(event_u8: torch.Tensor, time_f64: torch.Tensor, group_u8: torch.Tensor) -> torch.Tensor:
    """f64 [4] {O1, E1, V, n_events} of the two-group log-rank test, on the device (no sync)."""
    _chk(event_u8, time_f64, group_u8)
    n = event_u8.numel()
    assert event_u8.dtype == torch.uint8 and time_f64.dtype == torch.float64 and group_u8.dtype == torch.uint8
    assert event_u8.is_contiguous() and time_f64.is_contiguous() and group_u8.is_contiguous()
    if time_f64.numel() != n or group_u8.numel() != n:
        raise MirrorHipError(f"log-rank inputs differ in length: {n}, {time_f64.numel()}, {group_u8.numel()}")
    if n < 1 or n > COX_MAX_N:
        raise MirrorHipError(f"log-rank test needs 1 <= n <= {COX_MAX_N} samples, got {n}")
    stats = torch.empty((4,), device=event_u8.device, dtype=torch.float64)
    _lib.call("mh_logrank_stats", _p(event_u8), _p(time_f64), _p(group_u8), n, _p(stats), stream=_stream())
    return stats


# ----------------------------------------------------------------------------- subtyping step (train_subtyping.py)
CLS_RED = {"none": 0, "mean": 1, "sum": 2}
NO_IGNORE = -(1 << 63)          # ignore_index that no int32 label can equal (timm's loss has none)


def cls_labels(labels: torch.Tensor, device: torch.device, N: int) -> torch.Tensor:
    """Integer labels [N] as a contiguous int32 / int64 tensor on `device` (host labels are copied without blocking)."""
    if labels.dtype not in _SV_T:
        raise MirrorHipError(f"labels must be int32 or int64, got {labels.dtype}")
    if labels.numel() != N or labels.dim() > 1:
        raise MirrorHipError(f"labels must be [{N}], got {tuple(labels.shape)}")
    if not labels.is_cuda:
        labels = labels.to(device, non_blocking=True)
    return labels.reshape(-1).contiguous()


def _cls_logits(logits: torch.Tensor) -> torch.Tensor:
    _chk(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise MirrorHipError(f"classification logits must be f32 [N, C], got {logits.dtype} {tuple(logits.shape)}")
    if logits.shape[0] < 1 or logits.shape[1] < 1:
        raise MirrorHipError(f"classification logits must be non-empty, got {tuple(logits.shape)}")
    if logits.stride(1) != 1 and logits.shape[1] > 1:
        logits = logits.contiguous()
    return logits


def cls_ce_fwd(logits, labels, smoothing: float, ignore_index: int, mode: int, rows: Optional[torch.Tensor],
               out: Optional[torch.Tensor]) -> None:
    """rows [N] (optional unless mode is "none") = per-row losses; out [1] = their sum, or mean over the non-ignored rows."""
    logits = _cls_logits(logits)
    N, C = logits.shape
    t = cls_labels(labels, logits.device, N)
    _chk(out, rows)
    assert out is None or (out.dtype == torch.float32 and out.numel() >= 1)
    assert rows is None or (rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() == N)
    _lib.call("mh_cls_ce_fwd", _p(logits), _ld(logits), _p(t), _SV_T[t.dtype], N, C, smoothing, ignore_index, _p(rows), _p(out), mode,
              stream=_stream())


def cls_ce_bwd(logits, labels, smoothing: float, ignore_index: int, g: torch.Tensor, mode: int) -> torch.Tensor:
    """dlogits [N, C] f32 for the upstream g (one element, or one per row for mode "none")."""
    logits = _cls_logits(logits)
    N, C = logits.shape
    t = cls_labels(labels, logits.device, N)
    _chk(g)
    g = g.reshape(-1).contiguous().float()
    if g.numel() != (N if mode == CLS_RED["none"] else 1):
        raise MirrorHipError(f"cross-entropy upstream gradient has {g.numel()} elements for N = {N}, mode {mode}")
    dx = torch.empty((N, C), device=logits.device, dtype=torch.float32)
    _lib.call("mh_cls_ce_bwd", _p(logits), _ld(logits), _p(t), _SV_T[t.dtype], N, C, smoothing, ignore_index, _p(g), mode, _p(dx),
              stream=_stream())
    return dx


def cls_confusion(inp: torch.Tensor, labels: torch.Tensor, conf: torch.Tensor, bad: torch.Tensor) -> None:
    """conf [C, C] int64 += counts of (label, prediction) pairs; bad [1] int64 += rows with a label or prediction outside [0, C).
    inp: f32 scores [N, C] (prediction = first argmax) or int32 / int64 predicted labels [N]."""
    _chk(inp, conf, bad)
    C = conf.shape[0]
    assert conf.dtype == torch.int64 and conf.is_contiguous() and tuple(conf.shape) == (C, C)
    assert bad.dtype == torch.int64 and bad.numel() >= 1
    if inp.dim() == 2:
        if inp.dtype != torch.float32 or inp.shape[1] != C:
            raise MirrorHipError(f"scores must be f32 [N, {C}], got {inp.dtype} {tuple(inp.shape)}")
        if inp.stride(1) != 1 and C > 1:
            inp = inp.contiguous()
        dt_in, ld = 3, _ld(inp)
    elif inp.dim() == 1 and inp.dtype in _SV_T:
        inp, dt_in, ld = inp.contiguous(), _SV_T[inp.dtype], 0
    else:
        raise MirrorHipError(f"input must be f32 scores [N, C] or integer predictions [N], got {inp.dtype} {tuple(inp.shape)}")
    N = inp.shape[0]
    if N == 0:
        return
    t = cls_labels(labels, inp.device, N)
    _lib.call("mh_cls_confusion", _p(inp), ld, dt_in, _p(t), _SV_T[t.dtype], N, C, _p(conf), _p(bad), stream=_stream())


def auroc_counts(scores: torch.Tensor, labels_i64: torch.Tensor) -> torch.Tensor:
    """int64 [C, 4] {U2, P, Q, NaN count} per class on the device (no sync); scores f32 [N, C], labels int64 [N] on the device."""
    _chk(scores, labels_i64)
    assert scores.dim() == 2 and scores.dtype == torch.float32 and labels_i64.dtype == torch.int64
    if scores.stride(1) != 1:
        scores = scores.contiguous()
    labels_i64 = labels_i64.contiguous()
    N, C = scores.shape
    if not (1 <= N <= (1 << 20)) or not (2 <= C <= 1024) or labels_i64.numel() != N:
        raise MirrorHipError(f"auroc_counts: N = {N} (1..2^20), C = {C} (2..1024), {labels_i64.numel()} labels")
    counts = torch.empty((C, 4), device=scores.device, dtype=torch.int64)
    _lib.call("mh_auroc_counts", _p(scores), _ld(scores), _p(labels_i64), N, C, _p(counts), stream=_stream())
    return counts


def auroc_counts_many(scores: torch.Tensor, labels: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [E, C, 4] {U2, P, Q, NaN count} per (table, class) on the device (no sync): mh_auroc_counts of each of the E tables of
    scores f32 [E, N, C] against the one label vector int64 [N], in one launch (mh_auroc_counts_many).  scores may be a view with unit
    stride along the classes (row stride >= C, table stride >= N rows); counts may be passed to be overwritten."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 3 or scores.dtype != torch.float32:
        got = f"{scores.dtype} {tuple(scores.shape)}" if isinstance(scores, torch.Tensor) else type(scores).__name__
        raise ValueError(f"auroc_counts_many: scores must be f32 [E, N, C], got {got}")
    E, N, C = scores.shape
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"auroc_counts_many: labels must be int64 [{N}]")
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != (E, C, 4)
                               or not counts.is_contiguous()):
        raise ValueError(f"auroc_counts_many: counts must be a contiguous int64 [{E}, {C}, 4]")
    _chk(scores, labels, counts)
    if not (1 <= N <= (1 << 20)) or not (2 <= C <= 1024) or not (1 <= E and E * C <= 65535):
        raise MirrorHipError(f"auroc_counts_many: N = {N} (1..2^20), C = {C} (2..1024), E = {E} tables (E * C <= 65535)")
    scores = scores.detach()
    ld_row = scores.stride(1) if N > 1 else C
    ld_table = scores.stride(0) if E > 1 else N * ld_row
    if scores.stride(2) != 1 or ld_row < C or ld_table < N * ld_row:
        scores = scores.contiguous()
        ld_row, ld_table = C, N * C
    if counts is None:
        counts = torch.empty((E, C, 4), device=scores.device, dtype=torch.int64)
    _lib.call("mh_auroc_counts_many", _p(scores), ld_row, ld_table, _p(labels.contiguous()), N, C, E, _p(counts), stream=_stream())
    return counts


# ----------------------------------------------------------------------------- InfoNCE with explicit negative keys (csrc/infonce.hip)
def _nce_f32(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise MirrorHipError(f"infonce: {name} must be contiguous f32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t


def _nce_paired(qn: torch.Tensor, neg: torch.Tensor):
    _chk(qn, neg)
    if neg.dim() != 3 or not neg.is_contiguous():
        raise MirrorHipError(f"infonce: paired negative_keys must be contiguous [N, M, D], got {tuple(neg.shape)} strides {neg.stride()}")
    N, M, D = neg.shape
    _nce_f32(qn, (N, D), "the normalised query")
    if N < 1 or M < 1 or D < 1 or N > 65535 or N * M >= (1 << 31):
        raise MirrorHipError(f"infonce: paired negative_keys {tuple(neg.shape)}: need 1 <= N <= 65535, M, D >= 1 and N * M < 2^31")
    return N, M, D


def infonce_paired_fwd(qn: torch.Tensor, neg: torch.Tensor, eps: float):
    """(cos, inv) f32 [N, M]: cos[i, j] = qn[i] . neg[i, j] / max(|neg[i, j]|, eps), inv = 1 / max(|neg[i, j]|, eps); neg is read once,
    in its own dtype."""
    N, M, D = _nce_paired(qn, neg)
    cosv = torch.empty((N, M), device=neg.device, dtype=torch.float32)
    inv = torch.empty((N, M), device=neg.device, dtype=torch.float32)
    _lib.call("mh_infonce_paired_fwd", _p(qn), _p(neg), _p(cosv), _p(inv), N, M, D, eps, dt(neg), stream=_stream())
    return cosv, inv


def infonce_paired_chunk(N: int, M: int, D: int) -> int:
    """Rows j one workgroup of the paired backward walks: 16..256, small enough for ~2048 workgroups where the shape allows it
    (every chunk costs one [D] partial row of the query gradient)."""
    jc = 256
    while jc > 16 and N * -(-M // jc) < 2048:
        jc //= 2
    return jc


def infonce_paired_bwd(qn, neg, cosv, inv, dl, want_dneg: bool, want_dq: bool):
    """(dneg or None, dq_part or None): dneg like neg; dq_part f32 [N, chunks, D] for infonce_fold.  neg is read once."""
    N, M, D = _nce_paired(qn, neg)
    for t, nm in ((cosv, "cos"), (inv, "inv"), (dl, "dl")):
        _chk(t)
        _nce_f32(t, (N, M), nm)
    if not (want_dneg or want_dq):
        raise MirrorHipError("infonce_paired_bwd: nothing to compute")
    jc = infonce_paired_chunk(N, M, D)
    dneg = torch.empty_like(neg) if want_dneg else None
    part = torch.empty((N, -(-M // jc), D), device=neg.device, dtype=torch.float32) if want_dq else None
    _lib.call("mh_infonce_paired_bwd", _p(qn), _p(neg), _p(cosv), _p(inv), _p(dl), _p(dneg), _p(part), N, M, D, jc, dt(neg),
              stream=_stream())
    return dneg, part


def infonce_bank_split(M: int) -> int:
    """Slices S (a power of two <= 64 that divides M, slices of >= 256 rows) the unpaired query gradient dl @ bank is split into."""
    S = 1
    while S < 64 and M % (2 * S) == 0 and M // (2 * S) >= 256:
        S *= 2
    return S


def infonce_rows_fwd(qn, kn, neg, inv_t: float, coef: float, reduce: bool):
    """Label-0 cross-entropy of [qn . kn | neg] * inv_t.  neg f32 [N, M] (unit column stride).  Returns (pneg, lse, rows, out): f32 [N]
    each (pneg = 1 - softmax[:, 0]), out f32 [1] = coef * sum(rows) (None unless reduce)."""
    _chk(qn, kn, neg)
    if neg.dim() != 2 or neg.dtype != torch.float32 or (neg.stride(1) != 1 and neg.shape[1] > 1):
        raise MirrorHipError(f"infonce: cosines must be f32 [N, M] with unit column stride, got {neg.dtype} {tuple(neg.shape)}")
    N, M = neg.shape
    D = qn.shape[1]
    _nce_f32(qn, (N, D), "the normalised query")
    _nce_f32(kn, (N, D), "the normalised positive key")
    if N < 1 or M < 1 or D < 1:
        raise MirrorHipError(f"infonce: empty operand N={N} M={M} D={D}")
    pneg, lse, rows = (torch.empty((N,), device=neg.device, dtype=torch.float32) for _ in range(3))
    out = torch.empty((1,), device=neg.device, dtype=torch.float32) if reduce else None
    _lib.call("mh_infonce_rows_fwd", _p(qn), _p(kn), _p(neg), _ld(neg), N, M, D, inv_t, coef, _p(pneg), _p(lse), _p(rows), _p(out),
              stream=_stream())
    return pneg, lse, rows, out


def infonce_rows_bwd(neg, pneg, lse, g, gcoef: float, inv_t: float):
    """(dl f32 [N, M], dpos f32 [N]) for the upstream gcoef * g (g: one element, or one per row)."""
    _chk(neg, pneg, lse, g)
    N, M = neg.shape
    if N > 65535:
        raise MirrorHipError(f"infonce: N = {N} exceeds 65535 rows")
    _nce_f32(pneg, (N,), "pneg")
    _nce_f32(lse, (N,), "lse")
    g = g.reshape(-1).contiguous().float()
    if g.numel() not in (1, N):
        raise MirrorHipError(f"infonce: upstream gradient must have 1 or {N} elements, got {g.numel()}")
    dl = torch.empty((N, M), device=neg.device, dtype=torch.float32)
    dpos = torch.empty((N,), device=neg.device, dtype=torch.float32)
    _lib.call("mh_infonce_rows_bwd", _p(neg), _ld(neg), _p(pneg), _p(lse), _p(g), int(g.numel() == N and N > 1), gcoef, inv_t, N, M,
              _p(dl), _p(dpos), stream=_stream())
    return dl, dpos


def infonce_fold(dpos, qn, kn, part: Optional[torch.Tensor], want_dq: bool, want_dk: bool):
    """(dq, dk) f32 [N, D] (None where not wanted): dq = dpos[:, None] * kn + part.sum(1), dk = dpos[:, None] * qn."""
    _chk(dpos, qn, kn, part)
    N, D = qn.shape
    _nce_f32(kn, (N, D), "the normalised positive key")
    _nce_f32(dpos, (N,), "dpos")
    nparts = 0
    if want_dq:
        if part is None or part.dim() != 3 or part.shape[0] != N or part.shape[2] != D:
            raise MirrorHipError("infonce_fold: the query gradient needs its partial sums [N, parts, D]")
        nparts = part.shape[1]
        _nce_f32(part, (N, nparts, D), "part")
    dq = torch.empty((N, D), device=qn.device, dtype=torch.float32) if want_dq else None
    dk = torch.empty((N, D), device=qn.device, dtype=torch.float32) if want_dk else None
    _lib.call("mh_infonce_fold", _p(dpos), _p(qn), _p(kn), _p(part) if want_dq else None, nparts, _p(dq), _p(dk), N, D, stream=_stream())
    return dq, dk


# ----------------------------------------------------------------------------- cross-modal retrieval (csrc/retrieval.hip)
def retrieval_ranks(q: torch.Tensor, k: torch.Tensor, target: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [nq] on the device (no sync): ranks[i] = 1 + #{j != target[i]: not (q[i] . k[j] < q[i] . k[target[i]])}, the rank of each
    query's positive among the nk keys with ties and NaN counted against the query.  q f32 [nq, D], k f32 [nk, D] on the device;
    target int32 / int64 [nq] (None: the identity, needs nq == nk).  A host `target` is range-checked here (ValueError) and copied
    over; a device `target` is NOT checked (that would wait on the host) and the kernel clamps nothing: an entry outside [0, nk)
    reads no key and gives rank nk + 1.  The [nq, nk] similarities are never stored: the only allocations are the result and an
    f32 [nq] workspace."""
    if q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"retrieval_ranks: q [nq, D] and k [nk, D] must share D, got {tuple(q.shape)} and {tuple(k.shape)}")
    nq, D = q.shape
    nk = k.shape[0]
    if target is None and nq != nk:
        raise ValueError(f"retrieval_ranks: without a target the positives are the diagonal, which needs nq == nk (got {nq}, {nk})")
    if target is not None:
        if target.dim() != 1 or target.numel() != nq or target.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"retrieval_ranks: target must be int32 / int64 [{nq}], got {target.dtype} {tuple(target.shape)}")
        if not target.is_cuda and nq and (int(target.min()) < 0 or int(target.max()) >= nk):
            raise ValueError(f"retrieval_ranks: target holds entries outside [0, {nk})")
    _chk(q, k)
    if q.dtype != torch.float32 or k.dtype != torch.float32:
        raise MirrorHipError(f"retrieval_ranks: q and k must be f32 (ranks decided by a bf16 rounding are not a metric), got {q.dtype}, {k.dtype}")
    if not (1 <= nq <= (1 << 20)) or not (1 <= nk <= (1 << 20)) or not (1 <= D <= 4096):
        raise MirrorHipError(f"retrieval_ranks: nq = {nq}, nk = {nk} (1..2^20), D = {D} (1..4096)")
    q, k = q.detach().contiguous(), k.detach().contiguous()
    if target is not None:
        target = target.to(device=q.device, dtype=torch.int64, non_blocking=True).contiguous()
    ranks = torch.empty((nq,), device=q.device, dtype=torch.int32)
    ws_bytes = int(_lib.load().mh_retrieval_workspace_bytes(nq, nk, D))
    ws = torch.empty(((ws_bytes + 3) // 4,), device=q.device, dtype=torch.float32)
    _lib.call("mh_retrieval_ranks", _p(q), _p(k), nq, nk, D, _p(target), _p(ranks), _p(ws), stream=_stream())
    return ranks


def _retrieval_ids(ids: torch.Tensor, n: int, what: str, who: str = "retrieval_ranks_grouped") -> None:
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.numel() != n or ids.dtype not in (torch.int32, torch.int64):
        got = f"{ids.dtype} {tuple(ids.shape)}" if isinstance(ids, torch.Tensor) else type(ids).__name__
        raise ValueError(f"{who}: {what} must be int32 / int64 [{n}], got {got}")


def retrieval_ranks_grouped(q: torch.Tensor, k: torch.Tensor, qgroup: torch.Tensor, kgroup: torch.Tensor,
                            kcount: Optional[torch.Tensor] = None, key_order=None) -> torch.Tensor:
    """int32 [nq] on the device (no sync): the rank of the BEST positive of each query among the keys of other groups.  The positives
    of query i are the keys j with kgroup[j] == qgroup[i] (ids compared for equality only, all 64 bits; int32 ids are widened):
        d[i] = max over them of q[i] . k[j]  (NaN if there is none, or if one of them is NaN),
        ranks[i] = 1 + #{j of another group with kcount[j] != 0: not (q[i] . k[j] < d[i])}.
    kcount (bool or integer [nk], None: every key counts) never removes a positive; it only says which other keys can count.  Ties and
    NaN count against the query as in retrieval_ranks; a copy of the best positive in the query's own group does not.  q f32 [nq, D],
    k f32 [nk, D] on the device; the ids may come from the host.  The keys are ordered by group with one stable device sort (no sync);
    key_order = torch.sort(kgroup as int64 on the device, stable=True) hands over a sort the caller already has."""
    if q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"retrieval_ranks_grouped: q [nq, D] and k [nk, D] must share D, got {tuple(q.shape)} and {tuple(k.shape)}")
    nq, D = q.shape
    nk = k.shape[0]
    _retrieval_ids(qgroup, nq, "qgroup")
    _retrieval_ids(kgroup, nk, "kgroup")
    if kcount is not None and (not isinstance(kcount, torch.Tensor) or kcount.dim() != 1 or kcount.numel() != nk
                               or kcount.is_floating_point() or kcount.is_complex()):
        got = f"{kcount.dtype} {tuple(kcount.shape)}" if isinstance(kcount, torch.Tensor) else type(kcount).__name__
        raise ValueError(f"retrieval_ranks_grouped: kcount must be a bool / integer [{nk}], got {got}")
    _chk(q, k)
    if q.dtype != torch.float32 or k.dtype != torch.float32:
        raise MirrorHipError(f"retrieval_ranks_grouped: q and k must be f32 (ranks decided by a bf16 rounding are not a metric), got {q.dtype}, {k.dtype}")
    if not (1 <= nq <= (1 << 20)) or not (1 <= nk <= (1 << 20)) or not (1 <= D <= 4096):
        raise MirrorHipError(f"retrieval_ranks_grouped: nq = {nq}, nk = {nk} (1..2^20), D = {D} (1..4096)")
    q, k = q.detach().contiguous(), k.detach().contiguous()
    qgroup = qgroup.to(device=q.device, dtype=torch.int64, non_blocking=True).contiguous()
    kgroup = kgroup.to(device=q.device, dtype=torch.int64, non_blocking=True).contiguous()
    if kcount is not None:
        kcount = (kcount.to(device=q.device, non_blocking=True) != 0).to(torch.uint8).contiguous()
    if key_order is None:
        key_order = torch.sort(kgroup, stable=True)
    sgroup, perm = key_order
    for t, what in ((sgroup, "sorted ids"), (perm, "permutation")):
        if t.dtype != torch.int64 or tuple(t.shape) != (nk,) or t.device != q.device:
            raise ValueError(f"retrieval_ranks_grouped: key_order's {what} must be int64 [{nk}] on {q.device}")
    sgroup, perm = sgroup.contiguous(), perm.contiguous()
    ranks = torch.empty((nq,), device=q.device, dtype=torch.int32)
    ws_bytes = int(_lib.load().mh_retrieval_workspace_bytes(nq, nk, D))
    ws = torch.empty(((ws_bytes + 3) // 4,), device=q.device, dtype=torch.float32)
    _lib.call("mh_retrieval_ranks_grouped", _p(q), _p(k), nq, nk, D, _p(qgroup), _p(kgroup), _p(sgroup), _p(perm), _p(kcount), _p(ranks),
              _p(ws), stream=_stream())
    return ranks


# ----------------------------------------------------------------------------- top-k retrieval and the kNN vote (csrc/retrieval_topk.hip)
def retrieval_topk(q: torch.Tensor, k: torch.Tensor, kk: int, qgroup: Optional[torch.Tensor] = None,
                   kgroup: Optional[torch.Tensor] = None, parts: int = 0):
    """(val f32 [nq, kk], idx int32 [nq, kk]) on the device (no sync): for every query the kk eligible keys with the largest q[i] . k[j],
    best first, equal similarities by the smaller key index.  Key j is eligible for query i unless the similarity is NaN or, with
    qgroup [nq] / kgroup [nk] (int32 / int64, both or neither; int32 ids are widened, the host's are copied over), kgroup[j] == qgroup[i].
    Slots beyond the eligible keys hold idx -1, val -inf.  val is the f32 fmaf chain retrieval_ranks decides by, bit for bit.
    q f32 [nq, D], k f32 [nk, D] on the device, 1 <= kk <= 64 (kk > nk is allowed).  parts: the number of key strips (0: the library
    chooses; the result does not depend on it).  The [nq, nk] similarities are never stored: the allocations are the two results and
    the strips' lists [nq, parts, kk]."""
    if q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"retrieval_topk: q [nq, D] and k [nk, D] must share D, got {tuple(q.shape)} and {tuple(k.shape)}")
    nq, D = q.shape
    nk = k.shape[0]
    if isinstance(kk, bool) or not isinstance(kk, int) or not (1 <= kk <= 64):
        raise ValueError(f"retrieval_topk: kk must be an int in [1, 64], got {kk!r}")
    if isinstance(parts, bool) or not isinstance(parts, int) or parts < 0:
        raise ValueError(f"retrieval_topk: parts must be an int >= 0, got {parts!r}")
    if (qgroup is None) != (kgroup is None):
        raise ValueError("retrieval_topk: qgroup and kgroup go together")
    if qgroup is not None:
        _retrieval_ids(qgroup, nq, "qgroup", "retrieval_topk")
        _retrieval_ids(kgroup, nk, "kgroup", "retrieval_topk")
    _chk(q, k)
    if q.dtype != torch.float32 or k.dtype != torch.float32:
        raise MirrorHipError(f"retrieval_topk: q and k must be f32 (neighbours decided by a bf16 rounding are not a metric), got {q.dtype}, {k.dtype}")
    if not (1 <= nq <= (1 << 20)) or not (1 <= nk <= (1 << 20)) or not (1 <= D <= 4096):
        raise MirrorHipError(f"retrieval_topk: nq = {nq}, nk = {nk} (1..2^20), D = {D} (1..4096)")
    q, k = q.detach().contiguous(), k.detach().contiguous()
    if qgroup is not None:
        qgroup = qgroup.to(device=q.device, dtype=torch.int64, non_blocking=True).contiguous()
        kgroup = kgroup.to(device=q.device, dtype=torch.int64, non_blocking=True).contiguous()
    idx = torch.empty((nq, kk), device=q.device, dtype=torch.int32)
    val = torch.empty((nq, kk), device=q.device, dtype=torch.float32)
    ws_bytes = int(_lib.load().mh_retrieval_topk_workspace_bytes(nq, nk, D, kk, parts))
    ws = torch.empty(((ws_bytes + 7) // 8,), device=q.device, dtype=torch.int64)
    _lib.call("mh_retrieval_topk", _p(q), _p(k), nq, nk, D, kk, _p(qgroup), _p(kgroup), parts, _p(idx), _p(val), _p(ws), stream=_stream())
    return val, idx


def knn_scores(idx: torch.Tensor, val: torch.Tensor, labels: torch.Tensor, num_classes: int, inv_temperature: float) -> torch.Tensor:
    """f32 [nq, C] on the device (no sync): the temperature-weighted vote of a retrieval_topk result,
        score[i, c] = sum_s [labels[idx[i, s]] == c] exp((val[i, s] - val[i, 0]) inv_temperature) / the row's total,
    summed in slot order.  Empty slots (idx -1) and labels outside [0, C) contribute nothing, a row without contribution is all zeros,
    every other row sums to 1; inv_temperature = 0 is the unweighted vote.  idx int32 [nq, kk], val f32 [nq, kk] on the device, labels
    int32 / int64 [nk] (the bank's; the host's are copied over), 1 <= kk <= 64, 1 <= C <= 1024."""
    if not isinstance(idx, torch.Tensor) or not isinstance(val, torch.Tensor) or idx.dim() != 2 or tuple(idx.shape) != tuple(val.shape):
        raise ValueError("knn_scores: idx and val must both be [nq, kk]")
    if idx.dtype != torch.int32 or val.dtype != torch.float32:
        raise ValueError(f"knn_scores: idx must be int32 and val f32, got {idx.dtype}, {val.dtype}")
    nq, kk = idx.shape
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise ValueError(f"knn_scores: labels must be an int32 / int64 [nk] tensor, got {got}")
    nk = labels.numel()
    C = num_classes
    if isinstance(C, bool) or not isinstance(C, int) or not (1 <= C <= 1024):
        raise ValueError(f"knn_scores: num_classes must be an int in [1, 1024], got {C!r}")
    if not (1 <= kk <= 64):
        raise ValueError(f"knn_scores: kk = {kk} outside [1, 64]")
    inv_t = float(inv_temperature)
    if not (0.0 <= inv_t < float("inf")):
        raise ValueError(f"knn_scores: inv_temperature must be finite and >= 0, got {inv_temperature!r}")
    _chk(idx, val)
    if not (1 <= nq <= (1 << 20)) or not (1 <= nk <= (1 << 20)):
        raise MirrorHipError(f"knn_scores: nq = {nq}, nk = {nk} (1..2^20)")
    idx, val = idx.contiguous(), val.detach().contiguous()
    labels = labels.to(device=idx.device, dtype=torch.int64, non_blocking=True).contiguous()
    scores = torch.empty((nq, C), device=idx.device, dtype=torch.float32)
    _lib.call("mh_knn_scores", _p(idx), _p(val), _p(labels), nq, nk, kk, C, inv_t, _p(scores), stream=_stream())
    return scores


# ----------------------------------------------------------------------------- few-shot prototype probe (csrc/fewshot.hip)
FEWSHOT_METRIC = {"euclidean": 0, "cosine": 1}


def _fs_f32(t: torch.Tensor, what: str, device: bool = True) -> torch.Tensor:
    """device=False leaves the device check to the caller, who looks at every argument's type and shape first."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what} must be f32 [n, D], got {got}")
    if device:
        _chk(t)
    n, D = t.shape
    if not (1 <= n <= (1 << 20)) or not (1 <= D <= 4096):
        raise MirrorHipError(f"{what}: n = {n} (1..2^20), D = {D} (1..4096)")
    return t.detach().contiguous()


def fewshot_cp(C: int) -> int:
    """Key slots per episode: the next power of two >= C (pads hold 0 / -inf)."""
    return 1 << (int(C) - 1).bit_length()


def colmean(x: torch.Tensor) -> torch.Tensor:
    """f32 [D] on the device (no sync): the column means of x f32 [n, D], summed in a fixed order in f64 (mh_colmean)."""
    x = _fs_f32(x, "colmean: x")
    n, D = x.shape
    mu = torch.empty((D,), device=x.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.load().mh_colmean_workspace_bytes(n, D)) // 8,), device=x.device, dtype=torch.float64)
    _lib.call("mh_colmean", _p(x), n, D, _p(mu), _p(ws), stream=_stream())
    return mu


def center_l2norm(x: torch.Tensor, mu: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """f32 [n, D]: rows (x - mu) / max(|x - mu|, eps) (mh_center_l2norm)."""
    x = _fs_f32(x, "center_l2norm: x")
    n, D = x.shape
    if not isinstance(mu, torch.Tensor) or mu.dtype != torch.float32 or tuple(mu.shape) != (D,):
        raise ValueError(f"center_l2norm: mu must be f32 [{D}]")
    _chk(mu)
    y = torch.empty_like(x)
    _lib.call("mh_center_l2norm", _p(x), _p(mu.contiguous()), _p(y), n, D, float(eps), stream=_stream())
    return y


def fewshot_protos(y: torch.Tensor, rows: torch.Tensor, perm: Optional[torch.Tensor], metric: str):
    """(protos f32 [E, Cp, D], bias f32 [E, Cp] or None for "cosine") on the device (no sync): the means of the K support rows
    rows [E, C, K] (int64) of the prepared pool y f32 [n, D], through perm int64 [n] when given (mh_fewshot_protos: k-ordered f32 sums,
    pads 0 / -inf, an index outside the pool makes that prototype NaN)."""
    y = _fs_f32(y, "fewshot_protos: y")
    n, D = y.shape
    if metric not in FEWSHOT_METRIC:
        raise ValueError(f'fewshot_protos: metric must be "euclidean" or "cosine", got {metric!r}')
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or rows.dtype != torch.int64:
        got = f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"fewshot_protos: rows must be int64 [E, C, K], got {got}")
    E, C, Kk = rows.shape
    if perm is not None and (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or tuple(perm.shape) != (n,)):
        raise ValueError(f"fewshot_protos: perm must be int64 [{n}]")
    _chk(rows, perm)
    Cp = fewshot_cp(C) if C >= 1 else 1
    if not (2 <= C <= 64) or not (1 <= Kk <= 1024) or not (1 <= E and E * Cp <= (1 << 20)):
        raise MirrorHipError(f"fewshot_protos: C = {C} (2..64), K = {Kk} (1..1024), E = {E} (E * {Cp} <= 2^20)")
    rows = rows.contiguous()
    perm = None if perm is None else perm.contiguous()
    protos = torch.empty((E, Cp, D), device=y.device, dtype=torch.float32)
    bias = torch.empty((E, Cp), device=y.device, dtype=torch.float32) if metric == "euclidean" else None
    _lib.call("mh_fewshot_protos", _p(y), n, _p(rows), _p(perm), E, C, Cp, Kk, D, FEWSHOT_METRIC[metric], _p(protos), _p(bias), stream=_stream())
    return protos, bias


def fewshot_predict(q: torch.Tensor, protos: torch.Tensor, bias: Optional[torch.Tensor], C: int) -> torch.Tensor:
    """int32 [E, nq] on the device (no sync): per episode the class with the largest q[i] . protos[e, c] (+ bias[e, c]), NaN scores not
    eligible, ties to the smaller class, -1 when none is eligible (mh_fewshot_predict: the retrieval kernels' exact-f32 tile product;
    the [nq, E Cp] scores are never stored)."""
    q = _fs_f32(q, "fewshot_predict: q")
    nq, D = q.shape
    if isinstance(C, bool) or not isinstance(C, int) or not (2 <= C <= 64):
        raise ValueError(f"fewshot_predict: C must be an int in [2, 64], got {C!r}")
    Cp = fewshot_cp(C)
    if not isinstance(protos, torch.Tensor) or protos.dtype != torch.float32 or protos.dim() != 3 or tuple(protos.shape[1:]) != (Cp, D):
        raise ValueError(f"fewshot_predict: protos must be f32 [E, {Cp}, {D}]")
    E = protos.shape[0]
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (E, Cp)):
        raise ValueError(f"fewshot_predict: bias must be f32 [{E}, {Cp}]")
    _chk(protos, bias)
    if not (1 <= E and E * Cp <= (1 << 20)):
        raise MirrorHipError(f"fewshot_predict: E = {E} episodes of {Cp} keys outside [1, 2^20] keys")
    protos = protos.contiguous()
    bias = None if bias is None else bias.contiguous()
    pred = torch.empty((E, nq), device=q.device, dtype=torch.int32)
    _lib.call("mh_fewshot_predict", _p(q), _p(protos), _p(bias), nq, E, C, Cp, D, _p(pred), stream=_stream())
    return pred


def fewshot_tally(pred: torch.Tensor, labels: torch.Tensor, C: int):
    """(conf int32 [E, C, C], bad int32 [E], summary f64 [E, 3]) on the device (no sync): per episode the confusion counts
    [label, prediction] of pred int32 [E, nq] against labels int64 [nq], the rows left out (label outside [0, C) or prediction -1), and
    {accuracy %, balanced accuracy %, macro F1} from the integer counts (mh_fewshot_tally)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 2 or pred.dtype != torch.int32:
        raise ValueError("fewshot_tally: pred must be int32 [E, nq]")
    E, nq = pred.shape
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (nq,):
        raise ValueError(f"fewshot_tally: labels must be int64 [{nq}]")
    if isinstance(C, bool) or not isinstance(C, int) or not (2 <= C <= 64):
        raise ValueError(f"fewshot_tally: C must be an int in [2, 64], got {C!r}")
    _chk(pred, labels)
    if not (1 <= E <= (1 << 20)) or not (1 <= nq <= (1 << 20)):
        raise MirrorHipError(f"fewshot_tally: E = {E}, nq = {nq} (1..2^20)")
    pred, labels = pred.contiguous(), labels.contiguous()
    conf = torch.empty((E, C, C), device=pred.device, dtype=torch.int32)
    bad = torch.empty((E,), device=pred.device, dtype=torch.int32)
    summary = torch.empty((E, 3), device=pred.device, dtype=torch.float64)
    _lib.call("mh_fewshot_tally", _p(pred), _p(labels), nq, E, C, _p(conf), _p(bad), _p(summary), stream=_stream())
    return conf, bad, summary


# ----------------------------------------------------------------------------- linear probe: J softmax regressions at once (csrc/linprobe.hip)
def _lp_state(y: torch.Tensor, W: torch.Tensor, b: torch.Tensor, C: int, who: str):
    """(n, D, J, Cp) of prepared rows y f32 [n, D] and padded weights W f32 [J, Cp, D], b f32 [J, Cp], inside the limits the two entry
    points share."""
    y = _fs_f32(y, f"{who}: y", device=False)
    n, D = y.shape
    if isinstance(C, bool) or not isinstance(C, int) or not (2 <= C <= 64):
        raise ValueError(f"{who}: C must be an int in [2, 64], got {C!r}")
    Cp = fewshot_cp(C)
    if not isinstance(W, torch.Tensor) or W.dtype != torch.float32 or W.dim() != 3 or tuple(W.shape[1:]) != (Cp, D):
        raise ValueError(f"{who}: the weights must be f32 [J, {Cp}, {D}]")
    J = W.shape[0]
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or tuple(b.shape) != (J, Cp):
        raise ValueError(f"{who}: the bias must be f32 [{J}, {Cp}]")
    _chk(y, W, b)
    if not (1 <= J and J * Cp <= (1 << 20)) or n * J * Cp > (1 << 28):
        raise MirrorHipError(f"{who}: J = {J} jobs of {Cp} keys over n = {n} rows (J * Cp <= 2^20, n * J * Cp <= 2^28)")
    _contig(W, f"{who}: the weights")
    _contig(b, f"{who}: the bias")
    return y, n, D, J, Cp


def _lp_vec(t, dtype, J: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (J,):
        raise ValueError(f"{what} must be {dtype} [{J}]")
    _chk(t)
    return t.contiguous()


def linprobe_grad(y: torch.Tensor, Wz: torch.Tensor, bz: torch.Tensor, labels: torch.Tensor, fold: torch.Tensor, heldout: torch.Tensor,
                  rscale: torch.Tensor, C: int, G: Optional[torch.Tensor] = None, want_loss: bool = False):
    """(G f32 [n, J Cp], loss_part f64 [ceil(n / 128), J] or None) on the device (no sync): every job's logit gradient
    r_j (softmax(Wz y_i + bz) - onehot(label_i)) over its training rows (label in [0, C), fold >= 0, fold != heldout_j), 0 elsewhere
    and in the pad columns (mh_linprobe_grad).  G may be passed to be overwritten; want_loss asks for the per-row-tile data terms."""
    y, n, D, J, Cp = _lp_state(y, Wz, bz, C, "linprobe_grad")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
        raise ValueError(f"linprobe_grad: labels must be int64 [{n}]")
    if not isinstance(fold, torch.Tensor) or fold.dtype != torch.int32 or tuple(fold.shape) != (n,):
        raise ValueError(f"linprobe_grad: fold must be int32 [{n}]")
    _chk(labels, fold)
    heldout = _lp_vec(heldout, torch.int32, J, "linprobe_grad: heldout")
    rscale = _lp_vec(rscale, torch.float32, J, "linprobe_grad: rscale")
    tiles = (n + 127) // 128
    if G is None:
        G = torch.empty((n, J * Cp), device=y.device, dtype=torch.float32)
    elif not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J * Cp) or not G.is_contiguous():
        raise ValueError(f"linprobe_grad: G must be a contiguous f32 [{n}, {J * Cp}]")
    _chk(G)
    loss_part = torch.empty((tiles, J), device=y.device, dtype=torch.float64) if want_loss else None
    _lib.call("mh_linprobe_grad", _p(y), n, D, _p(Wz), _p(bz), _p(labels.contiguous()), _p(fold.contiguous()), _p(heldout), _p(rscale),
              J, C, Cp, _p(G), _p(loss_part), stream=_stream())
    return G, loss_part


def linprobe_step(y: torch.Tensor, G: torch.Tensor, Wx: torch.Tensor, bx: torch.Tensor, Wz: torch.Tensor, bz: torch.Tensor,
                  lam: torch.Tensor, eta: torch.Tensor, beta: float, C: int, gmax_part: Optional[torch.Tensor] = None,
                  want_gmax: bool = False):
    """One FISTA update of every job IN PLACE (no sync): g = G^T [y, 1] + lam_j Wz (the bias unpenalised), X' = Wz - eta_j g,
    Z' = X' + beta (X' - Wx), stored over Wx / bx and Wz / bz; pad slots untouched (mh_linprobe_step: one row-ordered f32 chain per
    element).  Returns gmax_part f32 [ceil((D + 1) / 128), J] (max |g| per column tile and job) or None."""
    y, n, D, J, Cp = _lp_state(y, Wz, bz, C, "linprobe_step")
    _lp_state(y, Wx, bx, C, "linprobe_step")
    if Wx.shape[0] != J:
        raise ValueError(f"linprobe_step: Wx has {Wx.shape[0]} jobs, Wz {J}")
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J * Cp) or not G.is_contiguous():
        raise ValueError(f"linprobe_step: G must be a contiguous f32 [{n}, {J * Cp}]")
    _chk(G)
    lam = _lp_vec(lam, torch.float32, J, "linprobe_step: lam")
    eta = _lp_vec(eta, torch.float32, J, "linprobe_step: eta")
    beta = float(beta)
    if not (0.0 <= beta <= 1.0):
        raise ValueError(f"linprobe_step: beta must lie in [0, 1], got {beta!r}")
    tiles = (D + 1 + 127) // 128
    if gmax_part is None and want_gmax:
        gmax_part = torch.empty((tiles, J), device=y.device, dtype=torch.float32)
    elif gmax_part is not None and (not isinstance(gmax_part, torch.Tensor) or gmax_part.dtype != torch.float32
                                    or tuple(gmax_part.shape) != (tiles, J) or not gmax_part.is_contiguous()):
        raise ValueError(f"linprobe_step: gmax_part must be a contiguous f32 [{tiles}, {J}]")
    _chk(gmax_part)
    _lib.call("mh_linprobe_step", _p(y), n, D, _p(G), _p(Wx), _p(bx), _p(Wz), _p(bz), _p(lam), _p(eta), beta, J, C, Cp, _p(gmax_part),
              stream=_stream())
    return gmax_part


def linprobe_proba(q: torch.Tensor, W: torch.Tensor, b: torch.Tensor, C: int, labels: Optional[torch.Tensor] = None,
                   P: Optional[torch.Tensor] = None, want_nll: bool = False, nll_part: Optional[torch.Tensor] = None):
    """(P f32 [E, nq, C], nll_part f64 [ceil(nq / 128), E] or None) on the device (no sync): softmax(W_e q_i + b_e) of the prepared rows
    q f32 [nq, D] under the E jobs of the padded weights, with the logits, lse and expf(v - lse) of mh_linprobe_grad bit for bit
    (mh_linprobe_proba).  want_nll (or a passed nll_part) asks for the per-row-tile sums of lse - v_label over the rows with a label in
    [0, C) and needs labels int64 [nq].  P and nll_part may be passed to be overwritten."""
    q, nq, D, E, Cp = _lp_state(q, W, b, C, "linprobe_proba")
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (nq,)):
        raise ValueError(f"linprobe_proba: labels must be int64 [{nq}]")
    want_nll = want_nll or nll_part is not None
    if want_nll and labels is None:
        raise ValueError("linprobe_proba: the log-loss needs labels")
    tiles = (nq + 127) // 128
    if P is None:
        P = torch.empty((E, nq, C), device=q.device, dtype=torch.float32)
    elif not isinstance(P, torch.Tensor) or P.dtype != torch.float32 or tuple(P.shape) != (E, nq, C) or not P.is_contiguous():
        raise ValueError(f"linprobe_proba: P must be a contiguous f32 [{E}, {nq}, {C}]")
    if nll_part is None and want_nll:
        nll_part = torch.empty((tiles, E), device=q.device, dtype=torch.float64)
    elif nll_part is not None and (not isinstance(nll_part, torch.Tensor) or nll_part.dtype != torch.float64
                                   or tuple(nll_part.shape) != (tiles, E) or not nll_part.is_contiguous()):
        raise ValueError(f"linprobe_proba: nll_part must be a contiguous f64 [{tiles}, {E}]")
    _chk(labels, P, nll_part)
    _lib.call("mh_linprobe_proba", _p(q), nq, D, _p(W), _p(b), E, C, Cp, _p(None if labels is None else labels.contiguous()), _p(P),
              _p(nll_part), stream=_stream())
    return P, nll_part


# ----------------------------------------------------------------------------- survival linear probe: J hazard regressions at once (csrc/survprobe.hip)
def _sp_bins(M, who: str) -> int:
    if isinstance(M, bool) or not isinstance(M, int) or not (2 <= M <= 64):
        raise ValueError(f"{who}: M must be an int in [2, 64], got {M!r}")
    return M


def survprobe_grad(y: torch.Tensor, Wz: torch.Tensor, bz: torch.Tensor, bins: torch.Tensor, event: torch.Tensor, fold: torch.Tensor,
                   heldout: torch.Tensor, rscale: torch.Tensor, w_cens: float, M: int, G: Optional[torch.Tensor] = None,
                   want_loss: bool = False):
    """(G f32 [n, J Mp], loss_part f64 [ceil(n / 128), J] or None) on the device (no sync): every job's hazard logit gradient
    r_j w_i (sigmoid(Wz y_i + bz) - [t = T_i] e_i) over the bins t <= T_i of its training rows (bin in [0, M), event in {0, 1},
    fold >= 0, fold != heldout_j; w_i = 1 for an event, w_cens otherwise), exactly 0 elsewhere and in the pad columns
    (mh_survprobe_grad).  G may be passed to be overwritten; want_loss asks for the per-row-tile data terms."""
    _sp_bins(M, "survprobe_grad")
    n = _fs_f32(y, "survprobe_grad: y", device=False).shape[0]          # every type and shape first, the device last
    for t, dtype, name in ((bins, torch.int64, "bins"), (event, torch.uint8, "event"), (fold, torch.int32, "fold")):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,):
            raise ValueError(f"survprobe_grad: {name} must be {dtype} [{n}]")
    if isinstance(w_cens, bool) or not isinstance(w_cens, (int, float)) or not (0.0 <= float(w_cens) <= 1.0):
        raise ValueError(f"survprobe_grad: w_cens must lie in [0, 1], got {w_cens!r}")
    y, n, D, J, Mp = _lp_state(y, Wz, bz, M, "survprobe_grad")
    _chk(bins, event, fold)
    heldout = _lp_vec(heldout, torch.int32, J, "survprobe_grad: heldout")
    rscale = _lp_vec(rscale, torch.float32, J, "survprobe_grad: rscale")
    tiles = (n + 127) // 128
    if G is None:
        G = torch.empty((n, J * Mp), device=y.device, dtype=torch.float32)
    elif not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J * Mp) or not G.is_contiguous():
        raise ValueError(f"survprobe_grad: G must be a contiguous f32 [{n}, {J * Mp}]")
    _chk(G)
    loss_part = torch.empty((tiles, J), device=y.device, dtype=torch.float64) if want_loss else None
    _lib.call("mh_survprobe_grad", _p(y), n, D, _p(Wz), _p(bz), _p(bins.contiguous()), _p(event.contiguous()), _p(fold.contiguous()),
              _p(heldout), _p(rscale), float(w_cens), J, M, Mp, _p(G), _p(loss_part), stream=_stream())
    return G, loss_part


def survprobe_risk(q: torch.Tensor, W: torch.Tensor, b: torch.Tensor, M: int) -> torch.Tensor:
    """f32 [S, nq] on the device (no sync): per job s the risk -sum_t prod_{u <= t} sigmoid(-(W[s] q_i + b[s])_u) of every row of
    q f32 [nq, D] under padded weights W f32 [S, Mp, D], b f32 [S, Mp] (mh_survprobe_risk: the retrieval kernels' exact-f32 tile
    product; the [nq, S Mp] logits are never stored)."""
    _sp_bins(M, "survprobe_risk")
    q, nq, D, S, Mp = _lp_state(q, W, b, M, "survprobe_risk")
    risk = torch.empty((S, nq), device=q.device, dtype=torch.float32)
    _lib.call("mh_survprobe_risk", _p(q), nq, D, _p(W), _p(b), S, M, Mp, _p(risk), stream=_stream())
    return risk


# ----------------------------------------------------------------------------- ridge Cox probe: J partial-likelihood regressions at once (csrc/coxprobe.hip)
COXPROBE_MAX_N = 65536


def _cp_weights(W, D: int, what: str) -> int:
    if not isinstance(W, torch.Tensor) or W.dtype != torch.float32 or W.dim() != 2 or W.shape[1] != D:
        got = f"{W.dtype} {tuple(W.shape)}" if isinstance(W, torch.Tensor) else type(W).__name__
        raise ValueError(f"{what} must be f32 [J, {D}], got {got}")
    return int(W.shape[0])


def _cp_out(t, dtype, shape, what: str) -> None:
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous {dtype} {list(shape)}")


def coxprobe_workspace(n: int, J: int, device) -> torch.Tensor:
    """The f64 workspace of coxprobe_grad for n rows and J jobs (mh_coxprobe_workspace_bytes: 28 bytes per score), nothing to zero."""
    nbytes = int(_lib.load().mh_coxprobe_workspace_bytes(n, J))
    if nbytes < 0:
        raise MirrorHipError(f"coxprobe_grad: J = {J} jobs over n = {n} rows (1 <= n <= {COXPROBE_MAX_N}, n * J <= 2^24)")
    return torch.empty((nbytes // 8,), device=device, dtype=torch.float64)


def coxprobe_scores(q: torch.Tensor, W: torch.Tensor, V: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f32 [J, nq], job-major, on the device (no sync): V[j, i] = q_i . W[j] of the prepared rows q f32 [nq, D] under the weight rows
    W f32 [J, D] (mh_coxprobe_scores: the retrieval kernels' exact-f32 tile product, one key per job).  V may be passed to be
    overwritten."""
    q = _fs_f32(q, "coxprobe_scores: q", device=False)                    # every type and shape first, the device last
    nq, D = q.shape
    J = _cp_weights(W, D, "coxprobe_scores: the weights")
    _cp_out(V, torch.float32, (J, nq), "coxprobe_scores: V")
    _chk(q, W, V)
    if not (1 <= J <= (1 << 20)) or nq * J > (1 << 28):
        raise MirrorHipError(f"coxprobe_scores: J = {J} jobs over nq = {nq} rows (1 <= J <= 2^20, nq * J <= 2^28)")
    _contig(W, "coxprobe_scores: the weights")
    if V is None:
        V = torch.empty((J, nq), device=q.device, dtype=torch.float32)
    _lib.call("mh_coxprobe_scores", _p(q), nq, D, _p(W), J, _p(V), stream=_stream())
    return V


def coxprobe_grad(V: torch.Tensor, time: torch.Tensor, event: torch.Tensor, fold: torch.Tensor, heldout: torch.Tensor,
                  rscale: torch.Tensor, ties: str, G: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None):
    """(G f32 [n, J], loss f64 [J]) on the device (no sync): every job's partial-likelihood score gradient
    r_j (w_k sum_i q_i ([t_k > t_i] + [t_k = t_i](1 - e_k f_i)) - e_k) over its training rows (event in {0, 1}, time not NaN, fold >= 0,
    fold != heldout_j), exactly 0 elsewhere, and the data term of its objective (mh_coxprobe_grad: f64 scans over the scores
    V f32 [J, n] of rows in NON-INCREASING time order, NaN times last; ties "breslow" / "efron").  G, loss and the workspace
    (coxprobe_workspace) may be passed to be overwritten."""
    if not isinstance(V, torch.Tensor) or V.dtype != torch.float32 or V.dim() != 2 or not V.is_contiguous():
        got = f"{V.dtype} {tuple(V.shape)}" if isinstance(V, torch.Tensor) else type(V).__name__
        raise ValueError(f"coxprobe_grad: V must be a contiguous f32 [J, n], got {got}")
    J, n = V.shape
    for t, dtype, name in ((time, torch.float64, "time"), (event, torch.uint8, "event"), (fold, torch.int32, "fold")):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,):
            raise ValueError(f"coxprobe_grad: {name} must be {dtype} [{n}]")
    for t, dtype, name in ((heldout, torch.int32, "heldout"), (rscale, torch.float32, "rscale")):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (J,):
            raise ValueError(f"coxprobe_grad: {name} must be {dtype} [{J}]")
    if ties not in COX_TIES:
        raise ValueError(f'coxprobe_grad: ties must be "breslow" or "efron", got {ties!r}')
    _cp_out(G, torch.float32, (n, J), "coxprobe_grad: G")
    _cp_out(loss, torch.float64, (J,), "coxprobe_grad: loss")
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float64 or workspace.dim() != 1
                                  or not workspace.is_contiguous()):
        raise ValueError("coxprobe_grad: workspace must be a contiguous 1-D f64 tensor (coxprobe_workspace)")
    _chk(V, time, event, fold, heldout, rscale, G, loss, workspace)
    if not (1 <= n <= COXPROBE_MAX_N) or not (1 <= J) or n * J > (1 << 24):
        raise MirrorHipError(f"coxprobe_grad: J = {J} jobs over n = {n} rows (1 <= n <= {COXPROBE_MAX_N}, n * J <= 2^24)")
    need = int(_lib.load().mh_coxprobe_workspace_bytes(n, J)) // 8
    if workspace is None:
        workspace = torch.empty((need,), device=V.device, dtype=torch.float64)
    elif workspace.numel() < need:
        raise ValueError(f"coxprobe_grad: workspace holds {workspace.numel()} f64, {need} are needed")
    if G is None:
        G = torch.empty((n, J), device=V.device, dtype=torch.float32)
    if loss is None:
        loss = torch.empty((J,), device=V.device, dtype=torch.float64)
    _lib.call("mh_coxprobe_grad", _p(V), n, J, _p(time.contiguous()), _p(event.contiguous()), _p(fold.contiguous()),
              _p(heldout.contiguous()), _p(rscale.contiguous()), COX_TIES[ties], _p(G), _p(loss), _p(workspace), stream=_stream())
    return G, loss


def coxprobe_step(y: torch.Tensor, G: torch.Tensor, Wx: torch.Tensor, Wz: torch.Tensor, lam: torch.Tensor, eta: torch.Tensor,
                  beta: float, gmax_part: Optional[torch.Tensor] = None, want_gmax: bool = False):
    """One FISTA update of every job IN PLACE (no sync): g = G^T y + lam_j Wz, X' = Wz - eta_j g, Z' = X' + beta (X' - Wx), stored over
    Wx / Wz f32 [J, D]; no intercept (mh_coxprobe_step: mh_linprobe_step's kernel with one key per job, one row-ordered f32 chain per
    element).  Returns gmax_part f32 [ceil((D + 1) / 128), J] (max |g| per column tile and job) or None."""
    y = _fs_f32(y, "coxprobe_step: y", device=False)
    n, D = y.shape
    J = _cp_weights(Wz, D, "coxprobe_step: Wz")
    if _cp_weights(Wx, D, "coxprobe_step: Wx") != J:
        raise ValueError(f"coxprobe_step: Wx has {Wx.shape[0]} jobs, Wz {J}")
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J) or not G.is_contiguous():
        raise ValueError(f"coxprobe_step: G must be a contiguous f32 [{n}, {J}]")
    for t, name in ((lam, "lam"), (eta, "eta")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (J,):
            raise ValueError(f"coxprobe_step: {name} must be {torch.float32} [{J}]")
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not (0.0 <= float(beta) <= 1.0):
        raise ValueError(f"coxprobe_step: beta must lie in [0, 1], got {beta!r}")
    tiles = (D + 1 + 127) // 128
    _cp_out(gmax_part, torch.float32, (tiles, J), "coxprobe_step: gmax_part")
    _chk(y, G, Wx, Wz, lam, eta, gmax_part)
    if not (1 <= n <= COXPROBE_MAX_N) or not (1 <= J) or n * J > (1 << 24):
        raise MirrorHipError(f"coxprobe_step: J = {J} jobs over n = {n} rows (1 <= n <= {COXPROBE_MAX_N}, n * J <= 2^24)")
    _contig(Wx, "coxprobe_step: Wx")
    _contig(Wz, "coxprobe_step: Wz")
    if gmax_part is None and want_gmax:
        gmax_part = torch.empty((tiles, J), device=y.device, dtype=torch.float32)
    _lib.call("mh_coxprobe_step", _p(y), n, D, _p(G), _p(Wx), _p(Wz), _p(lam.contiguous()), _p(eta.contiguous()), float(beta), J,
              _p(gmax_part), stream=_stream())
    return gmax_part


# ----------------------------------------------------------------------------- k-means and its agreement with labels (csrc/kmeans.hip)
KMEANS_METRIC = {"euclidean": 0, "cosine": 1}


def _km_cent(cent, D: int, who: str):
    """(R, K) of centroids f32 [R, K, D] inside the limits the k-means entry points share."""
    if not isinstance(cent, torch.Tensor) or cent.dim() != 3 or cent.dtype != torch.float32 or cent.shape[2] != D:
        got = f"{cent.dtype} {tuple(cent.shape)}" if isinstance(cent, torch.Tensor) else type(cent).__name__
        raise ValueError(f"{who}: cent must be f32 [R, K, {D}], got {got}")
    R, Kk = int(cent.shape[0]), int(cent.shape[1])
    if not (1 <= Kk <= 1024) or not (1 <= R <= 65535) or R * Kk > (1 << 20):
        raise MirrorHipError(f"{who}: K = {Kk} (1..1024), R = {R} (1..65535, R * K <= 2^20)")
    return R, Kk


def _km_assign(assign, R: Optional[int], n: int, who: str, what: str = "assign") -> None:
    if (not isinstance(assign, torch.Tensor) or assign.dim() != 2 or assign.dtype != torch.int32 or assign.shape[1] != n
            or (R is not None and assign.shape[0] != R)):
        got = f"{assign.dtype} {tuple(assign.shape)}" if isinstance(assign, torch.Tensor) else type(assign).__name__
        raise ValueError(f"{who}: {what} must be int32 [{'R' if R is None else R}, {n}], got {got}")


def kmeans_assign(x: torch.Tensor, cent: torch.Tensor, bias: Optional[torch.Tensor] = None, prev: Optional[torch.Tensor] = None,
                  changed: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_score: bool = False):
    """(assign int32 [R, n], score f32 [R, n] or None) on the device (no sync): per restart the centroid with the largest
    x[i] . cent[r, k] (+ bias[r, k]), NaN scores not eligible, ties to the smaller k, -1 when none is eligible (mh_kmeans_assign: the
    retrieval kernels' exact-f32 tile product over ceil(K / 128) key tiles; the [n, R K] scores are never stored).  With prev (int32
    [R, n]; it may be `out`) the int32 [R] row `changed`, zeroed by the caller, grows by the rows that differ from it."""
    x = _fs_f32(x, "kmeans_assign: x", device=False)
    n, D = x.shape
    R, Kk = _km_cent(cent, D, "kmeans_assign")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (R, Kk)):
        raise ValueError(f"kmeans_assign: bias must be f32 [{R}, {Kk}]")
    if (prev is None) != (changed is None):
        raise ValueError("kmeans_assign: prev and changed go together")
    if prev is not None:
        _km_assign(prev, R, n, "kmeans_assign", "prev")
        if not isinstance(changed, torch.Tensor) or changed.dtype != torch.int32 or tuple(changed.shape) != (R,) or not changed.is_contiguous():
            raise ValueError(f"kmeans_assign: changed must be a contiguous int32 [{R}] tensor")
        if not prev.is_contiguous():
            raise ValueError("kmeans_assign: prev must be contiguous")
    if out is not None:
        _km_assign(out, R, n, "kmeans_assign", "out")
        if not out.is_contiguous():
            raise ValueError("kmeans_assign: out must be contiguous")
    _chk(x, cent, bias, prev, changed, out)
    cent = cent.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    if out is None:
        out = torch.empty((R, n), device=x.device, dtype=torch.int32)
    score = torch.empty((R, n), device=x.device, dtype=torch.float32) if want_score else None
    _lib.call("mh_kmeans_assign", _p(x), _p(cent), _p(bias), n, R, Kk, D, _p(prev), _p(out), _p(score), _p(changed), stream=_stream())
    return out, score


def kmeans_update(x: torch.Tensor, assign: torch.Tensor, cent: torch.Tensor, bias: Optional[torch.Tensor], metric: str,
                  count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """count int32 [R, K] on the device (no sync); cent f32 [R, K, D] (and bias f32 [R, K], "euclidean") are updated IN PLACE: every
    cluster with a member becomes the mean of its rows, summed in ascending row order in f64 and rounded to f32 once ("cosine":
    normalised afterwards; "euclidean": bias = -|c|^2 / 2); an empty cluster keeps its centroid and bias (mh_kmeans_update)."""
    x = _fs_f32(x, "kmeans_update: x", device=False)
    n, D = x.shape
    if metric not in KMEANS_METRIC:
        raise ValueError(f'kmeans_update: metric must be "euclidean" or "cosine", got {metric!r}')
    R, Kk = _km_cent(cent, D, "kmeans_update")
    _km_assign(assign, R, n, "kmeans_update")
    if (bias is not None) != (metric == "euclidean"):
        raise ValueError("kmeans_update: the bias goes with the euclidean metric only")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (R, Kk)):
        raise ValueError(f"kmeans_update: bias must be f32 [{R}, {Kk}]")
    if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (R, Kk)):
        raise ValueError(f"kmeans_update: count must be int32 [{R}, {Kk}]")
    _chk(x, assign, cent, bias, count)
    if not cent.is_contiguous() or (bias is not None and not bias.is_contiguous()) or (count is not None and not count.is_contiguous()):
        raise ValueError("kmeans_update: cent, bias and count are written in place and must be contiguous")
    if count is None:
        count = torch.empty((R, Kk), device=x.device, dtype=torch.int32)
    _lib.call("mh_kmeans_update", _p(x), _p(assign.contiguous()), n, R, Kk, D, KMEANS_METRIC[metric], _p(cent), _p(bias), _p(count), None,
              stream=_stream())
    return count


def kmeans_bias(cent: torch.Tensor) -> torch.Tensor:
    """f32 [R, K] on the device (no sync): -|c|^2 / 2 of centroids f32 [R, K, D] that the update did not produce, in the update's own
    order of additions (mh_kmeans_bias)."""
    if not isinstance(cent, torch.Tensor) or cent.dim() != 3 or not (1 <= cent.shape[2] <= 4096):
        raise ValueError("kmeans_bias: cent must be f32 [R, K, D] with 1 <= D <= 4096")
    R, Kk = _km_cent(cent, int(cent.shape[2]), "kmeans_bias")
    _chk(cent)
    bias = torch.empty((R, Kk), device=cent.device, dtype=torch.float32)
    _lib.call("mh_kmeans_bias", _p(cent.detach().contiguous()), R, Kk, int(cent.shape[2]), _p(bias), stream=_stream())
    return bias


def kmeans_inertia(x: torch.Tensor, cent: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
    """f64 [R] on the device (no sync): the sum over the assigned rows of |x[i] - cent[r, assign[r, i]]|^2, every term and the sum in
    f64 in a fixed order (mh_kmeans_inertia)."""
    x = _fs_f32(x, "kmeans_inertia: x", device=False)
    n, D = x.shape
    R, Kk = _km_cent(cent, D, "kmeans_inertia")
    _km_assign(assign, R, n, "kmeans_inertia")
    _chk(x, cent, assign)
    inertia = torch.empty((R,), device=x.device, dtype=torch.float64)
    ws = torch.empty((int(_lib.load().mh_kmeans_inertia_workspace_bytes(n, R)) // 8,), device=x.device, dtype=torch.float64)
    _lib.call("mh_kmeans_inertia", _p(x), _p(cent.detach().contiguous()), _p(assign.contiguous()), n, R, Kk, D, _p(inertia), _p(ws),
              stream=_stream())
    return inertia


def kmeans_tally(assign: torch.Tensor, labels: torch.Tensor, K: int, C: int):
    """(cont int32 [R, K, C], bad int32 [R], summary f64 [R, 3]) on the device (no sync): per restart the contingency counts
    [cluster, label] of assign int32 [R, n] against labels int64 [n], the rows left out (label outside [0, C) or assign outside
    [0, K)), and {NMI (arithmetic mean, natural log), ARI, purity} from the integer counts (mh_kmeans_tally)."""
    if not isinstance(assign, torch.Tensor) or assign.dim() != 2 or assign.dtype != torch.int32:
        raise ValueError("kmeans_tally: assign must be int32 [R, n]")
    R, n = assign.shape
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
        raise ValueError(f"kmeans_tally: labels must be int64 [{n}]")
    for v, name in ((K, "K"), (C, "C")):
        if isinstance(v, bool) or not isinstance(v, int) or not (1 <= v <= 1024):
            raise ValueError(f"kmeans_tally: {name} must be an int in [1, 1024], got {v!r}")
    if K * C > 65536:
        raise MirrorHipError(f"kmeans_tally: K * C = {K * C} cells, 65536 at the most")
    _chk(assign, labels)
    if not (1 <= R <= (1 << 20)) or not (1 <= n <= (1 << 20)):
        raise MirrorHipError(f"kmeans_tally: R = {R}, n = {n} (1..2^20)")
    assign, labels = assign.contiguous(), labels.contiguous()
    cont = torch.empty((R, K, C), device=assign.device, dtype=torch.int32)
    bad = torch.empty((R,), device=assign.device, dtype=torch.int32)
    summary = torch.empty((R, 3), device=assign.device, dtype=torch.float64)
    _lib.call("mh_kmeans_tally", _p(assign), _p(labels), n, R, K, C, _p(cont), _p(bad), _p(summary), stream=_stream())
    return cont, bad, summary


# ----------------------------------------------------------------------------- seeding, silhouette, matched accuracy (csrc/cluster_ext.hip)
def silhouette(y: torch.Tensor, lab: torch.Tensor, K: int, metric: str, samples: bool = False):
    """(mean f64 [R], bad int32 [R], sil f64 [R, n] or None) on the device (no sync): the silhouette of every label row lab int32 [R, n]
    (cluster ids in [0, K); a row outside takes no part, counts in bad and has sil NaN) over the prepared rows y f32 [n, D], distances
    from the retrieval kernels' exact-f32 tile product in f64 (mh_silhouette: no [n, n] matrix; the product is formed once per label
    row).  "cosine" is 1 - y_i . y_j: y must hold unit rows."""
    y = _fs_f32(y, "silhouette: y", device=False)
    n, D = y.shape
    if metric not in KMEANS_METRIC:
        raise ValueError(f'silhouette: metric must be "euclidean" or "cosine", got {metric!r}')
    if isinstance(K, bool) or not isinstance(K, int) or not (1 <= K <= 1024):
        raise ValueError(f"silhouette: K must be an int in [1, 1024], got {K!r}")
    _km_assign(lab, None, n, "silhouette", "lab")
    R = int(lab.shape[0])
    _chk(y, lab)
    if not (1 <= R <= 65535):
        raise MirrorHipError(f"silhouette: R = {R} label rows (1..65535)")
    lab = lab.contiguous()
    mean = torch.empty((R,), device=y.device, dtype=torch.float64)
    bad = torch.empty((R,), device=y.device, dtype=torch.int32)
    sil = torch.empty((R, n), device=y.device, dtype=torch.float64) if samples else None
    ws = torch.empty((int(_lib.load().mh_silhouette_workspace_bytes(n, K, D)) // 8,), device=y.device, dtype=torch.float64)
    _lib.call("mh_silhouette", _p(y), _p(lab), n, R, K, D, KMEANS_METRIC[metric], _p(sil), _p(mean), _p(bad), _p(ws), stream=_stream())
    return mean, bad, sil


def kmeanspp_init(y: torch.Tensor, R: int, K: int, seed: int, offset: int):
    """(rows int64 [R, K], cent f32 [R, K, D]) on the device (no sync): k-means++ seeding (D^2 sampling, one draw per centre; not
    sklearn's greedy variant) of R restarts from the prepared rows y f32 [n, D]; restart r uses draw id offset + r of the data feed's
    stream under kind 2; cent are bit copies of y[rows] (mh_kmeanspp_init)."""
    y = _fs_f32(y, "kmeanspp_init: y", device=False)
    n, D = y.shape
    for v, name, hi in ((K, "K", 1024), (R, "R", 65535)):
        if isinstance(v, bool) or not isinstance(v, int) or not (1 <= v <= hi):
            raise ValueError(f"kmeanspp_init: {name} must be an int in [1, {hi}], got {v!r}")
    if R * K > (1 << 20):
        raise MirrorHipError(f"kmeanspp_init: R * K = {R * K} centres, 2^20 at the most")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"kmeanspp_init: seed must be an int, got {seed!r}")
    if isinstance(offset, bool) or not isinstance(offset, int) or not (0 <= offset and offset + R < (1 << 63)):
        raise ValueError(f"kmeanspp_init: draw ids offset .. offset + R must stay in [0, 2^63), got offset = {offset!r}")
    _chk(y)
    rows = torch.empty((R, K), device=y.device, dtype=torch.int64)
    cent = torch.empty((R, K, D), device=y.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.load().mh_kmeanspp_workspace_bytes(n, R)) // 8,), device=y.device, dtype=torch.float64)
    _lib.call("mh_kmeanspp_init", _p(y), n, R, K, D, seed & (2 ** 64 - 1), offset, _p(rows), _p(cent), _p(ws), stream=_stream())
    return rows, cent


def cluster_match(cont: torch.Tensor):
    """(match int32 [R, K], hits int64 [R]) on the device (no sync): per restart the one-to-one assignment of clusters to classes of
    largest total count in cont int32 [R, K, C] ([cluster, label], as kmeans_tally writes it): match[r, k] the class of cluster k or -1,
    hits[r] the matched rows: the exact optimum (mh_cluster_match: integer shortest augmenting paths)."""
    if not isinstance(cont, torch.Tensor) or cont.dim() != 3 or cont.dtype != torch.int32:
        got = f"{cont.dtype} {tuple(cont.shape)}" if isinstance(cont, torch.Tensor) else type(cont).__name__
        raise ValueError(f"cluster_match: cont must be int32 [R, K, C], got {got}")
    R, K, C = (int(v) for v in cont.shape)
    if not (1 <= K <= 1024) or not (1 <= C <= 1024) or K * C > 65536 or not (1 <= R <= (1 << 20)):
        raise MirrorHipError(f"cluster_match: K = {K}, C = {C} (1..1024, K * C <= 65536), R = {R} (1..2^20)")
    _chk(cont)
    cont = cont.contiguous()
    match = torch.empty((R, K), device=cont.device, dtype=torch.int32)
    hits = torch.empty((R,), device=cont.device, dtype=torch.int64)
    _lib.call("mh_cluster_match", _p(cont), R, K, C, _p(match), _p(hits), stream=_stream())
    return match, hits


# ----------------------------------------------------------------------------- recursive gene elimination: J squared-hinge jobs at once (csrc/geneselect.hip)
def _gs_f32(t: torch.Tensor, what: str, device: bool = True) -> torch.Tensor:
    """_fs_f32 at the limits of the gsel entry points (D up to 2^18)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what} must be f32 [n, D], got {got}")
    if device:
        _chk(t)
    n, D = t.shape
    if not (1 <= n <= (1 << 20)) or not (1 <= D <= (1 << 18)):
        raise MirrorHipError(f"{what}: n = {n} (1..2^20), D = {D} (1..2^18)")
    return t.detach().contiguous()


def _gs_state(y: torch.Tensor, W: torch.Tensor, b: torch.Tensor, C: int, who: str):
    """_lp_state at the limits of the gsel entry points."""
    y = _gs_f32(y, f"{who}: y", device=False)
    n, D = y.shape
    if isinstance(C, bool) or not isinstance(C, int) or not (2 <= C <= 64):
        raise ValueError(f"{who}: C must be an int in [2, 64], got {C!r}")
    Cp = fewshot_cp(C)
    if not isinstance(W, torch.Tensor) or W.dtype != torch.float32 or W.dim() != 3 or tuple(W.shape[1:]) != (Cp, D):
        raise ValueError(f"{who}: the weights must be f32 [J, {Cp}, {D}]")
    J = W.shape[0]
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or tuple(b.shape) != (J, Cp):
        raise ValueError(f"{who}: the bias must be f32 [{J}, {Cp}]")
    _chk(y, W, b)
    if not (1 <= J and J * Cp <= (1 << 20)) or n * J * Cp > (1 << 28):
        raise MirrorHipError(f"{who}: J = {J} jobs of {Cp} keys over n = {n} rows (J * Cp <= 2^20, n * J * Cp <= 2^28)")
    _contig(W, f"{who}: the weights")
    _contig(b, f"{who}: the bias")
    return y, n, D, J, Cp


def _gs_mask(mask, J: int, D: int, who: str) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (J, D) or not mask.is_contiguous():
        raise ValueError(f"{who}: mask must be a contiguous uint8 [{J}, {D}]")
    return mask


def colstats(x: torch.Tensor):
    """(mu f32 [D], rstd f32 [D]) on the device (no sync): the column means and reciprocal population standard deviations of x f32 [n, D],
    summed in a fixed order in f64, rstd = 0 for a constant column (mh_colstats)."""
    x = _gs_f32(x, "colstats: x")
    n, D = x.shape
    mu = torch.empty((D,), device=x.device, dtype=torch.float32)
    rstd = torch.empty((D,), device=x.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.load().mh_colstats_workspace_bytes(n, D)) // 8,), device=x.device, dtype=torch.float64)
    _lib.call("mh_colstats", _p(x), n, D, _p(mu), _p(rstd), _p(ws), stream=_stream())
    return mu, rstd


def standardize(x: torch.Tensor, mu: torch.Tensor, rstd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f32 [n, D]: (x - mu) * rstd (mh_standardize).  out may be x itself (in place)."""
    x = _gs_f32(x, "standardize: x", device=False)
    n, D = x.shape
    for t, name in ((mu, "mu"), (rstd, "rstd")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (D,):
            raise ValueError(f"standardize: {name} must be f32 [{D}]")
    if out is None:
        out = torch.empty_like(x)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, D) or not out.is_contiguous():
        raise ValueError(f"standardize: out must be a contiguous f32 [{n}, {D}]")
    _chk(x, mu, rstd, out)
    _lib.call("mh_standardize", _p(x), _p(mu.contiguous()), _p(rstd.contiguous()), _p(out), n, D, stream=_stream())
    return out


def gsel_rowsq(y: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """f32 [J, n] on the device (no sync): every row's sum of squares over the columns with mask[j, d] != 0 (mh_gsel_rowsq)."""
    y = _gs_f32(y, "gsel_rowsq: y", device=False)
    n, D = y.shape
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2:
        raise ValueError(f"gsel_rowsq: mask must be a contiguous uint8 [J, {D}]")
    J = mask.shape[0]
    _gs_mask(mask, J, D, "gsel_rowsq")
    _chk(y, mask)
    if not (1 <= J <= (1 << 19)) or n * J > (1 << 28):
        raise MirrorHipError(f"gsel_rowsq: J = {J} jobs over n = {n} rows (J <= 2^19, n * J <= 2^28)")
    out = torch.empty((J, n), device=y.device, dtype=torch.float32)
    _lib.call("mh_gsel_rowsq", _p(y), n, D, _p(mask), J, _p(out), stream=_stream())
    return out


def gsel_slices(n: int, nk: int, D: int) -> int:
    """The slices mh_gsel_grad cuts the contraction over D into for n rows and nk = J Cp keys (mh_gsel_slices; 0 outside the limits)."""
    return int(_lib.load().mh_gsel_slices(int(n), int(nk), int(D)))


def gsel_workspace(n: int, J: int, Cp: int, D: int, device) -> torch.Tensor:
    """The f32 workspace of mh_gsel_grad for this shape (mh_gsel_grad_workspace_bytes); nothing to zero."""
    nbytes = int(_lib.load().mh_gsel_grad_workspace_bytes(int(n), int(J), int(Cp), int(D)))
    if nbytes <= 0:
        raise MirrorHipError(f"gsel_workspace: n = {n}, J = {J}, Cp = {Cp}, D = {D} outside the limits of mh_gsel_grad")
    return torch.empty((nbytes // 4,), device=device, dtype=torch.float32)


def gsel_grad(y: torch.Tensor, Wz: torch.Tensor, bz: torch.Tensor, labels: torch.Tensor, fold: torch.Tensor, heldout: torch.Tensor,
              rscale: torch.Tensor, C: int, G: Optional[torch.Tensor] = None, want_loss: bool = False, want_pred: bool = False,
              workspace: Optional[torch.Tensor] = None):
    """(G f32 [n, J Cp], loss_part f64 [ceil(n / 128), J] or None, pred int32 [J, n] or None) on the device (no sync): every job's
    squared-hinge logit gradient -2 r_j t max(0, 1 - t v) over its training rows, 0 elsewhere and in the pad columns; the per-row-tile
    data terms; the class of the largest v_c of EVERY row (mh_gsel_grad).  G and the workspace (gsel_workspace) may be passed."""
    y, n, D, J, Cp = _gs_state(y, Wz, bz, C, "gsel_grad")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
        raise ValueError(f"gsel_grad: labels must be int64 [{n}]")
    if not isinstance(fold, torch.Tensor) or fold.dtype != torch.int32 or tuple(fold.shape) != (n,):
        raise ValueError(f"gsel_grad: fold must be int32 [{n}]")
    _chk(labels, fold)
    heldout = _lp_vec(heldout, torch.int32, J, "gsel_grad: heldout")
    rscale = _lp_vec(rscale, torch.float32, J, "gsel_grad: rscale")
    if G is None:
        G = torch.empty((n, J * Cp), device=y.device, dtype=torch.float32)
    elif not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J * Cp) or not G.is_contiguous():
        raise ValueError(f"gsel_grad: G must be a contiguous f32 [{n}, {J * Cp}]")
    need = int(_lib.load().mh_gsel_grad_workspace_bytes(n, J, Cp, D)) // 4
    if workspace is None:
        workspace = torch.empty((need,), device=y.device, dtype=torch.float32)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or workspace.dim() != 1
          or workspace.numel() < need or not workspace.is_contiguous()):
        raise ValueError(f"gsel_grad: workspace must be a contiguous f32 [{need}] at the least")
    _chk(G, workspace)
    loss_part = torch.empty(((n + 127) // 128, J), device=y.device, dtype=torch.float64) if want_loss else None
    pred = torch.empty((J, n), device=y.device, dtype=torch.int32) if want_pred else None
    _lib.call("mh_gsel_grad", _p(y), n, D, _p(Wz), _p(bz), _p(labels.contiguous()), _p(fold.contiguous()), _p(heldout), _p(rscale),
              J, C, Cp, _p(G), _p(loss_part), _p(pred), _p(workspace), stream=_stream())
    return G, loss_part, pred


def gsel_step(y: torch.Tensor, G: torch.Tensor, Wx: torch.Tensor, bx: torch.Tensor, Wz: torch.Tensor, bz: torch.Tensor,
              lam: torch.Tensor, eta: torch.Tensor, beta: float, mask: torch.Tensor, fit_intercept: bool, C: int,
              gmax_part: Optional[torch.Tensor] = None, want_gmax: bool = False):
    """linprobe_step under a feature mask uint8 [J, D] IN PLACE (no sync): a masked (job, column) is neither read nor written and takes
    no part in gmax_part; fit_intercept=False does the same to the bias (mh_gsel_step).  Returns gmax_part or None."""
    y, n, D, J, Cp = _gs_state(y, Wz, bz, C, "gsel_step")
    _gs_state(y, Wx, bx, C, "gsel_step")
    if Wx.shape[0] != J:
        raise ValueError(f"gsel_step: Wx has {Wx.shape[0]} jobs, Wz {J}")
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float32 or tuple(G.shape) != (n, J * Cp) or not G.is_contiguous():
        raise ValueError(f"gsel_step: G must be a contiguous f32 [{n}, {J * Cp}]")
    _chk(G)
    lam = _lp_vec(lam, torch.float32, J, "gsel_step: lam")
    eta = _lp_vec(eta, torch.float32, J, "gsel_step: eta")
    beta = float(beta)
    if not (0.0 <= beta <= 1.0):
        raise ValueError(f"gsel_step: beta must lie in [0, 1], got {beta!r}")
    _gs_mask(mask, J, D, "gsel_step")
    if not isinstance(fit_intercept, bool):
        raise ValueError(f"gsel_step: fit_intercept must be a bool, got {fit_intercept!r}")
    tiles = (D + 1 + 127) // 128
    if gmax_part is None and want_gmax:
        gmax_part = torch.empty((tiles, J), device=y.device, dtype=torch.float32)
    elif gmax_part is not None and (not isinstance(gmax_part, torch.Tensor) or gmax_part.dtype != torch.float32
                                    or tuple(gmax_part.shape) != (tiles, J) or not gmax_part.is_contiguous()):
        raise ValueError(f"gsel_step: gmax_part must be a contiguous f32 [{tiles}, {J}]")
    _chk(mask, gmax_part)
    _lib.call("mh_gsel_step", _p(y), n, D, _p(G), _p(Wx), _p(bx), _p(Wz), _p(bz), _p(lam), _p(eta), beta, _p(mask), int(fit_intercept),
              J, C, Cp, _p(gmax_part), stream=_stream())
    return gmax_part


def gsel_eliminate(Wx: torch.Tensor, Wz: torch.Tensor, mask: torch.Tensor, elim_round: torch.Tensor, k: int, round: int, C: int,
                   want_importance: bool = False):
    """Drop every job's k least important active features IN PLACE (no sync): mask 0, elim_round = round, Wx / Wz columns 0
    (mh_gsel_eliminate: importance = sum_c Wx[j, c, d]^2, ties to the smaller index, integer decisions only).  Returns importance f32
    [J, D] (before the removal, 0 for inactive features) or None."""
    if isinstance(C, bool) or not isinstance(C, int) or not (2 <= C <= 64):
        raise ValueError(f"gsel_eliminate: C must be an int in [2, 64], got {C!r}")
    Cp = fewshot_cp(C)
    if not isinstance(Wx, torch.Tensor) or Wx.dtype != torch.float32 or Wx.dim() != 3 or Wx.shape[1] != Cp or not Wx.is_contiguous():
        raise ValueError(f"gsel_eliminate: Wx must be a contiguous f32 [J, {Cp}, D]")
    J, _, D = Wx.shape
    if not isinstance(Wz, torch.Tensor) or Wz.dtype != torch.float32 or tuple(Wz.shape) != (J, Cp, D) or not Wz.is_contiguous():
        raise ValueError(f"gsel_eliminate: Wz must be a contiguous f32 [{J}, {Cp}, {D}]")
    _gs_mask(mask, J, D, "gsel_eliminate")
    if (not isinstance(elim_round, torch.Tensor) or elim_round.dtype != torch.int32 or tuple(elim_round.shape) != (J, D)
            or not elim_round.is_contiguous()):
        raise ValueError(f"gsel_eliminate: elim_round must be a contiguous int32 [{J}, {D}]")
    for v, name in ((k, "k"), (round, "round")):
        if isinstance(v, bool) or not isinstance(v, int) or not (0 <= v < (1 << 31)):
            raise ValueError(f"gsel_eliminate: {name} must be a non-negative int, got {v!r}")
    _chk(Wx, Wz, mask, elim_round)
    if not (1 <= D <= (1 << 18)) or not (1 <= J and J * Cp <= (1 << 20)):
        raise MirrorHipError(f"gsel_eliminate: J = {J} jobs of {Cp} keys, D = {D} (J * Cp <= 2^20, D in 1..2^18)")
    imp = torch.empty((J, D), device=Wx.device, dtype=torch.float32) if want_importance else None
    _lib.call("mh_gsel_eliminate", _p(Wx), _p(Wz), _p(mask), _p(elim_round), J, C, Cp, D, k, round, _p(imp), stream=_stream())
    return imp
