"""mh_gemm with a ragged contraction (K % BK != 0, K >= 8 BK, f32 C): ONE table of cases for the CPU and the GPU test.

csrc/gemm.hip splits such a product into a `K - K % BK` main launch and a remainder, and the remainder takes one of three routes:

  fold    the split-K fold pass adds it (GemmTail -> fold_partials_kernel<TAIL = true, PS = 4 or 1>, csrc/gemm_big.hip)
  rank    rank_update_kernel<TA, TB> after a main launch that did not fold (four dtype instances, flat or one batch axis)
  tiled   a second launch of the guarded 128 x 128 kernel (KT > 16, batch * KT > 256, K-contiguous operands, no accumulate)

Every case names the route it is built to reach; the shapes are the smallest at which the host still selects it
(gemm_try_big_bf16: >= 128 workgroups of 256 x 256, launch_big: >= 8 partial tiles, launch_fold: blocks1 < 1024 shares quads).
Operands follow functional._wgrad unless the layout says otherwise: A = dy.t() with the contraction index as its row, B = x
[K, N] row-major, C f32, accumulate, pre-filled with small integers (a store in place of an add shows up).

Integer data: main rows from {-1, 0, 1}, tail rows from [-3, 3].  Every K-slice's partial tile is then an integer (a half-integer at
alpha = 0.5) small enough to be a bf16 number (checked here, on the CPU), every f32 sum is exact, and the result must EQUAL the f64
product.  Random data (the four fold cases with rounding): tolerance and sensitivity condition in `random_case`.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
from dataclasses import dataclass

import torch

from mirror_amd._lib import MH_BF16, MH_F32, GemmDesc

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROW_PAD, COL_PAD, PAD_FILL = 3, 8, 7.0       # C is a window of a larger buffer filled with 7.0: what lies past M and N must stay
WINDOW_LEAD, WINDOW_EXTRA = 1, 3            # FW: B = x[:, 1:1 + K] of [batch, K + 3, N]
LAYOUTS = list(itertools.product([True, False], [True, False]))       # (A row-major [M, K]?, B given as [N, K]^T?)
WGRAD = (False, False)


@dataclass(frozen=True)
class Case:
    id: str
    M: int
    N: int
    kmain: int
    tail: int
    split_k: int
    batch: int
    route: str                      # "fold4" | "fold1" | "fold_notail" | "rank" | "tiled"
    bcast: bool = True              # batch > 1: every batch reduces into ONE C (out = dw.expand(...)); False: a C per batch
    layout: tuple = WGRAD
    dta: torch.dtype = bf16
    dtb: torch.dtype = bf16
    mma: int = MH_BF16
    alpha: float = 1.0
    accumulate: bool = True
    bias: bool = False
    diag: float = 0.0
    window: bool = False            # B is a row window of a taller buffer (sB != K * N, base one row in)
    partials: str = "bf16"          # kernels.SPLITK_PARTIALS for this case

    @property
    def K(self) -> int:
        return self.kmain + self.tail

    @property
    def folds(self) -> bool:
        return self.route.startswith("fold")

    def __str__(self) -> str:
        return self.id


def _cases():
    out = []
    for t, al in itertools.product((1, 7, 16), (1.0, 0.5)):
        out.append(Case(f"F4-t{t}-a{al}", 512, 512, 2048, t, 32, 1, "fold4", alpha=al))
    for t, al in itertools.product((1, 16), (1.0, 0.5)):
        out.append(Case(f"F1-t{t}-a{al}", 1024, 1024, 512, t, 8, 1, "fold1", alpha=al))
    for t, al in itertools.product((1, 16), (1.0, 0.5)):
        out.append(Case(f"FB-t{t}-a{al}", 512, 512, 512, t, 4, 8, "fold4", alpha=al))
    out.append(Case("FBL", 512, 512, 512, 16, 4, 16, "fold4"))
    out.append(Case("FBX", 512, 512, 512, 16, 4, 17, "fold_notail"))
    for t in (1, 16):
        out.append(Case(f"FW-t{t}", 512, 512, 512, t, 4, 8, "fold4", window=True))
    out.append(Case("RA", 512, 512, 2048, 16, 32, 1, "rank", partials="f32"))
    for (M, N), t, sk, bt, (da, db) in itertools.product(((200, 72), (130, 257)), (1, 16), (1, 4), (1, 3),
                                                          ((bf16, bf16), (f32, bf16), (bf16, f32))):
        nm = {bf16: "b", f32: "f"}
        out.append(Case(f"RU-{M}x{N}-t{t}-s{sk}-z{bt}-{nm[da]}{nm[db]}", M, N, 512, t, sk, bt, "rank", dta=da, dtb=db))
    for t, sk, bt in itertools.product((1, 15), (1, 4), (1, 3)):
        out.append(Case(f"RF-t{t}-s{sk}-z{bt}", 200, 72, 128, t, sk, bt, "rank", dta=f32, dtb=f32, mma=MH_F32))
    for (M, N), t, sk in itertools.product(((256, 256), (130, 257)), (17, 63), (1, 4)):
        out.append(Case(f"T-{M}x{N}-t{t}-s{sk}", M, N, 512, t, sk, 1, "tiled"))
    for (M, N), lay, f32mma, bt in itertools.product(((128, 128), (130, 257)), LAYOUTS, (False, True), (1, 3)):
        out.append(Case(f"NA-{M}x{N}-{'rm' if lay[0] else 'cm'}{'t' if lay[1] else 'n'}-{'f32' if f32mma else 'bf16'}-z{bt}", M, N,
                        128 if f32mma else 512, 5, 1, bt, "tiled", bcast=False, layout=lay, dta=f32 if f32mma else bf16,
                        dtb=f32 if f32mma else bf16, mma=MH_F32 if f32mma else MH_BF16, alpha=0.5, accumulate=False, bias=True,
                        diag=13.0 if M == N else 0.0))
    out.append(Case("NP", 4096, 2048, 512, 8, 1, 1, "tiled", layout=(True, False)))
    return out


CASES = _cases()
FOLD_IDS = ("F4", "F1", "FB", "FBL", "FBX", "FW")
RANDOM_CASES = [c for c in CASES if c.alpha == 1.0 and c.id.split("-")[0] in ("F4", "F1", "FB", "FBL")]


def by_id(cid: str) -> Case:
    return next(c for c in CASES if c.id == cid)


# ------------------------------------------------------------------------------------------ the host's decisions, restated
def bk(mma: int) -> int:
    return 64 if mma == MH_BF16 else 16


def k_slices(kmain: int, split_k: int, mma: int = MH_BF16):
    """[(k0, k1)] of the main launch: launch_one's k_per_split = ceil(ceil(K / split) / BK) * BK, every slice with work."""
    b = bk(mma)
    kps = -(-(-(-kmain // split_k)) // b) * b
    return [(k0, min(k0 + kps, kmain)) for k0 in range(0, kmain, kps)]


def desc_for(M: int, N: int, K: int, split_k: int, batch: int, bcast: bool, dta, dtb, mma: int, accumulate: bool,
             ldc: int = 0) -> GemmDesc:
    """The mh_gemm_desc kernels.gemm fills for A = dy.t() (batch in the second axis), B = x, f32 C — without pointers."""
    dt = {f32: MH_F32, bf16: MH_BF16}
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = M, N, ldc or N
    d.a_kc = d.b_kc = 0
    d.dtA, d.dtB, d.dtC, d.mma = dt[dta], dt[dtb], MH_F32, mma
    d.batch1, d.batch2 = 1, batch
    d.sA2, d.sB2 = (K * M, K * N) if batch > 1 else (0, 0)
    d.sC2 = 0 if (bcast or batch == 1) else (M + ROW_PAD) * (ldc or N)
    d.alpha, d.accumulate, d.split_k = 1.0, int(accumulate), split_k
    return d


def workspace_bytes(lib, c: Case) -> int:
    """What kernels.gemm asks mh_gemm_workspace_bytes for this case (it does not ask at all without accumulate or under
    SPLITK_PARTIALS = "f32")."""
    if not (c.accumulate and c.partials == "bf16"):
        return 0
    d = desc_for(c.M, c.N, c.K, c.split_k, c.batch, c.bcast, c.dta, c.dtb, c.mma, c.accumulate, c.N + COL_PAD)
    return int(lib.mh_gemm_workspace_bytes(ctypes.byref(d)))


def big_kernel_workgroups(M: int, N: int, kmain: int, split_k: int, batch: int) -> int:
    """gemm_try_big_bf16's count (it declines below 128): 256 x 256 tiles x K-slices x batches."""
    return (-(-M // 256)) * (N // 256) * len(k_slices(kmain, split_k)) * batch


# ------------------------------------------------------------------------------------------ data and f64 references
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def partials_f64(at: torch.Tensor, b: torch.Tensor, kmain: int, split_k: int, alpha: float, mma: int = MH_BF16) -> torch.Tensor:
    """[batch * slices, M, N] f64: alpha * A_z[:, k0:k1] B_z[k0:k1] for every slice of the main launch.  at [batch, K, M], b [batch, K, N]."""
    a64, b64 = at.double(), b.double()
    return torch.stack([alpha * (a64[z, k0:k1].t() @ b64[z, k0:k1]) for z in range(at.shape[0]) for k0, k1 in k_slices(kmain, split_k, mma)])


def assert_partials_are_bf16_numbers(at, b, kmain, split_k, alpha, what) -> None:
    p = partials_f64(at, b, kmain, split_k, alpha)
    assert bool((p.float().bfloat16().double() == p).all()), f"{what}: a K-slice's partial tile is no bf16 number: the exact check would not hold"
    assert float(p.abs().max()) <= 128.0, f"{what}: partial tile magnitude {float(p.abs().max())}"


@dataclass(frozen=True)
class Data:
    at: torch.Tensor            # [batch, K, M]  A's math transpose (dy), values as the device will hold them, f32 on the CPU
    b: torch.Tensor             # [batch, K, N]
    filler: torch.Tensor        # [batch, WINDOW_EXTRA, N] rows around B's window (window cases), else empty
    prefill: torch.Tensor       # [batch or 1, M, N] what C holds before the call
    bias: torch.Tensor          # [N] or empty
    want: torch.Tensor          # f64 [batch or 1, M, N]


def _product(c: Case, at, b, prefill, bias) -> torch.Tensor:
    prod = torch.matmul(at.double().transpose(-1, -2), b.double())
    if c.batch > 1 and c.bcast:
        prod = prod.sum(0, keepdim=True)
    want = c.alpha * prod
    if c.accumulate:
        want = want + prefill.double()
    if c.bias:
        want = want + bias.double()
    if c.diag:
        want = want + c.diag * torch.eye(c.M, dtype=f64)
    return want


@functools.lru_cache(maxsize=None)
def integer_case(c: Case, seed: int = 0) -> Data:
    gen = _gen(seed + 1000 * CASES.index(c))
    at = torch.randint(-1, 2, (c.batch, c.K, c.M), generator=gen).float()
    b = torch.randint(-1, 2, (c.batch, c.K, c.N), generator=gen).float()
    at[:, c.kmain:] = torch.randint(-3, 4, (c.batch, c.tail, c.M), generator=gen).float()
    b[:, c.kmain:] = torch.randint(-3, 4, (c.batch, c.tail, c.N), generator=gen).float()
    filler = torch.randint(-3, 4, (c.batch, WINDOW_EXTRA if c.window else 0, c.N), generator=gen).float()
    nc = 1 if (c.bcast or c.batch == 1) else c.batch
    prefill = torch.randint(-3, 4, (nc, c.M, c.N), generator=gen).float()
    bias = torch.randint(-3, 4, (c.N if c.bias else 0,), generator=gen).float()
    if c.folds:
        assert_partials_are_bf16_numbers(at, b, c.kmain, c.split_k, c.alpha, c.id)
    return Data(at, b, filler, prefill, bias, _product(c, at, b, prefill, bias))


@dataclass(frozen=True)
class RandomData:
    at: torch.Tensor
    b: torch.Tensor
    filler: torch.Tensor
    prefill: torch.Tensor
    bias: torch.Tensor
    want: torch.Tensor
    tol: torch.Tensor           # f64 [1, M, N]
    tail_part: torch.Tensor     # f64 [1, M, N] what the remainder alone contributes
    parts: int
    partial_max: float


TAIL_SCALE = 8.0
TAIL_VISIBLE_FRACTION = 0.8


@functools.lru_cache(maxsize=None)
def random_case(c: Case, seed: int = 0) -> RandomData:
    """randn operands as bf16 numbers, the tail rows of both scaled by 8.  Per-element tolerance, nothing of it measured on the device:

        parts * 2^-9 * max |partial|      the bound csrc/gemm_big.hip and kernels.py state for the bf16 partial tiles (one rounding per
                                          K-slice; max over every slice, batch and element of the f64 slices)
      + n * 2^-24 * (|A|^T |B|)           the worst case of f32 accumulation over the n = batch * K products of an element, whatever the order

    and the remainder's own contribution must exceed it in >= 80 % of the elements, so a dropped or misplaced tail cannot pass."""
    gen = _gen(seed)
    at = torch.randn((c.batch, c.K, c.M), generator=gen)
    b = torch.randn((c.batch, c.K, c.N), generator=gen)
    at[:, c.kmain:] *= TAIL_SCALE
    b[:, c.kmain:] *= TAIL_SCALE
    at, b = at.bfloat16().float(), b.bfloat16().float()
    prefill = torch.randint(-3, 4, (1, c.M, c.N), generator=gen).float()
    empty = torch.zeros(0)
    want = _product(c, at, b, prefill, empty)
    p = partials_f64(at, b, c.kmain, c.split_k, c.alpha)
    parts, partial_max = p.shape[0], float(p.abs().max())
    absprod = torch.matmul(at.double().abs().transpose(-1, -2), b.double().abs()).sum(0, keepdim=True)
    tol = parts * 2.0 ** -9 * partial_max + (c.batch * c.K) * 2.0 ** -24 * absprod
    tail_part = torch.matmul(at[:, c.kmain:].double().transpose(-1, -2), b[:, c.kmain:].double()).sum(0, keepdim=True)
    return RandomData(at, b, torch.zeros((c.batch, 0, c.N)), prefill, empty, want, tol, tail_part, parts, partial_max)


def tail_visible_fraction(r: RandomData) -> float:
    return float((r.tail_part.abs() > r.tol).double().mean())


# ------------------------------------------------------------------------------------------ device operands
def device_operands(c: Case, data, dev):
    """(A view [.., M, K], B view [.., K, N], C window [.., M, N] of the padded buffer, the padded buffer, bias or None) on `dev`."""
    a_rm, b_t = c.layout
    at, b = data.at, data.b
    if c.batch == 1:
        at, b = at[0], b[0]
    a_store = (at.transpose(-1, -2).contiguous() if a_rm else at).to(dev, c.dta)
    A = a_store if a_rm else a_store.transpose(-1, -2)
    if c.window:
        buf = torch.cat([data.filler[:, :WINDOW_LEAD], data.b, data.filler[:, WINDOW_LEAD:]], 1).to(dev, c.dtb)
        B = buf[:, WINDOW_LEAD:WINDOW_LEAD + c.K]
        assert not B.is_contiguous()
    else:
        b_store = (b.transpose(-1, -2).contiguous() if b_t else b).to(dev, c.dtb)
        B = b_store.transpose(-1, -2) if b_t else b_store
    nc = data.prefill.shape[0]
    full = torch.full((nc, c.M + ROW_PAD, c.N + COL_PAD), PAD_FILL, device=dev, dtype=f32)
    full[:, :c.M, :c.N] = data.prefill.to(dev)
    if nc == 1:
        win = full[0, :c.M, :c.N]
        out = win.expand(c.batch, c.M, c.N) if c.batch > 1 else win
    else:
        out = full[:, :c.M, :c.N]
    bias = data.bias.to(dev) if data.bias.numel() else None
    return A, B, out, full, bias


def pad_untouched(c: Case, full: torch.Tensor) -> bool:
    return bool((full[:, c.M:] == PAD_FILL).all()) and bool((full[:, :, c.N:] == PAD_FILL).all())
