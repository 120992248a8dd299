"""Every launch form of the kernels that walk the token sequence: ONE table of cases for the CPU and the GPU test.

csrc/ppeg.hip (mh_ppeg_fwd, mh_ppeg_wgrad) and the non-MFMA half of csrc/nystrom_aux.hip (mh_resconv_fwd / _wgrad / _bwd, mh_landmark_fwd /
_bwd, mh_seq_finish / _bwd) choose on the host between several kernels and up to four dtype instances each.  Every case names the form
it is built to reach ("<entry>:<form>", what kernels.last_form() answers after the call; mh_seq_finish has one kernel and notes nothing);
the sizes are the smallest at which that form or seam is still reached.  B = 2 unless the size says otherwise, so a wrong batch stride shows.

sizes / dtypes / place per entry (place: one letter code per operand, in the order given here):
  ppeg_fwd        (B, S, D), opt = flip          (x, y)            place (x, y)
  ppeg_wgrad      (B, S, D)                      (x, dout)         place (x, dout)
  resconv_fwd     (B, n_p, heads, dh, taps), opt = (transpose, accumulate)    (v, out)     place (v, out)
  resconv_wgrad   (B, n_p, heads, dh, taps)      (v, dout)         place (v, dout)
  resconv_bwd     (B, n_p, heads, dh, taps)      (v, dout)         place (dout, v, dv)       (dv has v's dtype)
  landmark_fwd    (B, m, l, D)                   (t,)              place (qkv, lm)
  landmark_bwd    (B, m, l, D)                   (t,)              place (dlm, dqkv)
  seq_finish, seq_finish_bwd    (B, N, add, D)   (t,)

Placement: "a" = a tensor of its own (256-byte aligned); "o" = a view one element into a larger buffer; "o4" = four elements in (a
bf16 pointer that is 8- but not 16-byte aligned); "blk" = the v column block of a [B, n_p, 3 C] buffer, as the model hands res_conv its
operands.  Outputs are windows of buffers filled with 7.0 (`Out.guards_ok`); for "blk" the q and k columns are part of the guard.

Data kinds:
  integer   small integers (filters in {-1, 0, 1}, inputs in [-2, 2], addends in [-8, 8]; landmarks: inputs in [-8, 8] with l a power of
            two): every f64 reference value is a number of the output dtype and every f32 partial sum stays below 2^24, so the result must
            EQUAL the reference (test_seq_forms_cpu checks both).
  random    operands rounded to their storage dtype first; a per-element bound `tol`, derived and never measured: an output that is a sum
            of T products in f32, in any order, is within (T + 2) 2^-23 sum |a_j| |b_j| (gamma_T with a factor 2 for its denominator; the sum
            by the f64 reference on absolute values), plus 2^-23 |addend| where the kernel accumulates, plus 2^-8 |want| once for a bf16
            output, plus 2^-22 |mean| for a landmark mean over an l that is no power of two (the multiply by 1.f / l).  For the weight
            gradients T counts every term (B x rows x columns), so the bound holds for any order of atomics.
            Every random case carries `wrong`: references with a bug of the class its form invites (see the builders).  Each differs
            from the true one by more than 10 tol somewhere (test_seq_forms_cpu), so the bound cannot hide such a bug.  The gradient
            operands of the weight-gradient cases are drawn around +1: a lost row is then a systematic 1 / rows of the sum.

References are plain f64 torch written from the definitions (sums over taps and rows), not conv2d.
"""
from __future__ import annotations

import functools
import itertools
import math
import zlib
from dataclasses import dataclass, field

import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
NM = {bf16: "b", f32: "f"}
FILL, LEAD, TAIL_PAD = 7.0, 8, 8
PAIRS = list(itertools.product((f32, bf16), repeat=2))            # ff, fb, bf, bb
EPS = 2.0 ** -23

PX_T, PY_T = 8, 16                                               # ppeg_strip_kernel: pixels along x per thread, grid rows per strip
PPEG_STRIP_S = (1, 7, 8, 9, 16, 17, 23)
PPEG_STRIP_D = (1, 33, 257)
PPEG_PAIR_S, PPEG_PAIR_D = (1, 4, 5), (2, 6, 514)
PPEG_WGRAD_S, PPEG_WGRAD_D = (1, 4, 5, 9), (1, 33, 65)
LM_L, LM_D, LM_M = (1, 2, 3, 4, 6, 9), (3, 4, 6, 8), (1, 5)
SEQ_NADD, SEQ_D = ((1, 0), (1, 1), (5, 5), (20, 5)), (1, 5, 24)


@dataclass(frozen=True)
class Case:
    entry: str
    id: str
    form: str                       # kernels.last_form() after the call ("" where the entry point notes none)
    kind: str                       # "integer" | "random"
    sizes: tuple
    dtypes: tuple
    place: tuple = ()               # () = all "a"
    opt: tuple = ()

    def __str__(self) -> str:
        return f"{self.entry}-{self.id}"

    def placed(self, i: int) -> str:
        return self.place[i] if self.place else "a"


def _dn(dts) -> str:
    return "".join(NM[d] for d in dts)


def _kinds(i: int) -> str:
    """Every third case of a list is an integer case: the period shares no factor with the flip / dtype / option loops it runs through."""
    return "integer" if i % 3 == 0 else "random"


# ------------------------------------------------------------------------------------------ the host rules, restated
def place_offset_bytes(how: str, dtype, C: int = 0) -> int:
    """Bytes between a 256-byte aligned allocation and the operand's first element."""
    esz = 4 if dtype == f32 else 2
    return {"a": 0, "o": esz, "o4": 4 * esz, "blk": (LEAD + 2 * C) * esz}[how]


def ppeg_fwd_form(D: int, dt_x, dt_y, off_x: int, off_y: int) -> str:
    """mh_ppeg_fwd: the channel-pair kernel for f32 -> f32, even D and 8-byte aligned pointers, ppeg_strip_kernel<TX, TY> otherwise."""
    return "ppeg_fwd:pair" if dt_x == f32 and dt_y == f32 and D % 2 == 0 and off_x % 8 == 0 and off_y % 8 == 0 else "ppeg_fwd:strip"


def _rows_ok(lds, offs) -> bool:
    return all(v % 8 == 0 for v in lds) and all(o % 16 == 0 for o in offs)


def resconv_fwd_form(heads: int, dh: int, taps: int, dt_v, dt_o, lds, offs) -> str:
    """mh_resconv_fwd.  lds = (ldv, v_bs, ldo, o_bs) in elements, offs = byte offsets of v and out."""
    if not (heads <= 8 or 255 // dh + 2 <= 8):
        return "resconv_fwd:none"
    if dt_v == bf16 and dt_o == bf16 and dh == 64 and taps == 33 and _rows_ok(lds, offs):
        return "resconv_fwd:mfma"
    if dh % 8 == 0 and _rows_ok(lds, offs) and (heads <= 8 or 511 // dh + 2 <= 8):
        return "resconv_fwd:vec"
    return "resconv_fwd:scalar"


def resconv_wgrad_form(heads: int, dh: int, taps: int, dt_v, dt_o, lds, offs) -> str:
    if dt_v == bf16 and dt_o == bf16 and dh == 64 and taps == 33 and _rows_ok(lds, offs):
        return "resconv_wgrad:mfma"
    return "resconv_wgrad:vec8" if dh % 8 == 0 and _rows_ok(lds, offs) else "resconv_wgrad:scalar"


def resconv_bwd_form(heads: int, dh: int, taps: int, dt_v, dt_o, lds, offs) -> str:
    """mh_resconv_bwd: one MFMA pass for bf16 / bf16 at dh = 64 with 33 taps and aligned rows, else mh_resconv_wgrad + mh_resconv_fwd."""
    if dt_v == bf16 and dt_o == bf16 and dh == 64 and taps == 33 and _rows_ok(lds, offs):
        return "resconv_bwd:mfma"
    return "resconv_bwd:two_pass"


def landmark_fwd_form(D: int, dtype, off_qkv: int, off_lm: int) -> str:
    quad = 4 * (4 if dtype == f32 else 2)
    return "landmark_fwd:quad" if D % 4 == 0 and off_qkv % quad == 0 and off_lm % quad == 0 else "landmark_fwd:scalar"


def landmark_bwd_form(D: int, dtype, off_dlm: int, off_dqkv: int) -> str:
    return "landmark_bwd:oct" if D % 8 == 0 and off_dlm % 16 == 0 and off_dqkv % 16 == 0 else "landmark_bwd:scalar"


def _ld(how: str, n_p: int, C: int):
    """(row stride, batch stride) in elements of a [B, n_p, C] operand placed `how`."""
    return (3 * C, n_p * 3 * C) if how == "blk" else (C, n_p * C)


def predicted_form(c: Case) -> str:
    """The form the host rule picks for case c, from its sizes, dtypes and placement alone."""
    d, P = c.dtypes, c.placed
    if c.entry == "ppeg_fwd":
        return ppeg_fwd_form(c.sizes[2], d[0], d[1], place_offset_bytes(P(0), d[0]), place_offset_bytes(P(1), d[1]))
    if c.entry == "ppeg_wgrad":
        return "ppeg_wgrad:strip"
    if c.entry in ("resconv_fwd", "resconv_wgrad", "resconv_bwd"):
        B, n_p, heads, dh, taps = c.sizes
        C = heads * dh
        if c.entry == "resconv_bwd":
            ops = ((P(1), d[0]), (P(0), d[1]), (P(2), d[0]))           # v, dout, dv
        else:
            ops = ((P(0), d[0]), (P(1), d[1]))
        lds = tuple(x for how, _ in ops for x in _ld(how, n_p, C))
        offs = tuple(place_offset_bytes(how, t, C) for how, t in ops)
        rule = {"resconv_fwd": resconv_fwd_form, "resconv_wgrad": resconv_wgrad_form, "resconv_bwd": resconv_bwd_form}[c.entry]
        return rule(heads, dh, taps, d[0], d[1], lds, offs)
    if c.entry in ("landmark_fwd", "landmark_bwd"):
        rule = landmark_fwd_form if c.entry == "landmark_fwd" else landmark_bwd_form
        return rule(c.sizes[3], d[0], place_offset_bytes(P(0), d[0]), place_offset_bytes(P(1), d[0]))
    return ""


# ------------------------------------------------------------------------------------------ the table
def _ppeg_cases():
    out = []

    def add(entry, form, B, S, D, dts, place=(), flip=None):
        cid = f"{_dn(dts)}-{B}x{S}x{D}" + ("" if flip is None else f"-flip{flip}") + ("-" + "".join(place) if place else "")
        out.append(Case(entry, cid, form, _kinds(len(out)), (B, S, D), dts, place, () if flip is None else (flip,)))
    # strip: every S x both flips x every dtype pair at D = 33; f32 -> f32 (odd D) at the other two D; the other pairs at the seams of D = 257
    for S, dts, flip in itertools.product(PPEG_STRIP_S, PAIRS, (0, 1)):
        add("ppeg_fwd", "ppeg_fwd:strip", 2, S, 33, dts, flip=flip)
    for S, D, flip in itertools.product(PPEG_STRIP_S, (1, 257), (0, 1)):
        add("ppeg_fwd", "ppeg_fwd:strip", 2, S, D, (f32, f32), flip=flip)
    for i, (S, dts) in enumerate(itertools.product((9, 17), PAIRS[1:])):
        add("ppeg_fwd", "ppeg_fwd:strip", 2, S, 257, dts, flip=i % 2)
    # pair, and the seam between the two forms: the same inputs at D = 6 aligned (pair) and with x or y one element into its buffer (strip)
    for S, D, flip in itertools.product(PPEG_PAIR_S, PPEG_PAIR_D, (0, 1)):
        for kind in ("integer", "random") if D == 6 else (_kinds(len(out)),):
            cid = f"ff-2x{S}x{D}-flip{flip}-{kind[0]}"
            out.append(Case("ppeg_fwd", cid, "ppeg_fwd:pair", kind, (2, S, D), (f32, f32), (), (flip,)))
            if D == 6:
                out.append(Case("ppeg_fwd", cid + "-oa", "ppeg_fwd:strip", kind, (2, S, D), (f32, f32), ("o", "a"), (flip,)))
    out.append(Case("ppeg_fwd", "ff-2x5x6-flip0-r-ao", "ppeg_fwd:strip", "random", (2, 5, 6), (f32, f32), ("a", "o"), (0,)))
    # weight gradient: strips per image 1, 1, 2, 3 (x 4 waves per workgroup: idle waves join the LDS reduction), D = 65: a second channel group of one lane
    for S, D, dts in itertools.product(PPEG_WGRAD_S, PPEG_WGRAD_D, PAIRS):
        add("ppeg_wgrad", "ppeg_wgrad:strip", 2, S, D, dts)
    for dts in PAIRS:        # S = 65: two equal strips of 33 + 32 rows
        out.append(Case("ppeg_wgrad", f"{_dn(dts)}-1x65x8", "ppeg_wgrad:strip", "integer" if dts[0] == dts[1] else "random", (1, 65, 8), dts))
    out.append(Case("ppeg_wgrad", "ff-2x9x33-oa", "ppeg_wgrad:strip", "random", (2, 9, 33), (f32, f32), ("o", "a")))
    return out


def _resconv_cases():
    out = []

    def add(entry, form, n_p, heads, dh, taps, dts, place=(), opt=(), kind=None, B=2):
        cid = f"{_dn(dts)}-{B}x{n_p}x{heads}x{dh}-t{taps}" + ("-" + "".join(str(v) for v in opt) if opt else "") + ("-" + ",".join(place) if place else "")
        kind = kind or _kinds(len(out))
        out.append(Case(entry, f"{cid}-{kind[0]}", form, kind, (B, n_p, heads, dh, taps), dts, place, opt))
    ta = list(itertools.product((0, 1), (0, 1)))
    # ---- resconv_fwd:vec
    for dts, opt in itertools.product(PAIRS, ta):                            # every instance x transpose x accumulate; n_p = 17 of 3 taps
        add("resconv_fwd", "resconv_fwd:vec", 17, 2, 8, 3, dts, opt=opt)
    for dts in ((f32, f32), (bf16, bf16)):
        add("resconv_fwd", "resconv_fwd:vec", 33, 3, 24, 33, dts, opt=(0, 0))      # a second 32-row block of one row
        add("resconv_fwd", "resconv_fwd:vec", 16, 12, 96, 33, dts, opt=(1, 0))     # 12 heads (511 / 96 + 2 = 7); n_p below the half-width
    for dts, opt in itertools.product(PAIRS, ((0, 0), (1, 1))):              # the template: C = 768, the second 512-column block starts at head 5, column 32
        add("resconv_fwd", "resconv_fwd:vec", 40, 8, 96, 33, dts, ("blk", "blk"), opt, kind="random" if opt == (0, 0) else "integer")
    add("resconv_fwd", "resconv_fwd:vec", 1, 1, 8, 1, (f32, f32), opt=(0, 1))
    add("resconv_fwd", "resconv_fwd:vec", 40, 2, 8, 63, (bf16, bf16), opt=(1, 1))
    add("resconv_fwd", "resconv_fwd:vec", 40, 2, 8, 63, (f32, f32), opt=(0, 0), kind="random")
    for kind in ("integer", "random"):                                       # bf16, dh = 64, one step outside the MFMA admission by its taps
        add("resconv_fwd", "resconv_fwd:vec", 33, 2, 64, 31, (bf16, bf16), opt=(0, 1), kind=kind)
    # ---- resconv_fwd:scalar
    for dts, opt in itertools.product(PAIRS, ta):
        add("resconv_fwd", "resconv_fwd:scalar", 17, 2, 4, 3, dts, opt=opt)
    for dts in ((f32, f32), (bf16, bf16)):
        add("resconv_fwd", "resconv_fwd:scalar", 33, 8, 12, 33, dts, opt=(0, 0))
    for kind in ("integer", "random"):                                       # 12 heads x 64: 511 / 64 + 2 = 9 heads in a 512-column block
        add("resconv_fwd", "resconv_fwd:scalar", 16, 12, 64, 33, (f32, f32), opt=(1, 1), kind=kind)
    add("resconv_fwd", "resconv_fwd:scalar", 17, 2, 8, 3, (bf16, bf16), ("o4", "a"), (0, 0))      # dh = 8, the pointer not 16-byte aligned
    add("resconv_fwd", "resconv_fwd:scalar", 17, 2, 8, 3, (f32, f32), ("o", "a"), (0, 1))
    add("resconv_fwd", "resconv_fwd:scalar", 17, 2, 8, 3, (f32, f32), ("a", "o"), (1, 1), kind="random")
    for kind in ("integer", "random"):                                       # bf16, dh = 64, 33 taps, one step outside the MFMA admission by its pointer
        add("resconv_fwd", "resconv_fwd:scalar", 40, 2, 64, 33, (bf16, bf16), ("o4", "a"), (0, 0), kind=kind)
    add("resconv_fwd", "resconv_fwd:scalar", 1, 1, 4, 1, (f32, f32), opt=(0, 0))
    add("resconv_fwd", "resconv_fwd:scalar", 40, 2, 4, 63, (f32, f32), opt=(1, 0), kind="random")
    add("resconv_fwd", "resconv_fwd:scalar", 40, 2, 4, 63, (bf16, bf16), opt=(0, 1), kind="integer")
    # ---- resconv_wgrad
    W = "resconv_wgrad"
    for dts, kind in itertools.product(PAIRS, ("integer", "random")):
        add(W, W + ":scalar", 65, 2, 4, 33, dts, kind=kind)
        add(W, W + ":vec8", 65, 2, 72, 33, dts, kind=kind)                   # dh = 72: a second chunk of 8 columns; n_p = 65: a second row block of one row
    add(W, W + ":scalar", 1, 1, 4, 1, (f32, f32), kind="random")
    add(W, W + ":scalar", 100, 2, 4, 63, (f32, f32), kind="random")
    add(W, W + ":scalar", 100, 2, 4, 63, (bf16, bf16), kind="integer")
    for dts in PAIRS[:3]:
        add(W, W + ":vec8", 64, 2, 64, 33, dts)
    add(W, W + ":vec8", 63, 2, 64, 63, (bf16, bf16), kind="random")        # 63 taps: both passes of a thread's two taps
    add(W, W + ":vec8", 63, 2, 64, 63, (bf16, bf16), kind="integer")
    for dts, kind in (((f32, f32), "random"), ((bf16, bf16), "integer")):    # the template's block placement, dh = 96 = 64 + 32
        add(W, W + ":vec8", 63, 8, 96, 33, dts, ("blk", "blk"), kind=kind)
    add(W, W + ":vec8", 100, 12, 96, 33, (f32, f32), kind="integer")       # the largest case: n_p = 100, C = 1152
    add(W, W + ":vec8", 1, 1, 136, 1, (f32, f32), kind="random")
    add(W, W + ":vec8", 64, 2, 136, 63, (f32, f32), kind="integer")        # 136 = 64 + 64 + 8
    add(W, W + ":vec8", 33, 2, 136, 63, (bf16, bf16), kind="random")
    add(W, W + ":scalar", 65, 2, 64, 33, (bf16, bf16), ("o4", "a"), kind="random")     # misaligned: neither MFMA nor 8-column loads
    add(W, W + ":scalar", 65, 2, 72, 33, (f32, f32), ("a", "o"), kind="integer")       # the scalar loads in the d0 loop
    # ---- resconv_bwd: the two-pass fall-back (dw by mh_resconv_wgrad, then dv += the transposed conv of dout)
    Bw = "resconv_bwd"
    for kind in ("integer", "random"):
        add(Bw, Bw + ":two_pass", 17, 2, 8, 3, (f32, f32), kind=kind)
        add(Bw, Bw + ":two_pass", 17, 2, 4, 3, (f32, f32), ("a", "blk", "blk"), kind=kind)
        add(Bw, Bw + ":two_pass", 33, 2, 8, 33, (bf16, f32), ("a", "blk", "blk"), kind=kind)          # bf16 v, f32 dout: the mixed second pass
        add(Bw, Bw + ":two_pass", 40, 8, 96, 33, (bf16, bf16), ("a", "blk", "blk"), kind=kind)
    return out


def _landmark_cases():
    out = []
    for entry in ("landmark_fwd", "landmark_bwd"):
        for l, D, m, t in itertools.product(LM_L, LM_D, LM_M, (f32, bf16)):
            if m == 1 and D in (4, 6):
                continue
            off = (0, 0)
            form = landmark_fwd_form(D, t, *off) if entry == "landmark_fwd" else landmark_bwd_form(D, t, *off)
            kind = "integer" if l in (1, 2, 4) and m == 5 else "random"
            out.append(Case(entry, f"{NM[t]}-2x{m}x{l}x{D}", form, kind, (2, m, l, D), (t,)))
        for t, place in itertools.product((f32, bf16), (("o", "a"), ("a", "o"))):     # D = 8 through a misaligned view: the scalar form
            out.append(Case(entry, f"{NM[t]}-2x5x6x8-{''.join(place)}", f"{entry}:scalar", "random", (2, 5, 6, 8), (t,), place))
    return out


def _seq_cases():
    out = []
    for entry in ("seq_finish", "seq_finish_bwd"):
        for (N, add), D, t in itertools.product(SEQ_NADD, SEQ_D, (f32, bf16)):
            out.append(Case(entry, f"{NM[t]}-2x{N}+{add}x{D}", "", "integer", (2, N, add, D), (t,)))
    return out


CASES = _ppeg_cases() + _resconv_cases() + _landmark_cases() + _seq_cases()
assert len({str(c) for c in CASES}) == len(CASES)


def by_id(name: str) -> Case:
    return next(c for c in CASES if str(c) == name)


# ------------------------------------------------------------------------------------------ f64 references, from the definitions
def _ppeg_pad(grid: torch.Tensor, clamp: bool) -> torch.Tensor:
    """[B, S, S, D] -> [B, S + 6, S + 6, D]: three rows / columns of zeros all round (clamp: of the nearest border pixel — a wrong reference)."""
    B, S, _, D = grid.shape
    if clamp:
        idx = torch.arange(-3, S + 3).clamp(0, S - 1)
        return grid[:, idx][:, :, idx]
    pad = torch.zeros(B, S + 6, S + 6, D, dtype=grid.dtype)
    pad[:, 3:3 + S, 3:3 + S] = grid
    return pad


def ppeg64(x, merged, bsum, S: int, flip: int, *, ring: bool = False, clamp: bool = False) -> torch.Tensor:
    """y[b, 1 + yy S + xx, c] = bsum[c] + sum_{ky, kx} merged[7 ky + kx, c] x[b, 1 + (yy + ky - 3) S + (xx + kx - 3), c] over the pixels
    inside the grid; flip: tap 48 - t in place of t and no bias (the adjoint).  Row 0 (cls) passes through.
    Wrong references: ring = the outermost ring of the 7 x 7 left out; clamp = the border clamped instead of zero-padded."""
    x, merged, bsum = x.double(), merged.double(), bsum.double()
    B, n, D = x.shape
    pad = _ppeg_pad(x[:, 1:].reshape(B, S, S, D), clamp)
    acc = torch.zeros(B, S, S, D, dtype=f64) if flip else bsum.expand(B, S, S, D).clone()
    for t in range(49):
        ky, kx = divmod(t, 7)
        if ring and (ky in (0, 6) or kx in (0, 6)):
            continue
        acc += merged[48 - t if flip else t] * pad[:, ky:ky + S, kx:kx + S]
    return torch.cat([x[:, :1], acc.reshape(B, S * S, D)], dim=1)


def ppeg_wgrad64(x, dout, S: int, *, drop_last_row: bool = False):
    """dmerged[7 ky + kx, c] = sum_{b, yy, xx} dout[b, yy, xx, c] x[b, yy + ky - 3, xx + kx - 3, c], dbsum[c] = sum dout (grid rows only).
    Wrong reference: drop_last_row = the last grid row of dout left out."""
    x, dout = x.double(), dout.double()
    B, n, D = x.shape
    pad = _ppeg_pad(x[:, 1:].reshape(B, S, S, D), False)
    g = dout[:, 1:].reshape(B, S, S, D).clone()
    if drop_last_row:
        g[:, S - 1] = 0.0
    dm = torch.stack([(g * pad[:, t // 7:t // 7 + S, t % 7:t % 7 + S]).sum((0, 1, 2)) for t in range(49)])
    return dm, g.sum((0, 1, 2))


def _tap_columns(w, heads: int, dh: int, j: int, mid_head: bool) -> torch.Tensor:
    """Tap j of every column's head: [C].  mid_head (a wrong reference): the columns from the start of a 512-column block that begins in
    the middle of a head up to that head's end take the NEXT head's taps."""
    C = heads * dh
    col = torch.arange(C)
    h = col // dh
    if mid_head:
        blk = col // 512 * 512
        h = torch.where((blk > 0) & (blk % dh != 0) & (col // dh == blk // dh), (h + 1) % heads, h)
    return w[h, j]


def resconv64(v, w, heads: int, transpose: int, *, shift: int = 0, drop_last_tap: bool = False, mid_head: bool = False) -> torch.Tensor:
    """out[b, t, c] = sum_j w[c / dh][jj] v[b, t + j - taps / 2, c] over the rows inside the sequence, jj = j, or taps - 1 - j transposed.
    Wrong references: shift = the window one row down; drop_last_tap; mid_head (see _tap_columns)."""
    v, w = v.double(), w.double()
    B, n_p, C = v.shape
    taps = w.shape[1]
    half, dh = taps // 2, C // heads
    pad = torch.zeros(B, n_p + 2 * half + 2, C, dtype=f64)
    pad[:, half + 1:half + 1 + n_p] = v                        # row r of v sits at r + half + 1
    out = torch.zeros(B, n_p, C, dtype=f64)
    for j in range(taps - 1 if drop_last_tap else taps):
        wj = _tap_columns(w, heads, dh, taps - 1 - j if transpose else j, mid_head)
        out += wj * pad[:, j + 1 + shift:j + 1 + shift + n_p]
    return out


def resconv_wgrad64(v, dout, heads: int, taps: int, *, drop_last_row: bool = False, cols_from: int = 0) -> torch.Tensor:
    """dw[h][j] = sum_{b, t, d} dout[b, t, h dh + d] v[b, t + j - taps / 2, h dh + d].
    Wrong references: drop_last_row = the last row of dout left out; cols_from = 64: the columns d >= 64 of every head left out."""
    v, g = v.double(), dout.double().clone()
    B, n_p, C = v.shape
    half, dh = taps // 2, C // heads
    if drop_last_row:
        g[:, n_p - 1] = 0.0
    if cols_from:
        g.view(B, n_p, heads, dh)[..., cols_from:] = 0.0
    pad = torch.zeros(B, n_p + 2 * half, C, dtype=f64)
    pad[:, half:half + n_p] = v
    return torch.stack([(g * pad[:, j:j + n_p]).view(B, n_p, heads, dh).sum((0, 1, 3)) for j in range(taps)], dim=1)      # [heads, taps]


def landmark64(qkv, l: int, *, drop_last: bool = False) -> torch.Tensor:
    """lm[b, j, c] = (1 / l) sum_t qkv[b, j l + t, c] for the q and k columns c < 2 D.  Wrong reference: the last row of each group left out."""
    B, n_p, D3 = qkv.shape
    g = qkv.double()[:, :, :2 * (D3 // 3)].reshape(B, n_p // l, l, 2 * (D3 // 3))
    return (g[:, :, :l - 1] if drop_last else g).sum(2) / l


def landmark_bwd64(dlm, dqkv, l: int, *, drop_last: bool = False) -> torch.Tensor:
    """dqkv[b, r, c] += dlm[b, r / l, c] / l for c < 2 D; the v columns stay.  Wrong reference: the last row of each group gets nothing."""
    B, n_p, D3 = dqkv.shape
    D2 = 2 * (D3 // 3)
    g = (dlm.double() / l).repeat_interleave(l, dim=1)
    if drop_last:
        g = g.clone()
        g[:, l - 1::l] = 0.0
    out = dqkv.double().clone()
    out[:, :, :D2] += g
    return out


# ------------------------------------------------------------------------------------------ data
@dataclass
class Built:
    inputs: dict                                    # name -> CPU f32 tensor holding the STORED values (rounded to the operand's dtype)
    want: dict                                      # output name -> f64 reference
    tol: dict = field(default_factory=dict)         # output name -> f64 per-element bound (random cases)
    wrong: dict = field(default_factory=dict)       # bug name -> {output name: f64 reference with that bug} (random cases)
    prefill: dict = field(default_factory=dict)     # output name -> what the output holds before the call
    f32_sum_bound: float = 0.0                      # integer cases: the largest |partial sum| any f32 accumulation can reach


def _gen(c: Case) -> torch.Generator:
    """Seeded by what the data depends on — not by the placement, so a case and its misaligned twin see the same inputs."""
    return torch.Generator().manual_seed(zlib.crc32(repr((c.entry, c.kind, c.sizes, c.opt)).encode()))


def _ints(gen, lo, hi, shape) -> torch.Tensor:
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def stored(t: torch.Tensor, dtype) -> torch.Tensor:
    """t as the device will hold it: rounded once to dtype, back as f32."""
    return t.float().to(dtype).float()


def _bf16_term(dtype, want):
    return 2.0 ** -8 * want.abs() if dtype == bf16 else torch.zeros_like(want)


def _operand(c: Case, gen, shape, dtype, lo, hi, centre: float = 0.0) -> torch.Tensor:
    if c.kind == "integer":
        return _ints(gen, lo, hi, shape)
    return stored(torch.randn(tuple(shape), generator=gen) * (0.5 if centre else 1.0) + centre, dtype)


def _build_ppeg_fwd(c: Case, gen) -> Built:
    B, S, D = c.sizes
    flip = c.opt[0]
    n = 1 + S * S
    x = _operand(c, gen, (B, n, D), c.dtypes[0], -2, 2)
    if c.kind == "integer":
        merged, bsum = _ints(gen, -1, 1, (49, D)), _ints(gen, -8, 8, (D,))
    else:
        merged, bsum = torch.randn(49, D, generator=gen) * 0.3, torch.randn(D, generator=gen)
    want = ppeg64(x, merged, bsum, S, flip)
    b = Built({"x": x, "merged": merged, "bsum": bsum}, {"y": want}, f32_sum_bound=49 * 2.0 + 8.0)
    if c.kind == "random":
        mag = ppeg64(x.abs(), merged.abs(), bsum.abs(), S, flip)       # sum |a| |b|, the bias a product with 1; the cls row is a copy
        mag[:, 0] = 0.0
        b.tol = {"y": (50 + 2) * EPS * mag + _bf16_term(c.dtypes[1], want)}
        b.wrong = {"clamp": {"y": ppeg64(x, merged, bsum, S, flip, clamp=True)}}
        if S >= 4:          # below, no pixel has a neighbour three away: the ring meets nothing but padding
            b.wrong["ring"] = {"y": ppeg64(x, merged, bsum, S, flip, ring=True)}
        if not flip:
            b.wrong["no_bias"] = {"y": ppeg64(x, merged, torch.zeros(D), S, 0)}
        else:
            b.wrong["bias"] = {"y": ppeg64(x, merged.flip(0), bsum, S, 0)}            # the adjoint must add none
            if S >= 2:      # a 1 x 1 grid meets the centre tap alone, which is its own mirror image
                b.wrong["no_flip"] = {"y": ppeg64(x, merged, torch.zeros(D), S, 0)}
    return b


def _build_ppeg_wgrad(c: Case, gen) -> Built:
    B, S, D = c.sizes
    n = 1 + S * S
    x = _operand(c, gen, (B, n, D), c.dtypes[0], -2, 2, centre=1.0)
    g = _operand(c, gen, (B, n, D), c.dtypes[1], -2, 2, centre=1.0)
    pre_m, pre_b = _ints(gen, -8, 8, (49, D)), _ints(gen, -8, 8, (D,))
    dm, dbs = ppeg_wgrad64(x, g, S)
    b = Built({"x": x, "dout": g}, {"dmerged": pre_m.double() + dm, "dbsum": pre_b.double() + dbs}, prefill={"dmerged": pre_m, "dbsum": pre_b},
              f32_sum_bound=4.0 * B * S * S + 8.0)
    if c.kind == "random":
        T = B * S * S
        am, ab = ppeg_wgrad64(x.abs(), g.abs(), S)
        b.tol = {"dmerged": (T + 2) * EPS * am + EPS * pre_m.abs().double(), "dbsum": (T + 2) * EPS * ab + EPS * pre_b.abs().double()}
        wm, wb = ppeg_wgrad64(x, g, S, drop_last_row=True)
        b.wrong = {"last_row": {"dmerged": pre_m.double() + wm, "dbsum": pre_b.double() + wb}}
    return b


def _resconv_operands(c: Case, gen, centre: float = 0.0):
    B, n_p, heads, dh, taps = c.sizes
    C = heads * dh
    v = _operand(c, gen, (B, n_p, C), c.dtypes[0], -2, 2, centre)
    w = _ints(gen, -1, 1, (heads, taps)) if c.kind == "integer" else torch.randn(heads, taps, generator=gen) * 0.3
    return B, n_p, heads, dh, taps, C, v, w


def _resconv_fwd_parts(c: Case, v, w, heads, transpose, dt_out, pre):
    """(want, tol, wrong) of out = pre + conv(v): shared by resconv_fwd and the second pass of resconv_bwd."""
    taps = w.shape[1]
    add = pre.double() if pre is not None else 0.0
    want = add + resconv64(v, w, heads, transpose)
    if c.kind != "random":
        return want, None, {}
    tol = (taps + 2) * EPS * resconv64(v.abs(), w.abs(), heads, transpose) + _bf16_term(dt_out, want)
    if pre is not None:
        tol = tol + EPS * pre.abs().double()
    wrong = {"shift": add + resconv64(v, w, heads, transpose, shift=1)}
    if v.shape[1] > taps // 2:      # a shorter sequence never reaches the last tap
        wrong["last_tap"] = add + resconv64(v, w, heads, transpose, drop_last_tap=True)
    C, dh = v.shape[2], v.shape[2] // heads
    if C > 512 and 512 % dh != 0:
        wrong["mid_head"] = add + resconv64(v, w, heads, transpose, mid_head=True)
    if taps > 1 and v.shape[1] > 1:
        wrong["transpose"] = add + resconv64(v, w, heads, 1 - transpose)
    return want, tol, wrong


def _build_resconv_fwd(c: Case, gen) -> Built:
    B, n_p, heads, dh, taps, C, v, w = _resconv_operands(c, gen)
    transpose, accumulate = c.opt
    pre = _operand(c, gen, (B, n_p, C), c.dtypes[1], -8, 8) if accumulate else None
    want, tol, wrong = _resconv_fwd_parts(c, v, w, heads, transpose, c.dtypes[1], pre)
    b = Built({"v": v, "w": w}, {"out": want}, f32_sum_bound=2.0 * taps + 8.0)
    if accumulate:
        b.prefill = {"out": pre}
    if c.kind == "random":
        b.tol, b.wrong = {"out": tol}, {k: {"out": t} for k, t in wrong.items()}
    return b


def _resconv_wgrad_parts(c: Case, v, g, heads, taps, pre):
    B, n_p, C = v.shape
    dh = C // heads
    want = pre.double() + resconv_wgrad64(v, g, heads, taps)
    if c.kind != "random":
        return want, None, {}
    T = B * n_p * dh
    tol = (T + 2) * EPS * resconv_wgrad64(v.abs(), g.abs(), heads, taps) + EPS * pre.abs().double()
    wrong = {"last_row": pre.double() + resconv_wgrad64(v, g, heads, taps, drop_last_row=True)}
    if dh > 64:
        wrong["cols_from_64"] = pre.double() + resconv_wgrad64(v, g, heads, taps, cols_from=64)
    return want, tol, wrong


def _build_resconv_wgrad(c: Case, gen) -> Built:
    B, n_p, heads, dh, taps, C, v, _ = _resconv_operands(c, gen, centre=1.0)
    g = _operand(c, gen, (B, n_p, C), c.dtypes[1], -2, 2, centre=1.0)
    pre = _ints(gen, -8, 8, (heads, taps))
    want, tol, wrong = _resconv_wgrad_parts(c, v, g, heads, taps, pre)
    b = Built({"v": v, "dout": g}, {"dw": want}, prefill={"dw": pre}, f32_sum_bound=4.0 * B * n_p * dh + 8.0)
    if c.kind == "random":
        b.tol, b.wrong = {"dw": tol}, {k: {"dw": t} for k, t in wrong.items()}
    return b


def _build_resconv_bwd(c: Case, gen) -> Built:
    """dv += the transposed conv of dout (dv in v's dtype), dw += the tap gradient."""
    B, n_p, heads, dh, taps, C, v, w = _resconv_operands(c, gen, centre=1.0)
    g = _operand(c, gen, (B, n_p, C), c.dtypes[1], -2, 2, centre=1.0)
    pre_w = _ints(gen, -8, 8, (heads, taps))
    pre_v = _operand(c, gen, (B, n_p, C), c.dtypes[0], -8, 8)
    dw, tol_w, wrong_w = _resconv_wgrad_parts(c, v, g, heads, taps, pre_w)
    dv, tol_v, wrong_v = _resconv_fwd_parts(c, g, w, heads, 1, c.dtypes[0], pre_v)
    b = Built({"v": v, "dout": g, "w": w}, {"dv": dv, "dw": dw}, prefill={"dv": pre_v, "dw": pre_w}, f32_sum_bound=4.0 * B * n_p * dh + 8.0)
    if c.kind == "random":
        b.tol = {"dv": tol_v, "dw": tol_w}
        b.wrong = {**{k: {"dv": dv, "dw": t} for k, t in wrong_w.items()}, **{k: {"dv": t, "dw": dw} for k, t in wrong_v.items()}}
    return b


def _lm_operands(c: Case, gen):
    B, m, l, D = c.sizes
    return B, m, l, D, m * l


def _build_landmark_fwd(c: Case, gen) -> Built:
    B, m, l, D, n_p = _lm_operands(c, gen)
    qkv = _operand(c, gen, (B, n_p, 3 * D), c.dtypes[0], -8, 8)
    want = landmark64(qkv, l)
    b = Built({"qkv": qkv}, {"lm": want}, f32_sum_bound=8.0 * l)
    if c.kind == "random":
        tol = (l + 2) * EPS * landmark64(qkv.abs(), l) + _bf16_term(c.dtypes[0], want)
        if l & (l - 1):
            tol = tol + 2.0 ** -22 * want.abs()
        b.tol, b.wrong = {"lm": tol}, {"last_row": {"lm": landmark64(qkv, l, drop_last=True)}}
    return b


def _build_landmark_bwd(c: Case, gen) -> Built:
    B, m, l, D, n_p = _lm_operands(c, gen)
    dlm = _operand(c, gen, (B, m, 2 * D), c.dtypes[0], -8, 8)
    pre = _operand(c, gen, (B, n_p, 3 * D), c.dtypes[0], -8, 8)
    want = landmark_bwd64(dlm, pre, l)
    b = Built({"dlm": dlm}, {"dqkv": want}, prefill={"dqkv": pre}, f32_sum_bound=16.0)
    if c.kind == "random":
        # one product (dlm x 1.f / l) and the addend: T = 1; the rounded 1.f / l of an l that is no power of two is 2^-22 of the product
        prod = landmark_bwd64(dlm.abs(), torch.zeros_like(pre), l)
        tol = (1 + 2) * EPS * prod + EPS * pre.abs().double() + _bf16_term(c.dtypes[0], want)
        if l & (l - 1):
            tol = tol + 2.0 ** -22 * prod
        b.tol, b.wrong = {"dqkv": tol}, {"last_row": {"dqkv": landmark_bwd64(dlm, pre, l, drop_last=True)}}
    return b


def _build_seq_finish(c: Case, gen) -> Built:
    """seq [B, 1 + N + add, D]: row 0 = cls, pad rows N + 1 .. N + add = rows 1 .. add; rows 1 .. N stay."""
    B, N, add, D = c.sizes
    seq, cls = _ints(gen, -8, 8, (B, 1 + N + add, D)), _ints(gen, -8, 8, (D,))
    want = seq.double().clone()
    want[:, 0] = cls.double()
    want[:, N + 1:] = want[:, 1:1 + add]
    return Built({"cls": cls}, {"seq": want}, prefill={"seq": seq}, f32_sum_bound=8.0)


def _build_seq_finish_bwd(c: Case, gen) -> Built:
    """dcls += sum_b dseq[b, 0]; dseq rows 1 .. add += the pad rows N + 1 .. N + add; everything else stays."""
    B, N, add, D = c.sizes
    dseq, pre = _ints(gen, -8, 8, (B, 1 + N + add, D)), _ints(gen, -3, 3, (D,))
    want = dseq.double().clone()
    want[:, 1:1 + add] += want[:, N + 1:]
    return Built({}, {"dseq": want, "dcls": pre.double() + dseq[:, 0].double().sum(0)}, prefill={"dseq": dseq, "dcls": pre}, f32_sum_bound=8.0 * B + 3.0)


_BUILDERS = {"ppeg_fwd": _build_ppeg_fwd, "ppeg_wgrad": _build_ppeg_wgrad, "resconv_fwd": _build_resconv_fwd, "resconv_wgrad": _build_resconv_wgrad,
             "resconv_bwd": _build_resconv_bwd, "landmark_fwd": _build_landmark_fwd, "landmark_bwd": _build_landmark_bwd,
             "seq_finish": _build_seq_finish, "seq_finish_bwd": _build_seq_finish_bwd}


@functools.lru_cache(maxsize=8)
def build(c: Case) -> Built:
    return _BUILDERS[c.entry](c, _gen(c))


def out_dtypes(c: Case) -> dict:
    """Output name -> dtype."""
    d = c.dtypes
    return {"ppeg_fwd": {"y": d[-1]}, "ppeg_wgrad": {"dmerged": f32, "dbsum": f32}, "resconv_fwd": {"out": d[-1]}, "resconv_wgrad": {"dw": f32},
            "resconv_bwd": {"dv": d[0], "dw": f32}, "landmark_fwd": {"lm": d[0]}, "landmark_bwd": {"dqkv": d[0]},
            "seq_finish": {"seq": d[0]}, "seq_finish_bwd": {"dseq": d[0], "dcls": f32}}[c.entry]


# ------------------------------------------------------------------------------------------ device operands and the call
@dataclass
class Out:
    win: torch.Tensor               # what the wrapper wrote into
    full: torch.Tensor              # the FILL-ed buffer around it
    inside: torch.Tensor            # bool, full's shape: the window

    def guards_ok(self) -> bool:
        return bool((self.full[~self.inside] == FILL).all())

    def untouched(self) -> bool:
        return bool((self.full == FILL).all())


_SHIFT = {"o": 1, "o4": 4}


def put(t: torch.Tensor, dtype, how: str, dev) -> torch.Tensor:
    if how == "a":
        return t.to(dev, dtype).contiguous()
    if how == "blk":                # the v column block of [B, n_p, 3 C]; the q and k columns hold 3.0
        B, n_p, C = t.shape
        buf = torch.full((B, n_p, 3 * C), 3.0, device=dev, dtype=dtype)
        buf[:, :, 2 * C:] = t.to(dev, dtype)
        return buf[:, :, 2 * C:]
    k = _SHIFT[how]
    buf = torch.zeros(t.numel() + k, device=dev, dtype=dtype)
    buf[k:] = t.reshape(-1).to(dev, dtype)
    v = buf[k:].view(t.shape)
    assert v.data_ptr() % 16 != 0 or (how == "o4" and dtype == f32)
    return v


def window(shape, dtype, how: str, dev, prefill=None) -> Out:
    n = int(math.prod(shape))
    if how == "blk":
        B, n_p, C = shape
        full = torch.full((LEAD + B * n_p * 3 * C + TAIL_PAD,), FILL, device=dev, dtype=dtype)
        inside = torch.zeros(full.shape, device=dev, dtype=torch.bool)
        win = full[LEAD:LEAD + B * n_p * 3 * C].view(B, n_p, 3 * C)[:, :, 2 * C:]
        inside[LEAD:LEAD + B * n_p * 3 * C].view(B, n_p, 3 * C)[:, :, 2 * C:] = True
    else:
        lead = LEAD if how == "a" else _SHIFT[how]
        full = torch.full((lead + n + TAIL_PAD,), FILL, device=dev, dtype=dtype)
        inside = torch.zeros(full.shape, device=dev, dtype=torch.bool)
        win = full[lead:lead + n].view(tuple(shape))
        inside[lead:lead + n] = True
    if prefill is not None:
        win.copy_(prefill.to(dev, dtype))
    return Out(win, full, inside)


def run(c: Case, K, dev) -> dict:
    """Place the operands, call the kernels.py wrapper, return {output name: Out}.  kernels.last_form() is the caller's to read."""
    b, d, P = build(c), c.dtypes, c.placed
    i = b.inputs
    if c.entry == "ppeg_fwd":
        B, S, D = c.sizes
        o = window((B, 1 + S * S, D), d[1], P(1), dev)
        assert K.ppeg(put(i["x"], d[0], P(0), dev), i["merged"].to(dev), i["bsum"].to(dev), S, bool(c.opt[0]), out_dtype=d[1], out=o.win) is o.win
        return {"y": o}
    if c.entry == "ppeg_wgrad":
        B, S, D = c.sizes
        dm, dbs = window((49, D), f32, "a", dev, b.prefill["dmerged"]), window((D,), f32, "a", dev, b.prefill["dbsum"])
        K.ppeg_wgrad(put(i["x"], d[0], P(0), dev), put(i["dout"], d[1], P(1), dev), dm.win, dbs.win, S)
        return {"dmerged": dm, "dbsum": dbs}
    if c.entry in ("resconv_fwd", "resconv_wgrad", "resconv_bwd"):
        B, n_p, heads, dh, taps = c.sizes
        shape = (B, n_p, heads * dh)
        if c.entry == "resconv_fwd":
            o = window(shape, d[1], P(1), dev, b.prefill.get("out"))
            K.resconv(put(i["v"], d[0], P(0), dev), i["w"].reshape(-1).to(dev), o.win, heads, bool(c.opt[0]), bool(c.opt[1]))
            return {"out": o}
        dw = window((heads, taps), f32, "a", dev, b.prefill["dw"])
        if c.entry == "resconv_wgrad":
            K.resconv_wgrad(put(i["v"], d[0], P(0), dev), put(i["dout"], d[1], P(1), dev), dw.win, heads)
            return {"dw": dw}
        dv = window(shape, d[0], P(2), dev, b.prefill["dv"])
        K.resconv_bwd(put(i["dout"], d[1], P(0), dev), put(i["v"], d[0], P(1), dev), i["w"].reshape(-1).to(dev), dv.win, dw.win, heads)
        return {"dv": dv, "dw": dw}
    if c.entry in ("landmark_fwd", "landmark_bwd"):
        B, m, l, D = c.sizes
        if c.entry == "landmark_fwd":
            o = window((B, m, 2 * D), d[0], P(1), dev)
            assert K.landmark_fwd(put(i["qkv"], d[0], P(0), dev), l, out=o.win) is o.win
            return {"lm": o}
        o = window((B, m * l, 3 * D), d[0], P(1), dev, b.prefill["dqkv"])
        K.landmark_bwd(put(i["dlm"], d[0], P(0), dev), o.win, l)
        return {"dqkv": o}
    B, N, add, D = c.sizes
    if c.entry == "seq_finish":
        o = window((B, 1 + N + add, D), d[0], "a", dev, b.prefill["seq"])
        K.seq_finish(o.win, i["cls"].to(dev), N, add)
        return {"seq": o}
    if c.entry == "seq_finish_bwd":
        o = window((B, 1 + N + add, D), d[0], "a", dev, b.prefill["dseq"])
        dcls = window((D,), f32, "a", dev, b.prefill["dcls"])
        K.seq_finish_bwd(o.win, dcls.win, N, add)
        return {"dseq": o, "dcls": dcls}
    raise KeyError(c.entry)
