"""The scalar, tail and mixed-dtype forms of the elementwise and row kernels: ONE table of cases for the CPU and the GPU test.

Almost every entry point of csrc/elementwise.hip and csrc/norm_softmax.hip chooses on the host between a 16-byte "quad" kernel (inner
size a multiple of 4, every pointer quad-aligned) and a scalar kernel; some also switch on a row count (mh_colsum), on the row length
(mh_softmax_*: a wave per row up to 1024 columns, a block per row above, quads only up to 12288) or on a workspace (mh_layernorm_bwd).
Every case names the form it is built to reach ("<entry>:<form>", what kernels.last_form() answers after the call); the sizes are the
smallest at which that form or boundary is still reached.

Data kinds:
  integer   small integers (for mh_cast: integers up to 1000, which bf16 has to round).  Every f64 reference value is a number of the
            output dtype and every f32 partial sum stays below 2^24, so the result must EQUAL the reference (test_row_forms_cpu checks both).
  random    randn operands rounded to their storage dtype first; per-element tolerance `tol`, nothing of it measured on the device,
            and `dropped` = the reference with the last n % 4 elements / cols % 4 columns left out (the last quad where that is 0):
            it must differ from the reference by more than 10 tol somewhere, so a kernel that loses its tail cannot pass.

The constant-row LayerNorm cases run at eps = 2^-16, so that rsqrt(eps) = 256 is an f32 number and "bit for bit" has one meaning.
softmax_bwd at one column is given a y that is no softmax output (0.5, ..): with y = 1 its dx = dy - dy is zero whatever the kernel reads.

References are plain f64 torch on the CPU.  A bf16 output of an integer case is exact; of a random case it may be off by one bf16
rounding (2^-8 relative) on top of the f32 bound.

Placement: "a" = a tensor of its own (256-byte aligned), "o" = a view one element into a larger buffer (never quad-aligned).  Outputs
are windows of a buffer filled with 7.0 (LEAD elements in front when aligned, one when not, TAIL_PAD behind): `Out.guards_ok`.
"""
from __future__ import annotations

import functools
import itertools
import math
from dataclasses import dataclass, field

import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
NM = {bf16: "b", f32: "f"}
FILL, LEAD, TAIL_PAD = 7.0, 8, 8
PAIRS = list(itertools.product((f32, bf16), repeat=2))
TRIPLES = list(itertools.product((f32, bf16), repeat=3))
EW_CAP, RELU_CAP = 16384, 4096            # EW_GRID's and mh_relu_bwd's grid caps (blocks of 256)
FLAT_SIZES = (0, 1, 3, 4, 5, 255, 257, 1000, 1003)
GELU_POINTS = (0.0, -0.0, 1e-4, -1e-4, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0, -1.0, 1.0)
SOFTMAX_COLS = (1, 2, 3, 63, 65, 257, 1023, 1024, 1025, 1028, 4350, 12288, 12289, 12292)
SOFTMAX_MIXED = (65, 257, 1025, 1028)
SOFTMAX_INPLACE = (257, 1025, 1028)
LN_D = (1, 2, 3, 30, 65, 257, 510, 513, 1026, 2047, 2048)
LN_ROWS = ((1, 1), (1, 5), (3, 23))       # (batches, rows per batch): 1, 5 and 69 rows
LN_PAD = 2
LN_EPS = 1e-5
LN_EPS_EXACT = 2.0 ** -16                 # the constant-row cases: rstd = rsqrt(eps) = 256
LN_MAX_D = 2048


@dataclass(frozen=True)
class Case:
    entry: str
    id: str
    form: str                       # kernels.last_form() after the call
    kind: str                       # "integer" | "random"
    sizes: tuple                    # add / cast / gelu_* / relu_bwd: (n,) or (B, R + 2, D) for the batch-strided relu_bwd;
                                    # colsum: (rows, cols, ld); row_scale / softmax_*: (rows, cols); layernorm_*: (batches, rows per batch, D)
    dtypes: tuple                   # the dispatch instance: operand dtypes in the entry point's order
    place: tuple = ()               # "a" / "o" per operand in the same order; () = all "a"
    opt: str = ""                   # "inplace" (softmax), "const" (layernorm rows of 3.0), "win" (relu_bwd 3-D)

    def __str__(self) -> str:
        return f"{self.entry}-{self.id}"

    def placed(self, i: int) -> str:
        return self.place[i] if self.place else "a"

    @property
    def aligned(self) -> bool:
        return all(p == "a" for p in self.place)


def _dn(dts) -> str:
    return "".join(NM[d] for d in dts)


def _flat_form(entry: str, n: int, place=()) -> str:
    if n == 0:
        return f"{entry}:none"
    return f"{entry}:quad" if n % 4 == 0 and all(p == "a" for p in place) else f"{entry}:scalar"


def _flat_cases():
    out = []
    for entry, insts in (("add", TRIPLES), ("cast", PAIRS), ("relu_bwd", TRIPLES)):
        k = len(insts[0])
        for dts, n in itertools.product(insts, FLAT_SIZES):
            out.append(Case(entry, f"{_dn(dts)}-n{n}", _flat_form(entry, n), "integer", (n,), dts))
        for dts in (insts[0], insts[-1]):         # n = 1000 with one operand at a time one element into its buffer
            for i in range(k):
                place = tuple("o" if j == i else "a" for j in range(k))
                out.append(Case(entry, f"{_dn(dts)}-n1000-off{i}", f"{entry}:scalar", "integer", (1000,), dts, place))
    # relu_bwd, batch-strided: y = buf[:, 1:8] of [3, 9, 8] (batch stride 72: quads) and of [3, 9, 7] (batch stride 63: scalar)
    for dts in ((f32, f32, f32), (f32, f32, bf16), (bf16, bf16, bf16)):
        out.append(Case("relu_bwd", f"{_dn(dts)}-win8", "relu_bwd:quad", "integer", (3, 9, 8), dts, opt="win"))
        out.append(Case("relu_bwd", f"{_dn(dts)}-win7", "relu_bwd:scalar", "integer", (3, 9, 7), dts, opt="win"))
    for entry, insts in (("gelu_fwd", PAIRS), ("gelu_bwd", PAIRS)):
        for dts, n in itertools.product(insts, (1, 257, 1003)):
            out.append(Case(entry, f"{_dn(dts)}-n{n}", f"{entry}:scalar", "random", (n,), dts))
    # past the grid cap: the second trip of the grid-stride loop
    wrap = EW_CAP * 256 + 257
    out.append(Case("add", "wrap-scalar", "add:scalar", "integer", (wrap,), (f32, f32, f32)))
    out.append(Case("add", "wrap-quad", "add:quad", "integer", (4 * wrap,), (f32, f32, f32)))
    out.append(Case("cast", "wrap-scalar", "cast:scalar", "integer", (wrap,), (f32, bf16)))
    out.append(Case("relu_bwd", "wrap-scalar", "relu_bwd:scalar", "integer", (RELU_CAP * 256 + 5,), (f32, f32, f32)))
    return out


def _row_cases():
    out = []
    for t in (f32, bf16):
        for D in (1, 3, 18, 64):
            out.append(Case("row_scale", f"{NM[t]}-5x{D}", "row_scale:quad" if D % 4 == 0 else "row_scale:scalar", "integer", (5, D), (t,)))
        out.append(Case("row_scale", f"{NM[t]}-5x64-offx", "row_scale:scalar", "integer", (5, 64), (t,), ("o", "a")))
        out.append(Case("row_scale", f"{NM[t]}-5x64-offy", "row_scale:scalar", "integer", (5, 64), (t,), ("a", "o")))
        out.append(Case("row_scale", f"{NM[t]}-65541x3", "row_scale:scalar", "integer", (65541, 3), (t,)))      # past the 16384-block cap
    cs = [("f-31x8", "scalar", (31, 8, 8), f32),          # rows < 32
          ("f-32x8", "f32quad", (32, 8, 8), f32),
          ("f-33x12", "f32quad", (33, 12, 12), f32),
          ("f-40x70", "scalar", (40, 70, 70), f32),        # cols % 4 != 0, two column blocks
          ("f-40x8-ld12", "f32quad", (40, 8, 12), f32),
          ("f-40x8-ld9", "scalar", (40, 8, 9), f32),
          ("f-513x5", "scalar", (513, 5, 5), f32),         # the CS_BAND edge: a second band of one row
          ("b-1023x16", "scalar", (1023, 16, 16), bf16),   # rows < 1024
          ("b-1024x16", "bf16oct", (1024, 16, 16), bf16),
          ("b-1031x520-ld528", "bf16oct", (1031, 520, 528), bf16),
          ("b-1031x516", "scalar", (1031, 516, 516), bf16)]
    for cid, form, sizes, t in cs:
        out.append(Case("colsum", cid, f"colsum:{form}", "integer", sizes, (t,)))
    return out


def _softmax_form(entry: str, cols: int, aligned: bool = True) -> str:
    quad = cols % 4 == 0 and cols <= 12288 and aligned
    return f"{entry}:{'wave' if cols <= 1024 else 'block'},{'quad' if quad else 'scalar'}"


def _softmax_cases():
    out = []
    for entry in ("softmax_fwd", "softmax_bwd"):
        for cols, rows in itertools.product(SOFTMAX_COLS, (1, 6)):
            out.append(Case(entry, f"ff-{rows}x{cols}", _softmax_form(entry, cols), "random", (rows, cols), (f32, f32)))
        for cols, dts in itertools.product(SOFTMAX_MIXED + (1024,), PAIRS[1:]):       # 1024: the mixed instances of the wave quad form
            out.append(Case(entry, f"{_dn(dts)}-6x{cols}", _softmax_form(entry, cols), "random", (6, cols), dts))
        for cols, t in itertools.product(SOFTMAX_INPLACE, (f32, bf16)):
            out.append(Case(entry, f"{NM[t]}{NM[t]}-6x{cols}-inplace", _softmax_form(entry, cols), "random", (6, cols), (t, t), opt="inplace"))
        out.append(Case(entry, "ff-6x1024-offin", _softmax_form(entry, 1024, False), "random", (6, 1024), (f32, f32), ("o", "a")))
        out.append(Case(entry, "ff-6x1024-offout", _softmax_form(entry, 1024, False), "random", (6, 1024), (f32, f32), ("a", "o")))
    return out


def _ln_bwd_form(rows: int, D: int, aligned: bool = True) -> str:
    if D % 4 or not aligned:
        return "layernorm_bwd:scalar"
    return "layernorm_bwd:ws" if rows >= 64 else "layernorm_bwd:quad"


def _ln_cases():
    out = []
    for (B, rpb), D in itertools.product(LN_ROWS, LN_D):
        rows = B * rpb
        insts = PAIRS if (rows == 5 or D in (30, 2048)) else PAIRS[:1]      # every dtype instance at 5 rows, and at 1 / 69 rows for one D per form
        for dts in insts:
            out.append(Case("layernorm_fwd", f"{_dn(dts)}-{rows}x{D}", f"layernorm_fwd:{'scalar' if D % 4 else 'quad'}", "random", (B, rpb, D), dts))
            out.append(Case("layernorm_bwd", f"{_dn(dts)}-{rows}x{D}", _ln_bwd_form(rows, D), "random", (B, rpb, D), dts))
    # a second trip of the 512-block grid of the scalar backward (4 rows per block)
    out.append(Case("layernorm_bwd", "ff-2053x30", "layernorm_bwd:scalar", "random", (1, 2053, 30), (f32, f32)))
    for dts in ((f32, f32), (bf16, bf16)):
        # D = 512 through an x one element into its buffer: alignment refuses the quad AND the workspace form
        out.append(Case("layernorm_fwd", f"{_dn(dts)}-69x512-offx", "layernorm_fwd:scalar", "random", (3, 23, 512), dts, ("o", "a")))
        out.append(Case("layernorm_bwd", f"{_dn(dts)}-69x512-offx", "layernorm_bwd:scalar", "random", (3, 23, 512), dts, ("o", "a")))
        out.append(Case("layernorm_bwd", f"{_dn(dts)}-5x512-offx", "layernorm_bwd:scalar", "random", (1, 5, 512), dts, ("o", "a")))
    for dts in ((bf16, f32), (bf16, bf16)):
        out.append(Case("layernorm_fwd", f"{_dn(dts)}-69x512", "layernorm_fwd:quad", "random", (3, 23, 512), dts))
        out.append(Case("layernorm_bwd", f"{_dn(dts)}-69x512", "layernorm_bwd:ws", "random", (3, 23, 512), dts))
    # rows of a constant 3.0 with integer gamma / beta: mean == 3, y == beta, rstd == rsqrt(eps), bit for bit
    for D, dts in itertools.product((3, 30, 513, 2048), PAIRS):
        out.append(Case("layernorm_fwd", f"{_dn(dts)}-5x{D}-const", f"layernorm_fwd:{'scalar' if D % 4 else 'quad'}", "integer", (1, 5, D), dts, opt="const"))
    return out


def _model_cases():
    """The row kernels the model reaches them through: the encoder-output fan-in, the mask-token select and the masked MSE."""
    out = []
    for t in (f32, bf16):               # fanout_bwd: the three operand subsets of test_fanout_bwd, alpha in {-1, 0.5}
        for D in (1, 3, 18, 22, 20):
            form = "fanout_bwd:quad" if D % 4 == 0 else "fanout_bwd:scalar"
            for sub, alpha in (("all", -1.0), ("all", 0.5), ("x", 0.5), ("x", -1.0), ("g", 0.0)):
                out.append(Case("fanout_bwd", f"{NM[t]}-3x5x{D}-{sub}{alpha}", form, "integer", (3, 5, D), (t,), opt=f"{sub},{alpha}"))
    for dts, D, first in itertools.product(PAIRS, (18, 20), (0, 1)):      # per-channel token; quads need f32 out
        form = "mask_apply_fwd:quad" if D % 4 == 0 and dts[1] == f32 else "mask_apply_fwd:scalar"
        out.append(Case("mask_apply_fwd", f"{_dn(dts)}-3x9x{D}-first{first}", form, "integer", (3, 9, D), dts, opt=f"{first},0"))
    for dts in PAIRS:                   # the RNA form: one scalar token over the channel axis
        out.append(Case("mask_apply_fwd", f"{_dn(dts)}-3x20x1-token1", "mask_apply_fwd:scalar", "integer", (3, 20, 1), dts, opt="0,1"))
    for dts, first in itertools.product(PAIRS, (0, 1)):
        # scalar form: D = 70 = two column blocks of 64, T = first + 65 = two MB_BAND bands
        out.append(Case("mask_apply_bwd", f"{_dn(dts)}-3x{first + 65}x70-first{first}", "mask_apply_bwd:scalar", "integer", (3, first + 65, 70), dts, opt=f"{first},0"))
        out.append(Case("mask_apply_bwd", f"{_dn(dts)}-3x20x1-first{first}", "mask_apply_bwd:d1", "integer", (3, 20 + first, 1), dts, opt=f"{first},1"))
    for dts in PAIRS[:2]:               # quad form (f32 dy, D >= 256): two bands of 16 rows, a batch that is no multiple of 8
        out.append(Case("mask_apply_bwd", f"{_dn(dts)}-3x18x256-first1", "mask_apply_bwd:quad", "integer", (3, 18, 256), dts, opt="1,0"))
    for dts in PAIRS:                   # masked MSE: (pred, target) and (pred, target, dpred)
        for D, opt, form in ((1, "", "flat"), (1, "win", "scalar"), (22, "", "scalar"), (23, "", "scalar"), (23, "win", "scalar"),
                             (24, "", "quad"), (24, "win", "quad"), (24, "win23", "scalar")):
            cid = f"3x6x{D}" + (f"-{opt}" if opt else "")
            out.append(Case("mse_masked_fwd", f"{_dn(dts)}-{cid}", f"mse_masked_fwd:{form}", "random", (3, 6, D), dts, opt=opt))
            bform = "scalar" if form == "flat" else form
            for dp in ((f32, bf16) if D in (22, 24) and opt != "win" else (dts[0],)):
                out.append(Case("mse_masked_bwd", f"{_dn(dts + (dp,))}-{cid}", f"mse_masked_bwd:{bform}", "random", (3, 6, D), dts + (dp,), opt=opt))
    # the form that leaves every block's column sums of dpred in a table (D in {256, .., 1024}, bf16 pred / f32 target / bf16 dpred)
    out.append(Case("mse_masked_bwd", "bfb-3x6x256-colsum", "mse_masked_bwd:colsum", "random", (3, 6, 256), (bf16, f32, bf16), opt="colsum"))
    return out


CASES = _flat_cases() + _row_cases() + _softmax_cases() + _ln_cases() + _model_cases()
assert len({str(c) for c in CASES}) == len(CASES)


def by_id(name: str) -> Case:
    return next(c for c in CASES if str(c) == name)


# ------------------------------------------------------------------------------------------ f64 references
def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def softmax64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd64(y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    y, dy = y.double(), dy.double()
    return y * (dy - (y * dy).sum(-1, keepdim=True))


def layernorm64(x, gamma, beta, eps):
    """(y, mean, rstd) of rows x [.., D] in f64 (biased variance, as torch.nn.functional.layer_norm)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * gamma.double() + beta.double(), mean.squeeze(-1), rstd.squeeze(-1)


def mse_masked64(pred, tgt, mask, D=None):
    """(sum_r mask[r] mean_D (pred - tgt)^2, sum_r mask[r]) in f64: the two accumulators of mh_mse_masked_fwd.  D: the divisor of the
    mean when the operands hold fewer columns than the row has (the lost-tail check)."""
    sq = (pred.double() - tgt.double()) ** 2
    return (sq.sum(-1) / (D or pred.shape[-1]) * mask.double()).sum(), mask.double().sum()


def mse_masked_bwd64(pred, tgt, mask, upstream: float):
    """(dpred, dtgt) of upstream * num / den (mse_masked64's pair): 2 upstream mask (pred - tgt) / (D den), and its negative."""
    dp = 2.0 * upstream / (pred.shape[-1] * mask.double().sum()) * mask.double().unsqueeze(-1) * (pred.double() - tgt.double())
    return dp, -dp


def layernorm_bwd64(dy, x, gamma, mean, rstd):
    """(dx, dgamma, dbeta) from the saved statistics: dx = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma."""
    dy, x = dy.double(), x.double()
    xhat = (x - mean.double().unsqueeze(-1)) * rstd.double().unsqueeze(-1)
    g = dy * gamma.double()
    dx = rstd.double().unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    red = tuple(range(dy.dim() - 1))
    return dx, (dy * xhat).sum(red), dy.sum(red)


# ------------------------------------------------------------------------------------------ data
@dataclass
class Built:
    inputs: dict                                    # name -> CPU tensor holding the STORED values (rounded to the operand's dtype)
    want: dict                                      # output name -> f64 reference
    tol: dict = field(default_factory=dict)         # output name -> f64 per-element bound (random cases)
    dropped: dict = field(default_factory=dict)     # output name -> the reference with the tail left out (random cases)
    prefill: dict = field(default_factory=dict)     # output name -> what the output holds before the call (accumulating entries)
    f32_sum_bound: float = 0.0                      # integer cases: the largest |partial sum| any f32 accumulation can reach


def _gen(c: Case) -> torch.Generator:
    return torch.Generator().manual_seed(1 + CASES.index(c))


def _ints(gen, lo, hi, shape) -> torch.Tensor:
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def stored(t: torch.Tensor, dtype) -> torch.Tensor:
    """t as the device will hold it: rounded once to dtype, back as f32."""
    return t.float().to(dtype).float()


def tail_len(n: int) -> int:
    """What `dropped` leaves out: the n % 4 elements no quad covers, or the last quad."""
    return min(n, n % 4 or 4)


def _bf16_term(dtype, want):
    return 2.0 ** -8 * want.abs() if dtype == bf16 else torch.zeros_like(want)


def _build_flat(c: Case, gen) -> Built:
    n = c.sizes[0]
    if c.entry == "add":
        a, b = _ints(gen, -8, 8, (n,)), _ints(gen, -8, 8, (n,))
        return Built({"a": a, "b": b}, {"y": a.double() + b.double()}, f32_sum_bound=16.0)
    if c.entry == "cast":
        x = stored(_ints(gen, -1000, 1000, (n,)), c.dtypes[0])
        return Built({"x": x}, {"y": x.to(c.dtypes[1]).double()})            # f32 -> bf16 rounds once, to nearest even
    if c.entry == "relu_bwd":
        shape = (n,) if c.opt != "win" else (c.sizes[0], c.sizes[1] - 2, c.sizes[2])
        y, dy = _ints(gen, -3, 3, shape), _ints(gen, -8, 8, shape)
        b = Built({"y": y, "dy": dy}, {"dx": (dy * (y > 0)).double()})
        if c.opt == "win":
            b.inputs["y_buf"] = _ints(gen, -3, 3, c.sizes)
            b.inputs["y_buf"][:, 1:c.sizes[1] - 1] = y
        return b
    x = torch.randn(n, generator=gen) * 2
    k = min(n, len(GELU_POINTS))
    x[n - k:] = torch.tensor(GELU_POINTS[len(GELU_POINTS) - k:])
    x = stored(x, c.dtypes[0])
    t = tail_len(n)
    if c.entry == "gelu_fwd":
        want = gelu64(x)
        tol = 1e-6 + 1e-6 * want.abs() + _bf16_term(c.dtypes[1], want)       # test_elementwise_family's bound
        inputs = {"x": x}
    else:
        dy = stored(torch.randn(n, generator=gen), c.dtypes[1])
        dy[n - t:] = stored(torch.full((t,), 1.5), c.dtypes[1])
        want = dy.double() * gelu_grad64(x)
        tol = 1e-6 + 1e-5 * want.abs() + _bf16_term(c.dtypes[1], want)
        inputs = {"x": x, "dy": dy}
    name = "y" if c.entry == "gelu_fwd" else "dx"
    drop = want.clone()
    drop[n - t:] = 0.0
    return Built(inputs, {name: want}, {name: tol}, {name: drop})


def _build_row_scale(c: Case, gen) -> Built:
    rows, D = c.sizes
    x = _ints(gen, -8, 8, (rows, D))
    scale = 2.0 ** torch.randint(-2, 3, (rows,), generator=gen).float() * (1 - 2 * torch.randint(0, 2, (rows,), generator=gen).float())
    return Built({"x": x, "scale": scale}, {"y": x.double() * scale.double().unsqueeze(1)})


def _build_colsum(c: Case, gen) -> Built:
    rows, cols, ld = c.sizes
    buf = _ints(gen, -3, 3, (rows, ld))
    pre = _ints(gen, -3, 3, (cols,))
    return Built({"x_buf": buf}, {"out": pre.double() + buf[:, :cols].double().sum(0)}, prefill={"out": pre}, f32_sum_bound=3.0 * rows + 3.0)


def _softmax_x(c: Case, gen, dtype) -> torch.Tensor:
    rows, cols = c.sizes
    x = torch.randn(rows, cols, generator=gen) * 3
    t = tail_len(cols)
    x[:, cols - t:] = 5.0 + 0.25 * torch.arange(rows).float().unsqueeze(1)       # the tail carries weight in every row
    if rows >= 4:
        x[1] = 1.5                                                           # equal values
        x[2, 1::3] = -math.inf                                               # -inf beside finite entries
        if cols >= 2:
            x[3] = (torch.linspace(-30.0, 30.0, cols)[torch.randperm(cols, generator=gen)]).float()      # a spread of 60
    return stored(x, dtype)


def _build_softmax_fwd(c: Case, gen) -> Built:
    cols = c.sizes[1]
    x = _softmax_x(c, gen, c.dtypes[0])
    want = softmax64(x)
    # __expf is exp2(x * log2e): the rounded product carries an absolute exponent error of ~|x - max| 2^-24, numerator and normaliser each
    dist = (x.double().max(-1, keepdim=True).values - x.double())
    dist = torch.where(torch.isinf(dist), torch.zeros_like(dist), dist)      # exp(-inf) is 0 exactly: want == 0 there, and so is tol
    tol = 2.0 ** -22 * (4.0 + dist) * want + _bf16_term(c.dtypes[1], want)
    keep = cols - tail_len(cols)
    drop = torch.zeros_like(want)
    if keep:
        drop[:, :keep] = softmax64(x[:, :keep])
    return Built({"x": x}, {"y": want}, {"y": tol}, {"y": drop})


def _build_softmax_bwd(c: Case, gen) -> Built:
    rows, cols = c.sizes
    y = softmax64(_softmax_x(c, gen, f32)).float()
    if cols == 1:       # mh_softmax_bwd takes any (y, dy): a softmax output of one column is 1 and dx = dy - dy, which no kernel can get wrong
        y = 0.5 + 0.0625 * torch.arange(rows).float().unsqueeze(1)
    y = stored(y, c.dtypes[0])
    dy = torch.randn(rows, cols, generator=gen)
    t = tail_len(cols)
    dy[:, cols - t:] = 2.0 + 0.5 * torch.arange(t).float()
    dy = stored(dy, c.dtypes[1])
    want = softmax_bwd64(y, dy)
    # dot = sum y dy in f32: a lane adds its ceil(cols / lanes) products in turn (64 lanes per row up to 1024 columns, 256 above), then
    # a tree of 6 (wave) or 9 (block) additions: no partial sum sees more than per_lane + 10 roundings, each 2^-24 of sum |y dy| at the
    # most.  Then (dy - dot) and the product round once each (2^-24 relative, on |dy| + |dot| at the most): 2^-22 leaves a factor 2
    y64, dy64 = y.double(), dy.double()
    absdot = (y64 * dy64).abs().sum(-1, keepdim=True)
    dot = (y64 * dy64).sum(-1, keepdim=True)
    per_lane = -(-cols // (64 if cols <= 1024 else 256))
    tol = y64.abs() * ((per_lane + 10) * 2.0 ** -24 * absdot + 2.0 ** -22 * (dy64.abs() + dot.abs())) + _bf16_term(c.dtypes[1], want)
    keep = cols - t
    drop = torch.zeros_like(want)
    if keep:
        drop[:, :keep] = softmax_bwd64(y[:, :keep], dy[:, :keep])
    return Built({"y": y, "dy": dy}, {"dx": want}, {"dx": tol}, {"dx": drop})


def _ln_operands(c: Case, gen):
    B, rpb, D = c.sizes
    if c.opt == "const":
        x = torch.full((B, rpb, D), 3.0)
        gamma, beta = _ints(gen, -4, 4, (D,)), _ints(gen, -4, 4, (D,))
    else:
        x = torch.randn(B, rpb, D, generator=gen) * 2 + 0.5
        gamma, beta = torch.randn(D, generator=gen), torch.randn(D, generator=gen)
    return stored(x, c.dtypes[0]), gamma, beta


def _build_ln_fwd(c: Case, gen) -> Built:
    B, rpb, D = c.sizes
    x, gamma, beta = _ln_operands(c, gen)
    eps = LN_EPS_EXACT if c.opt == "const" else LN_EPS
    y, mean, rstd = layernorm64(x, gamma, beta, eps)
    want = {"y": y, "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}
    b = Built({"x": x, "gamma": gamma, "beta": beta}, want, f32_sum_bound=3.0 * D)
    if c.kind == "random":       # test_layernorm_fwd_bwd's f32 bound for every f32 output of the launch
        b.tol = {k: 1e-5 + 1e-5 * v.abs() + (_bf16_term(c.dtypes[1], v) if k == "y" else 0.0) for k, v in want.items()}
        keep = D - tail_len(D)
        dy_, dm, dr = torch.zeros_like(y), torch.zeros_like(want["mean"]), torch.zeros_like(want["rstd"])
        if keep:
            y2, m2, r2 = layernorm64(x[..., :keep], gamma[:keep], beta[:keep], eps)
            dy_[..., :keep], dm, dr = y2, m2.reshape(-1), r2.reshape(-1)
        b.dropped = {"y": dy_, "mean": dm, "rstd": dr}
    return b


def _build_ln_bwd(c: Case, gen) -> Built:
    B, rpb, D = c.sizes
    x, gamma, _ = _ln_operands(c, gen)
    _, mean, rstd = layernorm64(x, gamma, torch.zeros(D), LN_EPS)
    mean, rstd = mean.reshape(-1).float(), rstd.reshape(-1).float()           # the statistics as the forward saved them (f32)
    dy = stored(torch.randn(B, rpb, D, generator=gen), c.dtypes[1])
    m3, r3 = mean.view(B, rpb), rstd.view(B, rpb)
    dx, dg, db = layernorm_bwd64(dy, x, gamma, m3, r3)
    rows = B * rpb
    grow = math.sqrt(max(rows, 69) / 69.0)        # test_ppeg's rule for f32 sums over more rows than the bound was stated for
    want = {"dx": dx, "dgamma": dg, "dbeta": db}
    tol = {"dx": 1e-4 + 1e-4 * dx.abs() + _bf16_term(c.dtypes[0], dx),        # test_layernorm_fwd_bwd's f32 bounds (dx follows x)
           "dgamma": 2e-4 * grow + 1e-4 * dg.abs(), "dbeta": 2e-4 * grow + 1e-4 * db.abs()}
    keep = D - tail_len(D)
    drop = {k: torch.zeros_like(v) for k, v in want.items()}
    if keep:
        d2 = layernorm_bwd64(dy[..., :keep], x[..., :keep], gamma[:keep], m3, r3)
        drop["dx"][..., :keep], drop["dgamma"][:keep], drop["dbeta"][:keep] = d2
    return Built({"x": x, "gamma": gamma, "mean": mean, "rstd": rstd, "dy": dy}, want, tol, drop)


def _build_fanout(c: Case, gen) -> Built:
    B, T, D = c.sizes
    sub, alpha = c.opt.split(",")
    alpha = float(alpha)
    gf = _ints(gen, -8, 8, (B, T, D)) if sub in ("all", "g") else None
    x = _ints(gen, -8, 8, (B, T - 1, D)) if sub in ("all", "x") else None
    cls = _ints(gen, -8, 8, (B, D)) if sub == "all" else None
    want = torch.zeros(B, T, D, dtype=f64) if gf is None else gf.double().clone()
    if x is not None:
        want[:, 1:] += alpha * x.double()
    if cls is not None:
        want[:, 0] += cls.double()
    return Built({k: v for k, v in (("gfull", gf), ("x", x), ("c", cls)) if v is not None}, {"dE": want}, f32_sum_bound=24.0)


def _mask_operands(c: Case, gen):
    B, T, D = c.sizes
    first, scalar = (int(v) for v in c.opt.split(","))
    mask = (torch.rand(B, T - first, generator=gen) > 0.5).float()
    mask[0, 0], mask[-1, -1] = 1.0, 0.0            # both kinds of row, whatever the draw
    return B, T, D, first, scalar, mask


def _build_mask_fwd(c: Case, gen) -> Built:
    B, T, D, first, scalar, mask = _mask_operands(c, gen)
    x, tok, pos = _ints(gen, -8, 8, (B, T, D)), _ints(gen, -8, 8, (1 if scalar else D,)), _ints(gen, -8, 8, (T, D))
    want = x.double().clone()
    want[:, first:] = torch.where(mask[..., None] > 0, tok.double().expand(B, T - first, D), want[:, first:])
    return Built({"x": x, "mask": mask, "token": tok, "pos": pos}, {"y": want + pos.double()}, f32_sum_bound=16.0)


def _build_mask_bwd(c: Case, gen) -> Built:
    B, T, D, first, scalar, mask = _mask_operands(c, gen)
    dy = _ints(gen, -8, 8, (B, T, D))
    pre_tok, pre_pos = _ints(gen, -3, 3, (1 if scalar else D,)), _ints(gen, -3, 3, (T, D))
    keep = torch.cat([torch.ones(B, first), 1 - mask], dim=1)[..., None].double()
    dtok = (dy[:, first:].double() * mask[..., None].double()).sum((0, 1))
    want = {"dx": dy.double() * keep, "dtoken": pre_tok.double() + (dtok.sum().reshape(1) if scalar else dtok), "dpos": pre_pos.double() + dy.double().sum(0)}
    return Built({"dy": dy, "mask": mask}, want, prefill={"dtoken": pre_tok, "dpos": pre_pos}, f32_sum_bound=8.0 * B * T * (D if scalar else 1) + 3.0)


MSE_G, MSE_GMUL, MSE_ACC0 = 0.7, 0.15, (1.0, 2.0)


def _mse_operands(c: Case, gen):
    B, N, D = c.sizes
    pred = stored(torch.randn(B, N, D, generator=gen), c.dtypes[0])
    tgt = stored(torch.randn(B, N, D, generator=gen), c.dtypes[1])
    mask = (torch.rand(B, N, generator=gen) > 0.4).float()
    mask[0, 0], mask[-1, -1] = 0.0, 1.0            # a dropped row, and the last row (whose tail is the buffer's last element) kept
    return pred, tgt, mask


def _build_mse_fwd(c: Case, gen) -> Built:
    D = c.sizes[2]
    pred, tgt, mask = _mse_operands(c, gen)
    pre = torch.tensor(MSE_ACC0)

    def acc(cols):
        return pre.double() + torch.stack(mse_masked64(pred[..., :cols], tgt[..., :cols], mask, D))
    want = acc(D)
    tol = 1e-6 + 1e-5 * want.abs()                 # test_masked_mse_row_window_target's bound on the loss, whose denominator is exact
    return Built({"pred": pred, "tgt": tgt, "mask": mask}, {"acc": want}, {"acc": tol}, {"acc": acc(D - tail_len(D))}, prefill={"acc": pre})


def _build_mse_bwd(c: Case, gen) -> Built:
    D = c.sizes[2]
    pred, tgt, mask = _mse_operands(c, gen)
    acc = torch.tensor([0.0, float(mask.sum())])
    dp, dt = mse_masked_bwd64(pred, tgt, mask, MSE_G * MSE_GMUL)
    want = {"dpred": dp, "dtgt": dt}
    tol = {"dpred": 1e-7 + 1e-5 * dp.abs() + _bf16_term(c.dtypes[2], dp), "dtgt": 1e-7 + 1e-5 * dp.abs() + _bf16_term(c.dtypes[1], dp)}
    if c.opt == "colsum":
        # this form defines dtgt as the negative of dpred AS STORED (mse_masked_bwd_cs_kernel rounds d to bf16 before it sums, stores
        # and negates it; test_masked_mse_bwd_leaves_column_sums pins dtgt == -dpred bit for bit), so the f32 dtgt carries dpred's rounding
        tol["dtgt"] = tol["dtgt"] + _bf16_term(c.dtypes[2], dp)
        # the table's column sums are of dpred AS STORED: every element within its own bound above, the f32 sums of <= rows terms on top
        rows = dp.shape[0] * dp.shape[1]
        want["colsum"] = dp.sum((0, 1))
        tol["colsum"] = tol["dpred"].sum((0, 1)) + rows * 2.0 ** -24 * dp.abs().sum((0, 1))
    drop = {n: v.clone() for n, v in want.items()}
    for v in drop.values():
        v[..., D - tail_len(D):] = 0.0
    return Built({"pred": pred, "tgt": tgt, "mask": mask, "acc": acc}, want, tol, drop)


_BUILDERS = {"fanout_bwd": _build_fanout, "mask_apply_fwd": _build_mask_fwd, "mask_apply_bwd": _build_mask_bwd,
             "mse_masked_fwd": _build_mse_fwd, "mse_masked_bwd": _build_mse_bwd,
             "add": _build_flat, "cast": _build_flat, "relu_bwd": _build_flat, "gelu_fwd": _build_flat, "gelu_bwd": _build_flat,
             "row_scale": _build_row_scale, "colsum": _build_colsum, "softmax_fwd": _build_softmax_fwd, "softmax_bwd": _build_softmax_bwd,
             "layernorm_fwd": _build_ln_fwd, "layernorm_bwd": _build_ln_bwd}


@functools.lru_cache(maxsize=8)
def build(c: Case) -> Built:
    return _BUILDERS[c.entry](c, _gen(c))


def out_dtypes(c: Case) -> dict:
    """Output name -> dtype."""
    d, e = c.dtypes, c.entry
    if e in ("layernorm_fwd", "layernorm_bwd"):
        return {"y": d[1], "mean": f32, "rstd": f32} if e == "layernorm_fwd" else {"dx": d[0], "dgamma": f32, "dbeta": f32}
    if e == "colsum":
        return {"out": f32}
    if e == "fanout_bwd":
        return {"dE": f32}
    if e == "mask_apply_bwd":
        return {"dx": d[1], "dtoken": f32, "dpos": f32}
    if e == "mse_masked_fwd":
        return {"acc": f32}
    if e == "mse_masked_bwd":
        return {"dpred": d[2], "dtgt": d[1], **({"colsum": f32} if c.opt == "colsum" else {})}
    return {{"relu_bwd": "dx", "gelu_bwd": "dx", "softmax_bwd": "dx"}.get(e, "y"): d[0] if e == "row_scale" else d[-1]}


# ------------------------------------------------------------------------------------------ device operands and the call
@dataclass
class Out:
    win: torch.Tensor               # what the wrapper wrote into
    full: torch.Tensor              # the FILL-ed buffer around it
    lead: int
    span: int                       # elements of the window, pad rows included
    zero_rows: torch.Tensor = None  # layernorm_fwd: the pad rows of y, which must stay zero

    def guards_ok(self) -> bool:
        return bool((self.full[:self.lead] == FILL).all()) and bool((self.full[self.lead + self.span:] == FILL).all())


def put(t: torch.Tensor, dtype, how: str, dev) -> torch.Tensor:
    if how == "a":
        return t.to(dev, dtype).contiguous()
    buf = torch.zeros(t.numel() + 1, device=dev, dtype=dtype)
    buf[1:] = t.reshape(-1).to(dev, dtype)
    v = buf[1:].view(t.shape)
    assert v.numel() == 0 or v.data_ptr() % (4 * v.element_size()) != 0
    return v


def window(shape, dtype, how: str, dev, prefill=None) -> Out:
    n = int(math.prod(shape))
    lead = LEAD if how == "a" else 1
    full = torch.full((lead + n + TAIL_PAD,), FILL, device=dev, dtype=dtype)
    win = full[lead:lead + n].view(tuple(shape))
    if prefill is not None:
        win.copy_(prefill.to(dev, dtype))
    return Out(win, full, lead, n)


def run(c: Case, K, dev) -> dict:
    """Place the operands, call the kernels.py wrapper, return {output name: Out}.  kernels.last_form() is the caller's to read."""
    b, d, P = build(c), c.dtypes, c.placed
    i = b.inputs
    if c.entry == "add":
        o = window(c.sizes, d[2], P(2), dev)
        K.add(put(i["a"], d[0], P(0), dev), put(i["b"], d[1], P(1), dev), out=o.win)
        return {"y": o}
    if c.entry == "cast":
        o = window(c.sizes, d[1], P(1), dev)
        K.cast(put(i["x"], d[0], P(0), dev), d[1], out=o.win)
        return {"y": o}
    if c.entry == "relu_bwd":
        if c.opt == "win":
            y = i["y_buf"].to(dev, d[0])[:, 1:c.sizes[1] - 1]
            assert not y.is_contiguous()
        else:
            y = put(i["y"], d[0], P(0), dev)
        o = window(i["dy"].shape, d[2], P(2), dev)
        K.relu_bwd(y, put(i["dy"], d[1], P(1), dev), out=o.win)
        return {"dx": o}
    if c.entry == "gelu_fwd":
        o = window(c.sizes, d[1], "a", dev)
        K.gelu_fwd(put(i["x"], d[0], "a", dev), out=o.win)
        return {"y": o}
    if c.entry == "gelu_bwd":
        o = window(c.sizes, d[1], "a", dev)
        K.gelu_bwd(put(i["x"], d[0], "a", dev), put(i["dy"], d[1], "a", dev), out=o.win)
        return {"dx": o}
    if c.entry == "row_scale":
        o = window(c.sizes, d[0], P(1), dev)
        K.row_scale(put(i["x"], d[0], P(0), dev), i["scale"].to(dev), out=o.win)
        return {"y": o}
    if c.entry == "colsum":
        rows, cols, ld = c.sizes
        o = window((cols,), f32, "a", dev, b.prefill["out"])
        K.colsum(i["x_buf"].to(dev, d[0])[:, :cols], o.win)
        return {"out": o}
    if c.entry == "softmax_fwd":
        if c.opt == "inplace":
            o = window(c.sizes, d[0], "a", dev, i["x"])
            assert K.softmax_fwd(o.win, y=o.win) is o.win
        else:
            o = window(c.sizes, d[1], P(1), dev)
            K.softmax_fwd(put(i["x"], d[0], P(0), dev), y=o.win)
        return {"y": o}
    if c.entry == "softmax_bwd":
        y = put(i["y"], d[0], P(0), dev)
        if c.opt == "inplace":           # dx defaulted to dy, the wrapper's documented default
            o = window(c.sizes, d[1], "a", dev, i["dy"])
            assert K.softmax_bwd(y, o.win) is o.win
        else:
            o = window(c.sizes, d[1], P(1), dev)
            K.softmax_bwd(y, put(i["dy"], d[1], "a", dev), dx=o.win)
        return {"dx": o}
    if c.entry == "fanout_bwd":
        B, T, D = c.sizes
        o = window(c.sizes, f32, "a", dev)
        g, x, cls = (None if i.get(k) is None else i[k].to(dev, t) for k, t in (("gfull", f32), ("x", d[0]), ("c", f32)))
        assert K.fanout_bwd(g, x, float(c.opt.split(",")[1]), cls, B, T, D, out=o.win) is o.win
        return {"dE": o}
    if c.entry in ("mask_apply_fwd", "mask_apply_bwd"):
        B, T, D = c.sizes
        first, scalar = (int(v) for v in c.opt.split(","))
        o = window(c.sizes, d[1], "a", dev)
        if c.entry == "mask_apply_fwd":
            K.mask_apply_fwd(i["x"].to(dev, d[0]), i["mask"].to(dev), i["token"].to(dev), i["pos"].to(dev), B, T, D, first, bool(scalar), out=o.win)
            return {"y": o}
        dtok = window(b.prefill["dtoken"].shape, f32, "a", dev, b.prefill["dtoken"])
        dpos = window((T, D), f32, "a", dev, b.prefill["dpos"])
        K.mask_apply_bwd(i["dy"].to(dev, d[0]), i["mask"].to(dev), dtok.win, dpos.win, B, T, D, first, bool(scalar), out=o.win)
        return {"dx": o, "dtoken": dtok, "dpos": dpos}
    if c.entry in ("mse_masked_fwd", "mse_masked_bwd"):
        B, N, D = c.sizes
        pred, mask = i["pred"].to(dev, d[0]), i["mask"].to(dev)
        if c.opt in ("", "colsum"):
            tgt = i["tgt"].to(dev, d[1])
        else:          # a row window: rows 1.. of [B, N + 1, D]; "win23": N rows of D = 24 per batch of a [B, N + 1, 23] buffer, so that the
            first = 0 if c.opt == "win23" else D           # batch stride (N + 1) * 23 is no multiple of 4 while the base stays aligned
            bs = (N + 1) * (23 if c.opt == "win23" else D)
            assert bs >= first + N * D and (c.opt != "win23" or bs % 4)
            buf = torch.zeros(B * bs, device=dev, dtype=d[1])
            tgt = buf.as_strided((B, N, D), (bs, D, 1), first)
            tgt.copy_(i["tgt"].to(dev, d[1]))
            assert not tgt.is_contiguous()
        if c.entry == "mse_masked_fwd":
            acc = window((2,), f32, "a", dev, b.prefill["acc"])
            K.mse_masked_fwd(pred, tgt, mask, acc.win, B * N, D)
            return {"acc": acc}
        dp, dtg = window(c.sizes, d[2], "a", dev), window(c.sizes, d[1], "a", dev)
        ws = None
        if c.opt == "colsum":          # every row of the table must be written: a row left at nan shows in the sum
            ws = window((K.MSE_CS_BLOCKS, D), f32, "a", dev, torch.full((K.MSE_CS_BLOCKS, D), float("nan")))
            assert K.mse_masked_bwd_colsum_ok(pred, tgt, dp.win, D)
        K.mse_masked_bwd(pred, tgt, mask, i["acc"].to(dev), torch.full((1,), MSE_G, device=dev), dp.win, dtg.win, B * N, D, gmul=MSE_GMUL,
                         colsum_ws=None if ws is None else ws.win)
        if ws is None:
            return {"dpred": dp, "dtgt": dtg}
        return {"dpred": dp, "dtgt": dtg, "colsum": Out(ws.win.double().sum(0), ws.full, ws.lead, ws.span)}
    B, rpb, D = c.sizes
    rows = B * rpb
    x = put(i["x"], d[0], P(0), dev)
    gamma = i["gamma"].to(dev)
    if c.entry == "layernorm_fwd":
        y = window((B, rpb + LN_PAD, D), d[1], "a", dev, torch.zeros(B, rpb + LN_PAD, D))
        mean, rstd = window((rows,), f32, "a", dev), window((rows,), f32, "a", dev)
        K.layernorm_fwd(x, gamma, i["beta"].to(dev), y.win[:, LN_PAD:], mean.win, rstd.win, B, rpb, D, rpb * D, (rpb + LN_PAD) * D,
                        LN_EPS_EXACT if c.opt == "const" else LN_EPS)
        y.zero_rows = y.win[:, :LN_PAD]
        y.win = y.win[:, LN_PAD:]
        return {"y": y, "mean": mean, "rstd": rstd}
    if c.entry == "layernorm_bwd":
        dyb = torch.zeros(B, rpb + LN_PAD, D)
        dyb[:, LN_PAD:] = i["dy"]
        dy = dyb.to(dev, d[1])[:, LN_PAD:]
        dx = window((B, rpb, D), d[0], "a", dev)
        dg, db = window((D,), f32, "a", dev, torch.zeros(D)), window((D,), f32, "a", dev, torch.zeros(D))
        K.layernorm_bwd(dy, x, gamma, i["mean"].to(dev), i["rstd"].to(dev), dx.win, dg.win, db.win, B, rpb, D, rpb * D, (rpb + LN_PAD) * D)
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    raise KeyError(c.entry)
