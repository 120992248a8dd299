"""The loss kernels at their launch-geometry edges: the case tables, seeded inputs and f64 references that tests/test_loss_edges_gpu.py
runs on the device and tests/test_loss_edges_cpu.py pins without one.

Inputs are drawn in f64 on the CPU and rounded to the dtype the kernel reads (f32; bf16 for the bf16 head attention), so the reference
sees the numbers the device sees.  References: oracle.mirror_oracle.mirror_loss / clip_loss / info_nce evaluated in f64 with autograd,
and the restatements below (the gathered CLIP term, the cross-entropy rows, the head attention, the flat terms).

Tolerances (the project's own, test_ce_rows_clip_loss / test_retention_style_cluster_losses):
    values     |got - ref| <= 1e-5 |ref| + 1e-6
    gradients  max |got - ref| <= 1e-4 max |ref| per tensor
    bf16       + 2^-8 |ref| elementwise (one rounding of the stored value)
`value_excess` / `grad_excess` return max(error / tolerance): <= 1 passes; a zero tolerance admits a zero error only.

Measured on the CPU (test_loss_edges_cpu.py asserts 8x these stay within the tolerances): an f32 evaluation of the same references
differs from f64 by at most
    MIRRORLoss (all LOSS_TERMS and COMPOSED_ONLY shapes, the unsaturated variants)   0.017 of the value tolerance, 0.012 of the gradient tolerance
    cross-entropy rows (CE_ROWS x CE_MODES)                                            0.112 / 0.078   (the +-100 logits, per-row losses near 0)
    gathered CLIP term                                                                 0.003 / 0.003
    InfoNCE                                                                            0.056 / 0.007
    style KL / symmetric KL / rownorm / exp / reparam                                  0.028 / 0.005
    head attention, f32 (inputs at half scale: 0.27 at unit scale)                     0.033 / 0.004
i.e. at most 1.7e-7 relative on the MIRRORLoss values and 1.2e-6 of max |ref| on its gradients.  The kernels themselves, on an MI355X,
reach at most 0.04 / 0.01 (MIRRORLoss, fused and composed), 0.11 / 0.08 (cross-entropy rows), 0.09 / 0.004 (head attention in f32) of
the same tolerances; the bf16 outputs sit at up to 0.99 of theirs, which is the one rounding the bf16 term stands for.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from oracle import mirror_oracle as O

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16

VAL_RTOL, VAL_ATOL, GRAD_RTOL, BF16_REL = 1e-5, 1e-6, 1e-4, 2.0 ** -8
SAT_ABS = 1e-5                     # saturated alignment: the kernel's own rounding w * s * 2^-23 per logit (about 6e-6 / B)


def f32_of(x: float) -> float:
    """A Python float as the f32 the C ABI passes on."""
    return float(torch.tensor(x, dtype=f32))


def _ratio(err: torch.Tensor, tol: torch.Tensor) -> float:
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    r = torch.where(torch.isfinite(err), r, torch.full_like(err, float("inf")))        # a nan / inf never passes
    return float(r.max())


def value_excess(got, ref, bf16_out: bool = False) -> float:
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = VAL_RTOL * ref.abs() + VAL_ATOL + (BF16_REL * ref.abs() if bf16_out else 0.0)
    return _ratio((got - ref).abs(), tol)


def grad_excess(got, ref, bf16_out: bool = False) -> float:
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = torch.full_like(ref, GRAD_RTOL * float(ref.abs().max()) if ref.numel() else 0.0)
    if bf16_out:
        tol = tol + BF16_REL * ref.abs()
    return _ratio((got - ref).abs(), tol)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(abs(hash_num(key)) % (2 ** 31))


def hash_num(k) -> int:
    """A seed contribution that does not depend on PYTHONHASHSEED."""
    if isinstance(k, (int, bool)):
        return int(k) + 1
    if isinstance(k, float):
        return int(k * 1000) + 3
    if isinstance(k, (tuple, list)):
        return sum((i + 2) * 31 * hash_num(v) for i, v in enumerate(k)) + 5
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(k))) + 7


def _r(gen, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=gen, dtype=f64)


def _raise_last(x: torch.Tensor, below: float) -> None:
    """The last column to `below` under the row's largest entry: it keeps a share of the row's softmax however peaked that is, so a
    kernel that lost it would show."""
    if x.shape[1] > 1:
        x[:, -1] = x[:, :-1].max(dim=1).values - below


def as_f32(t: torch.Tensor) -> torch.Tensor:
    """f64 values that are f32 numbers."""
    return t.float().double()


def _unit(t: torch.Tensor) -> torch.Tensor:
    return t / t.norm(dim=-1, keepdim=True)


# ================================================================================ MIRRORLoss
# (B, N, F, G, D, P, S)
LOSS_TERMS = [
    (1, 4, 4, 5, 8, 1, 2),                   # B = 1 and P = 1: alignment and cluster terms exactly 0, gradients exactly 0
    (5, 7, 12, 77, 33, 70, 9),               # D = 32 + 1, scalar staging
    (16, 3, 8, 2048, 512, 3000, 128),        # the workload's shape, quad staging, BM = 16
    (17, 3, 8, 300, 30, 256, 16),            # BM = 32 from B = 17, D < 32, P = one block trip
    (32, 3, 8, 300, 582, 4096, 16),          # the largest D that B = 32 admits; all three k-loops; the last register-path P
    (3, 2, 4, 9, 16, 4097, 4),               # first global-path P
    (32, 3, 8, 20000, 256, 257, 16),         # RNA term of 640 000 elements; the G = 5 rows above leave most RNA blocks empty
]
EXACT_SHAPE = LOSS_TERMS[0]
COMPOSED_ONLY = [(32, 3, 8, 300, 583, 4096, 16), (33, 3, 8, 300, 64, 256, 16)]     # beside the admission edge
BITWISE_SHAPES = [LOSS_TERMS[2], LOSS_TERMS[6]]
SK_E, LOSS_BMAX, LOSS_LDS = 16, 32, 150 * 1024

Variant = collections.namedtuple("Variant", "name scale spread ones sat")
VARIANTS = [Variant("s14.3-sp1", 14.3, 1.0, False, False), Variant("s14.3-sp12", 14.3, 12.0, False, False),
            Variant("s100-sp1", 100.0, 1.0, False, False), Variant("s100-sp12", 100.0, 12.0, False, False),
            Variant("ones", 14.3, 1.0, True, False), Variant("sat", 100.0, 1.0, False, True)]
VARIANT = {v.name: v for v in VARIANTS}
GRAD_IDX = (0, 1, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14)        # everything but the masks
ALIGN_IDX = (0, 7, 14)
W_KW = ("alignment_loss_weight", "wsi_retention_loss_weight", "rna_retention_loss_weight", "style_loss_weight", "cluster_loss_weight")
W_DEFAULT = (0.5, 0.1, 0.1, 0.1, 0.2)
W_ZEROS = (0.0, 0.3, 0.0, 0.1, 0.7)
COMBOS = {"total": (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), "single": (1.0, 3.0, 0.0, 0.5, 0.0, 2.0)}     # coefficients of the six results


def align_lds_bytes(B: int, D: int) -> int:
    return 4 * (2 * B * (D + 1) + B * (B + 1))


def fwd_form(shape, ext: bool = False) -> str:
    B, _, _, _, D, P, _ = shape
    return "loss_terms_fwd:%s,%s" % ("ext" if ext else ("quad" if D % 4 == 0 else "scalar"), "regs" if P <= 256 * SK_E else "global")


def bwd_form(shape, ext: bool = False) -> str:
    B, _, _, _, D, P, _ = shape
    return "loss_terms_bwd:%s,%s" % ("ext" if ext else ("bm16" if B <= 16 else "bm32"), "regs" if P <= 256 * SK_E else "global")


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, vname: str):
    """The 15 arguments of MIRRORLoss.forward as f64 CPU tensors holding f32 numbers (the order of oracle.OUTPUT_NAMES)."""
    B, N, Fd, G, D, P, S = shape
    v = VARIANT[vname]
    gen = _gen("loss", shape, vname)
    w_al = _unit(_r(gen, B, D))
    r_al = _unit(w_al + 1e-3 * _r(gen, B, D)) if v.sat else _unit(_r(gen, B, D))
    w_mask = (torch.rand(B, N, generator=gen) < 0.75).double()
    r_mask = torch.ones(B, G, dtype=f64) if v.ones else (torch.rand(B, G, generator=gen) < 0.75).double()
    w_mask[0, 0] = w_mask[-1, -1] = r_mask[0, 0] = r_mask[-1, -1] = 1.0
    ins = [w_al, _r(gen, B, N, Fd), _r(gen, B, N, Fd), w_mask, v.spread * _r(gen, B, P), _r(gen, B, S), 0.3 * _r(gen, B, S),
           r_al, _r(gen, B, G), _r(gen, B, G), r_mask, v.spread * _r(gen, B, P), _r(gen, B, S), 0.3 * _r(gen, B, S),
           torch.tensor(v.scale, dtype=f64)]
    ins[8][-1, -1] = ins[9][-1, -1] + 2.0           # the last RNA element carries a gradient a lost tail would miss
    for i in (4, 11):                               # and the last prototype a share of every row's softmax, at any spread
        _raise_last(ins[i], 0.5 if i == 4 else 1.0)
    return tuple(as_f32(t) for t in ins)


def _drop_inputs(ins, drop: str):
    """The inputs with the tail a kernel could lose left out: the last prototype ("P"), the last embedding column ("D"), the last
    RNA element ("G"), the last style element ("S") or the last batch row ("B")."""
    ins = [t.clone() for t in ins]
    if drop == "P":
        ins[4], ins[11] = ins[4][:, :-1], ins[11][:, :-1]
    elif drop == "D":
        ins[0], ins[7] = ins[0][:, :-1], ins[7][:, :-1]
    elif drop == "G":
        ins[10][-1, -1] = 0.0
    elif drop == "S":                       # exp(0) + 0 - 1 - 0 = 0: the element adds nothing
        for i in (5, 6, 12, 13):
            ins[i][-1, -1] = 0.0
    elif drop == "B":
        ins = [t if t.dim() == 0 else t[:-1] for t in ins]
    else:
        raise KeyError(drop)
    return ins


def drops_of(shape):
    B, _, _, _, D, P, _ = shape
    return [d for d, ok in (("P", P > 1), ("D", D > 1 and B > 1), ("G", True), ("S", True), ("B", B > 1)) if ok]


def pad_like(t: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """t in the leading corner of zeros of ref's shape (what a kernel that lost a tail leaves unwritten is not what is compared: the
    reference without the tail, zero where the tail was)."""
    out = torch.zeros_like(ref)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


@functools.lru_cache(maxsize=None)
def loss_reference(shape, vname: str, weights=W_DEFAULT, combo: str = "total", dtype=f64, drop=None):
    """(the six losses, {argument index: gradient of the combination of them named by `combo`}) of oracle.mirror_loss in `dtype`."""
    ins = loss_inputs(shape, vname)
    if drop is not None:
        ins = _drop_inputs(ins, drop)
    ins = [t.clone().to(dtype).requires_grad_(i in GRAD_IDX) for i, t in enumerate(ins)]
    outs = O.mirror_loss(ins, weights)
    sum(c * o for c, o in zip(COMBOS[combo], outs) if c != 0.0).backward()
    grads = {i: (ins[i].grad if ins[i].grad is not None else torch.zeros_like(ins[i])).double() for i in GRAD_IDX}
    return [o.detach().double() for o in outs], grads


# ================================================================================ cross-entropy rows
# (R, C, label_off)
CE_ROWS = [(1, 1, 0), (5, 5, 0), (16, 16, 0), (63, 63, 0), (64, 64, 0), (65, 65, 0), (130, 130, 0), (16, 128, 48), (5, 20, 15), (7, 65, 0)]
CeMode = collections.namedtuple("CeMode", "name scale mul")
CE_MODES = [CeMode("tensor", 14.3, 1.0), CeMode("none", None, f32_of(1.0 / 0.07)), CeMode("half", 14.3, 0.5), CeMode("pm100", 100.0, 1.0)]
CE_MODE = {m.name: m for m in CE_MODES}
CE_PAD = (3, 2)                 # the column window buf[:, 3:3 + C] of a buffer C + 5 wide


@functools.lru_cache(maxsize=None)
def ce_inputs(case, mname: str):
    """G [R, C], scale (0-d or None), the per-row upstream [R] and the summed form's upstream [1]."""
    R, C, off = case
    m = CE_MODE[mname]
    gen = _gen("ce", case, mname)
    if mname == "pm100":                    # unit rows at scale 100: logits in [-100, 100], both ends reached
        G = torch.rand(R, C, generator=gen, dtype=f64) * 2 - 1
        G[:, 0::3] = 1.0
        G[:, 1::3] = -1.0
        G[:, -1] = 1.0
    else:
        G = 0.4 * _r(gen, R, C)
        _raise_last(G, 0.02)
    scale = None if m.scale is None else as_f32(torch.tensor(m.scale, dtype=f64))
    return as_f32(G), scale, as_f32(0.5 + torch.rand(R, generator=gen, dtype=f64)), as_f32(torch.tensor([0.7], dtype=f64))


def ce_rows64(G, scale, mul, off, coef, up, per_row: bool, drop=None):
    """lse [R], loss (rows [R] or their sum [1]), dG [R, C], dscale (0-d or None) of sum_r coef (lse_r - L[r, off + r]), L = scale mul G,
    written out (no F.cross_entropy).  drop "C": the row sums miss the last column; "R": the last row is not computed."""
    R, C = G.shape
    s = (1.0 if scale is None else scale) * mul
    L = s * G
    seen = L[:, :-1] if drop == "C" else L
    mx = seen.max(dim=1, keepdim=True).values
    lse = mx[:, 0] + (seen - mx).exp().sum(1).log()
    rows = coef * (lse - L[torch.arange(R), off + torch.arange(R)])
    w = coef * (up if per_row else up.expand(R))
    onehot = torch.zeros_like(G)
    onehot[torch.arange(R), off + torch.arange(R)] = 1.0
    p = (L - lse[:, None]).exp() - onehot
    if drop == "C":
        p[:, -1] = 0.0
    dG = w[:, None] * s * p
    dscale = None if scale is None else mul * (w[:, None] * p * G).sum()
    if drop == "R":
        lse, rows, dG = lse.clone(), rows.clone(), dG.clone()
        lse[-1], rows[-1], dG[-1] = 0.0, 0.0, 0.0
        if dscale is not None:
            dscale = mul * (w[:-1, None] * p[:-1] * G[:-1]).sum()
    return {"lse": lse, "loss": rows if per_row else rows.sum().reshape(1), "dG": dG, "dscale": dscale}


def ce_reference(case, mname: str, per_row: bool, dtype=f64, drop=None):
    G, scale, up_rows, up_sum = ce_inputs(case, mname)
    R, C, off = case
    c = lambda t: None if t is None else t.to(dtype)
    out = ce_rows64(c(G), c(scale), CE_MODE[mname].mul, off, 0.5 / R, c(up_rows if per_row else up_sum), per_row, drop)
    return {k: (None if v is None else v.double()) for k, v in out.items()}


# ================================================================================ gathered CLIP term
# (B, world, rank, D): the local rows off = rank * B of a [world * B, D] set
GATHERED = [(16, 8, 3, 33), (5, 4, 3, 256), (7, 2, 0, 40)]


@functools.lru_cache(maxsize=None)
def gathered_inputs(case):
    B, world, rank, D = case
    gen = _gen("gathered", case)
    return as_f32(_unit(_r(gen, world * B, D))), as_f32(_unit(_r(gen, world * B, D))), as_f32(torch.tensor(14.3, dtype=f64))


def gathered_clip64(w_all, r_all, scale, off: int, B: int, drop=None):
    """0.5 / B sum over the local rows of (CE(s w r_all^T, off + r) + CE(s r w_all^T, off + r)), written out.  drop "C": the row sums
    miss the last gathered column."""
    w, r = w_all[off:off + B], r_all[off:off + B]
    lab = off + torch.arange(B)
    total = 0.0
    for L in (scale * w @ r_all.T, scale * r @ w_all.T):
        seen = L[:, :-1] if drop == "C" else L
        total = total + (torch.logsumexp(seen, 1) - L[torch.arange(B), lab]).sum()
    return (0.5 / B) * total


@functools.lru_cache(maxsize=None)
def gathered_reference(case, dtype=f64, drop=None):
    B, world, rank, D = case
    w, r, s = (t.clone().to(dtype).requires_grad_(True) for t in gathered_inputs(case))
    loss = gathered_clip64(w, r, s, rank * B, B, drop)
    loss.backward()
    return loss.detach().double(), [t.grad.double() for t in (w, r, s)]


# ================================================================================ InfoNCE without negatives
INFONCE = [(N, D, red, sym) for N in (1, 3, 65, 130) for D in (7, 256) for red in ("mean", "none") for sym in (False, True)]


@functools.lru_cache(maxsize=None)
def infonce_inputs(N: int, D: int):
    gen = _gen("infonce", N, D)
    return as_f32(_r(gen, N, D)), as_f32(_r(gen, N, D)), as_f32(0.5 + torch.rand(N, generator=gen, dtype=f64))


@functools.lru_cache(maxsize=None)
def infonce_reference(case, dtype=f64, drop=None):
    """O.info_nce at temperature 0.1 and its gradients (reduction "none": through sum(up * loss))."""
    N, D, red, sym = case
    q, k, up = infonce_inputs(N, D)
    if drop == "D":
        q, k = q[:, :-1], k[:, :-1]
    elif drop == "B":
        q, k, up = q[:-1], k[:-1], up[:-1]
    q, k = (t.clone().to(dtype).requires_grad_(True) for t in (q, k))
    loss = O.info_nce(q, k, 0.1, red, sym)
    ((loss * up.to(dtype)).sum() if red == "none" else loss).backward()
    return loss.detach().double(), [q.grad.double(), k.grad.double()]


# ================================================================================ flat and row kernels
FLAT_N = (1, 255, 256, 257, 262144, 262144 + 769)           # kl / clamp_: the grid is capped at 1024 blocks of 256
FLAT_CAP = 256 * 1024
SYMKL = [(1, 1), (3, 2), (4, 255), (4, 256), (4, 257), (2, 4096), (2, 4097), (16, 3000)]
SPREADS = (1.0, 12.0)
ROWNORM = [(rows, D) for rows in (1, 5, 300) for D in (1, 40, 64, 65, 3000)]
SMALL_N = (1, 257)
CLAMP_LO, CLAMP_HI = 0.0, f32_of(math.log(100.0))


@functools.lru_cache(maxsize=None)
def kl_inputs(n: int):
    gen = _gen("kl", n)
    return as_f32(_r(gen, n)), as_f32(0.3 * _r(gen, n)), as_f32(torch.tensor([0.7], dtype=f64))


def kl_reference(n: int, dtype=f64, drop=None):
    """coef sum(exp(ls) + mu^2 - 1 - ls) at coef = 0.5 / 16 and its gradients under the upstream."""
    mu, ls, up = kl_inputs(n)
    mu, ls = (t.clone().to(dtype).requires_grad_(True) for t in (mu, ls))
    keep = slice(0, n - 1) if drop == "n" else slice(0, n)
    loss = (0.5 / 16) * (ls[keep].exp() + mu[keep] ** 2 - 1 - ls[keep]).sum()
    (up.to(dtype)[0] * loss).backward()
    return loss.detach().double().reshape(1), [mu.grad.double(), ls.grad.double()]


@functools.lru_cache(maxsize=None)
def clamp_inputs(n: int):
    gen = _gen("clamp", n)
    return as_f32(4.0 * _r(gen, n) + 2.0)


@functools.lru_cache(maxsize=None)
def symkl_inputs(case, spread: float):
    B, P = case
    gen = _gen("symkl", case, spread)
    w, r = spread * _r(gen, B, P), spread * _r(gen, B, P)
    _raise_last(w, 0.5), _raise_last(r, 1.0)
    return as_f32(w), as_f32(r), as_f32(torch.tensor([0.7], dtype=f64))


def symkl_reference(case, spread: float, dtype=f64, drop=None):
    """coef sum_b sum_k (p_r - p_w)(log p_r - log p_w) at coef = 0.5 / B and its gradients under the upstream."""
    B, P = case
    w, r, up = symkl_inputs(case, spread)
    w, r = (t.clone().to(dtype).requires_grad_(True) for t in (w, r))
    ws, rs = (w[:, :-1], r[:, :-1]) if drop == "P" else ((w[:-1], r[:-1]) if drop == "B" else (w, r))
    lw, lr = F.log_softmax(ws, -1), F.log_softmax(rs, -1)
    loss = (0.5 / B) * ((lr.exp() - lw.exp()) * (lr - lw)).sum()
    (up.to(dtype)[0] * loss).backward()
    return loss.detach().double().reshape(1), [w.grad.double(), r.grad.double()]


@functools.lru_cache(maxsize=None)
def rownorm_inputs(case):
    rows, D = case
    w = 2.0 * _r(_gen("rownorm", case), rows, D)
    w[:, -1] = 2.0 * math.sqrt(D)           # half of the squared norm: a sum that lost it would show (and no row is unit as it stands)
    if rows > 1:
        w[rows // 2] = 0.0                  # one all-zero row: 0 / max(0, eps) = 0
    return as_f32(w)


def rownorm_reference(case, dtype=f64, drop=None, eps: float = 1e-12):
    w = rownorm_inputs(case).to(dtype)
    n = (w[:, :-1] if drop == "D" else w).norm(dim=1, keepdim=True).clamp_min(eps)
    out = w / n
    if drop == "B":
        out[-1] = w[-1]
    return out.double()


def zero_row(case):
    return None if case[0] == 1 else case[0] // 2


def weighted_sum_inputs(n: int):
    """Small integers: every product and partial sum is an f32 number, so the result is exact."""
    return [float(3 * i - 4) for i in range(n)], [float(2 * i + 1) for i in range(n)], 3.0            # terms, weights, upstream


@functools.lru_cache(maxsize=None)
def small_inputs(n: int):
    gen = _gen("small", n)
    return tuple(as_f32(_r(gen, n)) for _ in range(4))         # x / mu, logstd, eps, the upstream


def exp_reference(n: int, dtype=f64, drop=None):
    x, _, _, dy = (t.to(dtype) for t in small_inputs(n))
    y = x.exp()
    dx = dy * y
    if drop == "n":
        y, dx = y.clone(), dx.clone()
        y[-1], dx[-1] = 0.0, 0.0
    return y.double(), dx.double()


def reparam_reference(n: int, dtype=f64, drop=None):
    mu, ls, eps, dz = (t.to(dtype) for t in small_inputs(n))
    z, dmu, dls = mu + eps * (0.5 * ls).exp(), dz.clone(), dz * eps * 0.5 * (0.5 * ls).exp()
    if drop == "n":
        z, dls = z.clone(), dls.clone()
        z[-1], dmu[-1], dls[-1] = 0.0, 0.0, 0.0
    return z.double(), dmu.double(), dls.double()


# ================================================================================ head attention
# (B, H, hd)
HEADATTN = [(1, 1, 1), (5, 8, 4), (3, 17, 3), (2, 64, 1), (2, 64, 64), (2, 8, 512)]
HA_MAX_H, HA_MAX_D = 64, 4096


def ha_lds_bytes(H: int, hd: int, bwd: bool) -> int:
    return (16 * H * hd + 8 * H * H) if bwd else (12 * H * hd + 4 * H * H)


@functools.lru_cache(maxsize=None)
def headattn_inputs(case, dtype):
    """qkv [B, 3 H hd] and the upstream [B, H hd], quantised to `dtype` (f32 or bf16) first."""
    B, H, hd = case
    gen = _gen("headattn", case)
    q = lambda t: t.to(dtype).double()
    return q(0.5 * _r(gen, B, 3 * H * hd)), q(_r(gen, B, H * hd))      # at unit scale an f32 evaluation of D = 4096 is 0.27 of the tolerance


def headattn64(qkv: torch.Tensor, H: int, drop=None):
    """oracle.rna_attention without its linears, written out: attention over the HEADS axis, out[b, d H + h] = o[b, h, d].
    drop "D": the last feature of every head is left out of the scores; "H": the softmax misses the last head."""
    B, D3 = qkv.shape
    hd = D3 // 3 // H
    q, k, v = qkv.reshape(B, 3, H, hd).unbind(1)
    qs, ks = (q[..., :-1], k[..., :-1]) if drop == "D" else (q, k)
    s = torch.einsum("bhd,bgd->bhg", qs, ks) / math.sqrt(hd)
    e = (s - s.max(-1, keepdim=True).values).exp()
    if drop == "H":
        e = torch.cat([e[..., :-1], torch.zeros_like(e[..., -1:])], -1)
    a = e / e.sum(-1, keepdim=True)
    o = torch.einsum("bhg,bgd->bhd", a, v)
    return o.transpose(1, 2).reshape(B, H * hd), a


@functools.lru_cache(maxsize=None)
def headattn_reference(case, dtype, ref_dtype=f64, drop=None):
    """out, attn and dqkv under the upstream, on the values quantised to `dtype`."""
    B, H, hd = case
    qkv, dout = headattn_inputs(case, dtype)
    qkv = qkv.clone().to(ref_dtype).requires_grad_(True)
    out, attn = headattn64(qkv, H, drop)
    out.backward(dout.to(ref_dtype))
    return out.detach().double(), attn.detach().double(), qkv.grad.double()
