"""One pre-norm RNA Block (csrc/rna_block.hip: mh_rna_block_fwd / mh_rna_block_bwd) restated on the CPU by explicit formulas: the
forward, the input gradient and the twelve parameter gradients, with no autograd, so that every intermediate can be rounded
where the kernels round it.  Shared by tests/test_rna_block_ref_cpu.py and tests/test_rna_block_ref_gpu.py; shares no code with
mirror_amd.  Masks come from the host Philox stream (tests/philox_ref.py).

    h1 = LN1(x)        qkv = h1 Wqkv^T + bqkv      o = headattn(qkv)       x1 = x + m1 (o Wproj^T + bproj)
    h2 = LN2(x1)       u = h2 W1^T + b1            f = m2 gelu(u)          y  = x1 + m3 (f W2^T + b2)

`emulate=True` rounds where the kernels do (read from rna_block.hip and elementwise.hip's headattn kernels):
  * the four weight matrices are bf16 (the bf16 policy's shadows of the f32 masters);
  * h1, h2 are bf16 before their GEMMs (the weight gradients recompute the same rounded operand from the saved f32 stats);
  * qkv, o, u (before GELU) and f = gelu(unrounded pre-activation) m2 are stored in bf16; mean / rstd, attn, x1, y in f32;
  * G3 = bf16(dy m3), G1 = bf16(dx1 m1); bias gradients are column sums of the ROUNDED G, weight gradients G^T X of it;
  * dg = bf16((G3 W2) m2 gelu'(u as bf16)); dO and dqkv are bf16; dh2, dx1, dh1, dx are f32;
  * the head attention works in f32 on the bf16 qkv / dO and the saved f32 attn.
`emulate=False` is the exact Block in `dtype` arithmetic with no rounding at all.

`dtype` / `order` choose the arithmetic between the rounding points: float64 with torch's own summation (the reference), or
float32 with the contractions summed in another order (order 1: four interleaved groups of 32-wide k-steps, as a 4-wave split-K
does; order 2: two halves, the upper first) — a second draw of the rounding-boundary flips, used to measure the floor below.
"""
import functools
import json
import math
import os

import torch

from tests import philox_ref as PH

NAMES = ("g1", "be1", "w_qkv", "b_qkv", "w_proj", "b_proj", "g2", "be2", "w_fc1", "b_fc1", "w_fc2", "b_fc2")
GRAD_OF = {"g1": "dg1", "be1": "dbe1", "g2": "dg2", "be2": "dbe2", "w_qkv": "dw_qkv", "b_qkv": "db_qkv", "w_proj": "dw_proj", "b_proj": "db_proj",
           "w_fc1": "dw_fc1", "b_fc1": "db_fc1", "w_fc2": "dw_fc2", "b_fc2": "db_fc2"}
# Block parameter name (models/mirror.py) -> name here
MODULE_NAMES = {"norm1.weight": "g1", "norm1.bias": "be1", "attn.qkv.weight": "w_qkv", "attn.qkv.bias": "b_qkv", "attn.proj.weight": "w_proj",
                "attn.proj.bias": "b_proj", "norm2.weight": "g2", "norm2.bias": "be2", "mlp.fc1.weight": "w_fc1", "mlp.fc1.bias": "b_fc1",
                "mlp.fc2.weight": "w_fc2", "mlp.fc2.bias": "b_fc2"}
MUTATIONS = ("db_skip_last_row", "db_last_row_twice", "gelu_grad_without_mask2", "fc1_offset_plus_4", "dx1_without_residual",
             "dw_last_strip_zero", "ln2_operand_row16_zero", "dgamma_rows_0_15")


def q4(n):
    return (n + 3) // 4 * 4


def masks(B, D, Hh, p, seed, offset, base=None, fc1_shift=0):
    """The three keep-multipliers [B, D], [B, Hh], [B, D] (f32 numpy -> torch) of one call, or None in eval mode.  Site order: proj
    output at `offset`, fc1 activation q4(B D) behind it, fc2 output q4(B Hh) further; a device base is rounded down to 4."""
    if p <= 0.0:
        return None
    o2 = offset + q4(B * D)
    o3 = o2 + q4(B * Hh)
    t = lambda n, o, shape: torch.from_numpy(PH.dropout_mult(n, p, seed, o, base)).reshape(shape)  # noqa: E731
    return t(B * D, offset, (B, D)), t(B * Hh, o2 + fc1_shift, (B, Hh)), t(B * D, o3, (B, D))


class _Arith:
    def __init__(self, emulate, dtype, order):
        self.emulate, self.dt, self.order = emulate, dtype, (order if dtype != torch.float64 else 0)

    def bf(self, t):            # stored in / staged as bf16: from the f32 value the kernel holds, round to nearest even
        return t.to(torch.float32).to(torch.bfloat16).to(self.dt) if self.emulate else t

    def f32(self, t):           # stored in f32
        return t.to(torch.float32).to(self.dt) if self.emulate else t

    def mm(self, a, w):         # a [M, K] . w [N, K]^T
        K = a.shape[1]
        if self.order == 0 or K < 64:
            return a @ w.t() if self.order != 2 else (a.flip(1) @ w.flip(1).t())
        if self.order == 1:
            grp = (torch.arange(K) // 32) % 4
            parts = [a[:, grp == i] @ w[:, grp == i].t() for i in range(4)]
            return (parts[3] + parts[2]) + (parts[1] + parts[0])
        h = K // 2
        return a[:, h:] @ w[:, h:].t() + a[:, :h] @ w[:, :h].t()

    def rsum(self, t):          # sum over the last axis
        if self.order == 0:
            return t.sum(-1)
        n = t.shape[-1]
        if self.order == 1 and n % 4 == 0:
            return t.reshape(*t.shape[:-1], n // 4, 4).sum(-2).sum(-1)
        return t.flip(-1).sum(-1)

    def csum(self, t):          # sum over the rows
        return t.sum(0) if self.order == 0 else t.flip(0).sum(0)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def _ln_stats(A, x, eps):
    K = x.shape[1]
    mean = A.rsum(x) / K
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt(A.rsum(d * d) / K + eps)
    return A.f32(mean), A.f32(rstd)


def _ln_bwd(A, dh, x, mean, rstd, g, gamma_rows=None):
    K = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    a = dh * g
    c1, c2 = A.rsum(a) / K, A.rsum(a * xh) / K
    dxl = rstd[:, None] * (a - c1[:, None] - xh * c2[:, None])
    rows = slice(0, gamma_rows)
    return dxl, A.csum((dh * xh)[rows]), A.csum(dh[rows])


def _colsum(A, G, mut):
    s = A.csum(G)
    if mut == "db_skip_last_row":
        s = s - G[-1]
    if mut == "db_last_row_twice":
        s = s + G[-1]
    return s


def _wgrad(A, G, X, mut):       # G [B, M], X [B, K] -> [M, K]
    dw = A.mm(G.t().contiguous(), X.t().contiguous())
    if mut == "dw_last_strip_zero":
        dw = dw.clone()
        dw[:, -8:] = 0
    return dw


def block(x, dy, P, H, eps=1e-6, p=0.0, seed=0, offset=0, base=None, emulate=True, dtype=torch.float64, order=0, drop=None, mut=None):
    """x, dy [B, D]; P: name -> tensor (NAMES; b_qkv may be None).  drop: the three keep-multipliers handed in (else drawn from the
    host Philox stream when p > 0).  Returns a dict: y, the saved tensors (stats [4, B], qkv, attn, o, x1, u, f), dx and the
    parameter gradients under the kernels' names (GRAD_OF)."""
    assert mut is None or mut in MUTATIONS
    A = _Arith(emulate, dtype, order)
    B, D = x.shape
    Hh = P["w_fc1"].shape[0]
    hd = D // H
    if drop is None:
        drop = masks(B, D, Hh, p, seed, offset, base, 4 if mut == "fc1_offset_plus_4" else 0)
    one = torch.ones((), dtype=dtype)
    m1, m2, m3 = (one, one, one) if drop is None else [m.to(dtype) for m in drop]
    x, dy = x.to(dtype), dy.to(dtype)
    W = {k: (A.bf(v.to(dtype)) if k.startswith("w_") else v.to(dtype)) for k, v in P.items() if v is not None}
    bqkv = W.get("b_qkv")
    out = {}
    # ---------------------------------------------------------------- forward
    mean1, rstd1 = _ln_stats(A, x, eps)
    h1 = A.bf((x - mean1[:, None]) * rstd1[:, None] * W["g1"] + W["be1"])
    qkv = A.mm(h1, W["w_qkv"])
    qkv = A.bf(qkv + bqkv if bqkv is not None else qkv)
    q, k, v = qkv.reshape(B, 3, H, hd).unbind(1)
    scale = 1.0 / math.sqrt(hd)
    attn = A.f32(torch.softmax(torch.einsum("bhd,bgd->bhg", q, k) * scale, dim=-1))
    o = A.bf(torch.einsum("bhg,bgd->bhd", attn, v).transpose(1, 2).reshape(B, D))       # out[b, d H + h] = o[h][d]
    x1 = A.f32(x + (A.mm(o, W["w_proj"]) + W["b_proj"]) * m1)
    mean2, rstd2 = _ln_stats(A, x1, eps)
    h2 = A.bf((x1 - mean2[:, None]) * rstd2[:, None] * W["g2"] + W["be2"])
    h2_fwd = h2
    if mut == "ln2_operand_row16_zero":
        h2_fwd = h2.clone()
        h2_fwd[16:] = 0
    pre = A.mm(h2_fwd, W["w_fc1"]) + W["b_fc1"]
    u = A.bf(pre)
    f = A.bf(_gelu(pre) * m2)
    y = A.f32(x1 + (A.mm(f, W["w_fc2"]) + W["b_fc2"]) * m3)
    out.update(y=y, stats=torch.stack([mean1, rstd1, mean2, rstd2]), qkv=qkv, attn=attn, o=o, x1=x1, u=u, f=f)
    # ---------------------------------------------------------------- backward
    # fc2
    G3 = A.bf(dy * m3)
    out["db_fc2"] = _colsum(A, G3, mut)
    out["dw_fc2"] = _wgrad(A, G3, f, mut)
    dg = A.mm(G3, W["w_fc2"].t().contiguous())
    dg = A.bf(dg * ((m2 if mut != "gelu_grad_without_mask2" else one) * _gelu_grad(u)))
    # fc1
    out["db_fc1"] = _colsum(A, dg, mut)
    out["dw_fc1"] = _wgrad(A, dg, h2, mut)
    dh2 = A.f32(A.mm(dg, W["w_fc1"].t().contiguous()))
    # LN2' + residual, proj
    dxl, out["dg2"], out["dbe2"] = _ln_bwd(A, dh2, x1, mean2, rstd2, W["g2"], 16 if mut == "dgamma_rows_0_15" else None)
    dx1 = A.f32(dxl + dy if mut != "dx1_without_residual" else dxl)
    G1 = A.bf(dx1 * m1)
    out["db_proj"] = _colsum(A, G1, mut)
    out["dw_proj"] = _wgrad(A, G1, o, mut)
    dO = A.bf(A.mm(G1, W["w_proj"].t().contiguous()))
    # head attention
    dOh = dO.reshape(B, hd, H).transpose(1, 2)
    da = torch.einsum("bhd,bgd->bhg", dOh, v)
    ds = attn * (da - (da * attn).sum(-1, keepdim=True))
    dq = torch.einsum("bhg,bgd->bhd", ds, k) * scale
    dk = torch.einsum("bgh,bgd->bhd", ds, q) * scale
    dv = torch.einsum("bgh,bgd->bhd", attn, dOh)
    dqkv = A.bf(torch.stack([dq, dk, dv], dim=1).reshape(B, 3 * D))
    # qkv
    if bqkv is not None:
        out["db_qkv"] = _colsum(A, dqkv, mut)
    out["dw_qkv"] = _wgrad(A, dqkv, h1, mut)
    dh1 = A.f32(A.mm(dqkv, W["w_qkv"].t().contiguous()))
    dxl, out["dg1"], out["dbe1"] = _ln_bwd(A, dh1, x, mean1, rstd1, W["g1"], 16 if mut == "dgamma_rows_0_15" else None)
    out["dx"] = A.f32(dx1 + dxl)
    return out


# ------------------------------------------------------------------------------------------------ cases, distance, floor, bound
def make_case(B, D, H, Hh, qkv_bias=True, seed=0):
    """Deterministic inputs of one case: x, dy [B, D] and the twelve f32 parameters (weights ~ N(0, 1 / fan_in), LayerNorm weight
    1 + 0.1 N, biases 0.1 N)."""
    g = torch.Generator().manual_seed(1000003 * seed + 31 * B + 7 * D + Hh)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = {"g1": 1 + 0.1 * r(D), "be1": 0.1 * r(D), "w_qkv": r(3 * D, D) / math.sqrt(D), "b_qkv": 0.1 * r(3 * D) if qkv_bias else None,
         "w_proj": r(D, D) / math.sqrt(D), "b_proj": 0.1 * r(D), "g2": 1 + 0.1 * r(D), "be2": 0.1 * r(D), "w_fc1": r(Hh, D) / math.sqrt(D),
         "b_fc1": 0.1 * r(Hh), "w_fc2": r(D, Hh) / math.sqrt(Hh), "b_fc2": 0.1 * r(D)}
    return r(B, D), r(B, D), P


CHECKED = ("y", "stats", "u", "f", "dx") + tuple(GRAD_OF[n] for n in NAMES)


def dist(got, ref):
    """(relative Frobenius error, max-abs error relative to max |ref|), in float64."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300))


MARGIN = 4.0
# Eight f32 ulps.  The f32 run below uses the CPU's correctly rounded sqrt / exp / erf; the device's rsqrtf, __expf and erff are
# good to a few ulp each, so a measured floor under this line (a small case in which no bf16 rounding flipped) says how good the
# CPU's libm is, not how far a correct kernel may be from the reference.
FLOOR_MIN = 2.0 ** -20


def measure_floor(B, D, H, Hh, qkv_bias=True, p=0.0, draws=1):
    """name -> (Frobenius, max-abs) distance between the emulating reference in f64 and the same emulation in f32 arithmetic with
    its sums in another order (both orders), the largest over `draws` redraws of the inputs.  What separates the two runs is which
    side of a bf16 boundary an intermediate falls on: a small case has few roundings and a single draw often holds no flip in
    front of a given tensor, which is why the recorded floors (below) are taken over many draws."""
    fl = {}
    for s in range(draws):
        x, dy, P = make_case(B, D, H, Hh, qkv_bias, seed=100 + s)
        kw = dict(H=H, p=p, seed=0xF100 + s, offset=8 * s)
        ref = block(x, dy, P, **kw)
        for order in (1, 2):
            alt = block(x, dy, P, dtype=torch.float32, order=order, **kw)
            for k in CHECKED:
                if k in ref:
                    a, b = dist(alt[k], ref[k])
                    fa, fb = fl.get(k, (0.0, 0.0))
                    fl[k] = (max(fa, a), max(fb, b))
    return fl


def floor_draws(B, D, H, Hh):
    """Redraws behind a recorded floor: until about 2^21 bf16 roundings have been sampled, 2 at least, 128 at most (8 where the
    weights alone are above 4 M elements: those cases draw hundreds of flips in one run)."""
    n_round = B * (11 * D + 3 * Hh)
    return min(8 if 4 * D * D + 2 * D * Hh > (4 << 20) else 128, max(2, -(-(1 << 21) // n_round)))


P50_CASES = ((16, 96, 12, 192, True), (17, 768, 12, 1536, True))          # the two cases that also run at p = 0.5
FLOORS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rna_block_floors.json")


def floor_modes(case):
    return (0.0, 0.1, 0.5) if tuple(case) in P50_CASES else (0.0, 0.1)


def case_key(B, D, H, Hh, qkv_bias=True):
    return "%d,%d,%d,%d,%d" % (B, D, H, Hh, int(qkv_bias))


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FLOORS_FILE) as fh:
        return json.load(fh)


def floor(B, D, H, Hh, qkv_bias=True, p=0.0):
    """The recorded floor of a case at dropout probability p, name -> (Frobenius, max-abs): measure_floor over floor_draws(...) draws
    (tests/golden/rna_block_floors.json, written by `python -m tests.rna_block_ref`; test_rna_block_ref_cpu.py measures again), and
    never under FLOOR_MIN."""
    rec = _recorded()[case_key(B, D, H, Hh, qkv_bias)]["%g" % p]
    return {k: (max(a, FLOOR_MIN), max(b, FLOOR_MIN)) for k, (a, b) in rec.items()}


def bound(B, D, H, Hh, qkv_bias=True, p=0.0):
    return {k: (MARGIN * a, MARGIN * b) for k, (a, b) in floor(B, D, H, Hh, qkv_bias, p).items()}


def outside(got, ref, bd):
    """True when got is outside the bound in either measure."""
    a, b = dist(got, ref)
    return a > bd[0] or b > bd[1]


# (B, D, H, Hh, qkv_bias): the smallest shapes that reach each path of csrc/rna_block.hip (tests/test_rna_block_ref_gpu.py says which)
CASES = ((1, 32, 8, 32, True), (15, 96, 12, 192, True), (16, 96, 12, 192, True), (17, 96, 12, 192, True), (31, 96, 12, 192, True),
         (32, 96, 12, 192, True), (5, 64, 8, 128, False), (4, 1024, 8, 1024, True), (16, 256, 8, 4096, True), (2, 1632, 17, 64, True),
         (17, 768, 12, 1536, True), (16, 512, 8, 2048, True))


if __name__ == "__main__":          # python -m tests.rna_block_ref: measure and record the floors (CPU only, about a minute)
    rec = {}
    for c in CASES:
        rec[case_key(*c)] = {"%g" % p_: {k_: [float("%.3g" % a_), float("%.3g" % b_)]
                                         for k_, (a_, b_) in measure_floor(*c, p=p_, draws=floor_draws(*c[:4])).items()} for p_ in floor_modes(c)}
        print(case_key(*c), floor_draws(*c[:4]), flush=True)
    with open(FLOORS_FILE, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
