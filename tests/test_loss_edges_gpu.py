"""The loss kernels against f64 at their launch-geometry edges: every case of tests/loss_edge_cases.py is run through the kernels and
compared with the f64 reference of the same operation on the same (f32 / bf16) numbers — all six losses, lse / loss_rows / attn where
they exist, every input gradient — under the tolerances stated there (nothing of them measured here).  The fused MIRRORLoss and the
composed per-term kernels must each meet f64, not merely each other.  tests/test_loss_edges_cpu.py pins what the comparisons rest on.

Measured on the device: see the figures each test prints (pytest -s)."""
import math

import pytest
import torch

from mirror_amd import MirrorHipError
from mirror_amd import functional as Fn
from mirror_amd import kernels as K
from mirror_amd.losses import InfoNCE, MIRRORLoss
from mirror_amd.losses.mirror_loss import ClipLoss
from tests import loss_edge_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16
NAMES = L.O.OUTPUT_NAMES


def _ids(v):
    return str(v).replace(" ", "")


def dev(t, dtype=f32, grad=False):
    return t.to(dtype).to(DEV).requires_grad_(grad)


def check_values(got, ref, what, bf16_out=False):
    x = L.value_excess(got, ref, bf16_out)
    print(f"{what}: {x:.3f} of the value tolerance")
    assert x <= 1.0, f"{what}: {x:.3f} of the value tolerance"


def check_grad(got, ref, what, bf16_out=False):
    x = L.grad_excess(got, ref, bf16_out)
    print(f"{what}: {x:.3f} of the gradient tolerance")
    assert x <= 1.0, f"{what}: {x:.3f} of the gradient tolerance"


# ================================================================================================ MIRRORLoss
def _spy_forms(monkeypatch):
    """The form each direction of the fused loss noted, read in the thread that launched it (autograd runs the backward on its own)."""
    seen = {}
    for name in ("loss_terms_fwd", "loss_terms_bwd"):
        inner = getattr(K, name)

        def spy(weights, t, inner=inner, name=name):
            inner(weights, t)
            seen[name] = K.last_form()
        monkeypatch.setattr(K, name, spy)
    return seen


def _mirror_inputs(shape, vname):
    return [dev(t, grad=i in L.GRAD_IDX) for i, t in enumerate(L.loss_inputs(shape, vname))]


def _run_mirror(shape, vname, weights=L.W_DEFAULT, combo="total"):
    ins = _mirror_inputs(shape, vname)
    out = MIRRORLoss(**dict(zip(L.W_KW, weights)))(*ins)
    sum(c * o for c, o in zip(L.COMBOS[combo], out) if c != 0.0).backward()
    return out, ins


def _zero_if_none(ins, i):
    return torch.zeros_like(ins[i]) if ins[i].grad is None else ins[i].grad


def _check_mirror(out, ins, shape, vname, weights=L.W_DEFAULT, combo="total"):
    ref_l, ref_g = L.loss_reference(shape, vname, weights, combo)
    tag = f"{shape} {vname} {combo}"
    if not L.VARIANT[vname].sat:
        for name, got, ref in zip(L.O.LOSS_NAMES, out, ref_l):
            check_values(got, ref, f"{tag} {name}")
        for i in L.GRAD_IDX:
            check_grad(_zero_if_none(ins, i), ref_g[i], f"{tag} d {NAMES[i]}")
        return
    # saturated alignment: the f64 gradients are below 1e-12 (the CPU test asserts it); what the kernel may leave is its own rounding
    assert all(bool(torch.isfinite(o).all()) for o in out) and all(bool(torch.isfinite(_zero_if_none(ins, i)).all()) for i in L.GRAD_IDX)
    a = abs(float(out[1]))
    print(f"{tag}: alignment loss {a:.3e}")
    assert a <= L.SAT_ABS
    # the total carries weight[0] times the alignment term: its bound carries that share of the absolute one
    assert abs(float(out[0]) - float(ref_l[0])) <= L.VAL_RTOL * abs(float(ref_l[0])) + L.VAL_ATOL + weights[0] * L.SAT_ABS
    for name, got, ref in list(zip(L.O.LOSS_NAMES, out, ref_l))[2:]:
        check_values(got, ref, f"{tag} {name}")
    for i in L.GRAD_IDX:
        if i in L.ALIGN_IDX:
            g = float(ins[i].grad.abs().max())
            print(f"{tag} d {NAMES[i]}: max |g| {g:.3e}")
            assert g <= L.SAT_ABS
        else:
            check_grad(ins[i].grad, ref_g[i], f"{tag} d {NAMES[i]}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("vname", [v.name for v in L.VARIANTS])
@pytest.mark.parametrize("shape", L.LOSS_TERMS, ids=_ids)
def test_mirror_loss_meets_f64(shape, vname, fused, monkeypatch):
    monkeypatch.setattr(Fn, "_LOSS_FUSED", fused)
    seen = _spy_forms(monkeypatch)
    out, ins = _run_mirror(shape, vname)
    assert out[0].grad_fn.name().startswith("MirrorLossTermsFn") == fused
    if fused:
        assert seen == {"loss_terms_fwd": L.fwd_form(shape), "loss_terms_bwd": L.bwd_form(shape)}
    else:
        assert not seen
    _check_mirror(out, ins, shape, vname)
    if shape == L.EXACT_SHAPE and not L.VARIANT[vname].sat:        # B = 1, P = 1: exactly 0, values and gradients
        assert float(out[1]) == 0.0 and float(out[5]) == 0.0
        for i in L.ALIGN_IDX + (4, 11):
            assert float(ins[i].grad.abs().max()) == 0.0, NAMES[i]


@pytest.mark.parametrize("shape", L.LOSS_TERMS, ids=_ids)
def test_fused_loss_side_doors_meet_f64(shape, monkeypatch):
    """A backward through single returned terms, a weight tuple with zeros, and the form whose alignment term the caller supplies."""
    vname = L.VARIANTS[0].name
    seen = _spy_forms(monkeypatch)
    out, ins = _run_mirror(shape, vname, combo="single")
    assert out[0].grad_fn.name().startswith("MirrorLossTermsFn")
    _check_mirror(out, ins, shape, vname, combo="single")
    out, ins = _run_mirror(shape, vname, weights=L.W_ZEROS)
    _check_mirror(out, ins, shape, vname, weights=L.W_ZEROS)
    for i in L.ALIGN_IDX + (8, 9):                                 # weight 0: exactly no gradient
        assert float(ins[i].grad.abs().max()) == 0.0, NAMES[i]
    assert seen == {"loss_terms_fwd": L.fwd_form(shape), "loss_terms_bwd": L.bwd_form(shape)}
    # external alignment: the caller's term is the composed ClipLoss of the same embeddings
    ins = _mirror_inputs(shape, vname)
    w6 = L.W_DEFAULT[:3] + (L.W_DEFAULT[3],) + L.W_DEFAULT[3:]
    ext = ClipLoss()(ins[0], ins[7], ins[14]).reshape(())
    out = Fn.MirrorLossTermsFn.apply(w6, None, None, None, ext, ins[1], ins[2], ins[3], ins[1].shape[-1], None, ins[8], ins[9], ins[10],
                                     ins[5], ins[6], ins[12], ins[13], ins[4], ins[11])
    out[0].backward()
    assert seen == {"loss_terms_fwd": L.fwd_form(shape, ext=True), "loss_terms_bwd": L.bwd_form(shape, ext=True)}
    _check_mirror(out, ins, shape, vname)


@pytest.mark.parametrize("vname", [L.VARIANTS[0].name, L.VARIANTS[3].name, "sat"])
@pytest.mark.parametrize("shape", L.COMPOSED_ONLY, ids=_ids)
def test_past_the_admission_edge_the_composed_path_meets_f64(shape, vname):
    assert Fn._LOSS_FUSED
    out, ins = _run_mirror(shape, vname)
    assert not out[0].grad_fn.name().startswith("MirrorLossTermsFn")
    _check_mirror(out, ins, shape, vname)
    t = {"wsi_emb": ins[0].detach(), "rna_emb": ins[7].detach()}
    with pytest.raises(MirrorHipError):                             # and the descriptor refuses the shape outright
        K._loss_terms_desc((0.0,) * 6, t)


@pytest.mark.parametrize("shape", L.BITWISE_SHAPES, ids=_ids)
def test_two_launches_of_the_fused_pair_agree_bit_for_bit(shape):
    runs = []
    for _ in range(2):
        out, ins = _run_mirror(shape, L.VARIANTS[0].name)
        assert out[0].grad_fn.name().startswith("MirrorLossTermsFn")
        runs.append([o.detach().clone() for o in out] + [ins[i].grad.clone() for i in L.GRAD_IDX])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ================================================================================================ cross-entropy rows
def _ce_run(case, mname, per_row, window):
    R, C, off = case
    G64, scale64, up_rows, up_sum = L.ce_inputs(case, mname)
    mul, coef = L.CE_MODE[mname].mul, 0.5 / R
    if window:
        buf = torch.full((R, C + sum(L.CE_PAD)), 7.0, device=DEV)
        G = buf[:, L.CE_PAD[0]:L.CE_PAD[0] + C]
        G.copy_(dev(G64))
        assert G.stride(0) == C + 5 and (not G.is_contiguous() or R == 1)
    else:
        G = dev(G64)
    scale = None if scale64 is None else dev(scale64).reshape(1)
    out = torch.zeros(1, device=DEV)
    rows = torch.empty(R, device=DEV) if per_row else None
    lse = K.ce_rows_fwd(G, scale, mul, off, coef, out, rows)
    up = dev(up_rows if per_row else up_sum)
    ds0 = None if scale is None else torch.zeros(1, device=DEV)
    ds1 = None if scale is None else torch.ones(1, device=DEV)       # dscale accumulates: handed in holding 1.0
    dG = K.ce_rows_bwd(G, scale, mul, lse, up, per_row, coef, ds0, off)
    dG1 = K.ce_rows_bwd(G, scale, mul, lse, up, per_row, coef, ds1, off)
    assert torch.equal(dG, dG1)
    return {"lse": lse, "loss": rows if per_row else out, "dG": dG, "dscale": None if ds0 is None else ds0.reshape(()),
            "dscale_on_one": None if ds1 is None else ds1.reshape(())}


@pytest.mark.parametrize("mname", [m.name for m in L.CE_MODES])
@pytest.mark.parametrize("case", L.CE_ROWS, ids=_ids)
def test_ce_rows_meet_f64(case, mname):
    R, C, off = case
    for per_row in (False, True):
        ref = L.ce_reference(case, mname, per_row)
        for window in (False, True):
            got = _ce_run(case, mname, per_row, window)
            tag = f"ce {case} {mname} {'rows' if per_row else 'sum'} {'window' if window else 'contiguous'}"
            check_values(got["lse"], ref["lse"], tag + " lse")
            check_values(got["loss"], ref["loss"], tag + " loss")
            check_grad(got["dG"], ref["dG"], tag + " dG")
            if ref["dscale"] is not None:
                check_grad(got["dscale"], ref["dscale"], tag + " dscale")
                # handed in holding 1.0 it comes back holding 1 + dscale: each of the R atomic adds rounds a sum near 1 + |dscale| once
                x = abs(float(got["dscale_on_one"]) - 1.0 - float(ref["dscale"]))
                assert x <= L.GRAD_RTOL * abs(float(ref["dscale"])) + R * 2.0 ** -24 * (1.0 + abs(float(ref["dscale"]))), tag
            if C == 1:          # a single logit: exact
                assert float(got["loss"].abs().max()) == 0.0 and float(got["dG"].abs().max()) == 0.0
                assert got["dscale"] is None or float(got["dscale"]) == 0.0


@pytest.mark.parametrize("case", L.GATHERED, ids=_ids)
def test_gathered_clip_term_meets_f64(case):
    """CERowsFn + MatmulNTFn on the local rows of a [world * B, D] set, as clip_loss_terms composes them behind its all-gather."""
    B, world, rank, D = case
    w_all, r_all, s = (dev(t, grad=True) for t in L.gathered_inputs(case))
    off = rank * B
    w, r = w_all[off:off + B], r_all[off:off + B]
    li = Fn.CERowsFn.apply(Fn.MatmulNTFn.apply(w, r_all), s, 1.0, off, 0.5 / B, False)
    lt = Fn.CERowsFn.apply(Fn.MatmulNTFn.apply(r, w_all), s, 1.0, off, 0.5 / B, False)
    loss = (li + lt).reshape(())
    loss.backward()
    ref_l, ref_g = L.gathered_reference(case)
    check_values(loss, ref_l, f"gathered {case} loss")
    for name, t, ref in zip(("d w_all", "d r_all", "d scale"), (w_all, r_all, s), ref_g):
        check_grad(t.grad, ref, f"gathered {case} {name}")


@pytest.mark.parametrize("case", L.INFONCE, ids=_ids)
def test_infonce_without_negatives_meets_f64(case):
    N, D, red, sym = case
    q64, k64, up = L.infonce_inputs(N, D)
    q, k = dev(q64, grad=True), dev(k64, grad=True)
    loss = InfoNCE(temperature=0.1, reduction=red, symmetric=sym)(q, k)
    ((loss * dev(up)).sum() if red == "none" else loss).backward()
    ref_l, ref_g = L.infonce_reference(case)
    check_values(loss, ref_l, f"infonce {case} loss")
    if N == 1:          # a single logit: exact
        assert float(loss.abs().max()) == 0.0 and float(q.grad.abs().max()) == 0.0 and float(k.grad.abs().max()) == 0.0
        return
    check_grad(q.grad, ref_g[0], f"infonce {case} dq")
    check_grad(k.grad, ref_g[1], f"infonce {case} dk")


# ================================================================================================ flat and row kernels
@pytest.mark.parametrize("n", L.FLAT_N)
def test_kl_and_clamp_meet_f64(n):
    mu, ls, up = (dev(t) for t in L.kl_inputs(n))
    out = torch.zeros(1, device=DEV)
    K.kl_fwd(mu, ls, out, 0.5 / 16)
    dmu, dls = K.kl_bwd(mu, ls, up, 0.5 / 16)
    ref_l, (ref_mu, ref_ls) = L.kl_reference(n)
    check_values(out, ref_l, f"kl {n}")
    check_grad(dmu, ref_mu, f"kl {n} dmu")
    check_grad(dls, ref_ls, f"kl {n} dlogstd")
    x64 = L.clamp_inputs(n)
    x = dev(x64)
    K.clamp_(x, L.CLAMP_LO, L.CLAMP_HI)
    assert torch.equal(x.cpu(), x64.float().clamp(L.CLAMP_LO, L.CLAMP_HI))          # exact


def test_clamp_keeps_a_nan_and_bounds_the_infinities():
    lo, hi = L.CLAMP_LO, L.CLAMP_HI
    x = torch.tensor([float("nan"), float("-inf"), float("inf"), lo - 1, hi + 1, 0.5 * (lo + hi)], device=DEV)
    want = x.cpu().clamp(lo, hi)
    K.clamp_(x, lo, hi)
    got = x.cpu()
    assert math.isnan(float(got[0])) and torch.equal(got[1:], want[1:]) and got[1:].tolist() == [lo, hi, lo, hi, 0.5 * (lo + hi)]


@pytest.mark.parametrize("idx", [5, 41], ids=["quad-body", "scalar-tail"])
def test_adam_clamped_element_keeps_a_nan(idx):
    """One Adam step over 43 parameters (10 quads and a tail of 3) with a NaN gradient at the clamped index: parameter and bf16 shadow
    stay NaN, every other element is what the step without the clamp leaves."""
    n = 43
    gen = torch.Generator().manual_seed(17)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g0[idx] = float("nan")
    res = []
    for clamp in (None, (idx, 0.0, math.log(100.0))):
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.zeros(n, device=DEV, dtype=bf16)
        K.adam(p, g0.to(DEV), m, v, sh, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, clamp=clamp)
        res.append((p.cpu(), sh.cpu()))
    (p_free, sh_free), (p_cl, sh_cl) = res
    assert math.isnan(float(p_free[idx])) and math.isnan(float(p_cl[idx])) and math.isnan(float(sh_cl[idx].float()))
    keep = torch.arange(n) != idx
    assert torch.equal(p_cl[keep], p_free[keep]) and torch.equal(sh_cl[keep], sh_free[keep])
    assert bool(torch.isfinite(p_cl[keep]).all()) and not torch.equal(p_cl[keep], p0[keep])
    # a finite update past the bounds is clamped as before
    g1 = g0.clone()
    g1[idx] = 1.0
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lo, hi = float(p0[idx]) + 0.25, float(p0[idx]) + 0.5
    K.adam(p, g1.to(DEV), m, v, None, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, clamp=(idx, lo, hi))
    assert float(p[idx]) == L.f32_of(lo)


@pytest.mark.parametrize("spread", L.SPREADS)
@pytest.mark.parametrize("case", L.SYMKL, ids=_ids)
def test_symkl_meets_f64(case, spread):
    B, P = case
    w, r, up = (dev(t) for t in L.symkl_inputs(case, spread))
    out = torch.zeros(1, device=DEV)
    K.symkl_fwd(w, r, out, 0.5 / B)
    dw, dr = K.symkl_bwd(w, r, up, 0.5 / B)
    ref_l, (ref_w, ref_r) = L.symkl_reference(case, spread)
    check_values(out, ref_l, f"symkl {case} {spread}")
    check_grad(dw, ref_w, f"symkl {case} {spread} dw")
    check_grad(dr, ref_r, f"symkl {case} {spread} dr")
    if P == 1:          # exact
        assert float(out) == 0.0 and float(dw.abs().max()) == 0.0 and float(dr.abs().max()) == 0.0


@pytest.mark.parametrize("with_shadow", [False, True], ids=["f32", "shadow"])
@pytest.mark.parametrize("case", L.ROWNORM, ids=_ids)
def test_rownorm_meets_f64(case, with_shadow):
    w = dev(L.rownorm_inputs(case))
    sh = torch.full(case, 7.0, device=DEV, dtype=bf16) if with_shadow else None
    K.rownorm_(w, shadow=sh)
    ref = L.rownorm_reference(case)
    check_values(w, ref, f"rownorm {case}")
    if with_shadow:
        check_values(sh.float(), ref, f"rownorm {case} shadow", bf16_out=True)
        assert torch.equal(sh, w.bfloat16())
    z = L.zero_row(case)
    if z is not None:
        assert float(w[z].abs().max()) == 0.0 and (sh is None or float(sh[z].float().abs().max()) == 0.0)


@pytest.mark.parametrize("n", range(1, 7))
def test_weighted_sum_is_exact(n):
    terms, weights, up = L.weighted_sum_inputs(n)
    out = K.weighted_sum([torch.tensor(t, device=DEV) for t in terms], weights)
    assert float(out) == sum(t * w for t, w in zip(terms, weights))
    d = K.weighted_sum_bwd(torch.tensor([up], device=DEV), weights)
    assert d.cpu().tolist() == [w * up for w in weights]


@pytest.mark.parametrize("n", L.SMALL_N)
def test_exp_and_reparam_meet_f64(n):
    x, ls, eps, dy = (dev(t) for t in L.small_inputs(n))
    y = K.exp_fwd(x)
    dx = torch.zeros(n, device=DEV)
    K.exp_bwd(dy, y, dx, accumulate=True)
    ref_y, ref_dx = L.exp_reference(n)
    check_values(y, ref_y, f"exp {n}")
    check_grad(dx, ref_dx, f"exp {n} dx")
    z = K.reparam_fwd(x, ls, eps)
    dmu, dls = K.reparam_bwd(ls, eps, dy)
    ref_z, ref_dmu, ref_dls = L.reparam_reference(n)
    check_values(z, ref_z, f"reparam {n}")
    check_grad(dmu, ref_dmu, f"reparam {n} dmu")
    check_grad(dls, ref_dls, f"reparam {n} dlogstd")


# ================================================================================================ head attention
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", L.HEADATTN, ids=_ids)
def test_headattn_meets_f64(case, dtype):
    B, H, hd = case
    qkv64, dout64 = L.headattn_inputs(case, dtype)
    qkv = dev(qkv64, dtype, grad=True)
    out = Fn.HeadAttnFn.apply(qkv, H)
    out.backward(dev(dout64, dtype))
    _, attn = K.headattn_fwd(qkv.detach(), H)
    ref_out, ref_attn, ref_dqkv = L.headattn_reference(case, dtype)
    is_bf = dtype == bf16
    assert out.dtype == dtype and qkv.grad.dtype == dtype and attn.dtype == f32
    check_values(out.float(), ref_out, f"headattn {case} {dtype} out", bf16_out=is_bf)
    check_values(attn, ref_attn, f"headattn {case} {dtype} attn")
    check_grad(qkv.grad.float(), ref_dqkv, f"headattn {case} {dtype} dqkv", bf16_out=is_bf)


def test_headattn_refuses_in_the_forward_what_the_backward_cannot_run():
    """Both directions admit H <= 64 and H hd <= 4096 and nothing else: a forward that went through has a backward that launches (the
    (2, 64, 64) and (2, 8, 512) cases above run both past 64 KiB of LDS), and what one refuses the other refuses."""
    for H, hd in ((65, 1), (8, 513), (64, 65)):
        qkv = torch.zeros(2, 3 * H * hd, device=DEV)
        with pytest.raises(MirrorHipError, match="unsupported"):
            Fn.HeadAttnFn.apply(qkv, H)
        with pytest.raises(MirrorHipError, match="unsupported"):
            K.headattn_bwd(qkv, torch.zeros(2, H, H, device=DEV), torch.zeros(2, H * hd, device=DEV), H)
