"""Without a device: the preconditions of tests/test_loss_edges_gpu.py.  The tables of tests/loss_edge_cases.py only test the launch
forms of the loss kernels while their sizes sit where the kernels switch, and the comparisons with f64 only mean something while the
tolerances have room over a plain f32 evaluation, the data would show a lost tail, and the restated references are the operations
they claim to be — all pinned here."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from mirror_amd import _lib
from mirror_amd import kernels as K
from oracle import mirror_oracle as O
from tests import loss_edge_cases as L

f64, f32 = torch.float64, torch.float32
MARGIN = 8.0                    # the f32 CPU evaluation must stay this many times inside every tolerance
RANDOM_VARIANTS = [v.name for v in L.VARIANTS if not v.sat]
ALL_SHAPES = L.LOSS_TERMS + L.COMPOSED_ONLY


def _ids(v):
    return str(v).replace(" ", "")


# ------------------------------------------------------------------------------------------------ what the tables claim
def test_the_admission_edge_is_where_the_table_puts_it():
    assert K.loss_terms_ok(32, 582) and K.loss_terms_ok(16, 1024)
    assert not K.loss_terms_ok(32, 583) and not K.loss_terms_ok(33, 8)
    assert L.align_lds_bytes(32, 582) == 153472 <= L.LOSS_LDS == 153600 < L.align_lds_bytes(32, 583)
    for shape in L.LOSS_TERMS:
        assert K.loss_terms_ok(shape[0], shape[4]), shape
    for shape in L.COMPOSED_ONLY:
        assert not K.loss_terms_ok(shape[0], shape[4]), shape
    assert L.COMPOSED_ONLY[0][4] == 583 and L.COMPOSED_ONLY[0][0] == 32 and L.COMPOSED_ONLY[1][0] == L.LOSS_BMAX + 1
    assert (582 - 18 * 32) // 4 == 1 and 582 % 4 == 2                        # D = 582 walks the 32-wide, the 4-wide and the scalar k-loop


def test_the_sizes_straddle_the_switches():
    Ps = {s[5] for s in L.LOSS_TERMS}
    assert {1, 256, 257, 256 * L.SK_E, 256 * L.SK_E + 1} <= Ps                # one trip, the register / global switch
    Bs = {s[0] for s in L.LOSS_TERMS}
    assert {1, 16, 17, 32} <= Bs                                             # align_bwd<16> / <32>
    Ds = {s[4] for s in L.LOSS_TERMS}
    assert any(d % 4 for d in Ds if d > 32) and any(d % 4 == 0 for d in Ds) and any(d < 32 for d in Ds)
    assert any(s[0] * s[3] < 32 * 256 for s in L.LOSS_TERMS) and max(s[0] * s[3] for s in L.LOSS_TERMS) == 640000
    assert {f for s in L.LOSS_TERMS for f in (L.fwd_form(s), L.bwd_form(s))} == {
        "loss_terms_fwd:quad,regs", "loss_terms_fwd:scalar,regs", "loss_terms_fwd:quad,global",
        "loss_terms_bwd:bm16,regs", "loss_terms_bwd:bm32,regs", "loss_terms_bwd:bm16,global"}
    assert max(L.FLAT_N) > L.FLAT_CAP and L.FLAT_CAP in L.FLAT_N and {255, 256, 257} <= set(L.FLAT_N)
    Rs, Cs = {c[0] for c in L.CE_ROWS}, {c[1] for c in L.CE_ROWS}
    assert any(r % 4 for r in Rs) and {1, 5, 16} <= Rs and {63, 64, 65, 130} <= Cs and {63, 64, 65} <= Rs
    assert all(off + R <= C for R, C, off in L.CE_ROWS) and any(off > 0 and off + R == C for R, C, off in L.CE_ROWS)
    assert any(off > 0 and off + R < C for R, C, off in L.CE_ROWS)
    assert {(4, 255), (4, 256), (4, 257), (2, 4096), (2, 4097)} <= set(L.SYMKL)
    assert any(H * H > 256 for _, H, _ in L.HEADATTN) and max(H * hd for _, H, hd in L.HEADATTN) == L.HA_MAX_D
    for _, H, hd in L.HEADATTN:
        assert H <= L.HA_MAX_H and H * hd <= L.HA_MAX_D
    assert L.ha_lds_bytes(64, 64, True) == 96 * 1024 and L.ha_lds_bytes(8, 512, True) > 64 * 1024 >= L.ha_lds_bytes(8, 512, False)


def _desc(B, D):
    d = _lib.LossTermsDesc()
    for name, ctype in d._fields_:
        if ctype is ctypes.c_void_p:
            setattr(d, name, 256)               # never read: the call must return before any launch
    d.B, d.D, d.has_align, d.Bc, d.P, d.n_rna, d.n_wstyle, d.n_rstyle, d.rows_wstyle, d.rows_rstyle = B, D, 1, 4, 8, 8, 8, 8, 4, 4
    return d


def test_the_fused_loss_refuses_past_the_edge_and_notes_none():
    lib = _lib.load()
    for entry in ("mh_loss_terms_fwd", "mh_loss_terms_bwd"):
        for B, D in ((32, 583), (33, 8), (0, 8)):
            lib.mh_note_form(b"")
            assert getattr(lib, entry)(ctypes.byref(_desc(B, D)), None) == -1, (entry, B, D)          # MH_EINVAL
            assert K.last_form() == entry[3:] + ":none"
            assert f"B={B} D={D}" in lib.mh_last_error().decode()
    d = _desc(32, 582)
    d.P = 0
    assert lib.mh_loss_terms_fwd(ctypes.byref(d), None) == -1 and K.last_form() == "loss_terms_fwd:none"


def test_headattn_refuses_the_same_shapes_in_both_directions():
    lib = _lib.load()
    for H, hd in ((0, 8), (65, 1), (64, 65), (8, 513), (1, 4097)):
        assert lib.mh_headattn_fwd(None, None, None, 0, H, hd, _lib.MH_F32, None) == -1, (H, hd)
        assert lib.mh_headattn_bwd(None, None, None, None, 0, H, hd, _lib.MH_F32, None) == -1, (H, hd)


# ------------------------------------------------------------------------------------------------ the tolerances have room
def _loss_excess(shape, vname, weights, combo, dtype=None, drop=None):
    """(max value excess, max gradient excess) of an f32 / tail-less evaluation against the f64 reference."""
    ref_l, ref_g = L.loss_reference(shape, vname, weights, combo)
    got_l, got_g = L.loss_reference(shape, vname, weights, combo, dtype or f64, drop)
    v = max(L.value_excess(a, b) for a, b in zip(got_l, ref_l))
    g = max(L.grad_excess(L.pad_like(got_g[i], ref_g[i]), ref_g[i]) for i in L.GRAD_IDX)
    return v, g


@pytest.mark.parametrize("vname", RANDOM_VARIANTS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_mirror_loss_f32_evaluation_has_margin(shape, vname):
    for weights, combo in ((L.W_DEFAULT, "total"), (L.W_DEFAULT, "single"), (L.W_ZEROS, "total")):
        if (weights, combo) != (L.W_DEFAULT, "total") and vname != RANDOM_VARIANTS[0]:
            continue
        v, g = _loss_excess(shape, vname, weights, combo, dtype=f32)
        print(f"{shape} {vname} {combo}: f32 oracle at {v:.4f} of the value tolerance, {g:.4f} of the gradient tolerance")
        assert MARGIN * v <= 1.0 and MARGIN * g <= 1.0, (v, g)


@pytest.mark.parametrize("vname", RANDOM_VARIANTS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_mirror_loss_would_notice_a_lost_tail(shape, vname):
    for drop in L.drops_of(shape):
        v, g = _loss_excess(shape, vname, L.W_DEFAULT, "total", drop=drop)
        assert max(v, g) > 10.0, f"{shape} {vname}: leaving out the last of {drop} moves nothing by more than 10 tolerances ({v:.2f}, {g:.2f})"


def _ce_excess(case, mname, per_row, **kw):
    ref, got = L.ce_reference(case, mname, per_row), L.ce_reference(case, mname, per_row, **kw)
    v = max(L.value_excess(got[k], ref[k]) for k in ("lse", "loss"))
    g = max(L.grad_excess(got[k], ref[k]) for k in ("dG", "dscale") if ref[k] is not None)
    return v, g


@pytest.mark.parametrize("mname", [m.name for m in L.CE_MODES])
@pytest.mark.parametrize("case", L.CE_ROWS, ids=_ids)
def test_ce_rows_margin_and_tail(case, mname):
    R, C, off = case
    for per_row in (False, True):
        v, g = _ce_excess(case, mname, per_row, dtype=f32)
        print(f"ce {case} {mname} per_row={per_row}: f32 at {v:.4f} / {g:.4f}")
        assert MARGIN * v <= 1.0 and MARGIN * g <= 1.0, (v, g)
        for drop, possible in (("C", C > 1), ("R", R > 1)):
            if possible:
                assert max(_ce_excess(case, mname, per_row, drop=drop)) > 10.0, (case, mname, per_row, drop)
    if C == 1:          # a single logit: the loss and both gradients are exactly 0
        ref = L.ce_reference(case, mname, False)
        assert float(ref["loss"].abs().max()) == 0.0 and float(ref["dG"].abs().max()) == 0.0
        assert ref["dscale"] is None or float(ref["dscale"]) == 0.0


@pytest.mark.parametrize("case", L.GATHERED, ids=_ids)
def test_gathered_term_margin_tail_and_restatement(case):
    B, world, rank, D = case
    ref_l, ref_g = L.gathered_reference(case)
    got_l, got_g = L.gathered_reference(case, f32)
    v, g = L.value_excess(got_l, ref_l), max(L.grad_excess(a, b) for a, b in zip(got_g, ref_g))
    print(f"gathered {case}: f32 at {v:.4f} / {g:.4f}")
    assert MARGIN * v <= 1.0 and MARGIN * g <= 1.0
    drop_l, drop_g = L.gathered_reference(case, f64, "C")
    assert max(L.value_excess(drop_l, ref_l), max(L.grad_excess(a, b) for a, b in zip(drop_g, ref_g))) > 10.0
    # the restatement is F.cross_entropy over the gathered logits with labels off + r
    w, r, s = (t.clone().requires_grad_(True) for t in L.gathered_inputs(case))
    off, lab = rank * B, rank * B + torch.arange(B)
    ce = 0.5 * (F.cross_entropy(s * w[off:off + B] @ r.T, lab) + F.cross_entropy(s * r[off:off + B] @ w.T, lab))
    ce.backward()
    assert abs(float(ce.detach() - ref_l)) < 1e-12
    for a, b in zip((w.grad, r.grad, s.grad), ref_g):
        assert float((a - b).abs().max()) < 1e-12
    # and the rank-local term of the oracle when there is one rank
    w1, r1 = L.gathered_inputs(case)[0][:B], L.gathered_inputs(case)[1][:B]
    assert abs(float(L.gathered_clip64(w1, r1, s.detach(), 0, B) - O.clip_loss(w1, r1, s.detach()))) < 1e-12


@pytest.mark.parametrize("case", L.INFONCE, ids=_ids)
def test_infonce_margin_and_tail(case):
    N, D, red, sym = case
    ref_l, ref_g = L.infonce_reference(case)
    got_l, got_g = L.infonce_reference(case, f32)
    v, g = L.value_excess(got_l, ref_l), max(L.grad_excess(a, b) for a, b in zip(got_g, ref_g))
    print(f"infonce {case}: f32 at {v:.4f} / {g:.4f}")
    if N == 1:          # a single logit: exact
        assert float(ref_l.abs().max()) == 0.0 and all(float(t.abs().max()) < 1e-15 for t in ref_g)
        return
    assert MARGIN * v <= 1.0 and MARGIN * g <= 1.0
    for drop in ("D", "B"):
        drop_l, drop_g = L.infonce_reference(case, f64, drop)
        pad = lambda t, like: L.pad_like(t, like)
        moved = max(L.value_excess(pad(drop_l, ref_l), ref_l), max(L.grad_excess(pad(a, b), b) for a, b in zip(drop_g, ref_g)))
        assert moved > 10.0, (case, drop, moved)


def _pair_excess(ref, got):
    return L.value_excess(got[0], ref[0]), max(L.grad_excess(a, b) for a, b in zip(got[1], ref[1]))


def test_flat_and_row_kernels_margin_and_tail():
    worst_v = worst_g = 0.0
    for n in L.FLAT_N:
        ref = L.kl_reference(n)
        v, g = _pair_excess(ref, L.kl_reference(n, f32))
        worst_v, worst_g = max(worst_v, v), max(worst_g, g)
        assert max(_pair_excess(ref, L.kl_reference(n, f64, "n"))) > 10.0, n
        x = L.clamp_inputs(n)
        assert bool((x < L.CLAMP_LO).any()) or n == 1
        if n >= 255:
            assert bool((x[-1] < L.CLAMP_LO) | (x[-1] > L.CLAMP_HI)) or bool(((x < L.CLAMP_LO) | (x > L.CLAMP_HI))[-64:].any())
    for case in L.SYMKL:
        for spread in L.SPREADS:
            ref = L.symkl_reference(case, spread)
            v, g = _pair_excess(ref, L.symkl_reference(case, spread, f32))
            worst_v, worst_g = max(worst_v, v), max(worst_g, g)
            if case[1] == 1:    # one prototype: exactly 0
                assert float(ref[0]) == 0.0 and all(float(t.abs().max()) == 0.0 for t in ref[1])
                continue
            for drop in ("P", "B") if case[0] > 1 else ("P",):
                assert max(_pair_excess(ref, L.symkl_reference(case, spread, f64, drop))) > 10.0, (case, spread, drop)
    for case in L.ROWNORM:
        ref = L.rownorm_reference(case)
        worst_v = max(worst_v, L.value_excess(L.rownorm_reference(case, f32), ref))
        z = L.zero_row(case)
        assert z is None or float(ref[z].abs().max()) == 0.0
        assert float(ref.abs().max()) > 0.0
        for drop in (("D",) if case[1] > 1 else ()) + (("B",) if case[0] > 1 else ()):
            assert L.value_excess(L.rownorm_reference(case, f64, drop), ref) > 10.0, (case, drop)
    for n in L.SMALL_N:
        for fn in (L.exp_reference, L.reparam_reference):
            ref, got, drop = fn(n), fn(n, f32), fn(n, f64, "n")
            worst_v = max(worst_v, L.value_excess(got[0], ref[0]))
            worst_g = max([worst_g] + [L.grad_excess(a, b) for a, b in zip(got[1:], ref[1:])])
            assert L.value_excess(drop[0], ref[0]) > 10.0 and all(L.grad_excess(a, b) > 10.0 for a, b in zip(drop[1:], ref[1:]))
    print(f"flat and row kernels: f32 at {worst_v:.4f} / {worst_g:.4f}")
    assert MARGIN * worst_v <= 1.0 and MARGIN * worst_g <= 1.0
    for n in range(1, 7):           # weighted_sum: exact by construction
        terms, weights, up = L.weighted_sum_inputs(n)
        acc = torch.zeros((), dtype=f32)
        for t, w in zip(terms, weights):
            acc = acc + torch.tensor(w, dtype=f32) * torch.tensor(t, dtype=f32)
        assert float(acc) == sum(t * w for t, w in zip(terms, weights))


@pytest.mark.parametrize("case", L.HEADATTN, ids=_ids)
def test_headattn_margin_tail_and_restatement(case):
    B, H, hd = case
    ref = L.headattn_reference(case, f32)
    got = L.headattn_reference(case, f32, f32)
    v = max(L.value_excess(got[0], ref[0]), L.value_excess(got[1], ref[1]))
    g = L.grad_excess(got[2], ref[2])
    print(f"headattn {case}: f32 at {v:.4f} / {g:.4f}")
    assert MARGIN * v <= 1.0 and MARGIN * g <= 1.0
    for drop, possible in (("D", hd > 1), ("H", H > 1)):
        if possible:
            d = L.headattn_reference(case, f32, f64, drop)
            assert max(L.value_excess(d[0], ref[0]), L.value_excess(d[1], ref[1]), L.grad_excess(d[2], ref[2])) > 10.0, (case, drop)
    # the bf16 inputs are bf16 numbers
    qkv, dout = L.headattn_inputs(case, torch.bfloat16)
    assert bool((qkv.bfloat16().double() == qkv).all()) and bool((dout.bfloat16().double() == dout).all())
    # the restatement is oracle.rna_attention between its two linears
    if H * hd <= 256:
        gen = torch.Generator().manual_seed(3)
        D = H * hd
        x = torch.randn(B, D, generator=gen, dtype=f64).requires_grad_(True)
        sd = {"a.qkv.weight": torch.randn(3 * D, D, generator=gen, dtype=f64), "a.proj.weight": torch.eye(D, dtype=f64)}
        up = torch.randn(B, D, generator=gen, dtype=f64)
        O.rna_attention(x, sd, "a", H).backward(up)
        x2 = x.detach().clone().requires_grad_(True)
        out, _ = L.headattn64(F.linear(x2, sd["a.qkv.weight"]), H)
        out.backward(up)
        assert float((out.detach() - O.rna_attention(x.detach(), sd, "a", H)).abs().max()) < 1e-12
        assert float((x2.grad - x.grad).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ the degenerate cases
def test_the_exact_case_is_exact_in_f64():
    for vname in RANDOM_VARIANTS:
        losses, grads = L.loss_reference(L.EXACT_SHAPE, vname)
        assert float(losses[1]) == 0.0 and float(losses[5]) == 0.0               # B = 1: alignment; P = 1: cluster
        for i in L.ALIGN_IDX + (4, 11):
            assert float(grads[i].abs().max()) == 0.0, i
        assert float(losses[2]) > 0.0 and float(losses[3]) > 0.0 and float(losses[4]) > 0.0


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_ids)
def test_the_saturated_case_has_no_alignment_gradient_in_f64(shape):
    losses, grads = L.loss_reference(shape, "sat")
    assert all(bool(torch.isfinite(t).all()) for t in losses)
    assert 0.0 <= float(losses[1]) < 1e-12
    for i in L.ALIGN_IDX:
        assert float(grads[i].abs().max()) < 1e-12, (shape, i, float(grads[i].abs().max()))
    w, r = L.loss_inputs(shape, "sat")[0], L.loss_inputs(shape, "sat")[7]
    assert float((w * r).sum(-1).min()) > 0.999 and not torch.equal(w, r)


def test_the_zero_weights_zero_their_gradients():
    for shape in L.LOSS_TERMS:
        _, grads = L.loss_reference(shape, RANDOM_VARIANTS[0], L.W_ZEROS, "total")
        for i in L.ALIGN_IDX + (8, 9):                  # alignment and RNA retention carry weight 0
            assert float(grads[i].abs().max()) == 0.0
        assert float(grads[1].abs().max()) > 0.0 and float(grads[4].abs().max()) > 0.0 or shape[5] == 1


def test_inputs_are_f32_numbers_and_seeded():
    for shape in (L.LOSS_TERMS[1], L.LOSS_TERMS[3]):
        a = L.loss_inputs(shape, "s100-sp12")
        assert all(bool((t.float().double() == t).all()) for t in a)
        L.loss_inputs.cache_clear()
        b = L.loss_inputs(shape, "s100-sp12")
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert math.isclose(float(L.loss_inputs(L.LOSS_TERMS[1], "s14.3-sp1")[14]), 14.3, rel_tol=1e-7)
    assert float(L.loss_inputs(L.LOSS_TERMS[1], "ones")[10].min()) == 1.0 and float(L.loss_inputs(L.LOSS_TERMS[1], "s14.3-sp1")[10].min()) == 0.0
