"""Without a device: the preconditions of tests/test_seq_forms_gpu.py.  The table of tests/seq_form_cases.py only tests every launch form
of PPEG, res_conv and the landmark kernels while it holds a case for every form and dtype instance the host can select, and its exact /
toleranced comparisons only mean something while the data has the properties they rest on — both are pinned here."""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mirror_amd import _lib
from mirror_amd import kernels as K
from tests import seq_form_cases as Q

f32, bf16, f64 = torch.float32, torch.bfloat16, torch.float64
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")

# Every form an entry point of the two sources can note (":none" = it returned before any launch, or refused the call), written out
FORMS = {
    "ppeg_fwd": ["none", "pair", "strip"],
    "ppeg_wgrad": ["none", "strip"],
    "ppeg_bwd": ["none", "one", "one,drop"],
    "resconv_fwd": ["none", "mfma", "vec", "scalar"],
    "resconv_wgrad": ["none", "mfma", "vec8", "scalar"],
    "resconv_bwd": ["none", "mfma", "two_pass"],
    "landmark_fwd": ["none", "quad", "scalar"],
    "landmark_bwd": ["none", "oct", "scalar"],
}
PAIRS = ["ff", "fb", "bf", "bb"]
# (entry, form, dtype instance) the table reaches: every instantiation of ppeg_strip_kernel, ppeg_wgrad_strip_kernel, resconv_vec_kernel,
# resconv_kernel, resconv_wgrad_kernel (vec8 on and off) and of the four landmark kernels; the two-pass backward with equal and mixed
# dtypes.  The MFMA res_conv kernels and the one-pass mh_ppeg_bwd keep the tests they have.
REACHED = (
    [("ppeg_fwd", "ppeg_fwd:strip", p) for p in PAIRS] + [("ppeg_fwd", "ppeg_fwd:pair", "ff")]
    + [("ppeg_wgrad", "ppeg_wgrad:strip", p) for p in PAIRS]
    + [("resconv_fwd", f"resconv_fwd:{f}", p) for f in ("vec", "scalar") for p in PAIRS]
    + [("resconv_wgrad", f"resconv_wgrad:{f}", p) for f in ("vec8", "scalar") for p in PAIRS]
    + [("resconv_bwd", "resconv_bwd:two_pass", p) for p in ("ff", "bf", "bb")]
    + [(e, f"{e}:{f}", t) for e, forms in (("landmark_fwd", ("quad", "scalar")), ("landmark_bwd", ("oct", "scalar"))) for f in forms for t in "fb"]
    + [(e, "", t) for e in ("seq_finish", "seq_finish_bwd") for t in "fb"]
)
RANDOM = [c for c in Q.CASES if c.kind == "random"]
INTEGER = [c for c in Q.CASES if c.kind == "integer"]


def _noted_in_the_sources():
    """entry -> forms, from the mh_note_form("...") literals of the two sources (a `cond ? "a" : "b"` argument holds two)."""
    noted = collections.defaultdict(set)
    for name in ("ppeg.hip", "nystrom_aux.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            for call in re.findall(r"mh_note_form\(([^;]*)\);", fh.read()):
                for entry, form in re.findall(r'"(\w+):([\w,]+)"', call):
                    noted[entry].add(form)
    return noted


def test_the_written_out_forms_are_the_ones_the_library_notes():
    noted = _noted_in_the_sources()
    assert set(noted) == set(FORMS)
    for entry, forms in FORMS.items():
        assert noted[entry] == set(forms), entry


def test_the_table_reaches_exactly_the_listed_instances():
    have = {(c.entry, c.form, Q._dn(c.dtypes)) for c in Q.CASES}
    assert have == set(REACHED), have ^ set(REACHED)
    for entry, form, _ in REACHED:
        if form:
            assert form.split(":")[1] in FORMS[entry]
    # both kinds of data in every form (seq_finish: integer data only), and in every instance of the forms with four
    for entry, form, inst in REACHED:
        kinds = {c.kind for c in Q.CASES if (c.entry, c.form, Q._dn(c.dtypes)) == (entry, form, inst)}
        assert kinds == ({"integer"} if not form else {"integer", "random"}), (entry, form, inst, kinds)


@pytest.mark.parametrize("c", Q.CASES, ids=str)
def test_the_host_rule_predicts_the_form(c):
    """A pure-Python restatement of each entry point's rule, fed with the case's sizes, dtypes and placement, names the form the case claims."""
    assert Q.predicted_form(c) == c.form


def test_the_host_rules_at_their_edges():
    al = (8, 8, 8, 8), (0, 0)
    assert Q.resconv_fwd_form(8, 64, 33, bf16, bf16, *al) == "resconv_fwd:mfma"
    assert Q.resconv_fwd_form(8, 64, 31, bf16, bf16, *al) == "resconv_fwd:vec"
    assert Q.resconv_fwd_form(8, 64, 33, bf16, bf16, al[0], (8, 0)) == "resconv_fwd:scalar"
    assert Q.resconv_fwd_form(8, 64, 33, bf16, f32, *al) == "resconv_fwd:vec"
    assert Q.resconv_fwd_form(12, 96, 33, f32, f32, *al) == "resconv_fwd:vec" and 511 // 96 + 2 == 7
    assert Q.resconv_fwd_form(12, 64, 33, f32, f32, *al) == "resconv_fwd:scalar" and 511 // 64 + 2 == 9 and 255 // 64 + 2 == 5
    assert Q.resconv_fwd_form(16, 16, 33, f32, f32, *al) == "resconv_fwd:none" and 255 // 16 + 2 == 17
    assert Q.resconv_fwd_form(8, 96, 33, f32, f32, (2304, 40 * 2304, 2304, 40 * 2304), (2 * 768 * 4, 2 * 768 * 4)) == "resconv_fwd:vec"
    assert Q.ppeg_fwd_form(6, f32, f32, 0, 0) == "ppeg_fwd:pair" and Q.ppeg_fwd_form(6, f32, f32, 4, 0) == "ppeg_fwd:strip"
    assert Q.ppeg_fwd_form(7, f32, f32, 0, 0) == "ppeg_fwd:strip" and Q.ppeg_fwd_form(6, bf16, f32, 0, 0) == "ppeg_fwd:strip"
    assert Q.landmark_fwd_form(4, bf16, 8, 0) == "landmark_fwd:quad" and Q.landmark_fwd_form(4, f32, 8, 0) == "landmark_fwd:scalar"
    assert Q.landmark_bwd_form(8, f32, 0, 0) == "landmark_bwd:oct" and Q.landmark_bwd_form(4, f32, 0, 0) == "landmark_bwd:scalar"
    assert Q.place_offset_bytes("o4", f32) % 16 == 0 and Q.place_offset_bytes("o4", bf16) % 16 == 8       # why the shifted views are bf16
    for C in (8, 768):
        assert Q.place_offset_bytes("blk", f32, C) % 16 == 0 and Q.place_offset_bytes("blk", bf16, C) % 16 == 0


def _sel(entry, form=None, **kw):
    return [c for c in Q.CASES if c.entry == entry and (form is None or c.form == f"{entry}:{form}")
            and all(getattr(c, k) == v for k, v in kw.items())]


def test_the_sizes_and_seams_the_table_claims():
    strip = _sel("ppeg_fwd", "strip")
    for dts in Q.PAIRS:                 # every S, both flips, in every instance of the strip kernel
        assert {(c.sizes[1], c.opt[0]) for c in strip if c.dtypes == dts and c.sizes[2] == 33} == {(S, fl) for S in Q.PPEG_STRIP_S for fl in (0, 1)}
        assert {c.sizes[2] for c in strip if c.dtypes == dts} >= {33, 257}
    assert {c.sizes[2] for c in strip if c.dtypes == (f32, f32) and not c.place} == set(Q.PPEG_STRIP_D)
    assert {(c.sizes[1], c.sizes[2]) for c in strip if not c.place} >= {(S, D) for S in Q.PPEG_STRIP_S for D in Q.PPEG_STRIP_D}
    assert Q.PX_T - 1 in Q.PPEG_STRIP_S and Q.PX_T in Q.PPEG_STRIP_S and Q.PX_T + 1 in Q.PPEG_STRIP_S        # one short of, equal to, one past PX_T
    assert {Q.PY_T, Q.PY_T + 1, Q.PY_T + 7} <= set(Q.PPEG_STRIP_S) and 257 == 256 + 1                          # a second strip of 1 and of 7 rows
    pair = _sel("ppeg_fwd", "pair")
    assert {(c.sizes[1], c.sizes[2], c.opt[0]) for c in pair} == {(S, D, fl) for S in Q.PPEG_PAIR_S for D in Q.PPEG_PAIR_D for fl in (0, 1)}
    for c in pair:                      # the seam: the same inputs aligned (pair) and one element into a buffer (strip)
        if c.sizes[2] == 6:
            twin = Q.by_id(str(c) + "-oa")
            assert twin.form == "ppeg_fwd:strip" and twin.dtypes == (f32, f32)
            a, b = Q.build(c), Q.build(twin)
            assert all(torch.equal(a.inputs[k], b.inputs[k]) for k in a.inputs) and torch.equal(a.want["y"], b.want["y"])
    wg = _sel("ppeg_wgrad")
    for dts in Q.PAIRS:
        assert {(c.sizes[1], c.sizes[2]) for c in wg if c.dtypes == dts and not c.place} == \
            {(S, D) for S in Q.PPEG_WGRAD_S for D in Q.PPEG_WGRAD_D} | {(65, 8)}
    assert all(c.sizes[0] == (1 if c.sizes[1] == 65 else 2) for c in wg)
    assert [-(-S // 4) for S in Q.PPEG_WGRAD_S] == [1, 1, 2, 3] and -(-65 // -(-65 // 64)) == 33     # strips per image, of a workgroup's 4; 33 + 32 rows
    # res_conv: the geometries of the lists
    vec, sca = _sel("resconv_fwd", "vec"), _sel("resconv_fwd", "scalar")
    assert {c.sizes[3] for c in vec} == {8, 24, 64, 96} and {c.sizes[3] for c in sca} == {4, 8, 12, 64}
    assert {(c.sizes[2], c.sizes[3]) for c in vec} >= {(8, 96), (12, 96)} and (12, 64) in {(c.sizes[2], c.sizes[3]) for c in sca}
    assert {c.sizes[4] for c in vec} == {1, 3, 31, 33, 63} and {c.sizes[4] for c in sca} == {1, 3, 33, 63}
    assert {c.sizes[1] for c in vec} == {1, 16, 17, 33, 40} and 16 < 33 // 2 + 1
    for form, cs in (("vec", vec), ("scalar", sca)):
        for dts in Q.PAIRS:
            assert {c.opt for c in cs if c.dtypes == dts} >= {(0, 0), (0, 1), (1, 0), (1, 1)}, (form, dts)
    assert {c.dtypes for c in vec if c.place == ("blk", "blk") and c.sizes[2:4] == (8, 96)} == set(Q.PAIRS) and (512 % 96, 512 // 96) == (32, 5)
    assert any(c.dtypes == (bf16, bf16) and c.sizes[3:] == (64, 31) and not c.place for c in vec)
    assert any(c.dtypes == (bf16, bf16) and c.sizes[3:] == (64, 33) and c.place == ("o4", "a") for c in sca)
    assert any(c.sizes[3] == 8 and c.place == ("o4", "a") and c.dtypes == (bf16, bf16) for c in sca)
    w8, ws = _sel("resconv_wgrad", "vec8"), _sel("resconv_wgrad", "scalar")
    assert {c.sizes[3] for c in w8 + ws} == {4, 64, 72, 96, 136} and {c.sizes[3] for c in w8} == {64, 72, 96, 136}
    assert {c.sizes[1] for c in w8 + ws} == {1, 33, 63, 64, 65, 100} and {c.sizes[4] for c in w8 + ws} == {1, 33, 63}
    assert max(c.sizes[1] * c.sizes[2] * c.sizes[3] for c in Q.CASES if c.entry.startswith("resconv")) == 100 * 1152
    bw = _sel("resconv_bwd", "two_pass")
    assert {(c.dtypes, c.sizes[3]) for c in bw} >= {((f32, f32), 8), ((bf16, f32), 8), ((bf16, bf16), 96)}
    assert any(c.place == ("a", "blk", "blk") for c in bw)
    for entry in ("landmark_fwd", "landmark_bwd"):
        cs = _sel(entry)
        for t in (f32, bf16):
            assert {(c.sizes[2], c.sizes[3]) for c in cs if c.dtypes == (t,) and not c.place} == {(l, D) for l in Q.LM_L for D in Q.LM_D}
            assert {c.sizes[1] for c in cs if c.dtypes == (t,)} == set(Q.LM_M)
            assert any(c.place == ("o", "a") and c.sizes[3] == 8 and c.form.endswith("scalar") for c in cs if c.dtypes == (t,))
        assert all(c.sizes[2] in (1, 2, 4) for c in cs if c.kind == "integer")
    for entry in ("seq_finish", "seq_finish_bwd"):
        assert {(c.sizes[1:], c.dtypes[0]) for c in _sel(entry)} == {((N, a, D), t) for N, a in Q.SEQ_NADD for D in Q.SEQ_D for t in (f32, bf16)}
    assert all(c.sizes[0] == 2 for c in Q.CASES if c.sizes[1:] != (65, 8))


@pytest.mark.parametrize("c", INTEGER, ids=str)
def test_integer_cases_are_exact_by_construction(c):
    b = Q.build(c)
    assert not b.tol and not b.wrong and 0 < b.f32_sum_bound < 2 ** 24
    for name, dtype in Q.out_dtypes(c).items():
        want = b.want[name]
        assert want.dtype == f64 and bool(torch.isfinite(want).all())
        assert bool((want.to(dtype).double() == want).all()), f"{c}: {name} holds a value that is no {dtype} number"
        assert float(want.abs().max()) <= b.f32_sum_bound
    for name, t in list(b.inputs.items()) + list(b.prefill.items()):
        assert bool((t == t.round()).all()), (str(c), name)
    if c.entry in ("landmark_fwd", "landmark_bwd"):
        assert c.sizes[2] & (c.sizes[2] - 1) == 0


@pytest.mark.parametrize("c", RANDOM, ids=str)
def test_random_cases_would_notice_the_bugs_their_form_invites(c):
    """Every bound is finite and non-negative, the operands are numbers of their storage dtype, and EVERY wrong reference the case
    carries is more than 10 tolerances from the true one somewhere."""
    b = Q.build(c)
    assert set(b.tol) == set(b.want) == set(Q.out_dtypes(c)) and b.wrong
    for name, want in b.want.items():
        tol = b.tol[name]
        assert want.shape == tol.shape and bool(torch.isfinite(want).all()) and bool(torch.isfinite(tol).all()) and bool((tol >= 0).all())
        assert float(want.abs().max()) > 0.0, (str(c), name)
    for key, dtype in zip({"ppeg_fwd": ("x",), "ppeg_wgrad": ("x", "dout"), "resconv_fwd": ("v",), "resconv_wgrad": ("v", "dout"),
                           "resconv_bwd": ("v", "dout"), "landmark_fwd": ("qkv",), "landmark_bwd": ("dlm",)}[c.entry], c.dtypes):
        assert torch.equal(Q.stored(b.inputs[key], dtype), b.inputs[key]), (str(c), key)
    for bug, ref in b.wrong.items():
        assert set(ref) == set(b.want)
        moved = 0.0
        for name, want in b.want.items():
            diff = (want - ref[name]).abs()
            far = diff > 10 * b.tol[name]
            if bool(far.any()):
                moved = max(moved, float((diff / b.tol[name].clamp_min(1e-300))[far].max()))
        assert moved > 10.0, f"{c}: the wrong reference '{bug}' is within 10 tolerances of the true one everywhere"


def test_the_wrong_references_are_the_listed_ones():
    names = collections.defaultdict(set)
    for c in RANDOM:
        names[c.form].update(Q.build(c).wrong)
    assert names["ppeg_fwd:strip"] >= {"ring", "clamp"} and names["ppeg_fwd:pair"] >= {"ring", "clamp"}
    assert names["ppeg_wgrad:strip"] == {"last_row"}
    assert names["resconv_fwd:vec"] >= {"shift", "last_tap", "mid_head"} and names["resconv_fwd:scalar"] >= {"shift", "last_tap"}
    assert names["resconv_wgrad:vec8"] == {"last_row", "cols_from_64"} and names["resconv_wgrad:scalar"] >= {"last_row"}
    assert names["resconv_bwd:two_pass"] >= {"shift", "last_tap", "mid_head", "last_row", "cols_from_64"}
    for form in ("landmark_fwd:quad", "landmark_fwd:scalar", "landmark_bwd:oct", "landmark_bwd:scalar"):
        assert names[form] == {"last_row"}
    # the template's block: heads 5's columns 32 .. 95 open the second 512-column block, and the wrong reference moves exactly those
    c = next(c for c in RANDOM if c.entry == "resconv_fwd" and c.sizes[2:4] == (8, 96))
    b = Q.build(c)
    moved = ((b.want["out"] - b.wrong["mid_head"]["out"]).abs() > 0).any(0).any(0).nonzero().reshape(-1)
    assert int(moved.min()) == 512 and int(moved.max()) == 575


def test_the_tolerances_are_the_stated_ones():
    c = next(x for x in RANDOM if x.entry == "resconv_fwd" and x.dtypes == (f32, f32) and x.opt[1] == 1 and x.sizes[4] == 3 and not x.place)
    b = Q.build(c)
    v, w, pre = b.inputs["v"].double(), b.inputs["w"].double(), b.prefill["out"].double()
    B, n_p, heads, dh, taps = c.sizes
    t, col = 5, 2 * dh - 1
    mag = sum(abs(w[col // dh, taps - 1 - j if c.opt[0] else j]) * abs(v[1, t + j - taps // 2, col]) for j in range(taps))
    assert abs(float(b.tol["out"][1, t, col]) - ((taps + 2) * 2.0 ** -23 * float(mag) + 2.0 ** -23 * abs(float(pre[1, t, col])))) < 1e-15
    c = next(x for x in RANDOM if x.entry == "landmark_fwd" and x.dtypes == (bf16,) and x.sizes[2] == 6)
    b = Q.build(c)
    x, want = b.inputs["qkv"].double(), b.want["lm"]
    stated = 8 * 2.0 ** -23 * x[0, :6, 0].abs().sum() / 6 + (2.0 ** -8 + 2.0 ** -22) * want[0, 0, 0].abs()
    assert abs(float(b.tol["lm"][0, 0, 0] - stated)) < 1e-15
    c = next(x for x in RANDOM if x.entry == "ppeg_wgrad" and x.sizes[1:] == (9, 33) and not x.place)
    b = Q.build(c)
    g = b.inputs["dout"].double()[:, 1:, 4].abs().sum()            # the bias gradient: every term of the sum a product with 1
    assert abs(float(b.tol["dbsum"][4]) - ((2 * 81 + 2) * 2.0 ** -23 * float(g) + 2.0 ** -23 * abs(float(b.prefill["dbsum"][4])))) < 1e-12


def test_the_references_agree_with_each_other_and_with_f64_torch():
    """Forward against conv2d / conv1d in f64 (forward only); the adjoint and the weight-gradient references against f64 autograd THROUGH
    the forward reference, which is plain differentiable torch."""
    gen = torch.Generator().manual_seed(11)
    for S, D in ((1, 3), (4, 2), (9, 5)):
        B = 2
        x = torch.randn(B, 1 + S * S, D, generator=gen, dtype=f64).requires_grad_(True)
        m = torch.randn(49, D, generator=gen, dtype=f64).requires_grad_(True)
        bs = torch.randn(D, generator=gen, dtype=f64).requires_grad_(True)
        y = Q.ppeg64(x, m, bs, S, 0)
        img = x.detach()[:, 1:].reshape(B, S, S, D).permute(0, 3, 1, 2)
        ref = F.conv2d(img, m.detach().t().reshape(D, 1, 7, 7), bs.detach(), padding=3, groups=D).permute(0, 2, 3, 1).reshape(B, S * S, D)
        assert float((y.detach()[:, 1:] - ref).abs().max()) < 1e-12 and torch.equal(y.detach()[:, 0], x.detach()[:, 0])
        dy = torch.randn(B, 1 + S * S, D, generator=gen, dtype=f64)
        y.backward(dy)
        assert float((Q.ppeg64(dy, m.detach(), bs.detach(), S, 1) - x.grad).abs().max()) < 1e-12          # flip: the adjoint, no bias
        dm, dbs = Q.ppeg_wgrad64(x.detach(), dy, S)
        assert float((dm - m.grad).abs().max()) < 1e-12 and float((dbs - bs.grad).abs().max()) < 1e-12
    for n_p, heads, dh, taps in ((1, 1, 2, 1), (7, 2, 3, 5), (40, 3, 4, 33), (16, 2, 2, 63)):
        B, C = 2, heads * dh
        v = torch.randn(B, n_p, C, generator=gen, dtype=f64).requires_grad_(True)
        w = torch.randn(heads, taps, generator=gen, dtype=f64).requires_grad_(True)
        out = Q.resconv64(v, w, heads, 0)
        ref = F.conv1d(v.detach().transpose(1, 2), w.detach().repeat_interleave(dh, 0).unsqueeze(1), padding=taps // 2, groups=C).transpose(1, 2)
        assert float((out.detach() - ref).abs().max()) < 1e-12
        g = torch.randn(B, n_p, C, generator=gen, dtype=f64)
        out.backward(g)
        assert float((Q.resconv64(g, w.detach(), heads, 1) - v.grad).abs().max()) < 1e-12
        assert float((Q.resconv_wgrad64(v.detach(), g, heads, taps) - w.grad).abs().max()) < 1e-12
    for l, m_, D in ((1, 2, 3), (6, 5, 4), (9, 1, 8)):
        qkv = torch.randn(2, m_ * l, 3 * D, generator=gen, dtype=f64).requires_grad_(True)
        lm = Q.landmark64(qkv, l)
        assert float((lm.detach() - qkv.detach()[:, :, :2 * D].reshape(2, m_, l, 2 * D).mean(2)).abs().max()) < 1e-14
        g = torch.randn(2, m_, 2 * D, generator=gen, dtype=f64)
        lm.backward(g)
        pre = torch.randn(2, m_ * l, 3 * D, generator=gen, dtype=f64)
        assert float((Q.landmark_bwd64(g, pre, l) - (pre + qkv.grad)).abs().max()) < 1e-14 and float(qkv.grad[:, :, 2 * D:].abs().max()) == 0.0


def test_returns_before_a_launch_note_none():
    """A call that returns before any launch, or is refused, notes "<entry>:none": reached here with calls that touch no device."""
    lib = _lib.load()
    calls = {
        "ppeg_fwd": lambda: lib.mh_ppeg_fwd(None, None, None, None, 0, 3, 8, 0, _lib.MH_F32, _lib.MH_BF16, None),
        "ppeg_wgrad": lambda: lib.mh_ppeg_wgrad(None, None, None, None, 0, 3, 8, 0, 0, None),
        "resconv_fwd": lambda: lib.mh_resconv_fwd(None, 8, 8, None, None, 8, 8, 0, 4, 1, 8, 3, 0, 0, 0, 0, None),
        "resconv_wgrad": lambda: lib.mh_resconv_wgrad(None, 8, 8, None, 8, 8, None, 0, 4, 1, 8, 3, 0, 0, None),
        "landmark_fwd": lambda: lib.mh_landmark_fwd(None, None, 0, 6, 8, 3, 0, None),
        "landmark_bwd": lambda: lib.mh_landmark_bwd(None, None, 0, 6, 8, 3, 0, None),
    }
    for entry, call in calls.items():
        assert lib.mh_cast(None, None, 0, 0, 0, None) == 0 and K.last_form() == "cast:none"
        assert call() == 0, entry
        assert K.last_form() == f"{entry}:none", entry
    one = 1                         # a non-null pointer no refused call may follow
    bad = max(_lib.MH_F32, _lib.MH_BF16) + 5
    refused = {
        "ppeg_fwd": (lambda: lib.mh_ppeg_fwd(None, None, None, None, 1, 3, 8, 0, bad, _lib.MH_F32, None), "dtype"),
        "ppeg_wgrad": (lambda: lib.mh_ppeg_wgrad(None, None, None, None, 1, 3, 8, _lib.MH_BF16, bad, None), "dtype"),
        "ppeg_bwd": (lambda: lib.mh_ppeg_bwd(None, None, None, None, None, None, 1, 3, 8, None, None, 0.0, 0, 0, None, None), "null"),
        "resconv_fwd": (lambda: lib.mh_resconv_fwd(None, 8, 8, None, None, 8, 8, 1, 4, 1, 8, 3, 0, 0, _lib.MH_F32, bad, None), "dtype"),
        "resconv_wgrad": (lambda: lib.mh_resconv_wgrad(None, 8, 8, None, 8, 8, None, 1, 4, 1, 8, 3, bad, _lib.MH_F32, None), "dtype"),
        "resconv_bwd": (lambda: lib.mh_resconv_bwd(one, 8, 8, one, 8, 8, one, one, 8, 8, one, None, 0, 1, 4, 16, 16, 3, 0, 0, None), "more than 8 heads"),
        "landmark_fwd": (lambda: lib.mh_landmark_fwd(None, None, 1, 7, 8, 3, 0, None), "multiple"),
        "landmark_bwd": (lambda: lib.mh_landmark_bwd(None, None, 1, 7, 8, 3, 0, None), "multiple"),
    }
    assert set(refused) == set(FORMS)
    for entry, (call, word) in refused.items():
        assert lib.mh_cast(None, None, 0, 0, 0, None) == 0 and K.last_form() == "cast:none"
        assert call() != 0, entry
        assert K.last_form() == f"{entry}:none", entry
        assert word in lib.mh_last_error().decode(), (entry, lib.mh_last_error().decode())
    assert lib.mh_resconv_fwd(None, 8, 8, None, None, 8, 8, 1, 4, 16, 16, 3, 0, 0, 0, 0, None) != 0 and K.last_form() == "resconv_fwd:none"


def test_the_wrappers_take_an_output_of_the_callers(monkeypatch):
    """kernels.ppeg / kernels.landmark_fwd write into `out` when given one (the guarded windows of the GPU test) and refuse one that does not fit."""
    monkeypatch.setattr(K, "_chk", lambda *ts: None)
    monkeypatch.setattr(K, "_stream", lambda: 0)
    seen = []
    monkeypatch.setattr(K._lib, "call", lambda name, *a, **k: seen.append((name, a)))
    x, m, bs = torch.zeros(2, 5, 6), torch.zeros(49, 6), torch.zeros(6)
    out = torch.zeros(2, 5, 6, dtype=bf16)
    assert K.ppeg(x, m, bs, 2, False, out_dtype=bf16, out=out) is out and seen[-1][1][1] == out.data_ptr()
    assert K.ppeg(x, m, bs, 2, False).dtype == f32 and K.ppeg(x, m, bs, 2, False, out_dtype=bf16).dtype == bf16
    for wrong in (torch.zeros(2, 5, 7), torch.zeros(2, 6, 5).transpose(1, 2)):
        with pytest.raises(K.MirrorHipError, match="out"):
            K.ppeg(x, m, bs, 2, False, out=wrong)
    with pytest.raises(K.MirrorHipError, match="out"):
        K.ppeg(x, m, bs, 2, False, out_dtype=bf16, out=torch.zeros(2, 5, 6))
    qkv, lm = torch.zeros(2, 6, 12), torch.zeros(2, 2, 8)
    assert K.landmark_fwd(qkv, 3, out=lm) is lm and seen[-1][1][1] == lm.data_ptr()
    assert tuple(K.landmark_fwd(qkv, 3).shape) == (2, 2, 8)
    for wrong in (torch.zeros(2, 2, 9), torch.zeros(2, 2, 8, dtype=bf16)):
        with pytest.raises(K.MirrorHipError, match="out"):
            K.landmark_fwd(qkv, 3, out=wrong)
