"""GPU: the K % BK remainder of mh_gemm on every route it takes (tests/gemm_ragged_cases.py), against f64.

The remainder of a weight gradient is one row in 4097 per slide: dropped, read from the wrong batch or row, or scaled by the wrong
alpha it moves dW by ~2e-4 relative, below every whole-model tolerance of this suite.  Here it is a visible part of an exact result."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from mirror_amd import MirrorHipError, _lib  # noqa: E402
from mirror_amd import functional as Fn  # noqa: E402
from mirror_amd import kernels as K  # noqa: E402
from mirror_amd._lib import ACT_GELU, MH_BF16  # noqa: E402
from tests import gemm_ragged_cases as G  # noqa: E402

DEV = "cuda"
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64


def variant() -> str:
    return _lib.load().mh_gemm_variant_name().decode()


def exact(got, want, msg):
    got, want = got.detach().float().cpu().double().reshape(want.shape), want.double()
    bad = got != want
    assert not bad.any(), (f"{msg}: {int(bad.sum())}/{bad.numel()} elements differ from the f64 product, max |diff| "
                           f"{float((got - want).abs().max())}, first at {tuple(int(i) for i in bad.nonzero()[0])}")


def run(c, data, monkeypatch):
    """One K.gemm of the case; (result window, padded buffer, variant name)."""
    monkeypatch.setattr(K, "SPLITK_PARTIALS", c.partials)
    A, B, out, full, bias = G.device_operands(c, data, DEV)
    K.gemm(A, B, out=out, alpha=c.alpha, diag=c.diag, bias=bias, accumulate=c.accumulate, split_k=c.split_k, mma=c.mma)
    return full[:, :c.M, :c.N], full, variant()


def check_route(c, name):
    """mh_gemm_variant_name after the call.  rank_update_kernel and the fold are no tiled instances and leave the main launch's name;
    a second tiled launch names itself last."""
    if c.route in ("fold4", "fold1"):
        assert ",part" in name, (c.id, name)
    elif c.id == "RA":
        assert ",part" not in name and name.startswith("gemm_pp_kernel<float,"), (c.id, name)
    elif c.route == "rank":
        assert name.startswith("gemm_kernel<"), (c.id, name)
    else:       # "tiled", and FBX ("fold_notail": its fold is pinned by the workspace the CPU test asserts — without the fold pass the
        #         partial tiles would never reach C): the guarded 128 x 128 instance, FULL = 0
        assert c.route in ("tiled", "fold_notail")
        assert name.startswith("gemm_kernel<") and name.endswith(",0>"), (c.id, name)


@pytest.mark.parametrize("c", G.CASES, ids=str)
def test_ragged_k_remainder_is_exact_on_every_route(c, monkeypatch):
    data = G.integer_case(c)
    if c.id == "NP":        # the main part alone is a persistent-kernel product (in the full call the remainder's launch names itself last)
        main = G.Case("NP-main", c.M, c.N, c.kmain, 0, 1, 1, "none", layout=c.layout)
        md = G.Data(data.at[:, :c.kmain], data.b[:, :c.kmain], data.filler, data.prefill, data.bias, None)
        _, _, name = run(main, md, monkeypatch)
        assert name.startswith("gemm_pq_kernel<float,"), name
    got, full, name = run(c, data, monkeypatch)
    print(f"{c.id}: {name}")
    check_route(c, name)
    exact(got, data.want, c.id)
    assert G.pad_untouched(c, full), f"{c.id}: rows / columns past M, N of the padded C were written"


@pytest.mark.parametrize("c", G.RANDOM_CASES, ids=str)
def test_fold_with_tail_on_random_bf16_data_against_f64(c, monkeypatch):
    """The fold rows with rounding (bf16 partial tiles) on randn data whose tail rows are scaled by 8: tolerance and the
    tail-visibility condition are gemm_ragged_cases.random_case's, both from f64 values on the CPU.  On an MI355X the worst
    error / tolerance over the elements was 0.05 (FBL) to 0.36 (F1, t = 16)."""
    r = G.random_case(c)
    assert G.tail_visible_fraction(r) >= G.TAIL_VISIBLE_FRACTION       # (tests/test_gemm_ragged_k_cpu.py prints the figure)
    got, full, name = run(c, r, monkeypatch)
    assert ",part" in name, (c.id, name)
    err = (got.cpu().double() - r.want).abs()
    worst = float((err / r.tol).max())
    print(f"{c.id}: max err {float(err.max()):.3e}, worst err / tol {worst:.3f}, {name}")
    bad = err > r.tol
    assert not bad.any(), f"{c.id}: {int(bad.sum())}/{bad.numel()} elements off, worst err / tol {worst:.3f}"
    assert G.pad_untouched(c, full)


def test_no_tail_outlives_its_call(monkeypatch):
    """The offered tail is an argument of its own call (csrc/gemm.hip: mh_gemm hands a GemmTail on its stack down to launch_fold), not
    state that a later call could meet.  If one outlived a call whose main launch did not fold, one whose fold took it, or a refused
    call, it would be added silently to the next folded product."""
    ra, f4 = G.by_id("RA"), G.by_id("F4-t16-a1.0")
    plain = G.Case("F4-t0", f4.M, f4.N, f4.kmain, 0, f4.split_k, 1, "fold", alpha=1.0)
    pd = G.integer_case(f4, seed=7)
    plain_data = G.Data(pd.at[:, :f4.kmain], pd.b[:, :f4.kmain], pd.filler, pd.prefill, pd.bias,
                        G._product(plain, pd.at[:, :f4.kmain], pd.b[:, :f4.kmain], pd.prefill, pd.bias))
    G.assert_partials_are_bf16_numbers(plain_data.at, plain_data.b, plain.kmain, plain.split_k, 1.0, "F4 without a tail")

    def b_step(after):
        got, full, name = run(plain, plain_data, monkeypatch)
        assert ",part" in name, name
        exact(got, plain_data.want, f"K = {plain.kmain} folded product after {after}")
        assert G.pad_untouched(plain, full)

    got, _, name = run(ra, G.integer_case(ra), monkeypatch)               # a: offered, not folded
    assert ",part" not in name
    exact(got, G.integer_case(ra).want, "RA")
    b_step("a tail that the main launch did not fold")
    got, _, name = run(f4, G.integer_case(f4), monkeypatch)               # c: offered and taken
    assert ",part" in name
    exact(got, G.integer_case(f4).want, f4.id)
    b_step("a tail that the fold took")
    monkeypatch.setattr(K, "SPLITK_PARTIALS", "bf16")                      # d: refused before any launch
    A, B, out, full, _ = G.device_operands(f4, G.integer_case(f4), DEV)
    with pytest.raises(MirrorHipError):
        K.gemm(A, B, out=out, accumulate=True, split_k=f4.split_k, mma=MH_BF16, act=ACT_GELU)
    exact(full[:, :f4.M, :f4.N], G.integer_case(f4).prefill, "a refused call must not write")
    b_step("a refused call")


# ------------------------------------------------------------------------------------------ the production callers
def _wgrad_data(Bn, R, N, Kd, seed):
    gen = torch.Generator().manual_seed(seed)
    dy = torch.randint(-1, 2, (Bn, R, N), generator=gen).float()
    buf = torch.randint(-1, 2, (Bn, R + 2, Kd), generator=gen).float()        # x = buf[:, 1:1 + R]
    dy[:, -1] = torch.randint(-3, 4, (Bn, N), generator=gen).float()          # each slide's last row: the remainder's rows when batched
    buf[:, R] = torch.randint(-3, 4, (Bn, Kd), generator=gen).float()
    pre = torch.randint(-3, 4, (N, Kd), generator=gen).float()
    want = torch.matmul(dy.double().transpose(-1, -2), buf[:, 1:1 + R].double()).sum(0)
    return dy, buf, pre, want


def _check_partials_if_folded(dyt, x, rows, N, Kd, batch, prec):
    """Where the call goes through bf16 partial tiles, the exact comparison needs them to be bf16 numbers (as in integer_case)."""
    if prec is not Fn.BF16 or rows < 8 * 64 or rows % 64 == 0:
        return
    split = Fn._split_k_for(rows, N, Kd, batch=batch)
    d = G.desc_for(N, Kd, rows, split, batch, True, bf16, bf16, MH_BF16, True)
    if 0 < int(_lib.load().mh_gemm_workspace_bytes(ctypes.byref(d))) <= 2 ** 29:
        G.assert_partials_are_bf16_numbers(dyt, x, rows - rows % 64, split, 1.0, "wgrad")


@pytest.mark.parametrize("prec", [Fn.BF16, Fn.FP32], ids=lambda p: p.name)
@pytest.mark.parametrize("R", [257, 513])
def test_wgrad_flat_batched_window_and_prefilled(prec, R):
    """functional._wgrad as LinearFn.backward calls it: flat over B * R rows, as a batch of row windows reducing into one dW, and
    into a dW that already holds a gradient.  R = 257: the batched product is below 8 BK (one guarded launch, K ragged inside it)
    under bf16; R = 513 and every flat product split into main part + remainder."""
    Bn, N, Kd = 4, 512, 512
    dy, buf, pre, want = _wgrad_data(Bn, R, N, Kd, seed=R)
    x = buf[:, 1:1 + R]
    dy_d, buf_d = dy.to(DEV, prec.act), buf.to(DEV, prec.act)
    x_d = buf_d[:, 1:1 + R]
    assert not x_d.is_contiguous()
    _check_partials_if_folded(dy.reshape(1, Bn * R, N), x.reshape(1, Bn * R, Kd), Bn * R, N, Kd, 1, prec)
    _check_partials_if_folded(dy, x, R, N, Kd, Bn, prec)
    # flat
    dw = Fn._wgrad(dy_d.reshape(Bn * R, N), x_d.reshape(Bn * R, Kd), N, Kd, prec)
    print(f"flat {prec.name} R={R}: {variant()}")
    exact(dw, want, "flat _wgrad")
    # contiguous 3-d operands take the flat route too
    dw = Fn._wgrad(dy_d, x_d.contiguous(), N, Kd, prec)
    exact(dw, want, "_wgrad of contiguous batches")
    # batched window
    dw = Fn._wgrad(dy_d, x_d, N, Kd, prec)
    print(f"window {prec.name} R={R}: {variant()}")
    exact(dw, want, "batched-window _wgrad")
    # pre-filled dW, both forms
    dw = pre.to(DEV)
    assert Fn._wgrad(dy_d, x_d, N, Kd, prec, dw) is dw
    exact(dw, want + pre.double(), "batched-window _wgrad into a pre-filled dW")
    dw = pre.to(DEV)
    Fn._wgrad(dy_d.reshape(Bn * R, N), x_d.reshape(Bn * R, Kd), N, Kd, prec, dw)
    exact(dw, want + pre.double(), "flat _wgrad into a pre-filled dW")


@pytest.mark.parametrize("prec", [Fn.BF16, Fn.FP32], ids=lambda p: p.name)
@pytest.mark.parametrize("N", [260, 513])
def test_fc1_backward_weight_gradient_over_a_row_window_of_dh(prec, N):
    """The product of Fc1SeqFn.backward when the LayerNorm backward handed dh over: dh[:, :N] of [Bn, N + add_len, D] (a
    batch-strided operand), every slide reducing into one dW."""
    Bn, D, Fd, add_len = 4, 256, 512, 29
    gen = torch.Generator().manual_seed(N)
    dh_full = torch.randint(-1, 2, (Bn, N + add_len, D), generator=gen).float()
    xa = torch.randint(-1, 2, (Bn, N, Fd), generator=gen).float()
    dh_full[:, N - 1] = torch.randint(-3, 4, (Bn, D), generator=gen).float()
    xa[:, N - 1] = torch.randint(-3, 4, (Bn, Fd), generator=gen).float()
    dh_full[:, N:] = torch.randint(-3, 4, (Bn, add_len, D), generator=gen).float()     # rows past the window: never part of the product
    pre = torch.randint(-3, 4, (D, Fd), generator=gen).float()
    want = pre.double() + torch.matmul(dh_full[:, :N].double().transpose(-1, -2), xa.double()).sum(0)
    _check_partials_if_folded(dh_full[:, :N], xa, N, D, Fd, Bn, prec)
    dh = dh_full.to(DEV, prec.act)[:, :N]
    xa_d = xa.to(DEV, prec.act)
    dw = pre.to(DEV)
    K.gemm(dh.transpose(-1, -2), xa_d, out=dw.expand(Bn, D, Fd), accumulate=True, split_k=Fn._split_k_for(N, D, Fd, batch=Bn), mma=prec.mma)
    print(f"fc1 {prec.name} N={N}: {variant()}")
    exact(dw, want, "Fc1SeqFn.backward's dW")
