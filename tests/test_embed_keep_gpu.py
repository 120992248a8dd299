"""GPU: the compact retention embed (EmbedMaskPosFn with a keep map; mh_rank_mask_keep, mh_rows_gather, mh_mask_expand_fwd,
mh_mask_apply_bwd_keep, mh_rows_expand_zero of include/mirror_hip.h) against the dense MASKPOS launch and the composed ops.

retention_embed is only needed at the cls row and the kept 25 % of the tokens (models/mirror.py:636-643, :690-693): the compact path
multiplies those rows alone, forward and backward, and must give what the dense path gives.  Shapes: the smallest that hit each edge
(whole 256-row tiles on both paths; a 3-row tail on both; a compact row count the fused kernel refuses, at the template width;
nothing masked; one kept token; ties in the noise)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64

#        name        B   N     keep  K    D    ties
CASES = {"aligned": (4, 255, 127, 512, 512, False),
         "ragged": (3, 1024, 256, 512, 512, False),
         "small": (2, 300, 75, 256, 768, True),
         "keep_all": (2, 300, 300, 256, 256, False),
         "keep_one": (2, 300, 1, 256, 256, False)}


def _noise(B, N, ties, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(B, N, generator=g)
    if ties:
        noise = torch.floor(noise * 16) / 16        # 16 distinct values: the index breaks every tie
        noise[0, : N // 2] = 0.5                    # and one long run of a single value
    return noise.cuda()


@functools.lru_cache(maxsize=None)
def _run(name):
    """One forward + backward of the three forms (compact, dense launch, composed ops) on the same operands: computed once per case."""
    from mirror_amd import functional as Fn
    from mirror_amd import kernels as K
    B, N, keep, Kd, D, ties = CASES[name]
    T = N + 1
    prec = Fn.POLICIES["bf16"]
    g = torch.Generator().manual_seed(11)
    h32 = torch.randn(B, T, Kd, generator=g).cuda()
    token = (torch.randn(1, 1, D, generator=g) * 0.02).cuda().requires_grad_(True)
    pos = (torch.randn(1, T, D, generator=g) * 0.02).cuda().requires_grad_(True)
    up = torch.randn(B, T, D, generator=g).cuda()
    w = (torch.randn(D, Kd, generator=g) / Kd ** 0.5).cuda().requires_grad_(True)
    b = (torch.randn(D, generator=g) * 0.1).cuda().requires_grad_(True)
    mask = K.rank_mask(_noise(B, N, ties, 12), keep)
    assert mask._keep[2] == keep
    plain = mask.clone()          # the same mask without its map: the dense path
    res = {}
    gathered = []
    orig, was = K.rows_gather, Fn._EMBED_KEEP_TILES
    K.rows_gather = lambda *a, **k: (gathered.append(1), orig(*a, **k))[1]
    Fn._EMBED_KEEP_TILES = 0          # these shapes are below the size at which embed_mask_pos picks the compact path by itself
    try:
        for form in ("compact", "dense", "composed"):
            h = h32.clone().requires_grad_(True)
            for p in (w, b, token, pos):
                p.grad = None
            if form == "composed":
                y = Fn.MaskApplyFn.apply(Fn.linear(h, w, b, prec=prec), plain, token, pos, 1, False)
            else:
                h._bf16 = h32.to(bf16)
                y = Fn.embed_mask_pos(h, w, b, mask if form == "compact" else plain, token, pos, 1, prec)
                assert y.grad_fn.__class__.__name__.startswith("EmbedMaskPosFn")
            assert len(gathered) == (1 if form == "compact" else 0), "only a mask with its keep map takes the compact path"
            gathered.clear()
            y.backward(up.clone())
            res[form] = [y.detach().clone()] + [t.grad.clone() for t in (h, w, b, token, pos)]
    finally:
        K.rows_gather, Fn._EMBED_KEEP_TILES = orig, was
    # f64 reference of the forward on the bf16 operands the kernels read
    proj = h32.to(bf16).to(f64) @ w.detach().to(bf16).to(f64).t() + b.detach().to(f64)
    m = torch.cat([torch.zeros(B, 1, device="cuda"), plain], 1).bool()[..., None]
    ref = torch.where(m, token.detach().to(f64).expand(B, T, D), proj) + pos.detach().to(f64)
    torch.cuda.synchronize()
    return res, ref, float(proj.abs().max()), m[..., 0]


@pytest.mark.parametrize("B,N,keep,ties", [(4, 255, 127, False), (3, 1024, 256, True), (2, 300, 300, False), (2, 300, 1, True), (2, 77, 0, False)])
def test_keep_map_matches_the_mask_and_a_stable_host_argsort(B, N, keep, ties):
    from mirror_amd import kernels as K
    noise = _noise(B, N, ties, 5)
    mask = K.rank_mask(noise, keep)
    keep_idx, slot, k = mask._keep
    assert k == keep and keep_idx.dtype == slot.dtype == torch.int32
    assert tuple(keep_idx.shape) == (B, keep) and tuple(slot.shape) == (B, N)
    assert torch.equal(mask, K.rank_mask(noise, keep, keep_map=False)), "mh_rank_mask_keep's mask is mh_rank_mask's bit for bit"
    order = np.argsort(noise.cpu().numpy(), axis=1, kind="stable")
    want_slot = np.full((B, N), -1, dtype=np.int32)
    for bi in range(B):
        want_slot[bi, order[bi, :keep]] = np.arange(keep, dtype=np.int32)
    assert np.array_equal(keep_idx.cpu().numpy(), order[:, :keep].astype(np.int32))
    assert np.array_equal(slot.cpu().numpy(), want_slot)
    assert np.array_equal(mask.cpu().numpy(), (want_slot < 0).astype(np.float32))
    assert int((mask == 0).sum()) == B * keep


def test_aligned_forward_is_bit_identical_to_the_dense_launch_and_the_composed_ops():
    res, _, _, _ = _run("aligned")
    y = res["compact"][0]
    assert torch.equal(y, res["dense"][0]), float((y - res["dense"][0]).abs().max())
    assert torch.equal(y, res["composed"][0]), float((y - res["composed"][0]).abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_forward_error_against_f64_is_the_dense_path_s(name):
    """max |y - f64 reference| of the compact path <= the dense launch's on the same inputs + one bf16 ulp at the projection's magnitude
    (both round the projection to bf16 once; the two may run different GEMM kernels on the ragged rows)."""
    res, ref, pmax, _ = _run(name)
    e_compact = float((res["compact"][0].to(f64) - ref).abs().max())
    e_dense = float((res["dense"][0].to(f64) - ref).abs().max())
    ulp = 2.0 ** (math.floor(math.log2(pmax)) - 7)
    print(f"{name}: max error vs f64 compact {e_compact:.3e} dense {e_dense:.3e} (bf16 ulp at |proj| max {pmax:.3f} = {ulp:.3e})")
    assert e_compact <= e_dense + ulp


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_match_the_dense_path_and_masked_rows_get_exact_zeros(name):
    res, _, _, m = _run(name)
    (_, dh, dw, db, dtok, dpos), (_, dh0, dw0, db0, dtok0, dpos0) = res["compact"], res["dense"]
    assert int(m.sum()) == 0 or float(dh[m].abs().max()) == 0.0, "dh is exactly 0 on masked rows"
    assert not bool(m[:, 0].any()) and float(dh[~m].abs().max()) > 0
    for nm, a, c in (("dh", dh, dh0), ("dW", dw, dw0), ("db", db, db0), ("dtoken", dtok, dtok0), ("dpos", dpos, dpos0)):
        err, mx = float((a - c).abs().max()), float(c.abs().max())
        print(f"{name}: {nm} max |compact - dense| {err:.3e} of max {mx:.3e}")
        assert err <= 1e-5 * mx, nm         # f32 sums whose order may differ (split-K, atomics, another GEMM kernel on ragged rows)


@pytest.mark.parametrize("B,N,keep,D", [(4, 255, 127, 512), (3, 300, 75, 768), (9, 40, 40, 256)])
def test_streaming_kernels_against_their_dense_forms(B, N, keep, D):
    """mh_rows_gather / mh_rows_expand_zero against index ops, mh_mask_expand_fwd against mh_mask_apply_fwd on the dense projection (bit
    for bit), mh_mask_apply_bwd_keep against mh_mask_apply_bwd: the same dr rows bit for bit, the sums to 1e-5 x max (f32 atomics)."""
    from mirror_amd import kernels as K
    T, first = N + 1, 1
    g = torch.Generator().manual_seed(21)
    mask = K.rank_mask(_noise(B, N, True, 22), keep)
    keep_idx, slot, _ = mask._keep
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long, device="cuda"), keep_idx.long() + 1], 1)         # [B, first + keep] token rows
    x = torch.randn(B, T, D, generator=g).cuda().to(bf16)
    xc = K.rows_gather(x, keep_idx, first, keep)
    assert torch.equal(xc, torch.gather(x, 1, rows[..., None].expand(B, first + keep, D)))
    token, pos = (torch.randn(D, generator=g) * 0.02).cuda(), (torch.randn(T * D, generator=g) * 0.02).cuda()
    y = K.mask_expand_fwd(xc, slot, token, pos, T, first, keep, torch.empty(B, T, D, device="cuda"))
    y0 = torch.empty(B, T, D, device="cuda")
    K.mask_apply_fwd(x, mask, token, pos, B, T, D, first, False, out=y0)
    assert torch.equal(y, y0)
    dy = torch.randn(B, T, D, generator=g).cuda()
    outs = []
    for compact in (True, False):
        dtok, dpos, dbias = torch.zeros(D, device="cuda"), torch.zeros(T * D, device="cuda"), torch.zeros(D, device="cuda")
        dr = torch.full((B, first + keep if compact else T, D), float("nan"), device="cuda", dtype=bf16)
        if compact:
            K.mask_apply_bwd_keep(dy, slot, dtok, dpos, B, T, D, first, keep, out=dr, dbias=dbias)
        else:
            K.mask_apply_bwd(dy, mask, dtok, dpos, B, T, D, first, False, out=dr, dbias=dbias)
        outs.append((dr, dtok, dpos, dbias))
    (drc, dtok, dpos, dbias), (dr0, dtok0, dpos0, dbias0) = outs
    assert torch.equal(drc, torch.gather(dr0, 1, rows[..., None].expand(B, first + keep, D))), "every compact row is written, with dr's bits"
    for nm, a, c in (("dtoken", dtok, dtok0), ("dpos", dpos, dpos0), ("dbias", dbias, dbias0)):
        assert float((a - c).abs().max()) <= 1e-5 * max(float(c.abs().max()), 1e-30), nm
    dhc = torch.randn(B, first + keep, D, generator=g).cuda()
    dh = K.rows_expand_zero(dhc, slot, T, first, keep)
    want = torch.zeros(B, T, D, device="cuda").scatter_(1, rows[..., None].expand(B, first + keep, D), dhc)
    assert torch.equal(dh, want)


@pytest.mark.parametrize("B,N,D,compact", [(6, 4096, 768, True), (2, 1024, 512, False)])
def test_embed_mask_pos_picks_the_compact_path_above_one_round_of_tiles(B, N, D, compact):
    """By itself embed_mask_pos takes the compact path when the dense launch is more than one round of 256 x 256 tiles on 256 CUs
    (6 x 4097 rows x 768 columns = 97 x 3 tiles); below that the single MASKPOS launch stays (2 x 1025 x 512 = 9 x 2 tiles)."""
    from mirror_amd import functional as Fn
    from mirror_amd import kernels as K
    prec = Fn.POLICIES["bf16"]
    g = torch.Generator().manual_seed(41)
    T, Kd = N + 1, 256
    h = torch.randn(B, T, Kd, generator=g).cuda().to(bf16)
    w, b = (torch.randn(D, Kd, generator=g) / 16).cuda(), (torch.randn(D, generator=g) * 0.1).cuda()
    token, pos = (torch.randn(1, 1, D, generator=g) * 0.02).cuda(), (torch.randn(1, T, D, generator=g) * 0.02).cuda()
    mask = K.rank_mask(torch.rand(B, N, generator=g).cuda(), N // 4)
    kinds = []
    orig = K.linear_fused
    K.linear_fused = lambda *a, **k: (kinds.append(a[4].kind), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            y = Fn.embed_mask_pos(h, w, b, mask, token, pos, 1, prec)
            y0 = Fn.embed_mask_pos(h, w, b, mask.clone(), token, pos, 1, prec)
    finally:
        K.linear_fused = orig
    assert kinds == ([K.EPI_MASKPOS] if compact else [K.EPI_MASKPOS] * 2)
    # the few rows past whole tiles go through the weight-streaming kernel (f32 FMA order), and they are other tokens on the two paths:
    # at most one flip of the projection's bf16 rounding
    assert float((y - y0).abs().max()) <= 2.0 ** (math.floor(math.log2(float(y0.abs().max()))) - 7)


def test_a_mask_without_its_map_or_written_since_takes_the_dense_path():
    from mirror_amd import functional as Fn
    from mirror_amd import kernels as K
    mask = K.rank_mask(_noise(2, 300, False, 31), 75)
    assert Fn._keep_of(mask, 2, 300) is mask._keep
    assert Fn._keep_of(mask.clone(), 2, 300) is None and Fn._keep_of(mask, 2, 299) is None
    mask.mul_(1.0)          # an in-place write by torch: the map no longer vouches for the values
    assert Fn._keep_of(mask, 2, 300) is None
