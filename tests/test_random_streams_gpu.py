"""GPU: every kernel that draws from the two Philox streams against the host reference (tests/philox_ref.py), bit for bit, and the
host code that places the streams of consecutive forwards and steps.

include/mirror_hip.h promises that element i of a tensor is an exact word (10-round stream: word i & 3 of block (offset + i) >> 2) or an
exact 16-bit field (lite stream: field i & 7 of block (offset + i) >> 3) of an exact block.  The kernel inputs here are ones or small
integers in f32 / bf16, so that the product with the multiplier is exact and torch.equal applies.

The behavioural tests run the `tiny` golden model in train mode: bare forwards draw fresh noise at disjoint ranges, consecutive engine
steps do not draw shifted copies of each other's noise, and no Philox block is claimed by two sites of a step or by two steps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mirror_amd import functional as Fn  # noqa: E402
from mirror_amd import kernels as K  # noqa: E402
from tests import philox_ref as R  # noqa: E402
from tests.golden_util import ModelCase  # noqa: E402

DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16
BIG = (1 << 34) + 12          # a 10-round offset whose block index needs the high counter word
SEED_HI = (1 << 32) + 5       # a seed with a non-zero high key word


def _base(v):
    return None if v is None else torch.tensor([v], device=DEV, dtype=torch.int64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ints(n):
    """Small integers 1 .. 3 as f32: exact in bf16, their product with any f32 multiplier is one rounding."""
    return (torch.arange(n, device=DEV) % 3 + 1).to(f32)


# --------------------------------------------------------------------------------------------------------------- mh_dropout
# (n, p, seed, offset, base): every n, p, offset and seed of the list at least once, the high counter word with the high key word, the
# scalar tail (n = 5, 1027) with each; base 130 must behave as 128
DROPOUT_CASES = [(1, 0.1, 123, 0, None), (5, 0.5, 123, 4, None), (5, 2.0 ** -20, SEED_HI, BIG, None), (1027, 0.1, SEED_HI, 4, None),
                 (1027, 0.5, 123, BIG, 130), (4096, 0.1, 123, BIG, None), (4096, 2.0 ** -20, 123, 0, None), (4096, 0.5, SEED_HI, BIG, 128),
                 (4096, 0.1, 123, 4, 130), (1027, 2.0 ** -20, 123, 0, 128)]


@pytest.mark.parametrize("n,p,seed,offset,base", DROPOUT_CASES)
def test_dropout_equals_the_reference_stream(n, p, seed, offset, base):
    """mh_dropout (quad kernel for n % 4 == 0, scalar-tail kernel otherwise), f32 and bf16: y = x * mult bit for bit.  At p = 2^-20
    the threshold is 4096: a kernel that compared 16 or 24 bits would keep everything."""
    mult = R.dropout_mult(n, p, seed, offset, base)
    assert n < 1000 or ((mult > 0).any() and (p < 1e-3 or (mult == 0).any()))
    x = _ints(n)
    want = _t(x.cpu().numpy() * mult)
    got = K.dropout(x, p, seed, offset, dev_base=_base(base))
    assert torch.equal(got, want), int((got != want).sum())
    if base is not None:        # the kernels mask the base with ~3: 130 and 128 are the same base, and the same as a larger offset
        assert torch.equal(got, K.dropout(x, p, seed, offset + (base & ~3)))
    one = torch.ones(n, device=DEV, dtype=bf16)
    got16 = K.dropout(one, p, seed, offset, dev_base=_base(base))
    want16 = _t(mult).to(bf16)                     # 0 or bf16(1 / (1 - p)), round to nearest even
    assert got16.dtype == bf16 and torch.equal(got16, want16)
    got_mixed = K.dropout(one, p, seed, offset, out=torch.empty(n, device=DEV, dtype=f32), dev_base=_base(base))
    assert torch.equal(got_mixed, _t(mult))


@pytest.mark.parametrize("n,p,seed,offset,base", [c for c in DROPOUT_CASES if c[0] % 4 == 0])
def test_dropout_add_and_the_autograd_sites_equal_the_reference_stream(n, p, seed, offset, base):
    """mh_dropout_add (a + dropout(x)) and the two autograd sites that draw from the running state: DropoutFn and DropoutAddFn apply the
    reference mask of (seed, running offset, base) in the forward and regenerate the same mask in the backward."""
    mult = R.dropout_mult(n, p, seed, offset, base)
    a, x = _ints(n).flip(0).contiguous(), _ints(n)
    want = _t(a.cpu().numpy() + x.cpu().numpy() * mult)
    assert torch.equal(K.dropout_add(a, x, p, seed, offset, dev_base=_base(base)), want)
    assert torch.equal(K.dropout_add(a, x.to(bf16), p, seed, offset, dev_base=_base(base)), want)
    saved = dict(Fn._dropout_state)
    try:
        for site in ("dropout", "dropout_add"):
            Fn._dropout_state.update(seed=seed, offset=offset, base=_base(base))
            xg = x.clone().requires_grad_(True)
            up = _ints(n).roll(1).contiguous()
            if site == "dropout":
                y = Fn.dropout(xg, p, True)
                want_y = _t(x.cpu().numpy() * mult)
            else:
                y = Fn.dropout_add(a.clone(), xg, p, True)
                want_y = want
            assert Fn._dropout_state["offset"] == offset + n
            y.backward(up)
            assert torch.equal(y.detach(), want_y), site
            assert torch.equal(xg.grad, _t(up.cpu().numpy() * mult)), site
    finally:
        Fn._dropout_state.clear()
        Fn._dropout_state.update(saved)


# ---------------------------------------------------------------------------------------------------------- mh_dropout_lite
LITE_BIG = (1 << 35) + 8
LITE_P = [0.1, 0.0, 0.5 / 65536, 1.5 / 65536, 0.999995]      # thr16 = 6554, 0, 1 (half rounds up), 2, 65535 (the cap)
LITE_CASES = ([(4096, p, 123, 0, None) for p in LITE_P] + [(8, p, SEED_HI, LITE_BIG, None) for p in LITE_P]
              + [(4096, 0.1, SEED_HI, 64, 69), (4096, 0.5 / 65536, 123, LITE_BIG, 64), (8, 0.1, 123, 64, 64), (8, 0.999995, 123, 0, 69),
                 (4096, 1.5 / 65536, 123, 64, None)])


@pytest.mark.parametrize("n,p,seed,offset,base", LITE_CASES)
def test_dropout_lite_equals_the_reference_stream(n, p, seed, offset, base):
    """mh_dropout_lite: 7 rounds, 16-bit fields, thr16 = min(floor(p * 65536 + 0.5), 65535), multiplier 65536 / (65536 - thr16);
    plain, add_to and bf16-input forms.  Base 69 must behave as 64 (& ~7)."""
    assert [R.lite_thr16(q) for q in LITE_P] == [6554, 0, 1, 2, 65535]
    mult = R.lite_mult(n, p, seed, offset, base)
    x = _ints(n)
    want = _t(x.cpu().numpy() * mult)
    got = K.dropout_lite(x, p, seed, offset, _base(base))
    assert torch.equal(got, want), int((got != want).sum())
    if base is not None:
        assert torch.equal(got, K.dropout_lite(x, p, seed, offset + (base & ~7)))
    a = _ints(n).flip(0).contiguous()
    want_add = _t(a.cpu().numpy() + x.cpu().numpy() * mult)
    assert torch.equal(K.dropout_lite(x, p, seed, offset, _base(base), add_to=a), want_add)
    assert torch.equal(K.dropout_lite(x.to(bf16), p, seed, offset, _base(base), add_to=a), want_add)
    got16 = K.dropout_lite(torch.ones(n, device=DEV, dtype=bf16), p, seed, offset, _base(base))
    assert got16.dtype == bf16 and torch.equal(got16, _t(mult).to(bf16))


@pytest.mark.parametrize("p,seed,offset,base", [(0.1, 123, 64, None), (0.5, SEED_HI, LITE_BIG, 69)])
def test_dropout_lite_colsum_rows_and_columns_map_to_flat_elements(p, seed, offset, base):
    """mh_dropout_lite_colsum on [4, 256]: element (row, col) takes the reference mask at flat index row * 256 + col; db += the
    column sums of the bf16 values written (at most four equal bf16 numbers per column: exact in f32)."""
    rows, N = 4, 256
    assert K.dropout_lite_colsum_ok(N)
    mult = R.lite_mult(rows * N, p, seed, offset, base).reshape(rows, N)
    x = torch.ones(rows, N, device=DEV)
    out = torch.empty(rows, N, device=DEV, dtype=bf16)
    db = torch.full((N,), 3.0, device=DEV)
    K.dropout_lite_colsum(x, p, seed, offset, _base(base), out, db)
    want = _t(mult).to(bf16)
    assert torch.equal(out, want)
    assert torch.equal(db, 3.0 + want.float().sum(0))
    assert len({tuple(r) for r in (mult > 0).tolist()}) == rows      # the rows' masks differ: a kernel that ignored the row would fail


# ----------------------------------------------------------------------------------------------------------- MH_EPI_DROPADD
@pytest.mark.parametrize("p,seed,offset,base", [(0.1, 123, 64, None), (0.5, SEED_HI, LITE_BIG, 69)])
def test_dropadd_epilogue_indexes_the_lite_stream_by_flat_element(p, seed, offset, base):
    """The fused projection's smallest shape (M = 257 rows: the rule is M > 256; N = 256, K = 64) with a zero weight and bias 1:
    C = resid + mult, and the mask is the reference's at flat index row * N + col — the epilogue's own indexing."""
    M, N, Kd = 257, 256, 64
    x = torch.zeros(1, M, Kd, device=DEV, dtype=bf16)
    w = torch.zeros(N, Kd, device=DEV, dtype=bf16)
    assert K.linear_fused_ok(x, w) and K.linear_fused_tail(M) == 0
    bias = torch.ones(N, device=DEV)
    resid = _ints(M * N).view(1, M, N)
    out = torch.full((1, M, N), -7.0, device=DEV)
    K.linear_fused(x, w, bias, out, K.epi_dropadd(resid, p, seed, offset, _base(base)))
    mult = R.lite_mult(M * N, p, seed, offset, base)
    want = _t(resid.cpu().numpy().reshape(-1) + mult).view(1, M, N)
    assert torch.equal(out, want), int((out != want).sum())


# ---------------------------------------------------------------------------------------------------------------- RNA block
@pytest.mark.parametrize("B,D,Hh,H,offset,base", [(3, 64, 128, 2, 64, None), (3, 64, 128, 2, BIG, 130), (1, 32, 32, 2, 0, None)])
def test_rna_block_draws_its_three_masks_at_the_documented_offsets(B, D, Hh, H, offset, base):
    """mh_rna_block_fwd, p = 0.25, with zero weights so that all three masks are observable exactly: proj bias 1 -> x1 = x + m1;
    fc1 bias 8 (gelu(8) = 8 in f32) -> f = bf16(8 m2); fc2 bias 1 -> y = x1 + m3.  m1, m2, m3 are the 10-round stream at `offset`,
    + q4(B D), + q4(B Hh) more (q4 = round up to 4), element index = row * width + column.  The kernel accepts B = 1, D = Hh = 32."""
    p, seed = 0.25, SEED_HI
    assert K.rna_block_ok(torch.empty(B, D, device=DEV), D, Hh, H)
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=bf16)  # noqa: E731
    v = lambda n, c: torch.full((n,), c, device=DEV, dtype=f32)  # noqa: E731
    params = dict(w_qkv=z(3 * D, D), w_proj=z(D, D), w_fc1=z(Hh, D), w_fc2=z(D, Hh), b_qkv=v(3 * D, 0.0), b_proj=v(D, 1.0),
                  b_fc1=v(Hh, 8.0), b_fc2=v(D, 1.0), g1=v(D, 1.0), be1=v(D, 0.0), g2=v(D, 1.0), be2=v(D, 0.0))
    x = _ints(B * D).view(B, D)
    y, saved = K.rna_block_fwd(x, params, H, 1e-6, p, seed, offset, _base(base))
    q4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    m1 = R.dropout_mult(B * D, p, seed, offset, base)
    m2 = R.dropout_mult(B * Hh, p, seed, offset + q4(B * D), base)
    m3 = R.dropout_mult(B * D, p, seed, offset + q4(B * D) + q4(B * Hh), base)
    assert not np.array_equal(m1 > 0, m3 > 0) and (m2 == 0).any() and (m2 > 0).any()
    x1 = x.cpu().numpy().reshape(-1) + m1
    assert torch.equal(saved["x1"].view(-1), _t(x1))
    assert torch.equal(saved["u"].view(-1), torch.full((B * Hh,), 8.0, device=DEV, dtype=bf16))
    assert torch.equal(saved["f"].view(-1), _t(np.float32(8.0) * m2).to(bf16))
    assert torch.equal(y.view(-1), _t(x1 + m3))


# ----------------------------------------------------------------------------------------------------------- mh_noise_draws
NOISE_CASES = [(nn, off, base) for nn in (6, 256) for off in (64, 1 << 44) for base in (None, 130)]


@functools.lru_cache(maxsize=None)
def _noise_bound():
    """4 x the worst deviation of the float32 evaluation of the documented formula (numpy, CPU) from its float64 evaluation, relative to
    max(1, |z|), over the words of NOISE_CASES."""
    worst = 0.0
    for nn, off, base in NOISE_CASES:
        z64 = R.noise(64, nn, 123, off, base)[64:]
        z32 = R.noise(64, nn, 123, off, base, dtype=np.float32)[64:].astype(np.float64)
        worst = max(worst, float((np.abs(z32 - z64) / np.maximum(1.0, np.abs(z64))).max()))
    return 4.0 * worst, worst


@pytest.mark.parametrize("n_normal,offset,base", NOISE_CASES)
def test_noise_draws_equal_the_reference_words(n_normal, offset, base):
    """mh_noise_draws, 64 uniforms + 6 (ragged tail) or 256 normals, at offset 64 and at the noise range's own 2^44 (block 2^42: the high
    counter word), with and without a base.  Uniforms: (word >> 8) * 2^-24 exactly.  Normals: within 4 x the float32-vs-float64
    deviation of the same formula evaluated by numpy on these words, relative to max(1, |z|) — measured 1.007e-6 (at |z| = 3.08), so the
    bound is 4.03e-6; the factor covers the device's logf / sincosf against libm.  The pair with the smallest u1 of each case
    ((k + 1) * 2^-24 with k = 126144, 69156, 97888 of 2^24: |z| > 3) is asserted on its own."""
    bound, measured = _noise_bound()
    assert 1e-7 < measured < 4e-6, measured          # the float32 formula's own error: a few ulp of a value of size ~3
    n_u = 64
    got = K.noise_draws(n_u, n_normal, 123, offset, _base(base), DEV).double().cpu()
    want = torch.from_numpy(R.noise(n_u, n_normal, 123, offset, base))
    assert got.shape == want.shape and torch.equal(got[:n_u], want[:n_u])
    err = (got[n_u:] - want[n_u:]).abs() / want[n_u:].abs().clamp(min=1.0)
    print(f"noise normals n={n_normal} offset={offset} base={base}: worst {float(err.max()):.3e}, bound {bound:.3e}")
    assert float(err.max()) <= bound, (float(err.max()), bound)
    words = R.stream_words(n_u + (n_normal + 3) // 4 * 4, 123, offset, base)[n_u:n_u + n_normal // 2 * 2]
    i = int(np.argmin(words[0::2] >> np.uint64(8)))        # the pair with the smallest u1: the largest radius of the set
    pair_err = err[2 * i:2 * i + 2]
    assert float(pair_err.max()) <= bound and float(want[n_u + 2 * i:n_u + 2 * i + 2].norm()) == pytest.approx(
        (-2.0 * np.log((float(int(words[2 * i]) >> 8) + 1.0) * 2.0 ** -24)) ** 0.5, rel=1e-9)


# ------------------------------------------------------------------------------------ the tiny model in train mode: where the streams go
def _tiny(precision="fp32", p_zero=False):
    """The `tiny` golden model as test_model_gpu.py builds it, in train mode."""
    import mirror_amd.models as M
    case = ModelCase("tiny")
    c = case.cfg
    model = M.mirror(
        wsi_embed_dim=c.wsi_embed_dim, rna_embed_dim=c.rna_embed_dim, embed_dim=c.embed_dim,
        wsi_num_tokens=c.wsi_num_tokens, wsi_retention_decoder_depth=c.wsi_retention_decoder_depth,
        rna_encoder_depth=c.rna_encoder_depth, rna_mlp_ratio=c.rna_mlp_ratio, rna_norm_layer="layernorm",
        rna_act_layer="gelu", rna_retention_decoder_depth=c.rna_retention_decoder_depth,
        style_mlp_hidden_dim=c.style_mlp_hidden_dim, style_mlp_out_dim=c.style_mlp_out_dim,
        style_latent_dim=c.style_latent_dim, num_prototypes=c.num_prototypes, rna_num_heads=c.rna_num_heads)
    model.load_state_dict(case.sd, strict=True)
    model.precision = precision
    if p_zero:          # every dropout probability of the model
        n = 0
        for m in model.modules():
            for a in ("drop", "proj_drop", "pos_drop_rate"):
                if isinstance(getattr(m, a, None), float):
                    setattr(m, a, 0.0)
                    n += 1
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        assert n > 0
    wsi = case.wsi.to(DEV)
    return case, model.to(DEV).train(), (wsi if precision == "fp32" else wsi.to(bf16)), case.rna.to(DEV)


class _Streams:
    """Fresh stream state for a test, the tap on, Fn.noise_draws' four results recorded; everything restored on exit."""

    def __enter__(self):
        self.saved = dict(Fn._dropout_state)
        self.orig = Fn.noise_draws
        self.draws = []

        def recording(*a, **k):
            out = self.orig(*a, **k)
            self.draws.append(tuple(t.detach().clone() for t in out))
            return out
        Fn.noise_draws = recording
        Fn.dropout_device_base_off()
        Fn.manual_seed(4242)
        Fn._dropout_tap = []
        return self

    def __exit__(self, *exc):
        Fn.noise_draws = self.orig
        Fn._dropout_tap = None
        Fn._dropout_state.clear()
        Fn._dropout_state.update(self.saved)

    @staticmethod
    def take():
        recs, Fn._dropout_tap = Fn._dropout_tap, []
        return recs


def _noise_recs(recs):
    """(n_uniform, n_normal, seed, effective host offset) of the noise launches among tap records."""
    return [(r[0][0], r[0][1], r[2], r[3]) for r in recs if r[1] is None]


def _claims(recs, base=0):
    """Blocks claimed by the records of one forward run under device base `base`: (10-round stream incl. the noise range, lite stream)."""
    b10, b8 = [], []
    for shape, p, seed, offset, lite in recs:
        n = int(np.sum(shape)) if p is None else int(np.prod(shape))
        if lite:
            first = offset + (base & ~7)
            b8.append(range(first >> 3, ((first + n - 1) >> 3) + 1))
        else:
            first = offset + (base & ~3)
            b10.append(range(first >> 2, ((first + n - 1) >> 2) + 1))
    return b10, b8


def _assert_disjoint(ranges, what):
    ranges = sorted(ranges, key=lambda r: r.start)
    for a, b in zip(ranges[:-1], ranges[1:]):
        assert a.stop <= b.start, f"{what}: blocks [{a.start}, {a.stop}) and [{b.start}, {b.stop}) overlap"


def _bare_forward(case, model, wsi, rna):
    from mirror_amd.losses import MIRRORLoss
    outs = model(wsi, rna, wsi_mask_ratio=case.ratios[0], rna_mask_ratio=case.ratios[1])
    MIRRORLoss()(*outs)[0].backward()
    return outs


@pytest.mark.parametrize("stale_base", [False, True])
def test_two_bare_training_forwards_draw_fresh_noise(stale_base):
    """model.train()(wsi, rna) with no engine: the WSI token noise, the RNA noise and both style eps of two consecutive forwards differ,
    their launches occupy disjoint blocks of the noise range, and the draws are the reference's for the recorded (seed, offset).  Also
    with a device base that dropout_step_begin left behind and no engine step advances."""
    case, model, wsi, rna = _tiny()
    with _Streams() as st:
        if stale_base:
            Fn.dropout_step_begin(torch.device("cuda", torch.cuda.current_device()))
        _bare_forward(case, model, wsi, rna)
        r0 = st.take()
        _bare_forward(case, model, wsi, rna)
        r1 = st.take()
        d0, d1 = st.draws
        for a, b, nm in zip(d0, d1, ("wsi_mask", "rna_mask", "wsi_eps", "rna_eps")):
            assert a.shape == b.shape and not torch.equal(a, b), f"{nm}: two bare forwards drew the same noise"
        (n0,), (n1,) = _noise_recs(r0), _noise_recs(r1)
        B, N, D, L = case.batch, case.cfg.wsi_num_tokens, case.cfg.embed_dim, case.cfg.style_latent_dim
        assert n0[:2] == n1[:2] == ((B * N + 3) // 4 * 4 + (B * D + 3) // 4 * 4, 2 * B * L) and n0[2] == n1[2] == 4242
        blocks = [range(o >> 2, (o + nu + nn + 3) >> 2) for nu, nn, _, o in (n0, n1)]
        _assert_disjoint(blocks, "noise ranges of two bare forwards")
        for (nu, nn, seed, off), d in ((n0, d0), (n1, d1)):         # what the model was handed is the reference stream at that offset
            ref = torch.from_numpy(R.noise(nu, nn, seed, off, 0 if stale_base else None))
            n_a = (B * N + 3) // 4 * 4
            assert torch.equal(d[0].double().cpu().view(-1), ref[:B * N]) and torch.equal(d[1].double().cpu().view(-1), ref[n_a:n_a + B * D])
            assert float((d[2].double().cpu().view(-1) - ref[nu:nu + B * L]).abs().max()) <= 1e-5


def test_manual_seed_reproduces_the_bare_sequence():
    case, model, wsi, rna = _tiny()
    with _Streams() as st:
        runs = []
        for _ in range(2):
            Fn.manual_seed(7)
            del st.draws[:]
            _bare_forward(case, model, wsi, rna)
            _bare_forward(case, model, wsi, rna)
            runs.append((list(st.draws), _noise_recs(st.take())))
        (da, ra), (db, rb) = runs
        assert ra == rb and ra[0][2] == 7 and ra[0][3] == Fn._NOISE_OFFSET
        for fa, fb in zip(da, db):
            assert all(torch.equal(a, b) for a, b in zip(fa, fb))
        assert not torch.equal(da[0][0], da[1][0])


def _engine_steps(precision, graph, steps, p_zero):
    """TrainEngine steps on the tiny model: per step (device base before, device base after, tap records)."""
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    case, model, wsi, rna = _tiny(precision, p_zero=p_zero)
    eng = TrainEngine(model, MIRRORLoss(), lr=1e-4, precision=precision, graph=graph, wsi_mask_ratio=case.ratios[0],
                      rna_mask_ratio=case.ratios[1])
    out = []
    for _ in range(steps):
        base = Fn._dropout_state["base"]
        before = 0 if base is None else int(base)
        eng.step(wsi, rna)
        out.append((before, int(Fn._dropout_state["base"]), _Streams.take()))
    return case, eng, out


def test_consecutive_engine_steps_do_not_draw_shifted_noise():
    """TrainEngine, eager, every dropout probability 0, two steps: the device base grows by at least the n_uniform + n_normal noise
    elements of the step, and step 1's uniform draws (regenerated by the reference from the tap record and the base the step ran
    under) are no shifted copy of step 0's: for every shift s at most one position with u1[i] == u0[i + s] (independent 24-bit draws
    of a few hundred elements coincide twice at one shift with probability ~1e-8)."""
    with _Streams():
        case, eng, steps = _engine_steps("fp32", False, 2, p_zero=True)
        us = []
        for before, after, recs in steps:
            assert [r for r in recs if r[1] is not None] == [], "a dropout site ran at p = 0"
            (nu, nn, seed, off), = _noise_recs(recs)
            assert off == Fn._NOISE_OFFSET, "inside an engine step the noise launch's offset is the constant a captured step bakes in"
            assert after - before >= nu + nn, f"the base grew by {after - before} < {nu + nn} noise elements"
            us.append(R.noise(nu, 0, seed, off, before))
        u0, u1 = us
        assert steps[1][0] == steps[0][1]
        worst = max((int(np.sum(u1[:len(u1) - s] == u0[s:])), s) for s in range(len(u0)))
        assert worst[0] <= 1, f"{worst[0]} of {len(u0) - worst[1]} positions equal at shift {worst[1]}"


def test_graphed_engine_steps_advance_the_base_past_the_noise():
    """The same growth under the default whole-step graph (two eager steps, the capture, replays): one device scalar around engine.step."""
    with _Streams():
        case, eng, steps = _engine_steps("bf16", None, 5, p_zero=True)
        assert eng._graph is not None, "the step was not captured"
        B, N, D, L = case.batch, case.cfg.wsi_num_tokens, case.cfg.embed_dim, case.cfg.style_latent_dim
        n_noise = (B * N + 3) // 4 * 4 + (B * D + 3) // 4 * 4 + 2 * B * L
        for before, after, _ in steps:
            assert after - before >= n_noise, (before, after, n_noise)


def test_no_philox_block_is_claimed_twice_within_a_forward_or_across_steps():
    """Tap records of the tiny model in train mode with its default dropout.  One bare forward: no block of the 10-round stream (noise
    range included; block = (offset + i) >> 2) and no block of the lite stream (>> 3) is claimed by two sites.  Two engine steps: the
    ranges shifted by each step's device base, after the kernels' & ~3 / & ~7 masking, are disjoint as well."""
    case, model, wsi, rna = _tiny()
    with _Streams() as st:
        _bare_forward(case, model, wsi, rna)
        recs = st.take()
        assert len(_noise_recs(recs)) == 1 and any(r[4] for r in recs) and any(r[1] is not None and not r[4] for r in recs), recs
        b10, b8 = _claims(recs)
        _assert_disjoint(b10, "10-round stream, one forward")
        _assert_disjoint(b8, "lite stream, one forward")
    with _Streams():
        case, eng, steps = _engine_steps("fp32", False, 2, p_zero=False)
        all10, all8 = [], []
        for before, after, recs in steps:
            assert any(r[4] for r in recs) and len(_noise_recs(recs)) == 1
            b10, b8 = _claims(recs, before)
            all10 += b10
            all8 += b8
        _assert_disjoint(all10, "10-round stream, two engine steps")
        _assert_disjoint(all8, "lite stream, two engine steps")
