"""MI355X: the survival step of train_survival.py through the C ABI (csrc/survival.hip) — NLLSurvLoss / CrossEntropySurvLoss and
their logit gradients against the unmodified reference (tests/golden/golden_surv.npz), determinism and graph replay, the risk
score, the censored concordance index against the numpy restatement, and a linear probe at the survival template geometry."""
import os

import numpy as np
import pytest
import torch

from mirror_amd import survival as SV
from mirror_amd.losses import CrossEntropySurvLoss, NLLSurvLoss
from tests.test_survival_cpu import ALPHAS, MS, NS, REDUCTIONS, cindex_np

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_surv.npz")
CASES = [(k, n, m) for k in ("nll", "ce") for n in NS for m in MS]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _inputs(z, kind, N, M):
    G = f"{kind}/N{N}_M{M}"
    x, t, c = (torch.from_numpy(z[f"{G}/{k}"]).cuda() for k in ("logits", "event_times", "censoring"))
    return G, x, t, c, torch.from_numpy(z[f"{G}/w"]).cuda(), torch.from_numpy(z[f"{G}/gs"]).cuda()


def _loss_fn(kind, alpha, red):
    return NLLSurvLoss(alpha=float(alpha), reduction=red) if kind == "nll" else CrossEntropySurvLoss(reduction=red)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


@pytest.mark.parametrize("kind,N,M", CASES)
def test_loss_and_dlogits_match_reference_golden(z, kind, N, M):
    G, x, t, c, w, gs = _inputs(z, kind, N, M)
    feeds = [(t, c)]
    if c.dtype == torch.int64 and not (c == 2).any():
        feeds.append((t.to(torch.int64), c.bool()))              # the bool censoring path reads the same values
    for a in ALPHAS[kind]:
        for red in REDUCTIONS:
            want, dwant = z[f"{G}/a{a}/{red}/loss"], z[f"{G}/a{a}/{red}/dlogits"]
            for tt, cc in feeds:
                xl = x.clone().requires_grad_(True)
                loss = _loss_fn(kind, a, red)(xl, tt, cc)
                assert tuple(loss.shape) == want.shape, (G, red, tuple(loss.shape))
                assert loss.dtype == torch.float32
                err = _rel(loss.detach().cpu().numpy(), want)
                assert err <= 1e-5, (G, a, red, err)
                (loss * (w if red == "none" else gs)).sum().backward()
                dg = xl.grad.cpu().numpy()
                derr = _rel(dg, dwant)
                assert derr <= 1e-5, (G, a, red, derr)
                sat = np.abs(z[f"{G}/logits"]) >= 20
                assert np.all(dg[sat] == 0), (G, a, red)


def test_ce_out_of_range_uncensored_time_gives_nan_row():
    x = torch.randn(5, 4, device="cuda", requires_grad=True)
    t = torch.tensor([0, 5, 2, 4, 1], device="cuda", dtype=torch.int32)       # row 1: uncensored T = M + 1
    c = torch.tensor([1, 1, 0, 1, 0], device="cuda")
    loss = CrossEntropySurvLoss(reduction="none")(x, t, c)
    assert loss.shape == (5, 1)
    bad = torch.isnan(loss[:, 0]).cpu().tolist()
    assert bad == [False, True, False, False, False]
    loss.sum().backward()
    gbad = torch.isnan(x.grad).cpu().numpy()
    assert gbad[1].all() and not gbad[[0, 2, 3, 4]].any()


@pytest.mark.parametrize("kind", ["nll", "ce"])
def test_deterministic_and_graph_replay_matches_eager(z, kind):
    G, x, t, c, w, gs = _inputs(z, kind, 257, 20)
    fn = _loss_fn(kind, 0.4 if kind == "nll" else 0, "mean")

    def step(xs):
        xl = xs.detach().requires_grad_(True)
        loss = fn(xl, t, c)
        (dx,) = torch.autograd.grad(loss, xl)
        return loss.detach(), dx

    l1, d1 = step(x)
    l2, d2 = step(x)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)
    static_x = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(static_x)                                   # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gl, gd = step(static_x)
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    el, ed = step(x * 0.5)
    assert torch.equal(gl, el) and torch.equal(gd, ed)
    static_x.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gl, l1) and torch.equal(gd, d1)


@pytest.mark.parametrize("N", NS)
def test_risk_scores_match_golden(z, N):
    for M in MS:
        x = torch.from_numpy(z[f"nll/N{N}_M{M}/logits"]).cuda()
        want = z[f"risk/N{N}_M{M}"]
        got = SV.risk_scores(x)
        assert got.shape == (N,) and got.dtype == torch.float32
        assert _rel(got.cpu().numpy(), want) <= 1e-5, (N, M)
        # a row window of a wider buffer (row stride > M) reads the same rows
        wide = torch.zeros(N, M + 3, device="cuda")
        wide[:, :M] = x
        assert torch.equal(SV.risk_scores(wide[:, :M]), got)


def _cindex_case(n, seed, heavy_ties):
    g = np.random.default_rng(seed)
    event = g.random(n) < 0.6
    time = g.exponential(30.0, n)
    est = g.normal(size=n).astype(np.float32)
    if heavy_ties:
        time = np.round(time / 30.0 * 12.0)                      # rounded months: many equal times
        est = (np.round(est * 4) / 4).astype(np.float32)         # quantised risks: many exact ties
    event[0] = True
    return event, time, est


@pytest.mark.parametrize("n", [2, 37, 1000, 4097])
@pytest.mark.parametrize("heavy_ties", [False, True])
def test_concordance_index_matches_restatement(n, heavy_ties):
    event, time, est = _cindex_case(n, 100 + n, heavy_ties)
    if n == 2:
        time[1] = time[0] + 1.0                                  # one comparable pair
    want = cindex_np(event, time, est)
    got = SV.concordance_index_censored(torch.from_numpy(event).cuda(), torch.from_numpy(time).cuda(), torch.from_numpy(est).cuda(),
                                        tied_tol=1e-8)
    assert tuple(int(v) for v in got[1:]) == want[1:], (got, want)
    assert float(got[0]) == want[0]
    assert got[0].item() == want[0]                              # numpy scalar: train_survival.py:1465 calls .item()
    if heavy_ties and n >= 37:
        assert want[3] > 0 and want[4] > 0                       # the tie paths were exercised


def test_concordance_index_raises_where_the_reference_does():
    t = torch.tensor([1.0, 2.0, 3.0], device="cuda", dtype=torch.float64)
    e = torch.tensor([0.1, 0.5, 0.9], device="cuda")
    with pytest.raises(ValueError, match="censored"):
        SV.concordance_index_censored(torch.zeros(3, dtype=torch.bool, device="cuda"), t, e)
    with pytest.raises(ValueError, match="comparable"):
        SV.concordance_index_censored(torch.tensor([False, False, True], device="cuda"), t, e)


def _f64_nll(logits, t, c, eps=1e-7):
    """losses/nll_surv.py restated in f64 torch (alpha = 0, mean)."""
    N, M = logits.shape
    h = torch.sigmoid(logits).clamp(min=eps, max=1 - eps)
    tr = torch.arange(M, device=logits.device)[None, :]
    tt = t[:, None].long()
    unc, cen = (c == 1)[:, None], (c == 0)[:, None]
    lh, l1 = torch.log(h), torch.log(1 - h)
    u = -((l1 * ((tr < tt) & unc)).sum(1) + (lh * ((tr == tt) & unc)).sum(1))
    ce = -(l1 * ((tr <= tt) & cen)).sum(1)
    return torch.where(unc[:, 0], u, torch.where(cen[:, 0], ce, torch.zeros_like(u))).mean()


def _template_classifier():
    import mirror_amd.models as M
    torch.manual_seed(0)
    model = M.create_model("mirror_classifier", wsi_embed_dim=768, rna_embed_dim=10234, embed_dim=768, num_classes=4,
                           rna_encoder_depth=2, rna_mlp_ratio=4.0, rna_norm_layer="layernorm", rna_act_layer="gelu", fusion="concat")
    # linear probe (train_survival.py:768-775)
    model.head.weight.data.normal_(mean=0.0, std=0.01)
    model.head.bias.data.zero_()
    for _, p in model.named_parameters():
        p.requires_grad = False
    for _, p in model.head.named_parameters():
        p.requires_grad = True
    return model.cuda()


def test_linear_probe_at_the_survival_template_geometry():
    model = _template_classifier()
    model.precision = "fp32"
    model.eval()
    g = torch.Generator().manual_seed(1)
    B = 16
    wsi = torch.randn(B, 2048, 768, generator=g).cuda()
    rna = torch.randn(B, 10234, generator=g).cuda()
    labels = torch.randint(0, 4, (B,), generator=g).to(torch.int32).cuda()
    cens = torch.randint(0, 2, (B,), generator=g).cuda()
    loss = NLLSurvLoss()(model(wsi, rna), labels, cens)
    loss.backward()
    for name, p in model.named_parameters():
        if not name.startswith("head."):
            assert p.grad is None, name
    with torch.no_grad():
        feats = torch.cat((model.wsi_encoder(wsi), model.rna_encoder(rna)), dim=1).double()
    W = model.head.weight.detach().double().requires_grad_(True)
    b = model.head.bias.detach().double().requires_grad_(True)
    ref = _f64_nll(feats @ W.t() + b, labels, cens)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    for got, want in ((model.head.weight.grad, W.grad), (model.head.bias.grad, b.grad)):
        assert _rel(got.double().cpu().numpy(), want.cpu().numpy()) <= 1e-4

    # one bf16-policy train-mode step: finite loss and head gradients
    model.zero_grad(set_to_none=True)
    model.precision = "bf16"
    model.train()
    loss = NLLSurvLoss()(model(wsi, rna).float(), labels, cens)
    loss.backward()
    assert torch.isfinite(loss)
    assert torch.isfinite(model.head.weight.grad).all() and torch.isfinite(model.head.bias.grad).all()
