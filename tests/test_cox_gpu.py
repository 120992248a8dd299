"""MI355X: the Cox partial-likelihood loss and the log-rank test through the C ABI (csrc/cox.hip) against the f64 restatements of
tests/cox_ref.py — parity over the wave / tile edges, tie structures, event fractions and score ranges; the NaN rules;
determinism and graph replay; a Cox linear probe against its f64 host loop; log-rank statistics.

Tolerance of the parity test (derived, not measured): every sum and the log are f64 on both sides (error about N * 1e-16), only
the final store rounds to f32 (6e-8 relative), so |got - want| <= 1e-6 * max(1, |want|) per element."""
import math

import numpy as np
import pytest
import torch

from mirror_amd import survival as SV
from mirror_amd.losses import CoxSurvLoss
from mirror_amd.optim import ArenaOptimizer
from tests import cox_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 64, 65, 255, 256, 257, 513, 1000)
TIMES = ("distinct", "ties", "equal")
FRACS = (0.0, 0.6, 1.0)
SCORES = ("n1", "n3", "u100")
C_DTYPES = (torch.bool, torch.int64, torch.float32)
GS = 0.625          # the scalar upstream gradient


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= 1e-6, (what, worst)
    return worst


def _logits(r: np.ndarray, layout: str) -> torch.Tensor:
    """A leaf holding r: a [N] vector, or an [N, 4] matrix whose column 2 the loss reads in place as [N, 1]."""
    if layout == "vec":
        return torch.from_numpy(r).cuda().requires_grad_(True)
    base = torch.randn(len(r), 4, generator=torch.Generator().manual_seed(len(r)))
    base[:, 2] = torch.from_numpy(r)
    return base.cuda().requires_grad_(True)


def _run(leaf, layout, t, c, ties, red, up):
    """(loss, d(up . loss) / d scores) through CoxSurvLoss."""
    x = leaf if layout == "vec" else leaf[:, 2:3]
    assert layout == "vec" or not x.is_contiguous() or len(x) == 1
    leaf.grad = None
    loss = CoxSurvLoss(ties=ties, reduction=red)(x, t, c)
    (loss * up).sum().backward()
    grad = leaf.grad if layout == "vec" else leaf.grad[:, 2]
    if layout != "vec":
        other = leaf.grad[:, [0, 1, 3]]
        assert not other.any()
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("times", TIMES)
@pytest.mark.parametrize("N", NS)
def test_loss_and_gradient_match_f64_restatement(N, times):
    worst, combo = 0.0, 0
    for fi, frac in enumerate(FRACS):
        for si, scores in enumerate(SCORES):
            r, t, c = R.make_case(N, times, frac, scores, 7000 + 10 * N + 3 * fi + si)
            up = np.random.RandomState(N + combo).uniform(-0.5, 1.5, N).astype(np.float32)
            nev = max(int((c == 1).sum()), 1)
            for ties in R.TIES:
                # the restatement once per input: per-row losses, the gradient for ones and for the per-row weights; the
                # reduced forms follow by linearity
                rows, g_one = R.cox_pair(r, t, c, ties, "none")
                _, g_up = R.cox_pair(r, t, c, ties, "none", up.astype(np.float64))
                assert np.isfinite(rows).all() and np.isfinite(g_one).all()
                layout = ("vec", "col")[combo % 2]
                cdt = C_DTYPES[combo % 3]
                combo += 1
                leaf = _logits(r, layout)
                tt = torch.from_numpy(t).cuda() if combo % 4 else torch.from_numpy(t.astype(np.float32)).cuda()
                cc = torch.from_numpy(c).cuda().to(cdt)
                t_ref = t if combo % 4 else t.astype(np.float32).astype(np.float64)
                if not np.array_equal(t_ref, t):         # f32 times (rounded, maybe newly tied) are other inputs
                    rows, g_one = R.cox_pair(r, t_ref, c, ties, "none")
                    _, g_up = R.cox_pair(r, t_ref, c, ties, "none", up.astype(np.float64))
                for red, coef in (("none", None), ("sum", 1.0), ("mean", 1.0 / nev), ("batch", 1.0 / N)):
                    what = (N, times, frac, scores, ties, red, layout, str(cdt))
                    if red == "none":
                        loss, grad = _run(leaf, layout, tt, cc, ties, red, torch.from_numpy(up).cuda())
                        worst = max(worst, _close(loss, rows, what), _close(grad, g_up, what))
                        loss1, grad1 = _run(leaf, layout, tt, cc, ties, red, 1.0)
                        worst = max(worst, _close(loss1, rows, what), _close(grad1, g_one, what))
                    else:
                        loss, grad = _run(leaf, layout, tt, cc, ties, red, GS)
                        worst = max(worst, _close(loss, coef * rows.sum(), what), _close(grad, coef * GS * g_one, what))
                    if frac == 0.0:
                        assert not np.any(loss) and not np.any(grad), what
    print(f"cox parity N={N} {times}: largest |got - want| / max(1, |want|) = {worst:.3e}")


def test_integer_times_and_int32_uint8_censoring():
    r, t, c = R.make_case(300, "ties", 0.6, "n1", 21)
    rows, grad = R.cox_pair(r, t, c, "efron", "none")
    for tdt, cdt in ((torch.int64, torch.int32), (torch.int32, torch.uint8), (torch.float64, torch.int64)):
        leaf = _logits(r, "vec")
        got, dgot = _run(leaf, "vec", torch.from_numpy(t).cuda().to(tdt), torch.from_numpy(c).cuda().to(cdt), "efron", "none", 1.0)
        _close(got, rows, (tdt, cdt))
        _close(dgot, grad, (tdt, cdt))
    # anything but 1 is censored
    c2 = np.where(c == 1, 1, 2)
    got, _ = _run(_logits(r, "vec"), "vec", torch.from_numpy(t).cuda(), torch.from_numpy(c2).cuda(), "efron", "none", 1.0)
    _close(got, rows, "censoring 2")


def test_nan_time_and_nan_logit_follow_the_edge_rules():
    N, bad = 300, 77
    r, t, c = R.make_case(N, "ties", 0.6, "n1", 22)
    c[bad] = 1
    t2 = t.copy()
    t2[bad] = np.nan
    keep = np.arange(N) != bad
    for ties in R.TIES:
        rows, grad = R.cox_pair(r, t2, c, ties, "none")
        assert np.isnan(rows[bad]) and np.isfinite(rows[keep]).all()
        loss = CoxSurvLoss(ties=ties, reduction="none")
        leaf = _logits(r, "vec")
        got = loss(leaf, torch.from_numpy(t2).cuda(), torch.from_numpy(c).cuda())
        got.sum().backward()
        got, dgot = got.detach().cpu().numpy(), leaf.grad.cpu().numpy()
        assert np.isnan(got[bad]) and np.isnan(dgot[bad])
        _close(got[keep], rows[keep], "nan time rows")
        _close(dgot[keep], grad[keep], "nan time grad")
        # the row is in no other row's risk set: the others are what they are without it
        rows_k, _ = R.cox_pair(r[keep], t[keep], c[keep], ties, "none")
        _close(got[keep], rows_k, "nan time: row removed")
        assert math.isnan(float(CoxSurvLoss(ties=ties)(_logits(r, "vec"), torch.from_numpy(t2).cuda(), torch.from_numpy(c).cuda()).detach()))
    # a NaN logit propagates
    r2 = r.copy()
    r2[bad] = np.nan
    leaf = _logits(r2, "vec")
    out = CoxSurvLoss()(leaf, torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda())
    out.backward()
    assert math.isnan(float(out.detach())) and bool(torch.isnan(leaf.grad[bad]))


def test_wide_scores_come_back_finite_where_the_f32_matrix_form_overflows():
    r, t, c = R.make_case(513, "ties", 0.6, "u100", 23)
    x, tt, cc = torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda()
    naive = (torch.exp(x)[None, :] * (tt[None, :] >= tt[:, None])).sum(1)          # exp(theta) * R_mat in f32
    assert not bool(torch.isfinite(naive).all())
    leaf = x.clone().requires_grad_(True)
    loss = CoxSurvLoss()(leaf, tt, cc)
    loss.backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(leaf.grad).all())


def _step(r, t, c, ties="efron", red="mean"):
    leaf = r.detach().clone().requires_grad_(True)
    loss = CoxSurvLoss(ties=ties, reduction=red)(leaf, t, c)
    (grad,) = torch.autograd.grad(loss.sum(), leaf)
    return loss.detach(), grad


def test_two_runs_are_bit_equal():
    r, t, c = R.make_case(1000, "ties", 0.6, "n3", 24)
    x, tt, cc = torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda()
    for ties in R.TIES:
        for red in R.REDUCTIONS:
            a, b = _step(x, tt, cc, ties, red), _step(x, tt, cc, ties, red)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replay_equals_eager_after_the_inputs_change_in_place():
    N = 257
    r, t, c = R.make_case(N, "ties", 0.6, "n1", 25)
    r2, t2, c2 = R.make_case(N, "distinct", 0.3, "n3", 26)
    assert int((c == 1).sum()) != int((c2 == 1).sum())
    sr, st, sc = torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda()
    first = _step(sr, st, sc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(sr, st, sc)                                # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = _step(sr, st, sc)
    sr.copy_(torch.from_numpy(r2))
    st.copy_(torch.from_numpy(t2))
    sc.copy_(torch.from_numpy(c2))
    g.replay()
    torch.cuda.synchronize()
    eager = _step(torch.from_numpy(r2).cuda(), torch.from_numpy(t2).cuda(), torch.from_numpy(c2).cuda())
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
    want, dwant = R.cox_pair(r2, t2, c2, "efron", "mean")
    _close(captured[0].cpu().numpy(), want, "replayed loss")
    _close(captured[1].cpu().numpy(), dwant, "replayed gradient")
    sr.copy_(torch.from_numpy(r))
    st.copy_(torch.from_numpy(t))
    sc.copy_(torch.from_numpy(c))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], first[0]) and torch.equal(captured[1], first[1])


def test_cox_linear_probe_tracks_its_f64_host_loop():
    """A Linear(64, 1) head on synthetic embeddings (N = 512, exponential times from a planted beta, about 30 % censored), full-batch
    Adam steps under CoxSurvLoss; step count and lr were chosen on the host with the f64 loop of cox_ref.probe_loop_f64."""
    want_loss, want_ci = R.probe_loop_f64()
    x, t, event, w0, b0 = R.probe_problem()
    assert 0.2 < 1.0 - event.mean() < 0.4
    head = torch.nn.Linear(R.PROBE["D"], 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(w0))
        head.bias.copy_(torch.from_numpy(b0))
    head = head.cuda()
    X, T, C = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(event).cuda()
    opt = ArenaOptimizer(list(head.parameters()), opt="adam", lr=R.PROBE["lr"], precision="fp32")
    loss_fn = CoxSurvLoss(ties="efron", reduction="mean")
    for _ in range(R.PROBE["steps"]):
        opt.zero_grad()
        loss_fn(head(X), T, C).backward()
        opt.step()
    with torch.no_grad():
        scores = head(X)
        got_loss = float(loss_fn(scores, T, C))
        got_ci = float(SV.concordance_index_censored(C == 1, T, scores.reshape(-1))[0])
    print(f"cox probe: loss {got_loss:.6f} (f64 loop {want_loss:.6f}), c-index {got_ci:.4f} (f64 loop {want_ci:.4f})")
    assert want_ci > 0.7                                   # the planted signal was learned
    assert abs(got_loss - want_loss) <= 1e-3 * abs(want_loss)
    assert abs(got_ci - want_ci) <= 0.01


def _logrank_case(N, seed):
    rng = np.random.RandomState(seed)
    if N == 2:
        return np.array([True, True]), np.array([1.0, 2.0]), np.array([False, True])
    grp = rng.uniform(size=N) < 0.45
    t = rng.randint(0, 12, N).astype(np.float64) + 2.0 * grp * (rng.uniform(size=N) < 0.5)
    return rng.uniform(size=N) < 0.7, t, grp


@pytest.mark.parametrize("N", [2, 65, 257, 1000])
def test_logrank_matches_restatement(N):
    ev, t, grp = _logrank_case(N, 300 + N)
    chi2, p, O1, E1, V, nev = R.logrank(ev, t, grp)
    for e_t, t_t, g_t in ((torch.from_numpy(ev).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(grp).cuda()),
                          (torch.from_numpy(ev.astype(np.int64)).cuda(), torch.from_numpy(t.astype(np.int64) if N == 2 else t).cuda(),
                           torch.from_numpy(grp.astype(np.float32)).cuda())):
        got = SV.logrank_test(e_t, t_t, g_t)
        assert all(isinstance(v, float) for v in got) and len(got) == 5
        stats = SV.K.logrank_stats(torch.from_numpy(ev).cuda().view(torch.uint8), torch.from_numpy(t).cuda(),
                                   torch.from_numpy(grp).cuda().view(torch.uint8)).cpu().numpy()
        assert stats[0] == O1 and stats[3] == nev              # exact
        assert got[2] == O1
        assert got[3] == pytest.approx(E1, rel=1e-10) and got[4] == pytest.approx(V, rel=1e-10)
        assert got[0] == pytest.approx(chi2, rel=1e-10)
        assert abs(got[1] - p) <= 1e-9


def test_logrank_degenerate_inputs_raise_and_median_split():
    t = torch.arange(1.0, 9.0).cuda()
    grp = (torch.arange(8) % 2 == 1).cuda()
    with pytest.raises(ValueError):                         # no events
        SV.logrank_test(torch.zeros(8, dtype=torch.bool).cuda(), t, grp)
    with pytest.raises(ValueError):                         # group 1 empty at every event time
        SV.logrank_test(torch.ones(8, dtype=torch.bool).cuda(), t, torch.zeros(8, dtype=torch.bool).cuda())
    with pytest.raises(ValueError):                         # group 0 empty
        SV.logrank_test(torch.ones(8, dtype=torch.bool).cuda(), t, torch.ones(8, dtype=torch.bool).cuda())
    ev, tm, _ = _logrank_case(257, 9)
    risk = np.random.RandomState(10).normal(size=257).astype(np.float32) - 0.2 * tm.astype(np.float32)
    e_t, t_t, r_t = torch.from_numpy(ev).cuda(), torch.from_numpy(tm).cuda(), torch.from_numpy(risk).cuda()
    split = r_t > r_t.median()
    assert SV.logrank_by_median(e_t, t_t, r_t) == SV.logrank_test(e_t, t_t, split)
    want = R.logrank(ev, tm, risk > np.sort(risk)[(257 - 1) // 2])
    assert SV.logrank_by_median(e_t, t_t, r_t)[0] == pytest.approx(want[0], rel=1e-10)
