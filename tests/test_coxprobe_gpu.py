"""MI355X: the ridge Cox probe (csrc/coxprobe.hip, the step in csrc/linprobe.hip, mirror_amd/coxprobe.py) against the float64
restatement of tests/coxprobe_ref.py.

Each kernel is compared on what the device itself handed to it (mh_coxprobe_grad gets the device's own V, mh_coxprobe_step the device's
own G, the end-to-end checks the device's own prepared rows and weights), so a kernel's tolerance is that kernel's rounding, derived
from the number formats:

  scores       delta[i, j] = 2 D 2^-24 |y_i| |w_j|: the k-ordered f32 chain of the tile product (D roundings of partial sums that stay
               below |y_i| |w_j|, with a factor 2 to spare).  The chain is the retrieval kernels': mh_retrieval_topk hands its values
               out (`val` is "the f32 fmaf chain, bit for bit"), so for up to 64 keys at a time the equality is shown bit for bit.
               mh_survprobe_risk / mh_linprobe_proba run the same retr_product but never store a raw logit.
  gradient     every sum, exp and log of mh_coxprobe_grad is f64 and only the store rounds to f32, so nothing is measured:
               |G - G_ref| <= 2^-24 |G_ref| + n 2^-45 r_j per element (one f32 rounding of the result; n f64 roundings, 2^-53 each,
               of sums whose terms w_k q_i are O(1), with 2^8 to spare), |loss - ref| <= n 2^-45 r_j sum_i |term_i|.
               Against float64 scores of float64 weights the allowance grows by (e^{2 delta_j} - 1) r_j w_k sum_i q_i: a score
               moves by delta at the most, so every ratio w_k / den_i moves by a factor e^{+-2 delta} at the most; the loss by
               2 delta_j r_j n_events_j (log den_i - v_i is 1-Lipschitz in each of the two).
  weight sums  as tests/test_linprobe_gpu.py derives them: B[j, d] = n 2^-24 sum_i |G[i, j]| |y[i, d]|, one row-ordered f32 chain of
               n terms, carried through the update with 2^-24 of each of its four results.

mh_coxprobe_grad gives thread t of its 256 the rows [t c, (t + 1) c) with c = ceil(n / 256): the per-thread chunk grows by one at
every multiple of the block width, so n = 255, 256, 257 and 511, 512, 513 stand one below, at and one above both; at n = 1025
(c = 5) the last 51 threads own nothing.
"""
import numpy as np
import pytest
import torch

from mirror_amd import CoxProbe, kernels as K
from mirror_amd.linprobe import fista_betas
from tests import coxprobe_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # half an ulp of a number in [1, 2)
U64 = 2.0 ** -45          # 2^8 f64 roundings per row
SCORE_CASES = [(1, 1, 1), (127, 3, 33), (128, 16, 128), (129, 17, 129), (300, 40, 5)]                    # nq, D, J
GRAD_N = [1, 2, 255, 256, 257, 511, 512, 513, 1025]
GRAD_J = [1, 5, 130]
PATTERNS = ["distinct", "ints", "equal"]
STEP_CASES = [(1, 1, 1), (129, 127, 3), (300, 128, 130), (257, 129, 5)]                                  # n, D, J


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ 1. mh_coxprobe_scores
def score_case(nq, D, J):
    rng = np.random.default_rng(1000 * nq + 10 * D + J)
    y = rng.standard_normal((nq, D))
    y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    w = rng.standard_normal((J, D))
    W = (w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0, 10, (J, 1))).astype(np.float32)
    return y, W


@pytest.mark.parametrize("shape", SCORE_CASES, ids=lambda s: "nq%d-D%d-J%d" % s)
def test_scores_against_float64_and_the_retrieval_chain(shape):
    nq, D, J = shape
    y, W = score_case(*shape)
    yd, Wd = dev(y), dev(W)
    V = torch.full((J, nq), float("nan"), device="cuda")
    out = K.coxprobe_scores(yd, Wd, V=V)
    assert out is V and not torch.isnan(V).any()                               # STORED: every sentinel is gone
    got = host(V).astype(np.float64)
    ref = W.astype(np.float64) @ y.astype(np.float64).T
    delta = 2 * D * U * np.linalg.norm(W.astype(np.float64), axis=1)[:, None] * np.linalg.norm(y.astype(np.float64), axis=1)[None, :]
    print(f"{shape}: |V - V_ref| / delta <= {(np.abs(got - ref) / np.maximum(delta, 1e-300)).max():.3f}")
    assert (np.abs(got - ref) <= delta).all()
    assert torch.equal(K.coxprobe_scores(yd, Wd), V)                           # allocated by the launcher: the same bits
    # bit for bit the retrieval kernels' chain, 64 keys at a time
    for a in range(0, J, 64):
        kk = min(64, J - a)
        val, idx = K.retrieval_topk(yd, Wd[a:a + kk].contiguous(), kk)
        back = torch.empty((nq, kk), device="cuda")
        back.scatter_(1, idx.long(), val)
        assert torch.equal(back.t().contiguous(), V[a:a + kk])
    # and it does not depend on where a row or a key falls in a tile
    if nq > 3 and J > 2:
        sub = K.coxprobe_scores(yd[3:].contiguous(), Wd[2:].contiguous())
        assert torch.equal(sub, V[2:, 3:])


# ------------------------------------------------------------------ 2. mh_coxprobe_grad
def grad_case(n, J, pattern, seed=0, scale=1.0):
    """Scores N(0, scale) f32 [J, n], times in non-increasing order, events in {0, 1, 2}, folds in [-1, 2], heldout in [-1, 2];
    (row 0, job 0) is a training event, also at n = 1."""
    rng = np.random.default_rng(100000 * seed + 100 * n + J)
    time = {"distinct": lambda: np.sort(rng.random(n) * 10.0)[::-1].copy(),
            "ints": lambda: np.sort(rng.integers(0, 8, n))[::-1].astype(np.float64),
            "equal": lambda: np.full(n, 2.5)}[pattern]()
    V = (rng.standard_normal((J, n)) * scale).astype(np.float32)
    event = rng.choice(np.array([0, 1, 1, 2], dtype=np.uint8), n)
    fold = rng.integers(-1, 3, n).astype(np.int32)
    held = rng.integers(-1, 3, J).astype(np.int32)
    event[0], fold[0], held[0] = 1, 0, -1
    return finish(dict(n=n, J=J, V=V, time=time, event=event, fold=fold, held=held))


def finish(c):
    ntrain = np.array([R.train_mask(c["event"], c["time"], c["fold"], h).sum() for h in c["held"]])
    c["r"] = np.where(ntrain > 0, 1.0 / np.maximum(ntrain, 1), 0.0).astype(np.float32)
    c["ntrain"] = ntrain
    return c


def run_grad(c, ties, V=None):
    n, J = c["n"], c["J"]
    G = torch.full((n, J), float("nan"), device="cuda")
    loss = torch.full((J,), float("nan"), device="cuda", dtype=torch.float64)
    out = K.coxprobe_grad(dev(c["V"]) if V is None else V, dev(c["time"]), dev(c["event"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]),
                          ties, G=G, loss=loss)
    assert out[0] is G and out[1] is loss
    return G, loss


def grad_reference(c, ties, V=None):
    """(G_ref [n, J], loss_ref [J], mask [n, J], abs_loss [J], wq [n, J]) in float64 from the f32 scores."""
    n, J = c["n"], c["J"]
    V = c["V"] if V is None else V
    G, wq, mask = np.zeros((n, J)), np.zeros((n, J)), np.zeros((n, J), dtype=bool)
    loss, absl = np.zeros(J), np.zeros(J)
    for j in range(J):
        mask[:, j] = R.train_mask(c["event"], c["time"], c["fold"], c["held"][j])
        f = R.scan(V[j].astype(np.float64), c["time"], c["event"], mask[:, j], ties, float(c["r"][j]), full=True)
        G[:, j], loss[j], absl[j], wq[:, j] = f["g"], f["loss"], f["abs_loss"], f["wq"]
    return G, loss, mask, absl, wq


def check_grad(c, ties, G, loss, tag, extra_g=0.0, extra_l=0.0):
    """The derived bound, the exact zeros off the training rows and the column sums; returns the reference."""
    n = c["n"]
    Gr, lr, mask, absl, wq = grad_reference(c, ties)
    got, gl = host(G).astype(np.float64), host(loss)
    r = c["r"].astype(np.float64)
    tol = U * np.abs(Gr) + n * U64 * r[None, :] + extra_g
    ltol = n * U64 * absl + extra_l
    assert (got[~mask] == 0).all() and not np.signbit(got[~mask]).any()         # exactly +0 off the training rows, over the NaN sentinels
    assert not np.isnan(got).any() and not np.isnan(gl).any()
    eg = np.abs(got - Gr)
    print(f"{tag}: |G - G_ref| / tol <= {(eg / np.maximum(tol, 1e-300)).max():.3f} (|G_ref| up to {np.abs(Gr).max():.2e}), "
          f"|loss - ref| / tol <= {(np.abs(gl - lr) / np.maximum(ltol, 1e-300)).max():.3f}")
    assert (eg <= tol).all(), (tag, np.unravel_index(np.argmax(eg - tol), eg.shape))
    assert (np.abs(gl - lr) <= ltol).all(), (tag, gl, lr)
    assert (gl[absl == 0] == 0).all()                                           # no training event: exactly 0
    # the partial likelihood does not see a shift of the scores: a job's column sums to 0 within the roundings of its elements
    assert (np.abs(got.sum(0)) <= tol.sum(0)).all()
    return Gr, lr, mask


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", GRAD_N)
def test_grad_against_float64_scan_of_the_same_scores(n, pattern):
    for J in GRAD_J:
        c = grad_case(n, J, pattern)
        Vd = dev(c["V"])
        for ties in R.TIES:
            G, loss = run_grad(c, ties, Vd)
            check_grad(c, ties, G, loss, f"n {n} J {J} {pattern} {ties}")
            G2, loss2 = run_grad(c, ties, Vd)                                   # two launches: the same bits
            assert torch.equal(G, G2) and torch.equal(loss, loss2)


def test_grad_from_device_scores_against_float64_weights():
    """scores then grad on the device against float64 scores of the float64 weights: the allowance of the docstring."""
    for (n, D, J), pattern in (((300, 40, 5), "ints"), ((129, 17, 129), "distinct")):
        y, W = score_case(n, D, J)
        W = (W * 0.5).astype(np.float32)
        c = grad_case(n, J, pattern, seed=1)
        Vd = K.coxprobe_scores(dev(y), dev(W))
        c64 = dict(c, V=W.astype(np.float64) @ y.astype(np.float64).T)
        delta = 2 * D * U * np.linalg.norm(W.astype(np.float64), axis=1) * np.linalg.norm(y.astype(np.float64), axis=1).max()      # [J]
        for ties in R.TIES:
            G, loss = run_grad(c, ties, Vd)
            _, _, mask, _, wq = grad_reference(c64, ties)
            nev = np.array([(mask[:, j] & (c["event"] == 1)).sum() for j in range(J)])
            check_grad(c64, ties, G, loss, f"n {n} D {D} J {J} {pattern} {ties} (f64 weights)", extra_g=np.expm1(2 * delta)[None, :] * wq,
                       extra_l=2 * delta * c["r"] * nev)


def edge(n, J, pattern, **over):
    c = grad_case(n, J, pattern, seed=2)
    c.update(over)
    return finish(c)


def test_grad_job_without_a_training_row():
    n = 300
    c = edge(n, 3, "ints", fold=np.ones(n, dtype=np.int32), held=np.array([1, -1, 0], dtype=np.int32))
    assert c["ntrain"][0] == 0 and c["r"][0] == 0 and c["ntrain"][1] > 0
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        check_grad(c, ties, G, loss, f"no training row, {ties}")
        assert (host(G)[:, 0] == 0).all() and float(loss[0]) == 0.0


def test_grad_job_with_one_training_row():
    n = 300
    fold = np.full(n, -1, dtype=np.int32)
    fold[137] = 0
    event = np.ones(n, dtype=np.uint8)
    c = edge(n, 2, "ints", fold=fold, event=event, held=np.array([-1, 1], dtype=np.int32))
    assert (c["ntrain"] == 1).all() and (c["r"] == 1).all()
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        check_grad(c, ties, G, loss, f"one training row, {ties}")
        assert (host(G) == 0).all() and (host(loss) == 0).all()                # den = w = 1: log 1 + m - v = 0, g = 1 * 1 - 1 = 0


def test_grad_job_with_training_rows_but_no_event():
    n = 300
    c = grad_case(n, 3, "ints", seed=3)
    event = c["event"].copy()
    event[c["fold"] != 1] = np.minimum(event[c["fold"] != 1], 0) + 2 * (event[c["fold"] != 1] == 2)      # events only in fold 1
    c = edge(n, 3, "ints", event=event, fold=c["fold"], held=np.array([1, -1, 0], dtype=np.int32))
    assert c["ntrain"][0] > 10
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        _, _, mask = check_grad(c, ties, G, loss, f"no training event, {ties}")
        assert not (mask[:, 0] & (c["event"] == 1)).any() and (host(G)[:, 0] == 0).all() and float(loss[0]) == 0.0
        assert (host(G)[:, 1] != 0).any()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_grad_every_row_an_event(pattern):
    n = 513
    c = edge(n, 2, pattern, event=np.ones(n, dtype=np.uint8), fold=np.zeros(n, dtype=np.int32), held=np.array([-1, 1], dtype=np.int32))
    assert (c["ntrain"] == n).all()
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        check_grad(c, ties, G, loss, f"every row an event, {pattern}, {ties}")


def test_grad_score_spread_of_600():
    n = 513
    c = grad_case(n, 5, "ints", seed=4)
    rng = np.random.default_rng(9)
    V = rng.uniform(-300.0, 300.0, (5, n)).astype(np.float32)
    V[:, 0], V[:, 1] = 300.0, -300.0
    c = finish(dict(c, V=V))
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        check_grad(c, ties, G, loss, f"spread 600, {ties}")


def test_grad_nan_score_off_the_training_rows_leaves_the_job_exact():
    n = 300
    c = grad_case(n, 5, "ints", seed=5)
    mask = np.stack([R.train_mask(c["event"], c["time"], c["fold"], h) for h in c["held"]])            # [J, n]
    assert (~mask).sum(1).min() > 0
    V = c["V"].copy()
    V[~mask] = np.nan                                                           # every score a job does not train on
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        Gn, ln = run_grad(c, ties, dev(V))
        assert torch.equal(G, Gn) and torch.equal(loss, ln) and not torch.isnan(Gn).any()


def test_grad_nan_score_on_a_training_row_poisons_only_its_job():
    n = 300
    c = grad_case(n, 5, "ints", seed=6)
    mask = np.stack([R.train_mask(c["event"], c["time"], c["fold"], h) for h in c["held"]])
    V = c["V"].copy()
    row = int(np.flatnonzero(mask[2])[7])
    V[2, row] = np.nan
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        Gn, ln = run_grad(c, ties, dev(V))
        g, gn = host(G), host(Gn)
        others = [0, 1, 3, 4]
        assert np.array_equal(g[:, others], gn[:, others]) and np.array_equal(host(loss)[others], host(ln)[others])
        assert np.isnan(gn[mask[2], 2]).all() and (gn[~mask[2], 2] == 0).all() and np.isnan(host(ln)[2])


def test_grad_nan_time_trains_nowhere_and_is_in_no_risk_set():
    n = 300
    c = grad_case(n, 5, "ints", seed=7)
    time = c["time"].copy()
    time[-2:] = np.nan                                                          # NaN times come last, each a group of its own
    event = c["event"].copy()
    event[-2:] = 1
    fold = c["fold"].copy()
    fold[-2:] = 0
    c = finish(dict(c, time=time, event=event, fold=fold))
    short = finish({k: (v[:-2] if k in ("time", "event", "fold") else v[:, :-2] if k == "V" else v) for k, v in c.items()} | dict(n=n - 2))
    assert np.array_equal(c["ntrain"], short["ntrain"])
    for ties in R.TIES:
        G, loss = run_grad(c, ties)
        check_grad(c, ties, G, loss, f"NaN time, {ties}")
        assert (host(G)[-2:] == 0).all()
        Gs, ls, _, _, _ = grad_reference(short, ties)                           # the same job without the two rows
        Gr, lr, _, _, _ = grad_reference(c, ties)
        assert np.array_equal(Gr[:-2], Gs) and np.array_equal(lr, ls)


# ------------------------------------------------------------------ 3. mh_coxprobe_step
def chain_bound(G, y):
    """B [J, D] = n 2^-24 sum_i |G[i, j]| |y[i, d]|."""
    return len(y) * U * (np.abs(G).T @ np.abs(y))


def fenced(a):
    """A device copy of a [J, D] inside NaN sentinel rows: (the whole buffer, the [J, D] view)."""
    J, D = a.shape
    buf = torch.full((J + 2, D), float("nan"), device="cuda")
    buf[1:J + 1] = dev(a)
    return buf, buf[1:J + 1]


def fence_ok(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("shape", STEP_CASES, ids=lambda s: "n%d-D%d-J%d" % s)
def test_step_against_float64_and_bit_for_bit_against_gsel_step(shape):
    n, D, J = shape
    rng = np.random.default_rng(7 + n)
    y, _ = score_case(n, D, 1)
    c = grad_case(n, J, "ints", seed=8)
    Gd, _ = run_grad(c, "efron")
    yd = dev(y)
    G, y64 = host(Gd).astype(np.float64), y.astype(np.float64)
    full = G.T @ y64                                                            # [J, D]: the weight gradient without the penalty
    B = chain_bound(G, y64)
    lam = rng.uniform(1e-3, 0.1, J).astype(np.float32)
    tiles = (D + 1 + 127) // 128

    # (a) Wz = 0, eta = 1, beta = 0: Wx becomes minus the chain, exactly
    ones = torch.ones((J,), device="cuda")
    bx, Wx = fenced(np.zeros((J, D), dtype=np.float32))
    bz, Wz = fenced(np.zeros((J, D), dtype=np.float32))
    gm = K.coxprobe_step(yd, Gd, Wx, Wz, dev(lam), ones, 0.0, want_gmax=True)
    assert tuple(gm.shape) == (tiles, J) and fence_ok(bx) and fence_ok(bz)
    got = -host(Wx).astype(np.float64)
    print(f"{shape}: dW err / bound <= {(np.abs(got - full) / np.maximum(B, 1e-300)).max():.3f} (bound up to {B.max():.2e})")
    assert (np.abs(got - full) <= B).all() and torch.equal(Wx, Wz)              # beta = 0: Z' = X'
    assert (np.abs(host(gm.amax(0)) - np.abs(full).max(1)) <= B.max(1)).all()

    # (b) a general state, beta = 0.5
    beta = 0.5
    eta = rng.uniform(0.5, 1.0, J).astype(np.float32)
    X0, Z0 = rng.standard_normal((J, D)).astype(np.float32), rng.standard_normal((J, D)).astype(np.float32)
    bx, Wx = fenced(X0)
    bz, Wz = fenced(Z0)
    gmax = torch.full((tiles, J), float("nan"), device="cuda")
    K.coxprobe_step(yd, Gd, Wx, Wz, dev(lam), dev(eta), beta, gmax_part=gmax)
    assert fence_ok(bx) and fence_ok(bz) and not torch.isnan(gmax).any()
    lamk, etak = lam.astype(np.float64)[:, None], eta.astype(np.float64)[:, None]
    Zf, Xf = Z0.astype(np.float64), X0.astype(np.float64)
    g = full + lamk * Zf
    Xn = Zf - etak * g
    Zn = Xn + beta * (Xn - Xf)
    tg = B + U * (np.abs(g) + B)                                                # each rounding is of the DEVICE's value: |ref| + its error
    tX = etak * tg + U * (np.abs(Xn) + etak * tg)
    td = tX + U * (np.abs(Xn - Xf) + tX)                                        # X' - X, X exact
    tZ = tX + beta * td + U * (np.abs(Zn) + tX + beta * td)
    gotX, gotZ = host(Wx).astype(np.float64), host(Wz).astype(np.float64)
    print(f"{shape}: X' err / tol <= {(np.abs(gotX - Xn) / tX).max():.3f}, Z' err / tol <= {(np.abs(gotZ - Zn) / tZ).max():.3f}")
    assert (np.abs(gotX - Xn) <= tX).all() and (np.abs(gotZ - Zn) <= tZ).all()
    assert (np.abs(host(gmax.amax(0)) - np.abs(g).max(1)) <= tg.max(1)).all()

    # (c) the same bits as mh_gsel_step at C = 2 with a zero second key, a mask of ones and no intercept
    G2 = torch.zeros((n, 2 * J), device="cuda")
    G2[:, 0::2] = Gd
    Wx2, Wz2 = torch.zeros((J, 2, D), device="cuda"), torch.zeros((J, 2, D), device="cuda")
    Wx2[:, 0], Wz2[:, 0] = dev(X0), dev(Z0)
    b2x, b2z = torch.zeros((J, 2), device="cuda"), torch.zeros((J, 2), device="cuda")
    gm2 = K.gsel_step(yd, G2, Wx2, b2x, Wz2, b2z, dev(lam), dev(eta), beta, torch.ones((J, D), device="cuda", dtype=torch.uint8), False, 2,
                      want_gmax=True)
    assert torch.equal(Wx2[:, 0], Wx) and torch.equal(Wz2[:, 0], Wz) and torch.equal(gm2, gmax)
    assert not Wx2[:, 1].any() and not Wz2[:, 1].any() and not b2x.any() and not b2z.any()


# ------------------------------------------------------------------ 4. end to end
def pair_tables(ev, t, r):
    """(comparable [i, j], r_j - r_i) in float64: i has the event and j outlives it."""
    same = t[None, :] == t[:, None]
    comp = ev[:, None] & ((t[None, :] > t[:, None]) | (same & ~ev[None, :]))
    return comp, r[None, :] - r[:, None]


@pytest.fixture(scope="module")
def case():
    x, event, time, fold = R.e2e_case()
    perm = R.sort_rows(time)
    return dict(x=x, event=event, time=time, fold=fold, perm=perm)


def fit(case, ties="efron", **kw):
    c = R.E2E
    train_rows = kw.pop("train_rows", None)
    p = CoxProbe(**{**dict(strengths=c["strengths"], ties=ties, max_iter=c["steps"], tol=0.0, device="cuda"), **kw})
    return p.fit(dev(case["x"]), dev(case["event"]), dev(case["time"]), dev(case["fold"]), train_rows=train_rows)


@pytest.mark.parametrize("ties", R.TIES)
def test_fit_end_to_end(case, ties):
    """The input condition (no comparable pair with a float64 risk gap near the f32 score tolerance) is checked on the CPU from float64
    alone: tests/test_coxprobe_cpu.py::test_end_to_end_inputs_are_decided_in_float64."""
    c, perm = R.E2E, case["perm"]
    F, S, D, k = c["F"], len(c["strengths"]), c["D"], c["steps"]
    J = (F + 1) * S
    p = fit(case, ties)
    assert p.n_iter_ == k and tuple(p.coef_.shape) == (J, D) and p.coef_.dtype == torch.float32
    assert p.loss_.dtype == torch.float64 and tuple(p.loss_.shape) == (J,) and tuple(p.grad_inf_.shape) == (J,)
    assert np.array_equal(host(p._perm), perm)                                  # time descending and stable, the NaN time last
    event, time, fold = case["event"][perm], case["time"][perm], case["fold"][perm]
    assert np.isnan(time[-1]) and np.array_equal(host(p._time)[:-1], time[:-1]) and np.array_equal(host(p._event), event == 1)
    y = host(p._y).astype(np.float64)                                           # the device's own prepared rows, sorted
    y_ref, _ = R.prepare(case["x"], case["x"])
    assert np.abs(y - y_ref[perm]).max() <= 1e-6
    W = host(p.coef_).astype(np.float64)
    held, lam = R.jobs(F, c["strengths"])
    masks = [R.train_mask(event, time, fold, h) for h in held]
    assert np.array_equal(host(p.n_train_), [m.sum() for m in masks]) and p.n_train_.dtype == torch.int64
    assert np.array_equal(host(p.n_events_), [(m & (event == 1)).sum() for m in masks])
    assert masks[-1].sum() == int((fold >= 0).sum()) - 2                        # the event of 2 and the NaN time train nowhere
    ymax = np.linalg.norm(y, axis=1).max()
    w64 = {}
    for j in range(J):
        ws, Fs = R.optimum(y, time, event, masks[j], lam[j], ties)
        nev, nt = R.counts_of(event, masks[j])
        L = R.lipschitz(y, lam[j], nev, nt)
        bound = 2.0 * L * float(ws @ ws) / (k + 1) ** 2
        delta = 2 * D * U * ymax * np.linalg.norm(W[j])
        ltol = 2 * delta * nev / nt + 1e-12                                     # the scores' f32 chain; 1e-12: the f64 sums on both sides
        Fj = R.objective(W[j], y, time, event, masks[j], lam[j], ties)
        got = float(p.loss_[j])
        print(f"{ties} job {j} (lambda {lam[j]:g}, holds out {held[j]}): loss_ = {got:.9f}, F64 = {Fj:.9f}, F* = {Fs:.9f}, "
              f"bound {bound:.2e}, f32 tolerance {ltol:.2e}, max |v| = {np.abs(y @ W[j]).max():.1f}, top L = {L:.4f}")
        assert abs(got - Fj) <= ltol
        assert Fs - 1e-12 <= Fj <= Fs + bound + ltol
        w64[j] = R.fista(y, time, event, masks[j], lam[j], ties, k)

    out = p.evaluate()
    counts, per_job = host(out["counts"]), host(out["per_job"])
    assert counts.shape == (F, S, 5) and counts.dtype == np.int64 and per_job.shape == (F, S) and per_job.dtype == np.float64
    assert out["coxprobe_folds"] == F and out["coxprobe_n"] == int((fold >= 0).sum()) and out["coxprobe_strengths"] == c["strengths"]
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        ev, t = event[rows] == 1, time[rows]
        risks = host(K.coxprobe_scores(p._y.index_select(0, dev(rows)), p._Wx[f * S:(f + 1) * S]))
        for s in range(S):
            j = f * S + s
            want = R.cindex_counts(ev, t, risks[s])                             # the counts of the device's own risks, exactly: integers
            assert np.array_equal(counts[f, s], want), (f, s, counts[f, s], want)
            assert per_job[f, s] == (want[0] + 0.5 * want[2]) / want[4]
            # float64 FISTA at the same step count: the c-index differs by the undecided pairs at the most
            r64 = y[rows] @ w64[j]
            rtol = 2 * D * U * ymax * np.linalg.norm(w64[j])
            comp, diff = pair_tables(ev, t, r64)
            undecided = int((comp & (np.abs(diff) < 2 * rtol)).sum())
            c64 = float((comp & (diff < 0)).sum() + 0.5 * (comp & (diff == 0)).sum()) / comp.sum()
            print(f"{ties} fold {f} lambda {lam[j]:g}: c-index {per_job[f, s]:.6f}, float64 FISTA {c64:.6f}, {undecided} of {comp.sum()} "
                  f"comparable pairs undecided (score tolerance {rtol:.2e}), max |risk - risk64| = {np.abs(risks[s] - r64).max():.2e}")
            assert comp.sum() == want[4]
            if undecided <= R.MAX_UNDECIDED * comp.sum():
                assert abs(per_job[f, s] - c64) <= undecided / comp.sum() + 1e-15
    mean = per_job.mean(0)
    best = max(range(S), key=lambda s: (mean[s], c["strengths"][s]))
    assert out["coxprobe_best_strength"] == c["strengths"][best] and out["coxprobe_cindex"] == pytest.approx(mean[best], rel=1e-14)
    assert out["coxprobe_cindex_mean"] == pytest.approx(tuple(mean), rel=1e-14)
    assert np.allclose(out["coxprobe_cindex_std"], per_job.std(0, ddof=1), rtol=1e-12, atol=0)
    assert 0.55 < out["coxprobe_cindex"] <= 1.0                                 # the synthetic hazard is linear in x: there is signal

    again = fit(case, ties)                                                     # two fits: the same bits
    assert torch.equal(again.coef_, p.coef_) and torch.equal(again.loss_, p.loss_) and torch.equal(again.grad_inf_, p.grad_inf_)


def test_train_rows_keep_the_other_rows_out_of_training_and_in_the_scores(case):
    c, perm = R.E2E, case["perm"]
    F, S = c["F"], len(c["strengths"])
    rng = np.random.default_rng(5)
    shots = np.sort(rng.choice(c["n"], 60, replace=False)).astype(np.int64)     # the CALLER's rows
    p = fit(case, train_rows=dev(shots), max_iter=32)
    inside = np.zeros(c["n"], dtype=bool)
    inside[shots] = True
    event, time, fold, inside = case["event"][perm], case["time"][perm], case["fold"][perm], inside[perm]
    held, _ = R.jobs(F, c["strengths"])
    masks = np.stack([R.train_mask(event, time, fold, h) & inside for h in held])
    assert np.array_equal(host(p.n_train_), masks.sum(1)) and 0 < masks.sum(1).min() and masks.sum(1).max() <= 60
    ev, fd, heldout, rscale = p._train
    assert np.array_equal(host(fd), np.where(inside, np.maximum(fold, -1), -1))
    G, _ = K.coxprobe_grad(K.coxprobe_scores(p._y, p._Wx), p._time, ev, fd, heldout, rscale, "efron")
    G = host(G)
    assert (G[~inside] == 0).all() and all((G[masks[j], j] != 0).any() for j in range(len(held)))
    out = p.evaluate()
    counts = host(out["counts"])
    for f in range(F):                                                          # every row of the fold is scored, few-shot or not
        rows = np.flatnonzero(fold == f)
        comp, _ = pair_tables(event[rows] == 1, time[rows], np.zeros(len(rows)))
        assert (counts[f, :, 4] == comp.sum()).all() and (~inside[rows]).sum() > 0
    assert out["coxprobe_n"] == int((fold >= 0).sum())


def test_predict_risk_and_oof_risk(case):
    c, fold = R.E2E, case["fold"]                                               # the caller's order
    F, S, D = c["F"], len(c["strengths"]), c["D"]
    p = fit(case, max_iter=64)
    best = p.evaluate()["coxprobe_best_strength"]
    rng = np.random.default_rng(3)                                              # 50 fresh rows: rows of the pool under new noise
    fresh = (case["x"][rng.choice(c["n"], 50, replace=False)] + rng.standard_normal((50, D))).astype(np.float32)
    got = host(p.predict_risk(dev(fresh)))
    assert got.dtype == np.float32 and got.shape == (50,)
    q, _ = R.prepare(case["x"], fresh)                                          # with the POOL's mean
    W = host(p.coef_).astype(np.float64)
    for strength, res in ((best, got), (c["strengths"][0], host(p.predict_risk(dev(fresh), strength=c["strengths"][0])))):
        j = F * S + c["strengths"].index(strength)                              # the all-rows job of that strength
        ref = q @ W[j]
        tol = (2 * D * U + 1e-6) * np.linalg.norm(W[j])                         # the chain, and q itself is f32 on the device (|q| = 1)
        assert (np.abs(res - ref) <= tol).all(), (strength, np.abs(res - ref).max() / tol)
    with pytest.raises(ValueError, match="strength must be one of"):
        p.predict_risk(dev(fresh), strength=0.5)
    s = c["strengths"].index(best)
    oof = p.oof_risk()
    assert oof.dtype == torch.float32 and tuple(oof.shape) == (c["n"],)
    assert np.array_equal(np.isnan(host(oof)), fold < 0)                        # NaN outside every fold, and only there, in the CALLER's order
    inv = np.empty(c["n"], dtype=np.int64)
    inv[case["perm"]] = np.arange(c["n"])
    for f in range(F):
        rows = np.flatnonzero(fold == f)                                        # the caller's rows; their sorted positions are inv[rows]
        want = K.coxprobe_scores(p._y.index_select(0, dev(inv[rows])), p._Wx[f * S + s:f * S + s + 1])[0]
        assert torch.equal(oof.index_select(0, dev(rows)), want)                # the job that held the row's fold out
    inside = dev(np.flatnonzero(fold >= 0))
    assert not torch.equal(p.oof_risk(strength=c["strengths"][1 - s])[inside], oof[inside])


def test_fit_stops_at_a_check_below_the_tolerance(case):
    x, event, time, fold = (dev(case[k]) for k in ("x", "event", "time", "fold"))
    p = CoxProbe(strengths=(1e-2, 1e-1), max_iter=2000, tol=1e-3, check_every=16, device="cuda").fit(x, event, time, fold)
    g = host(p.grad_inf_)
    print(f"stopped after {p.n_iter_} iterations, grad_inf_ {g.max():.2e}")
    assert p.n_iter_ % 16 == 0 and 16 <= p.n_iter_ < 2000 and g.shape == (8,) and (g <= 1e-3).all()
    ok = ~np.isnan(case["time"])
    q = CoxProbe(strengths=(1e-2, 1e-1), max_iter=40, tol=1e-3, check_every=16, device="cuda").fit(x, dev(case["event"] == 1), time)
    assert q.n_folds_ == 0 and tuple(q.coef_.shape) == (2, case["x"].shape[1]) and q.n_iter_ <= 40
    assert np.array_equal(host(q.n_train_), [ok.sum()] * 2)                     # fold=None: every row with a time (a bool event is 0 / 1)
    with pytest.raises(ValueError, match="needs folds"):
        q.evaluate()
    with pytest.raises(ValueError, match="needs folds"):
        q.oof_risk(strength=1e-2)
    with pytest.raises(ValueError, match="no best strength"):
        q.predict_risk(x)
    assert tuple(q.predict_risk(x, strength=1e-1).shape) == (240,)


def test_a_job_without_training_events_keeps_zero_weights(case):
    c = R.E2E
    event = case["event"].copy()
    event[case["fold"] != 1] = 0                                                # events only in fold 1: the jobs that hold it out see none
    p = CoxProbe(strengths=c["strengths"], max_iter=16, tol=0.0, device="cuda").fit(dev(case["x"]), dev(event), dev(case["time"]),
                                                                                    dev(case["fold"]))
    S = len(c["strengths"])
    assert (host(p.n_events_)[S:2 * S] == 0).all() and (host(p.n_events_)[:S] > 0).all()
    assert not p.coef_[S:2 * S].any() and not p.loss_[S:2 * S].any() and not p.grad_inf_[S:2 * S].any()
    assert p.coef_[:S].any()


def test_a_nan_row_poisons_exactly_the_jobs_that_train_on_it(case):
    c, fold = R.E2E, case["fold"]
    F, S = c["F"], len(c["strengths"])
    x = case["x"].copy()
    row = int(np.flatnonzero((fold == 1) & (case["event"] <= 1) & ~np.isnan(case["time"]))[0])
    x[row, 3] = np.nan
    kw = dict(strengths=c["strengths"], max_iter=32, tol=0.0, center=False, device="cuda")
    p = CoxProbe(**kw).fit(dev(x), dev(case["event"]), dev(case["time"]), dev(case["fold"]))
    held, _ = R.jobs(F, c["strengths"])
    trains = held != 1                                                          # the row lies in fold 1 and is valid
    assert trains.sum() == (F + 1) * S - S
    assert np.array_equal(host(torch.isnan(p.coef_).any(1)), trains)
    assert np.array_equal(host(torch.isnan(p.loss_)), trains) and np.array_equal(host(torch.isnan(p.grad_inf_)), trains)
    keep = np.arange(c["n"]) != row                                             # the jobs that hold fold 1 out never saw the row
    clean = CoxProbe(**kw).fit(dev(x[keep]), dev(case["event"][keep]), dev(case["time"][keep]), dev(case["fold"][keep]))
    assert np.array_equal(host(p.n_train_)[~trains], host(clean.n_train_)[~trains])
    # the same sums with one zero term less: 1e-5 is far above any re-association of f32 sums over 32 steps and far below what a
    # changed training set or step size would do to weights of size 1
    assert np.abs(host(p.coef_)[~trains] - host(clean.coef_)[~trains]).max() <= 1e-5


def test_one_iteration_replays_bit_for_bit_from_a_graph():
    n, D, J = 300, 40, 33
    y, W = score_case(n, D, J)
    c = grad_case(n, J, "ints", seed=9)
    yd, tm, ev, fold, held, r = dev(y), dev(c["time"]), dev(c["event"]), dev(c["fold"]), dev(c["held"]), dev(c["r"])
    lam = dev(np.linspace(1e-3, 0.1, J).astype(np.float32))
    eta = 1.0 / (0.5 + lam)
    beta = fista_betas(4)[3]
    V, G = torch.empty((J, n), device="cuda"), torch.empty((n, J), device="cuda")
    loss = torch.empty((J,), device="cuda", dtype=torch.float64)
    ws = K.coxprobe_workspace(n, J, "cuda")
    gm = torch.empty(((D + 1 + 127) // 128, J), device="cuda")

    def start():
        return [dev(W * 0.1), dev(W * 0.2)]

    def run(st):                                                                # three launches and nothing else
        K.coxprobe_scores(yd, st[1], V=V)
        K.coxprobe_grad(V, tm, ev, fold, held, r, "efron", G=G, loss=loss, workspace=ws)
        K.coxprobe_step(yd, G, st[0], st[1], lam, eta, beta, gmax_part=gm)

    eager = start()
    run(eager)
    keep = [t.clone() for t in (gm, loss, G)]
    torch.cuda.synchronize()
    st = start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(st)
    for t, s0 in zip(st, start()):                                              # the same start again: capture ran nothing
        t.copy_(s0)
    for t in (gm, G, V):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(st, eager)) and all(torch.equal(a, b_) for a, b_ in zip((gm, loss, G), keep))
    assert float(eager[0].abs().max()) > 0 and not torch.isnan(eager[0]).any()
