"""MI355X: recursive gene elimination (csrc/geneselect.hip, mh_gsel_step in csrc/linprobe.hip, mirror_amd/geneselect.py) against the
float64 restatement of tests/geneselect_ref.py.

Each kernel is compared on what the device itself handed to it (the step gets the device's own G, the elimination is checked on the
device's own importances), so a kernel's tolerance is that kernel's f32 rounding, derived from the case, with U = 2^-24:

  logits       S[i, jc] = sum_d |y_id| |w_jcd| + |b_jc| bounds every partial sum of the split chain; there are D fmaf roundings, Z - 1
               adds of slices and one add of the bias, each at most U times a partial sum: delta = 2 (D + Z) U S, a factor 2 to spare.
  hinge        m = 1 -/+ v rounds once: delta_m = delta + U (1 + |v|).  G = 2 r m rounds once more.  The hinge is exactly 0 wherever
               float64 says m < -delta_m.  The loss term sum_c m^2 is a chain of C fmaf: each term is off by 2 |m| delta_m + delta_m^2,
               each rounding by U times the sum.
  weight sums  B[k, d] = 2 n U sum_i |G[i, k]| |y[i, d]|: one row-ordered f32 chain of n terms; carried through g = fmaf(lam, Z, sum),
               X' = fmaf(-eta, g, Z), X' - X and Z' = fmaf(beta, X' - X, X') with U of each result.
  importance   integer-valued weights: exact.  Otherwise C = 2 is used, where the chain rounds twice, each time by half an ulp of a
               partial sum that does not exceed the result: 1 ulp.
"""
import math

import numpy as np
import pytest
import torch

from mirror_amd import GeneSelect, kernels as K
from tests import geneselect_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


def cp_of(C):
    return 1 << (C - 1).bit_length()


def slices(n, nk, D):
    """mh_gsel_slices restated: (Z, ks)."""
    tiles = ((n + 127) // 128) * ((nk + 127) // 128)
    zmax = min(max(768 // tiles, 1), 128)
    z0 = min((D + 255) // 256, zmax)
    ks = ((D + z0 - 1) // z0 + 15) // 16 * 16
    return (D + ks - 1) // ks, ks


def ragged_D(n, nk):
    """The smallest D that is cut into more than one slice with a ragged last one."""
    for D in range(1, 1 << 18):
        Z, ks = slices(n, nk, D)
        if Z > 1 and D % ks:
            return D
    raise AssertionError


# ------------------------------------------------------------------ 1. mh_colstats, mh_standardize
@pytest.mark.parametrize("shape", [(1, 1), (129, 5), (300, 130), (40, 4100)], ids=lambda s: "n%d-D%d" % s)
def test_standardize_against_float64(shape):
    n, D = shape
    rng = np.random.default_rng(n + D)
    x = (rng.standard_normal((n, D)) * rng.uniform(0.5, 3, D) + 2 * rng.standard_normal(D)).astype(np.float32)
    x[:, 0] = np.float32(3.7)                                                 # a constant column
    xd = dev(x)
    mu, rstd = K.colstats(xd)
    y = K.standardize(xd, mu, rstd)
    x64 = x.astype(np.float64)
    mu64 = x64.mean(0)
    assert (np.abs(host(mu) - mu64) <= U * np.abs(mu64) + 1e-300).all()       # rounded once
    mud = host(mu).astype(np.float64)
    var = ((x64 - mud) ** 2).mean(0)                                          # the second pass is over the DEVICE's mean
    want = np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
    assert (np.abs(host(rstd) - want) <= U * want + 1e-12 * want).all()
    assert host(rstd)[0] == 0.0 and (host(y)[:, 0] == 0.0).all() and host(mu)[0] == np.float32(3.7)
    if n == 1:
        assert (host(rstd) == 0).all() and (host(y) == 0).all()
    y64 = (x64 - mud) * host(rstd).astype(np.float64)
    assert (np.abs(host(y) - y64) <= 3 * U * np.abs(y64)).all()               # a subtraction and a product, each rounded once
    ref_y, _, _ = R.standardize(x64)
    if n > 1:
        assert np.abs(host(y) - ref_y).max() <= 1e-4 * max(np.abs(ref_y).max(), 1.0)
    z = xd.clone()
    assert K.standardize(z, mu, rstd, out=z) is z and torch.equal(z, y)       # in place, bit for bit
    mu2, rstd2 = K.colstats(xd)
    assert torch.equal(mu, mu2) and torch.equal(rstd, rstd2)


# ------------------------------------------------------------------ 2. mh_gsel_rowsq
def test_rowsq_against_float64_with_a_mask_per_job():
    n, D, J = 37, 4100, 3
    rng = np.random.default_rng(5)
    y = rng.standard_normal((n, D)).astype(np.float32)
    mask = (rng.random((J, D)) < np.array([1.0, 0.5, 0.01])[:, None]).astype(np.uint8)
    out = K.gsel_rowsq(dev(y), dev(mask))
    assert out.dtype == torch.float32 and tuple(out.shape) == (J, n)
    want = np.einsum("nd,jd->jn", y.astype(np.float64) ** 2, mask.astype(np.float64))
    tol = 2 * (D // 64 + 1 + 6) * U * want                                    # a lane's chain, then six butterfly adds
    assert (np.abs(host(out) - want) <= tol).all()
    assert torch.equal(out, K.gsel_rowsq(dev(y), dev(mask)))


# ------------------------------------------------------------------ 3. mh_gsel_grad
NS = [1, 127, 129, 300]
CJ = [(2, 70), (3, 5), (5, 3), (64, 3)]                                      # 140 and 192 keys cross a 128-key tile
GRAD_CASES = [(n, dk, CJ[(a + b) % 4]) for a, n in enumerate(NS) for b, dk in enumerate([3, 37, 4100, "ragged"])]


def grad_case(n, D, C, J):
    rng = np.random.default_rng(1000 * n + 10 * D + C)
    Cp = cp_of(C)
    y = rng.standard_normal((n, D))
    y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    W = np.zeros((J, Cp, D), np.float32)
    b = np.zeros((J, Cp), np.float32)
    w = rng.standard_normal((J, C, D))
    W[:, :C] = w / np.linalg.norm(w, axis=2, keepdims=True) * rng.uniform(0, 6, (J, C, 1))
    b[:, :C] = rng.standard_normal((J, C))
    W[:, C:], b[:, C:] = 7.0, 7.0                                             # pad slots: whatever they hold is never read
    labels = rng.integers(-1, C + 1, n).astype(np.int64)
    fold = rng.integers(-1, 3, n).astype(np.int32)
    held = rng.integers(-1, 3, J).astype(np.int32)
    labels[0], fold[0], held[0] = C - 1, 0, -1                                # (row 0, job 0) trains whatever the draw
    W[0, 1, :], b[0, 1] = W[0, 0, :], b[0, 0]                                 # job 0: classes 0 and 1 tie on every row, bit for bit
    W[0, 2:C], b[0, 2:C] = 0.0, -100.0                                        # and no other class comes near
    train = np.stack([(labels >= 0) & (labels < C) & (fold >= 0) & (fold != h) for h in held])
    r = (1.0 / np.maximum(train.sum(1), 1)).astype(np.float32)
    return dict(n=n, D=D, C=C, J=J, Cp=Cp, y=y, W=W, b=b, labels=labels, fold=fold, held=held, r=r, train=train)


def run_grad(c, ws=None, y=None):
    return K.gsel_grad(dev(c["y"] if y is None else y), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]),
                       dev(c["r"]), c["C"], want_loss=True, want_pred=True, workspace=ws)


@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda s: "n%d-D%s-C%d-J%d" % (s[0], s[1], s[2][0], s[2][1]))
def test_grad_against_float64(case):
    n, dk, (C, J) = case
    Cp = cp_of(C)
    D = ragged_D(n, J * Cp) if dk == "ragged" else dk
    Z, ks = slices(n, J * Cp, D)
    assert K.gsel_slices(n, J * Cp, D) == Z
    if dk == "ragged":
        assert Z > 1 and D % ks and K.gsel_slices(n, J * Cp, D - 1) == 1
    c = grad_case(n, D, C, J)
    G, part, pred = run_grad(c)
    assert tuple(G.shape) == (n, J * Cp) and tuple(part.shape) == ((n + 127) // 128, J) and tuple(pred.shape) == (J, n)
    assert pred.dtype == torch.int32 and part.dtype == torch.float64
    got = host(G).astype(np.float64).reshape(n, J, Cp)
    y, W, b = c["y"].astype(np.float64), c["W"][:, :C].astype(np.float64), c["b"][:, :C].astype(np.float64)
    r, train = c["r"].astype(np.float64), c["train"].T                        # train [n, J]
    V = np.einsum("nd,jcd->njc", y, W) + b[None]
    S = np.einsum("nd,jcd->njc", np.abs(y), np.abs(W)) + np.abs(b)[None]
    delta = 2 * (D + Z) * U * S
    T = R.targets(c["labels"], C)[:, None, :]
    m = 1.0 - T * V
    dm = delta + U * (1 + np.abs(V))
    assert train[0, 0] and (n == 1 or not train.all())
    assert not np.isnan(got).any()
    assert (got[:, :, C:] == 0).all() and (got[~train] == 0).all()            # pad columns, rows out of train: exactly 0
    off = train[:, :, None] & (m < -dm)
    assert (got[:, :, :C][off] == 0).all() and (n < 100 or off.sum() > 0)     # the hinge inactive by more than the bound: exactly 0
    want = -2 * r[None, :, None] * T * np.maximum(m, 0) * train[:, :, None]
    tol = 2 * r[None, :, None] * (dm + 2 * U * (np.abs(m) + dm))
    err = np.abs(got[:, :, :C] - want)
    print(f"{case}: D = {D}, Z = {Z}, worst err / tol = {(err / tol).max():.3f}, max delta = {delta.max():.3e}")
    assert (err <= tol).all()
    # classes: decided rows, and the constructed tie of job 0
    p = host(pred).T                                                          # [n, J]
    top = np.sort(V, axis=2)
    decided = top[:, :, -1] - top[:, :, -2] > 2 * np.sort(delta, axis=2)[:, :, -1]
    decided[:, 0] = False
    assert (p[decided] == V.argmax(2)[decided]).all() and (n == 1 or decided.mean() > 0.5)
    assert (p[:, 0] == 0).all()                                               # equal scores go to the smaller class
    # loss
    h = np.maximum(m, 0) * train[:, :, None]
    row_tol = ((2 * h * dm + dm ** 2) * train[:, :, None]).sum(2) + (C + 1) * U * ((h + dm) ** 2 * train[:, :, None]).sum(2)
    loss, lwant = host(part).sum(0), r * (h ** 2).sum((0, 2))
    assert (np.abs(loss - lwant) <= r * row_tol.sum(0) + 1e-15).all()
    tile = np.arange(n) // 128
    for t in range((n + 127) // 128):
        assert (np.abs(host(part)[t] - r * (h[tile == t] ** 2).sum((0, 2))) <= r * row_tol[tile == t].sum(0) + 1e-15).all()
    # deterministic; the workspace need not be zeroed
    ws = K.gsel_workspace(n, J, Cp, D, "cuda")
    assert ws.numel() == Z * n * J * Cp
    ws.fill_(math.nan)
    G2, part2, pred2 = run_grad(c, ws=ws)
    assert torch.equal(G, G2) and torch.equal(part, part2) and torch.equal(pred, pred2)
    G3, none, none2 = K.gsel_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]), C)
    assert none is None and none2 is None and torch.equal(G, G3)
    # a NaN row: no class, NaN gradients for exactly the jobs that train on it
    if n > 1:
        i = int(np.nonzero(train.any(1) & ~train.all(1))[0][0]) if (train.any(1) & ~train.all(1)).any() else 0
        yn = c["y"].copy()
        yn[i, D // 2] = np.nan
        Gn, partn, predn = run_grad(c, y=yn)
        gn = host(Gn).reshape(n, J, Cp)
        assert (host(predn)[:, i] == -1).all()
        assert np.isnan(gn[i, :, :C][train[i]]).all() and (gn[i][~train[i]] == 0).all() and (gn[i, :, C:] == 0).all()
        others = np.arange(n) != i
        assert np.array_equal(gn[others], host(G).reshape(n, J, Cp)[others]) and np.array_equal(host(predn)[:, others], host(pred)[:, others])
        assert (np.isnan(host(partn)[i // 128]) == train[i]).all()


# ------------------------------------------------------------------ 4. mh_gsel_step
@pytest.mark.parametrize("D", [127, 128, 129])
@pytest.mark.parametrize("fit_intercept", [True, False])
def test_step_on_the_devices_own_gradient(D, fit_intercept):
    n, C, J = 37, 3, 70                                                       # n is no multiple of 16; 280 keys cross two tiles
    Cp = cp_of(C)
    c = grad_case(n, D, C, J)
    rng = np.random.default_rng(D)
    y = c["y"].copy()
    y[:, 5] *= 1000.0                                                         # a column whose gradient dwarfs the others
    mask = (rng.random((J, D)) < 0.6).astype(np.uint8)
    mask[0, 5], mask[1, 5] = 0, 1
    G = K.gsel_grad(dev(y), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]), C)[0]
    Wz, bz = c["W"].copy(), c["b"].copy()
    Wx = (Wz + 0.1 * rng.standard_normal(Wz.shape)).astype(np.float32)
    bx = (bz + 0.1 * rng.standard_normal(bz.shape)).astype(np.float32)
    dead = np.broadcast_to(mask[:, None, :] == 0, Wx.shape)
    Wx[dead], Wz[dead] = 12345.0, -54321.0                                    # sentinels in the masked positions
    lam = rng.uniform(1e-3, 1e-1, J).astype(np.float32)
    eta = rng.uniform(0.01, 0.2, J).astype(np.float32)
    beta = 0.37
    dWx, dbx, dWz, dbz = dev(Wx), dev(bx), dev(Wz), dev(bz)
    gmax = K.gsel_step(dev(y), G, dWx, dbx, dWz, dbz, dev(lam), dev(eta), beta, dev(mask), fit_intercept, C, want_gmax=True)
    assert tuple(gmax.shape) == ((D + 1 + 127) // 128, J)
    g = host(G).astype(np.float64).reshape(n, J, Cp)
    y64, b32 = y.astype(np.float64), np.float32(beta).astype(np.float64)
    S = np.einsum("njc,nd->jcd", g, y64)
    B = 2 * n * U * np.einsum("njc,nd->jcd", np.abs(g), np.abs(y64))
    l64, e64 = lam.astype(np.float64)[:, None, None], eta.astype(np.float64)[:, None, None]
    gw = S + l64 * Wz.astype(np.float64)
    tg = B + 2 * U * np.abs(gw)
    xn = Wz.astype(np.float64) - e64 * gw
    tx = e64 * tg + 2 * U * np.abs(xn)
    zn = xn + b32 * (xn - Wx.astype(np.float64))
    tz = (1 + b32) * tx + 2 * U * (np.abs(xn - Wx) + np.abs(zn))
    live = ~dead
    live[:, C:, :] = False
    gx, gz = host(dWx), host(dWz)
    assert (np.abs(gx - xn)[live] <= tx[live]).all() and (np.abs(gz - zn)[live] <= tz[live]).all()
    keep = ~live                                                              # masked columns and pad slots: bit for bit what they held
    assert np.array_equal(gx[keep], Wx[keep]) and np.array_equal(gz[keep], Wz[keep])
    gb = g.sum(0)
    tb = 2 * n * U * np.abs(g).sum(0)
    if fit_intercept:
        bn = bz.astype(np.float64) - eta.astype(np.float64)[:, None] * gb
        tbx = eta.astype(np.float64)[:, None] * (tb + 2 * U * np.abs(gb)) + 2 * U * np.abs(bn)
        assert (np.abs(host(dbx) - bn)[:, :C] <= tbx[:, :C]).all()
        assert np.array_equal(host(dbx)[:, C:], bx[:, C:]) and np.array_equal(host(dbz)[:, C:], bz[:, C:])
    else:
        assert np.array_equal(host(dbx), bx) and np.array_equal(host(dbz), bz)          # the bias is pinned: untouched
    # gmax_part: the active columns of the tile only (column 5 of job 0 would dwarf them), the bias only with fit_intercept
    act = np.where(np.broadcast_to(mask[:, None, :] != 0, gw[:, :C].shape), np.abs(gw[:, :C]), 0.0)
    tact = np.where(np.broadcast_to(mask[:, None, :] != 0, gw[:, :C].shape), tg[:, :C], 0.0)
    for t in range((D + 1 + 127) // 128):
        lo, hi = t * 128, min((t + 1) * 128, D)
        want = act[:, :, lo:hi].max((1, 2)) if hi > lo else np.zeros(J)
        tol = tact[:, :, lo:hi].max((1, 2)) if hi > lo else np.zeros(J)
        if fit_intercept and lo <= D < (t + 1) * 128:
            want, tol = np.maximum(want, np.abs(gb[:, :C]).max(1)), np.maximum(tol, tb[:, :C].max(1) + 1e-30)
        assert (np.abs(host(gmax)[t] - want) <= tol).all()
    assert np.abs(gw[0, :C, 5]).max() > 10 * host(gmax)[0, 0]                 # job 0 masks column 5: its would-be gradient is not in the maximum


@pytest.mark.parametrize("D", [127, 128, 129])
def test_step_with_a_mask_of_ones_is_linprobe_step_bit_for_bit(D):
    n, C, J = 37, 3, 70
    c = grad_case(n, D, C, J)
    rng = np.random.default_rng(D + 1)
    G = K.gsel_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]), C)[0]
    Wx = (c["W"] + 0.1 * rng.standard_normal(c["W"].shape)).astype(np.float32)
    bx = (c["b"] + 0.1 * rng.standard_normal(c["b"].shape)).astype(np.float32)
    lam, eta = dev(rng.uniform(1e-3, 1e-1, J).astype(np.float32)), dev(rng.uniform(0.01, 0.2, J).astype(np.float32))
    a = [dev(Wx), dev(bx), dev(c["W"]), dev(c["b"])]
    b = [t.clone() for t in a]
    ga = K.gsel_step(dev(c["y"]), G, *a, lam, eta, 0.5, torch.ones((J, D), device="cuda", dtype=torch.uint8), True, C, want_gmax=True)
    gb = K.linprobe_step(dev(c["y"]), G, *b, lam, eta, 0.5, C, want_gmax=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(ga, gb)
    assert not torch.equal(a[0], dev(Wx))


# ------------------------------------------------------------------ 5. mh_gsel_eliminate
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("D", [1, 2, 63, 65, 1000, 4097, 70001])
def test_eliminate_against_a_stable_argsort(D, J):
    for C, integer in ((3, True), (2, False)):
        Cp = cp_of(C)
        rng = np.random.default_rng(10 * D + J + C)
        if integer:                                                           # runs of equal importance straddle every cut
            Wx = rng.integers(-2, 3, (J, Cp, D)).astype(np.float32)
            if D >= 63:
                Wx[:, 0, 7], Wx[:, 1, 11], Wx[:, 0, 40], Wx[:, :, 41] = np.inf, np.nan, np.inf, 0.0
        else:
            Wx = rng.standard_normal((J, Cp, D)).astype(np.float32)
        Wz = rng.standard_normal((J, Cp, D)).astype(np.float32)
        mask = (rng.random((J, D)) < np.linspace(1.0, 0.5, J)[:, None]).astype(np.uint8)
        mask[:, 0] = 1
        if D >= 63:
            mask[:, [7, 11, 40, 41]] = 1
        elim = np.where(mask != 0, -1, 0).astype(np.int32)
        active0 = int(mask[0].sum())
        for k in sorted({0, 1, max(active0 - 1, 0), active0}):
            dWx, dWz, dm, de = dev(Wx), dev(Wz), dev(mask), dev(elim)
            imp = host(K.gsel_eliminate(dWx, dWz, dm, de, k, 7, C, want_importance=True))
            w64 = Wx[:, :C].astype(np.float64)
            exact = (w64 ** 2).sum(1)
            on = mask != 0
            assert (imp[~on] == 0).all()
            if integer:
                assert np.array_equal(imp[on], exact[on].astype(np.float32), equal_nan=True)
            else:
                assert (np.abs(imp[on] - exact[on]) <= np.spacing(exact[on].astype(np.float32))).all()
            eW, eZ, em, ee = Wx.copy(), Wz.copy(), mask.copy(), elim.copy()
            for j in range(J):
                act = np.nonzero(on[j])[0]
                drop = act[np.argsort(bits(imp[j, act]), kind="stable")][:k]  # the key: the bits of the DEVICE's importance, then the index
                em[j, drop], ee[j, drop] = 0, 7
                eW[j][:C, drop], eZ[j][:C, drop] = 0.0, 0.0
            assert np.array_equal(host(dm), em) and np.array_equal(host(de), ee), (D, J, C, k)
            assert np.array_equal(bits(host(dWx)), bits(eW)) and np.array_equal(bits(host(dWz)), bits(eZ))      # pads and the rest untouched
            if k == 0:
                assert K.gsel_eliminate(dWx, dWz, dm, de, 0, 8, C) is None and np.array_equal(host(de), elim)


# ------------------------------------------------------------------ 6. end to end
CFG = dict(step=4, min_features=1, max_iter=1024, tol=1e-4)
SK_SUPPORT = [0, 3, 5, 16]            # RFECV(LinearSVC(C=1, fit_intercept=False, dual=False, tol=1e-10, max_iter=500000), step=4,
#                                       cv=PredefinedSplit(fold)).support_ on the standardised planted set (test_geneselect_cpu.py holds
#                                       the restatement against that run)


@pytest.fixture(scope="module")
def planted_fit():
    x, lab, fold = R.planted(0)
    g = GeneSelect(3, fit_intercept=False, device="cuda", **CFG).fit(dev(x), dev(lab), dev(fold))
    ref = R.rfecv(x, lab, fold, 3, fit_intercept=False, iters=g.n_iter_, final_iters=g.n_iter_final_, **CFG)
    return x, lab, fold, g, ref


def test_planted_set_end_to_end(planted_fit):
    x, lab, fold, g, ref = planted_fit
    print(f"n_iter_ = {g.n_iter_}, final {g.n_iter_final_}, restatement gap at those counts = {ref['gap']:.3e}")
    assert ref["gap"] >= 1e-4                                                 # far above f32 rounding: what the identities below rest on
    assert len(g.n_iter_) == 11 and all(1 <= k <= 1024 for k in g.n_iter_)
    assert g.elim_round_.dtype == torch.int32 and np.array_equal(host(g.elim_round_), ref["elim_round"])
    for f in range(4):
        assert np.array_equal(host(g.cv_results_[f"split{f}_test_score"]), ref["cv_results"][f"split{f}_test_score"])
    assert g.cv_results_["n_features"] == ref["cv_results"]["n_features"] == [1, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    assert np.allclose(host(g.cv_results_["mean_test_score"]), ref["cv_results"]["mean_test_score"], rtol=1e-15, atol=0)
    assert np.allclose(host(g.cv_results_["std_test_score"]), ref["cv_results"]["std_test_score"], rtol=1e-12, atol=1e-15)
    assert g.n_features_ == 4 == ref["n_features"]
    assert g.support_.dtype == torch.bool and np.array_equal(host(g.support_), ref["support"])
    assert g.ranking_.dtype == torch.int64 and np.array_equal(host(g.ranking_), ref["ranking"])
    assert np.nonzero(host(g.support_))[0].tolist() == SK_SUPPORT
    # the final fit: in the support only, close to the restatement's at the same count
    coef = host(g.coef_)
    assert tuple(coef.shape) == (3, 40) and (coef[:, ~ref["support"]] == 0).all() and (host(g.intercept_) == 0).all()
    assert np.abs(coef - ref["coef"]).max() <= 1e-4 * np.abs(ref["coef"]).max()
    assert np.abs(host(g.mu_) - ref["mu"]).max() <= 1e-6 * np.abs(ref["mu"]).max()


def test_two_fits_agree_bit_for_bit(planted_fit):
    x, lab, fold, g, _ = planted_fit
    h = GeneSelect(3, fit_intercept=False, device="cuda", **CFG).fit(dev(x), dev(lab), dev(fold))
    assert h.n_iter_ == g.n_iter_ and h.n_iter_final_ == g.n_iter_final_
    assert torch.equal(h.elim_round_, g.elim_round_) and torch.equal(h.coef_, g.coef_) and torch.equal(h.ranking_, g.ranking_)
    assert all(torch.equal(h.cv_results_[k], g.cv_results_[k]) for k in g.cv_results_ if k != "n_features")


def test_with_an_intercept_and_without_folds():
    x, lab, fold = R.planted(0)
    g = GeneSelect(3, fit_intercept=True, device="cuda", **CFG).fit(dev(x), dev(lab), dev(fold))
    ref = R.rfecv(x, lab, fold, 3, fit_intercept=True, iters=g.n_iter_, final_iters=g.n_iter_final_, **CFG)
    print(f"fit_intercept=True: gap {ref['gap']:.3e}, n_features {g.n_features_}")
    assert ref["gap"] >= 1e-4
    assert np.array_equal(host(g.elim_round_), ref["elim_round"]) and np.array_equal(host(g.ranking_), ref["ranking"])
    assert g.n_features_ == ref["n_features"]
    assert np.abs(host(g.intercept_) - ref["intercept"]).max() <= 1e-4 * max(np.abs(ref["intercept"]).max(), 1.0)
    assert np.abs(host(g.intercept_)).max() > 0
    p = GeneSelect(3, step=4, min_features=8, max_iter=1024, tol=1e-4, fit_intercept=False, device="cuda").fit(dev(x), dev(lab))
    ref = R.rfecv(x, lab, None, 3, step=4, min_features=8, max_iter=1024, tol=1e-4, fit_intercept=False, iters=p.n_iter_,
                  final_iters=p.n_iter_final_)
    assert ref["gap"] >= 1e-4
    assert p.cv_results_ is None and p.n_features_ == 8 and tuple(p.elim_round_.shape) == (1, 40)
    assert np.array_equal(host(p.elim_round_), ref["elim_round"]) and np.array_equal(host(p.ranking_), ref["ranking"])
    assert int(p.support_.sum()) == 8 and sorted(set(host(p.ranking_).tolist())) == list(range(1, 10))


def test_predict_score_selected_on_held_out_draws(planted_fit):
    x, lab, fold, g, ref = planted_fit
    xq, lq = R.planted_more(0, 200)
    pred = host(g.predict(dev(xq)))
    coef, mu, rstd = host(g.coef_).astype(np.float64), host(g.mu_).astype(np.float64), host(g.rstd_).astype(np.float64)
    yq = (xq.astype(np.float32).astype(np.float64) - mu) * rstd
    V = yq @ coef.T
    top = np.sort(V, axis=1)
    bound = 2 * (40 + 1) * U * (np.abs(yq) @ np.abs(coef).T).max(1) + 4 * U * (np.abs(yq) @ np.abs(coef).T).max(1)
    decided = top[:, -1] - top[:, -2] > 2 * bound
    assert decided.mean() > 0.9 and (pred[decided] == V.argmax(1)[decided]).all()
    s = g.score(dev(xq), dev(lq))
    conf = host(s["confusion"])
    assert conf.sum() == 200 and np.array_equal(conf, np.array([[((lq == a) & (pred == b)).sum() for b in range(3)] for a in range(3)]))
    want = R.report(conf)
    assert list(s)[:4] == ["accuracy", "precision", "recall", "f1"]
    assert all(abs(s[k] - want[k]) <= 1e-14 for k in want) and s["accuracy"] > 0.6
    assert host(g.selected()).tolist() == SK_SUPPORT
    keep = torch.tensor([16, 2, 39, 2])
    assert host(g.selected(keep=keep)).tolist() == [0, 2, 3, 5, 16, 39]
    t = g.transform(dev(xq.astype(np.float32)))
    assert np.array_equal(host(t), xq.astype(np.float32)[:, SK_SUPPORT])
    with pytest.raises(ValueError, match="outside"):
        g.selected(keep=torch.tensor([40]))


def test_one_iteration_replays_bit_for_bit_from_a_graph():
    n, D, C, J = 300, 273, 3, 5
    c = grad_case(n, D, C, J)
    Cp = c["Cp"]
    assert K.gsel_slices(n, J * Cp, D) > 1
    rng = np.random.default_rng(3)
    y, lab, fd, held, r = dev(c["y"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"])
    lam, eta = dev(np.full(J, 0.01, np.float32)), dev(np.full(J, 0.1, np.float32))
    mask = dev((rng.random((J, D)) < 0.7).astype(np.uint8))
    state = [dev(c["W"]), dev(c["b"]), dev(c["W"]), dev(c["b"])]

    def iteration(st, G, ws, gmax):
        K.gsel_grad(y, st[2], st[3], lab, fd, held, r, C, G=G, workspace=ws)
        K.gsel_step(y, G, *st, lam, eta, 0.25, mask, True, C, gmax_part=gmax)

    def buffers():
        return (torch.empty((n, J * Cp), device="cuda"), K.gsel_workspace(n, J, Cp, D, "cuda"),
                torch.empty(((D + 1 + 127) // 128, J), device="cuda"))

    eager = [t.clone() for t in state]
    be = buffers()
    iteration(eager, *be)
    torch.cuda.synchronize()
    st = [t.clone() for t in state]
    bg = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iteration(st, *bg)
    for _ in range(2):
        for t, s0 in zip(st, state):
            t.copy_(s0)
        bg[0].fill_(-1.0)
        bg[2].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(st, eager)) and torch.equal(bg[0], be[0]) and torch.equal(bg[2], be[2])
    assert not torch.equal(eager[0], state[0])
