"""CPU (no GPU): the float64 restatement of the linear probe (tests/linprobe_ref.py) against sklearn and against the rate FISTA
guarantees, the input condition of the end-to-end GPU test from float64 alone, LinearProbe's argument checks, and the MH_EINVAL
refusals of the two entry points (null pointers: nothing is launched)."""
import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import LinearProbe, _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from mirror_amd.linprobe import fista_betas
from tests import linprobe_ref as R


@pytest.fixture(scope="module")
def small():
    """n = 90, D = 6, C = 3, lambda = 1e-2, Gaussian blobs; sklearn's optimum and the reference iterates at k = 10, 50, 200, 5000."""
    x, labels = R.blobs(90, 6, 3, sep=3.0, seed=5)
    y, _ = R.prepare(x, x)
    mask = R.train_mask(labels, np.zeros(90, dtype=np.int64), -1, 3)
    lam = 1e-2
    Ws, bs, Fs = R.sklearn_optimum(y, labels, mask, lam, 3)
    W, b, kept = R.fista(y, labels, mask, lam, 3, 5000, keep=(10, 50, 200))
    return dict(y=y, labels=labels, mask=mask, lam=lam, Ws=Ws, bs=bs, Fs=Fs, W=W, b=b, kept=kept)


def test_restatement_against_sklearn(small):
    s = small
    assert s["mask"].all()
    dW, db = R.gradient(s["Ws"], s["bs"], s["y"], s["labels"], s["mask"], s["lam"])
    gmax = max(np.abs(dW).max(), np.abs(db).max())
    F = R.objective(s["W"], s["b"], s["y"], s["labels"], s["mask"], s["lam"])
    print(f"gradient at sklearn's solution {gmax:.2e}; F(5000 steps) = {F:.12f}, sklearn {s['Fs']:.12f}")
    assert gmax <= 1e-6
    assert abs(F - s["Fs"]) <= 1e-8 * abs(s["Fs"])
    # the gradient is the objective's: central differences at a point away from the optimum
    rng = np.random.default_rng(0)
    W0, b0 = rng.standard_normal((3, 6)), rng.standard_normal(3)
    dW, db = R.gradient(W0, b0, s["y"], s["labels"], s["mask"], s["lam"])
    for (c, d) in ((0, 0), (2, 5), (1, 3)):
        E = np.zeros((3, 6))
        E[c, d] = 1e-6
        num = (R.objective(W0 + E, b0, s["y"], s["labels"], s["mask"], s["lam"])
               - R.objective(W0 - E, b0, s["y"], s["labels"], s["mask"], s["lam"])) / 2e-6
        assert abs(num - dW[c, d]) <= 1e-8
    e = np.array([0.0, 1e-6, 0.0])
    num = (R.objective(W0, b0 + e, s["y"], s["labels"], s["mask"], 0.0) - R.objective(W0, b0 - e, s["y"], s["labels"], s["mask"], 0.0)) / 2e-6
    assert abs(num - db[1]) <= 1e-8
    assert np.abs(R.logit_grad(W0, b0, s["y"], s["labels"], s["mask"]).sum(1)).max() <= 1e-16


def test_iterates_obey_the_stated_rate(small):
    """F(X_k) - F* <= 2 L (|W*|^2 + |b*|^2) / (k + 1)^2: the guarantee of THIS iteration (t_0 = 1, step 1 / L, from zero)."""
    s = small
    L = R.lipschitz(s["y"], s["lam"])
    r2 = float((s["Ws"] ** 2).sum() + (s["bs"] ** 2).sum())
    for k in (10, 50, 200):
        W, b = s["kept"][k]
        gap = R.objective(W, b, s["y"], s["labels"], s["mask"], s["lam"]) - s["Fs"]
        bound = 2.0 * L * r2 / (k + 1) ** 2
        print(f"k = {k}: F - F* = {gap:.3e}, bound {bound:.3e}")
        assert -1e-12 <= gap <= bound
    assert fista_betas(4) == R.betas(4) and fista_betas(1) == [0.0]
    t1 = (1 + np.sqrt(5)) / 2
    t2 = (1 + np.sqrt(1 + 4 * t1 * t1)) / 2
    assert R.betas(3)[1:] == pytest.approx([(t1 - 1) / t2, (t2 - 1) / ((1 + np.sqrt(1 + 4 * t2 * t2)) / 2)])


def test_jobs_masks_and_prediction_by_hand():
    held, lam = R.jobs(2, (0.1, 0.2, 0.3))
    assert list(held) == [0, 0, 0, 1, 1, 1, -1, -1, -1] and list(lam) == [0.1, 0.2, 0.3] * 3
    labels, fold = np.array([0, 1, 2, 3, -1, 1]), np.array([0, 1, -1, 0, 1, 1])
    assert list(R.train_mask(labels, fold, 0, 3)) == [False, True, False, False, False, True]
    assert list(R.train_mask(labels, fold, -1, 3)) == [True, True, False, False, False, True]
    W, b = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([0.0, 0.0, 0.5])
    pred, margin = R.predict(W, b, np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.0]]))
    assert list(pred) == [0, 2, 0] and list(margin) == [0.0, 1.5, 0.0]           # ties go to the smaller class


def test_end_to_end_inputs_are_decided_in_float64():
    """The condition of the GPU end-to-end test: float64 alone leaves at most 5 % of the held-out rows with a top-two logit margin
    under 1e-3 (here: far fewer, so the cap is met with room to spare)."""
    x, labels, fold = R.e2e_case()
    c = R.E2E
    assert x.shape == (c["n"], c["D"]) and (fold == -1).sum() == 6 and set(fold) == {-1, 0, 1, 2}
    y, ref = R.e2e_reference(x, labels, fold)
    assert len(ref) == 16
    under = total = 0
    for job in ref[:c["F"] * len(c["strengths"])]:
        rows = np.flatnonzero(fold == job["heldout"])
        _, margin = R.predict(job["W"], job["b"], y[rows])
        under += int((margin < R.MARGIN).sum())
        total += len(rows)
    print(f"{under} of {total} held-out (row, job) pairs under the margin")
    assert total == len(c["strengths"]) * int((fold >= 0).sum())
    assert under <= 0.01 * total < R.MAX_UNDECIDED * total


# ------------------------------------------------------------------ the public face
def test_probe_is_exported_and_checks_its_arguments():
    assert mirror_amd.LinearProbe is LinearProbe and "LinearProbe" in mirror_amd.__all__
    for kw in (dict(num_classes=1), dict(num_classes=65), dict(num_classes=True), dict(num_classes=3.0), dict(num_classes=3, strengths=()),
               dict(num_classes=3, strengths=0.1), dict(num_classes=3, strengths=(0.1, 0.0)), dict(num_classes=3, strengths=(-1.0,)),
               dict(num_classes=3, strengths=(float("inf"),)), dict(num_classes=3, strengths=("a",)), dict(num_classes=3, max_iter=0),
               dict(num_classes=3, max_iter=2.0), dict(num_classes=3, tol=-1e-3), dict(num_classes=3, tol=float("nan")),
               dict(num_classes=3, tol="x"), dict(num_classes=3, center=1), dict(num_classes=3, check_every=0),
               dict(num_classes=3, check_every=True)):
        with pytest.raises(ValueError):
            LinearProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        LinearProbe(3, device="cpu")
    p = LinearProbe(3, device="cuda")
    assert (p.num_classes, p.strengths, p.max_iter, p.tol, p.center, p.check_every) == (3, (1e-4, 1e-3, 1e-2, 1e-1), 2000, 1e-4, True, 16)
    y3 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros((3, 2), dtype=torch.int64), y3)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros(3), y3)
    with pytest.raises(MirrorHipError, match="D = 4097"):
        p.fit(torch.zeros((3, 4097)), y3)
    with pytest.raises(ValueError, match="labels must be"):
        p.fit(torch.zeros((3, 2)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels must be"):
        p.fit(torch.zeros((3, 2)), torch.zeros(3))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(torch.zeros((3, 2)), y3, fold=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(torch.zeros((3, 2)), y3, fold=torch.zeros(3))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(torch.zeros((3, 2)), y3, fold=[0, 1, 2])
    with pytest.raises(ValueError, match=r"no row of fold\(s\) \[1\]"):
        p.fit(torch.zeros((3, 2)), y3, fold=torch.tensor([0, 2, 0]))
    with pytest.raises(MirrorHipError, match="J \\* Cp <= 2\\^20"):         # 2^18 folds x 4 strengths x 4 slots
        p.fit(torch.zeros((3, 2)), y3, fold=torch.tensor([0, 1, (1 << 18)]))
    with pytest.raises(MirrorHipError, match="n \\* J \\* Cp <= 2\\^28"):
        LinearProbe(33, strengths=(0.1,) * 64, device="cuda").fit(torch.zeros(((1 << 16) + 1, 1)), torch.zeros((1 << 16) + 1, dtype=torch.int64))
    for call in (p.evaluate, lambda: p.predict(torch.zeros((3, 2)))):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()


def test_launchers_check_before_they_launch():
    y = torch.zeros((6, 8))
    W, b = torch.zeros((2, 4, 8)), torch.zeros((2, 4))
    lab, fold = torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)
    held, r = torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    G = torch.zeros((6, 8))
    with pytest.raises(ValueError, match="must be f32"):
        K.linprobe_grad(y.double(), W, b, lab, fold, held, r, 3)
    with pytest.raises(ValueError, match="C must be"):
        K.linprobe_grad(y, W, b, lab, fold, held, r, 65)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 4, 8\]"):
        K.linprobe_grad(y, torch.zeros((2, 3, 8)), b, lab, fold, held, r, 3)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 4, 8\]"):
        K.linprobe_step(y, G, W, b, torch.zeros((2, 8, 8)), b, r, r, 0.0, 3)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):           # there is no CPU path
        K.linprobe_grad(y, W, b, lab, fold, held, r, 3)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.linprobe_step(y, G, W, b, W, b, r, r, 0.0, 3)


# ------------------------------------------------------------------ the declarations and their refusals
def test_the_entry_points_are_bound_within_the_same_abi_generation():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 123 and lib.mh_version() == 123
    for name, nargs in {"mh_linprobe_grad": 14, "mh_linprobe_step": 15}.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    # mh_linprobe_grad(y, n, D, Wz, bz, labels, fold, heldout, rscale, J, C, Cp, G, loss_part)
    grad = lambda n=10, D=64, J=4, C_=3, Cp=4: ("mh_linprobe_grad", None, n, D, None, None, None, None, None, None, J, C_, Cp, None, None)  # noqa: E731
    # mh_linprobe_step(y, n, D, G, Wx, bx, Wz, bz, lam, eta, beta, J, C, Cp, gmax_part)
    step = lambda n=10, D=64, J=4, C_=3, Cp=4, beta=0.5: ("mh_linprobe_step", None, n, D, None, None, None, None, None, None, None, beta, J, C_, Cp, None)  # noqa: E731
    for mk in (grad, step):
        name = mk()[0]
        _refused(name, r"C = 1 outside \[2, 64\]", *mk(C_=1, Cp=1)[1:])
        _refused(name, r"C = 65 outside \[2, 64\]", *mk(C_=65, Cp=128)[1:])
        _refused(name, "Cp = 6 is not the next power of two", *mk(C_=5, Cp=6)[1:])
        _refused(name, "Cp = 3 is not the next power of two", *mk(C_=3, Cp=3)[1:])
        _refused(name, "Cp = 8 is not the next power of two", *mk(C_=3, Cp=8)[1:])     # a power of two, but not the next one
        _refused(name, "Cp = 2 is not the next power of two", *mk(C_=3, Cp=2)[1:])
        _refused(name, r"D = 4097 outside \[1, 4096\]", *mk(D=4097)[1:])
        _refused(name, r"D = 0 outside \[1, 4096\]", *mk(D=0)[1:])
        _refused(name, r"n = 0 outside \[1, 2\^20\]", *mk(n=0)[1:])
        _refused(name, r"n = 1048577 outside \[1, 2\^20\]", *mk(n=(1 << 20) + 1)[1:])
        _refused(name, "J = 0 jobs", *mk(J=0)[1:])
        _refused(name, r"J = 262145 jobs of Cp = 4 keys outside \[1, 2\^20\]", *mk(n=1, J=(1 << 18) + 1)[1:])
        _refused(name, r"n J Cp = 65537 x 1024 x 4 logit gradients", *mk(n=(1 << 16) + 1, J=1024)[1:])
        _refused(name, "null pointer", *mk(n=1 << 16, J=1024)[1:])                   # exactly 2^28, everything in range: the pointers
        _refused(name, "null pointer", *mk()[1:])                                    # are looked at last
    _refused("mh_linprobe_step", r"beta = 1.5 outside \[0, 1\]", *step(beta=1.5)[1:])
    _refused("mh_linprobe_step", r"beta = -0.1 outside \[0, 1\]", *step(beta=-0.1)[1:])
    _refused("mh_linprobe_step", r"beta = nan outside \[0, 1\]", *step(beta=float("nan"))[1:])
