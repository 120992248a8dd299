"""The linear probe (csrc/linprobe.hip, mirror_amd/linprobe.py) restated in float64 numpy from the header text: the objective of one job,
its gradient, the FISTA iteration and the prediction.  Shared by tests/test_linprobe_{cpu,gpu}.py; the preparation of the rows and the
tally are tests/fewshot_ref.py's.  `fista(..., round_grad=True)` rounds every gradient to f32 before it is used: the yardstick for how
far f32 arithmetic may move an iterate, not code under test.

    F(W, b) = r sum_{i in train} CE(softmax(W y_i + b), label_i) + (lam / 2) |W|^2,      r = 1 / |train|
"""
import numpy as np

from tests.fewshot_ref import cp_of, prepare, tally  # noqa: F401  (re-exported)


def train_mask(labels, fold, heldout, C):
    labels, fold = np.asarray(labels), np.asarray(fold)
    return (labels >= 0) & (labels < C) & (fold >= 0) & (fold != heldout)


def jobs(F, strengths):
    """(heldout [J], lam [J]) in the fold-major job order: job f S + s holds out fold f at strength s, the last S hold out nothing."""
    S = len(strengths)
    held = np.array([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=np.int64)
    return held, np.array(list(strengths) * (F + 1), dtype=np.float64)


def log_softmax(v):
    m = v.max(1, keepdims=True)
    return v - m - np.log(np.exp(v - m).sum(1, keepdims=True))


def row_ce(W, b, y, labels, mask):
    """CE of the training rows (0 elsewhere), float64 [n]."""
    ce = np.zeros(len(y))
    idx = np.flatnonzero(mask)
    ce[idx] = -log_softmax(y[idx] @ W.T + b)[np.arange(len(idx)), np.asarray(labels)[idx]]
    return ce


def logit_grad(W, b, y, labels, mask):
    """r (softmax - onehot) on the training rows, 0 elsewhere: float64 [n, C]."""
    C = W.shape[0]
    G = np.zeros((len(y), C))
    idx = np.flatnonzero(mask)
    if len(idx):
        p = np.exp(log_softmax(y[idx] @ W.T + b))
        p[np.arange(len(idx)), np.asarray(labels)[idx]] -= 1.0
        G[idx] = p / len(idx)
    return G


def objective(W, b, y, labels, mask, lam):
    m = int(mask.sum())
    data = row_ce(W, b, y, labels, mask).sum() / m if m else 0.0
    return data + 0.5 * lam * float((W * W).sum())


def gradient(W, b, y, labels, mask, lam):
    G = logit_grad(W, b, y, labels, mask)
    return G.T @ y + lam * W, G.sum(0)


def lipschitz(y, lam):
    """L = rho / 2 + lam, rho = 1 + max_i |y_i|^2: the softmax Hessian is <= 1 / 2 and the bias is a feature of value 1."""
    return 0.5 * (1.0 + float((y * y).sum(1).max())) + lam


def betas(steps):
    out, t = [], 1.0
    for _ in range(steps):
        t1 = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t1)
        t = t1
    return out


def fista(y, labels, mask, lam, C, steps, round_grad=False, keep=()):
    """(W, b) = X_steps of plain FISTA from zero with step 1 / L; `keep`: iteration counts k whose X_k are returned as a dict too."""
    n, D = y.shape
    eta = 1.0 / lipschitz(y, lam)
    Wx, bx = np.zeros((C, D)), np.zeros(C)
    Wz, bz = Wx.copy(), bx.copy()
    kept = {}
    for k, beta in enumerate(betas(steps)):
        dW, db = gradient(Wz, bz, y, labels, mask, lam)
        if round_grad:
            dW, db = dW.astype(np.float32).astype(np.float64), db.astype(np.float32).astype(np.float64)
        Wn, bn = Wz - eta * dW, bz - eta * db
        Wz, bz = Wn + beta * (Wn - Wx), bn + beta * (bn - bx)
        Wx, bx = Wn, bn
        if k + 1 in keep:
            kept[k + 1] = (Wx.copy(), bx.copy())
    return (Wx, bx, kept) if keep else (Wx, bx)


def predict(W, b, q):
    """(class int64 [n'], top-two logit margin float64 [n']): the largest logit, ties to the smaller class."""
    v = q @ W.T + b
    s = np.sort(v, axis=1)
    return np.argmax(v, axis=1), s[:, -1] - s[:, -2]


def sklearn_optimum(y, labels, mask, lam, C):
    """(W*, b*, F*) from sklearn's LogisticRegression(C = 1 / (lam n_train)) with lbfgs; b* shifted to zero sum (the softmax does not see
    the shift, the bias is not penalised: the minimiser of least norm, the one the iteration from zero approaches)."""
    from sklearn.linear_model import LogisticRegression
    idx = np.flatnonzero(mask)
    clf = LogisticRegression(C=1.0 / (lam * len(idx)), tol=1e-10, max_iter=10000, solver="lbfgs")
    clf.fit(y[idx], np.asarray(labels)[idx])
    assert list(clf.classes_) == list(range(C))
    W, b = clf.coef_.astype(np.float64), clf.intercept_.astype(np.float64)
    b = b - b.mean()
    return W, b, objective(W, b, y, labels, mask, lam)


def blobs(n, D, C, sep, seed):
    """Gaussian blobs around C centres of norm `sep` plus a common offset; labels cycle through the classes."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((C, D))
    cent *= sep / np.linalg.norm(cent, axis=1, keepdims=True)
    labels = (np.arange(n) % C).astype(np.int64)
    x = cent[labels] + rng.standard_normal((n, D)) + 2.0 * rng.standard_normal(D)
    return x.astype(np.float32), labels


# the end-to-end case of tests/test_linprobe_gpu.py; tests/test_linprobe_cpu.py checks its margin condition from float64 alone
E2E = dict(n=300, D=24, C=3, F=3, strengths=(1e-4, 1e-3, 1e-2, 1e-1), steps=300, sep=3.0, seed=41)
MARGIN = 1e-3             # a held-out row whose top two logits lie closer in float64 is not compared
MAX_UNDECIDED = 0.05      # and at most this share of the held-out rows may be such


def e2e_case():
    """(x f32 [n, D], labels int64 [n], fold int64 [n]): 6 rows in no fold, 2 rows with a label outside the classes."""
    c = E2E
    x, labels = blobs(c["n"], c["D"], c["C"], c["sep"], c["seed"])
    rng = np.random.default_rng(c["seed"] + 1)
    fold = rng.integers(0, c["F"], c["n"]).astype(np.int64)
    fold[rng.choice(c["n"], 6, replace=False)] = -1
    labels = labels.copy()
    labels[7], labels[150] = c["C"], -1
    return x, labels, fold


def e2e_reference(x, labels, fold, steps=None):
    """Per job of the end-to-end case: dict(mask, lam, heldout, W, b) with (W, b) the float64 iterate after E2E["steps"] steps."""
    c = E2E
    y, _ = prepare(x, x)
    held, lam = jobs(c["F"], c["strengths"])
    out = []
    for h, l in zip(held, lam):
        mask = train_mask(labels, fold, h, c["C"])
        W, b = fista(y, labels, mask, l, c["C"], c["steps"] if steps is None else steps)
        out.append(dict(mask=mask, lam=l, heldout=int(h), W=W, b=b))
    return y, out
