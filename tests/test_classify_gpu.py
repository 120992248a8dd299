"""MI355X: the subtyping step of train_subtyping.py through the C ABI (csrc/classify.hip) — LabelSmoothingCrossEntropy /
CrossEntropyLoss and their logit gradients against tests/golden/golden_cls.npz, NaN rows, determinism and graph replay; the
F1 / AUROC metrics and top-1 accuracy against the fixture, chunked updates, merged states and a two-rank sync_and_compute; and a
linear probe at the subtyping template's head geometry against f64 torch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mirror_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
from mirror_amd.metrics import MulticlassAUROC, MulticlassF1Score, accuracy, sync_and_compute
from tests.test_classify_cpu import CASES, REDUCTIONS, SS, argmax_np, confusion_np, f1_np

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_cls.npz")
F1_AVERAGES = ("micro", "macro", "weighted", None)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _metric_case(z, key):
    """(scores f32, labels int64) of a metric case of the fixture, on the device."""
    if key == "met/nan":
        sc = z["met/nan/scores"]
    elif key.endswith("/f"):
        sc = z["cls/" + key.split("/")[1] + "/logits"]
    else:
        sc = z[key + "/scores"].astype(np.float32)
    return torch.from_numpy(sc).cuda(), torch.from_numpy(z[key + "/labels"]).cuda()


METRIC_KEYS = [f"met/N{n}_C{c}/{v}" for n, c in CASES for v in ("f", "i")] + ["met/nan"]


@pytest.mark.parametrize("N,C", CASES)
def test_loss_and_dlogits_match_golden(z, N, C):
    G = f"cls/N{N}_C{C}"
    x = torch.from_numpy(z[f"{G}/logits"]).cuda()
    y = torch.from_numpy(z[f"{G}/labels"])
    ii = int(z[f"{G}/ignore_index"])
    w, gs = torch.from_numpy(z[f"{G}/w"]).cuda(), torch.from_numpy(z[f"{G}/gs"]).cuda()
    for s in SS:
        for red in REDUCTIONS:
            fns = [CrossEntropyLoss(ignore_index=ii, reduction=red, label_smoothing=float(s))]
            if red == "mean" and not (y == ii).any():
                fns.append(LabelSmoothingCrossEntropy(smoothing=float(s)))
            for fn in fns:
                for yy in (y.cuda(), y):                              # device labels, and host labels copied by the loss
                    xl = x.clone().requires_grad_(True)
                    loss = fn(xl, yy)
                    want = z[f"{G}/s{s}/{red}/loss"]
                    assert tuple(loss.shape) == want.shape and loss.dtype == torch.float32
                    assert _rel(loss.detach().cpu().numpy(), want) <= 1e-5, (G, s, red, type(fn).__name__)
                    (loss * (w if red == "none" else gs)).sum().backward()
                    key = f"{G}/s{s}/{red}/dx"
                    if key in z:
                        assert _rel(xl.grad.cpu().numpy(), z[key]) <= 1e-5, (G, s, red)
                    else:                                             # "sum" of the largest case: the "mean" gradient times n
                        n = int((y != ii).sum())
                        want_dx = z[f"{G}/s{s}/mean/dx"].astype(np.float64) * n
                        assert _rel(xl.grad.cpu().numpy(), want_dx) <= 1e-5, (G, s, red)


def test_out_of_range_label_gives_nan_row_and_leaves_the_others():
    torch.manual_seed(3)
    x = torch.randn(6, 5, device="cuda")
    good = torch.tensor([0, 4, 2, 1, 3, -100], device="cuda")
    bad = torch.tensor([0, 5, 2, -1, 3, -100], device="cuda")                 # rows 1 and 3 out of range, row 5 ignored
    fn = CrossEntropyLoss(reduction="none", label_smoothing=0.1)
    xg, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    lg, lb = fn(xg, good), fn(xb, bad)
    nan = torch.isnan(lb).cpu().tolist()
    assert nan == [False, True, False, True, False, False]
    keep = [0, 2, 4, 5]
    assert torch.equal(lb[keep], lg[keep]) and float(lb[5].detach()) == 0.0
    lg.sum().backward()
    lb.sum().backward()
    assert torch.isnan(xb.grad[[1, 3]]).all() and torch.equal(xb.grad[keep], xg.grad[keep])
    assert torch.isnan(CrossEntropyLoss()(x, bad))
    assert torch.isnan(LabelSmoothingCrossEntropy()(x, torch.tensor([0, 1, 2, 3, 4, 7], device="cuda")))


@pytest.mark.parametrize("red", ["mean", "none"])
def test_deterministic_and_graph_replay_matches_eager(red):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(257, 33, generator=g) * 4).cuda()
    y = torch.randint(0, 33, (257,), generator=g).cuda()
    y[::13] = -100
    fn = CrossEntropyLoss(reduction=red, label_smoothing=0.1)
    up = torch.rand(257, generator=g).cuda() if red == "none" else torch.tensor(0.75, device="cuda")

    def step(xs):
        xl = xs.detach().requires_grad_(True)
        loss = fn(xl, y)
        (dx,) = torch.autograd.grad(loss, xl, grad_outputs=up)
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
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        gl, gd = step(static_x)
    static_x.copy_(x * 0.5)
    gr.replay()
    torch.cuda.synchronize()
    el, ed = step(x * 0.5)
    assert torch.equal(gl, el) and torch.equal(gd, ed)
    static_x.copy_(x)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(gl, l1) and torch.equal(gd, d1)


def test_metric_update_and_accuracy_under_graph_replay():
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(64, 5, generator=g).cuda() for _ in range(3)]
    ys = [torch.randint(0, 5, (64,), generator=g).cuda() for _ in range(3)]
    eager = MulticlassF1Score(num_classes=5, average="macro")
    for x, y in zip([xs[0]] + xs, [ys[0]] + ys):
        eager.update(x, y)
    graphed = MulticlassF1Score(num_classes=5, average="macro")
    sx, sy = xs[0].clone(), ys[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graphed.update(sx, sy)                           # warm-up: allocates the state, counts the first batch once
        accuracy(sx, sy)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        graphed.update(sx, sy)
        acc = accuracy(sx, sy)[0]
    for x, y in zip(xs, ys):
        sx.copy_(x)
        sy.copy_(y)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, accuracy(x, y)[0])
    assert torch.equal(graphed.conf, eager.conf)
    assert torch.equal(graphed.compute(), eager.compute())


@pytest.mark.parametrize("key", METRIC_KEYS)
def test_metrics_match_golden(z, key):
    x, y = _metric_case(z, key)
    C = x.shape[1]
    auc = MulticlassAUROC(num_classes=C, average=None).update(x, y).compute()
    assert auc.dtype == torch.float64 and auc.device.type == "cuda" and auc.shape == (C,)
    want = z[key + "/auroc"]
    np.testing.assert_allclose(auc.cpu().numpy(), want, rtol=0, atol=1e-12, equal_nan=True)
    macro = MulticlassAUROC(num_classes=C).update(x, y).compute()
    assert macro.shape == () and np.allclose(macro.item(), want.mean(), rtol=0, atol=1e-12, equal_nan=True)
    for avg in F1_AVERAGES:
        f1 = MulticlassF1Score(num_classes=C, average=avg).update(x, y).compute()
        w = z[f"{key}/f1_{avg or 'none'}"]
        assert f1.dtype == torch.float64 and tuple(f1.shape) == w.shape
        np.testing.assert_allclose(f1.cpu().numpy(), w, rtol=0, atol=1e-12)
    pred = torch.from_numpy(argmax_np(x.cpu().numpy())).cuda()            # predicted labels instead of scores
    f1p = MulticlassF1Score(num_classes=C, average="macro").update(pred, y.to(torch.int32)).compute()
    assert abs(f1p.item() - z[key + "/f1_macro"]) <= 1e-12
    assert abs(MulticlassF1Score().update(x, y).compute().item() - z[key + "/f1_micro"]) <= 1e-12
    acc = accuracy(x, y, topk=(1,))
    assert isinstance(acc, list) and len(acc) == 1 and acc[0].shape == ()
    assert abs(acc[0].item() / 100 - z[key + "/acc"]) <= 1e-6


def test_chunked_updates_and_merge_state_equal_one_update(z):
    x, y = _metric_case(z, "met/N1000_C5/i")
    one_a = MulticlassAUROC(num_classes=5, average=None).update(x, y).compute()
    one_f = MulticlassF1Score(num_classes=5, average=None).update(x, y).compute()
    bounds = [0, 1, 300, 301, 777, 1000]
    ca, cf = MulticlassAUROC(num_classes=5, average=None), MulticlassF1Score(num_classes=5, average=None)
    parts_a, parts_f = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        ca.update(x[a:b], y[a:b])
        cf.update(x[a:b], y[a:b])
        parts_a.append(MulticlassAUROC(num_classes=5, average=None).update(x[a:b], y[a:b]))
        parts_f.append(MulticlassF1Score(num_classes=5, average=None).update(x[a:b], y[a:b]))
    assert torch.equal(ca.compute(), one_a) and torch.equal(cf.compute(), one_f)
    ma = parts_a[0].merge_state(parts_a[1:])
    mf = parts_f[0].merge_state(parts_f[1:])
    assert torch.equal(ma.compute(), one_a) and torch.equal(mf.compute(), one_f)
    assert torch.equal(ca.compute(), ca.compute())                        # compute() leaves the state alone
    ca.reset()
    cf.reset()
    with pytest.raises(ValueError):
        ca.compute()
    with pytest.raises(ValueError):
        cf.compute()


def test_out_of_range_labels_raise_at_compute():
    x = torch.randn(8, 4, device="cuda")
    y = torch.tensor([0, 1, 2, 3, 4, 0, 1, -1], device="cuda")
    f1 = MulticlassF1Score(num_classes=4, average="macro").update(x, y)      # update() does not wait on the host
    with pytest.raises(ValueError, match="outside"):
        f1.compute()
    with pytest.raises(ValueError, match="outside"):
        MulticlassAUROC(num_classes=4).update(x, y).compute()
    acc = accuracy(x, y)[0].item()                                           # timm counts such rows as wrong
    want = (argmax_np(x.cpu().numpy()) == y.cpu().numpy()).mean() * 100
    assert abs(acc - want) <= 1e-4


def _sorted_u2(y, s, c):
    """U2 of class c by sorting (no pair loop): 2 #{neg < pos} + #{neg == pos}."""
    pos, neg = np.sort(s[y == c, c]), np.sort(s[y != c, c])
    lo, hi = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
    return int(2 * lo.sum() + (hi - lo).sum())


def test_large_inputs_and_wide_confusion():
    g = np.random.default_rng(7)
    N, C = 70000, 3                                       # more j chunks than blocks along y: the chunk loop strides
    s = g.integers(-20, 21, (N, C)).astype(np.float32)
    y = g.integers(0, C, N)
    auc = MulticlassAUROC(num_classes=C, average=None).update(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()).compute()
    for c in range(C):
        P = int((y == c).sum())
        assert auc[c].item() == _sorted_u2(y, s, c) / (2.0 * P * (N - P))
    C = 100                                               # C * C above the LDS copy: global atomics
    x = g.normal(size=(5000, C)).astype(np.float32)
    yl = g.integers(0, C, 5000)
    conf = confusion_np(yl, argmax_np(x), C)
    for avg in F1_AVERAGES:
        got = MulticlassF1Score(num_classes=C, average=avg).update(torch.from_numpy(x).cuda(), torch.from_numpy(yl).cuda()).compute()
        np.testing.assert_allclose(got.cpu().numpy(), f1_np(conf, avg), rtol=0, atol=1e-12)


def _worker_sync(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(40 + rank)
        n = 300 + 137 * rank                              # ranks hold different sample counts: the padded gather
        x = torch.randint(-3, 4, (n, 4), generator=g).float().cuda()
        y = torch.randint(0, 4, (n,), generator=g).cuda()
        auc = MulticlassAUROC(num_classes=4).update(x, y)
        f1 = MulticlassF1Score(num_classes=4, average="weighted").update(x, y)
        q.put((rank, sync_and_compute(auc).item(), sync_and_compute(f1).item(), f1.conf.cpu().numpy(), x.cpu().numpy(),
               y.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_sync_and_compute_over_two_gloo_ranks_equals_the_union():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 90)
    procs = [ctx.Process(target=_worker_sync, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    x = torch.from_numpy(np.concatenate([res[0][4], res[1][4]])).cuda()
    y = torch.from_numpy(np.concatenate([res[0][5], res[1][5]])).cuda()
    auc = MulticlassAUROC(num_classes=4).update(x, y).compute().item()
    f1 = MulticlassF1Score(num_classes=4, average="weighted").update(x, y).compute().item()
    assert res[0][1] == res[1][1] == auc
    assert res[0][2] == res[1][2] == f1
    assert res[0][3].sum() == 300                         # each rank's own metric kept its state


def test_linear_probe_at_the_subtyping_template_geometry():
    import mirror_amd.models as M
    torch.manual_seed(0)
    model = M.create_model("mirror_classifier", wsi_embed_dim=768, rna_embed_dim=10234, embed_dim=768, num_classes=4,
                           rna_encoder_depth=2, rna_mlp_ratio=4.0, rna_norm_layer="layernorm", rna_act_layer="gelu", fusion="concat")
    model.head.weight.data.normal_(mean=0.0, std=0.01)
    model.head.bias.data.zero_()
    for _, p in model.named_parameters():
        p.requires_grad = False
    for _, p in model.head.named_parameters():
        p.requires_grad = True
    model = model.cuda()
    model.precision = "fp32"
    model.eval()
    assert model.head.in_features == 1536 and model.head.out_features == 4
    g = torch.Generator().manual_seed(1)
    B = 16
    wsi = torch.randn(B, 2048, 768, generator=g).cuda()
    rna = torch.randn(B, 10234, generator=g).cuda()
    labels = torch.randint(0, 4, (B,), generator=g)                 # host labels, as the trainer leaves them
    with torch.no_grad():
        feats = torch.cat((model.wsi_encoder(wsi), model.rna_encoder(rna)), dim=1).double().cpu()
    W = model.head.weight.detach().double().cpu().requires_grad_(True)
    b = model.head.bias.detach().double().cpu().requires_grad_(True)
    lr = 1e-3
    opt = torch.optim.Adam(model.head.parameters(), lr=lr)
    opt_ref = torch.optim.Adam([W, b], lr=lr)
    loss_fn = LabelSmoothingCrossEntropy(smoothing=0.1)
    W0 = W.detach().clone()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(wsi, rna), labels)
        loss.backward()
        opt.step()
        opt_ref.zero_grad(set_to_none=True)
        ref = torch.nn.functional.cross_entropy(feats @ W.t() + b, labels, label_smoothing=0.1)
        ref.backward()
        assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
        assert _rel(model.head.weight.grad.double().cpu().numpy(), W.grad.numpy()) <= 1e-4
        assert _rel(model.head.bias.grad.double().cpu().numpy(), b.grad.numpy()) <= 1e-4
        opt_ref.step()
    for name, p in model.named_parameters():
        if not name.startswith("head."):
            assert p.grad is None, name
    dW_got = model.head.weight.detach().double().cpu() - W0
    dW_ref = W.detach() - W0
    assert float((dW_got - dW_ref).norm()) <= 1e-2 * float(dW_ref.norm())
