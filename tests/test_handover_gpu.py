"""GPU: the three backward hand-overs of functional.py (_Handover) where the taker must REJECT the by-product, bf16 policy.

A backward node whose kernel writes a gradient g may leave a by-product of g for the node that receives g: the Dropout-masked bf16
copy + its column sums (LayerNormFn -> ToOutDropAddFn), the per-block column sums (masked-MSE backward -> HeadSqErrFn), the
ReLU-masked bf16 copy + its column sums (NormQkvLmFn -> Fc1SeqFn).  With a second consumer of the tensor, or a gradient hook on it,
what arrives is not g and the taker has to run its own pass.  Every case compares against the same graph with the producer-side
fusion switched off (_DROP_IN_LN_BWD, _BIAS_IN_PRODUCER, _RELU_IN_LN_BWD) at the bars of test_fused_epilogue_gpu.py — masked and
data gradients torch.equal, bias and weight gradients within 1e-5 of max|ref| (f32 atomics / split-K order) — and asserts through
Fn._handover_tap that the hand-over was offered, and accepted or rejected: a shape off a gate cannot pass vacuously."""
import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32

VARIANTS = ("single", "second_before", "second_after", "hook_mul")
VERDICT = {"single": "accepted", "second_before": "rejected", "second_after": "rejected", "hook_mul": "rejected"}


def _w(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).cuda().requires_grad_(True)
    b = (torch.randn(n, generator=g) * 0.1).cuda().requires_grad_(True)
    return w, b


def _consume(t, variant, c, main):
    """loss = main(t) [+ (t * c).sum() as a second consumer of t, created before or after main's node]; hook_mul: t's gradient is
    doubled in place on its way to t's producer."""
    if variant == "hook_mul":
        t.register_hook(lambda g: g.mul_(2))
    side = (t * c).sum() if variant == "second_before" else None
    loss = main(t)
    if variant == "second_after":
        side = (t * c).sum()
    return loss if side is None else loss + side.to(loss.dtype)


def _compare(got, ref, exact, label):
    """exact: indices of the masked / data gradients (bit-equal); the rest are f32 sums whose order may differ."""
    figures = []
    for i, (a, c) in enumerate(zip(got, ref)):
        d, top = float((a.float() - c.float()).abs().max()), float(c.float().abs().max())
        figures.append((i, d, top))
    print(label, "max |got - ref|, max |ref| per gradient:", figures)
    for i, d, top in figures:
        if i in exact:
            assert d == 0.0 and torch.equal(got[i], ref[i]), (label, i, d, top)
        else:
            assert d <= 1e-5 * top, (label, i, d, top)


@pytest.mark.parametrize("variant", VARIANTS)
def test_dropout_site_is_claimed_only_for_the_layernorms_own_dx(variant, monkeypatch):
    """x = resid + Dropout(to_out(core)) read by a LayerNorm: its backward leaves the Dropout's backward of its dx for ToOutDropAddFn.
    [2, 300, 256]: 600 flat rows = two whole 256-row tiles + a ragged one, more than one block of the LayerNorm backward."""
    from mirror_amd import functional as Fn
    prec = Fn.POLICIES["bf16"]
    g = torch.Generator().manual_seed(31)
    core0 = torch.randn(2, 300, 256, generator=g).cuda().to(bf16)
    resid0 = torch.randn(2, 300, 256, generator=g).cuda()
    up = torch.randn(2, 300, 256, generator=g).cuda()
    c = torch.randn(2, 300, 256, generator=g).cuda()
    gam0, bet0 = torch.randn(256, generator=g).cuda(), torch.randn(256, generator=g).cuda()
    w, b = _w(256, 256, 32)
    res, tap = [], []
    for fused in (True, False):
        monkeypatch.setattr(Fn, "_DROP_IN_LN_BWD", fused)
        monkeypatch.setattr(Fn, "_handover_tap", tap if fused else None)
        Fn.manual_seed(77)
        Fn._dropout_state["offset"] = 4096          # a non-zero call offset, a multiple of 8
        core, resid = core0.clone().requires_grad_(True), resid0.clone().requires_grad_(True)
        gam, bet = gam0.clone().requires_grad_(True), bet0.clone().requires_grad_(True)
        w.grad = b.grad = None
        x = Fn.to_out_dropout_add(resid, core, w, b, 0, 300, 0.1, True, prec)
        assert x.grad_fn.__class__.__name__.startswith("ToOutDropAddFn") and hasattr(x, "_drop_site") == fused
        _consume(x, variant, c, lambda t: (Fn.layer_norm(t, gam, bet, 1e-5) * up).sum()).backward()
        res.append([t.grad.clone() for t in (core, resid, w, b, gam, bet)])
    torch.cuda.synchronize()
    _compare(res[0], res[1], exact=(0, 1), label=f"dropout site, {variant}:")
    assert tap == [("drop", "offered"), ("drop", VERDICT[variant])], tap


def _head_and_loss(Fn, variant, tgt_edit=None):
    prec = Fn.POLICIES["bf16"]
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, 257, 256, generator=g).cuda().to(bf16).requires_grad_(True)
    tgt = torch.randn(2, 256, 256, generator=g).cuda()
    mask = (torch.rand(2, 256, generator=g) < 0.75).float().cuda()
    c = torch.randn(2, 256, 256, generator=g).cuda().to(bf16)
    w, b = _w(256, 256, 42)
    pred = Fn.head_sqerr(x, w, b, 1, 256, prec, tgt, mask)
    assert hasattr(pred, "_sq"), "the fused path was not taken"
    if tgt_edit is not None:
        tgt_edit(tgt)
    loss = _consume(pred, variant, c, lambda t: Fn.masked_mse(t, tgt, mask, 256))
    return loss, pred, tgt, mask, (x, w, b)


@pytest.mark.parametrize("variant", VARIANTS)
def test_column_sum_table_is_claimed_only_for_the_mse_backwards_own_dpred(variant, monkeypatch):
    """pred = retention_head(x)[:, 1:] with the squared error in its epilogue, then the masked MSE: its backward leaves the per-block
    column sums of dpred for the head's bias gradient.  [2, 256, 256]: 512 flat rows = two 256-row tiles, several MSE blocks."""
    from mirror_amd import functional as Fn
    res, tap = [], []
    for fused in (True, False):
        monkeypatch.setattr(Fn, "_BIAS_IN_PRODUCER", fused)
        monkeypatch.setattr(Fn, "_handover_tap", tap if fused else None)
        loss, pred, _, _, leaves = _head_and_loss(Fn, variant)
        assert (pred._sq_cs is not None) == fused
        loss.backward()
        res.append([t.grad.clone() for t in leaves])
    torch.cuda.synchronize()
    _compare(res[0], res[1], exact=(0,), label=f"column-sum table, {variant}:")
    assert tap == [("colsum", "offered"), ("colsum", VERDICT[variant])], tap


def test_squared_error_accumulator_is_dropped_when_the_target_was_written_since(monkeypatch):
    """The target is written in place between the head's launch and the loss: the accumulator on the prediction belongs to the old
    contents, and the loss must be mh_mse_masked_fwd's on the new ones, bit for bit: the loss then runs that very launch (block-ordered
    sums: the same inputs give the same bits) and divides the same way; nothing is offered for the bias gradient either."""
    from mirror_amd import functional as Fn
    tap = []
    monkeypatch.setattr(Fn, "_handover_tap", tap)
    loss, pred, tgt, mask, leaves = _head_and_loss(Fn, "single", tgt_edit=lambda t: t.add_(1.0))
    stale = Fn._div(pred._sq[0])
    acc0 = torch.zeros(2, device="cuda")
    Fn.K.mse_masked_fwd(pred.detach(), tgt, mask, acc0, 2 * 256, 256)
    want = float(acc0[0] / acc0[1])
    print("loss", float(loss), "mse kernel on the new target", want, "accumulator of the old target", float(stale))
    assert float(loss) == want
    assert abs(float(stale) - want) > 1e-2 * want, "the edit did not move the loss: the case checks nothing"
    assert Fn._sq_of(pred, tgt, mask) is None
    loss.backward()
    torch.cuda.synchronize()
    assert tap == [] and all(t.grad is not None for t in leaves)
    # and the mask: the same rule
    loss2, pred2, tgt2, mask2, _ = _head_and_loss(Fn, "single")
    assert Fn._sq_of(pred2, tgt2, mask2) is pred2._sq[0]
    mask2.zero_()
    assert Fn._sq_of(pred2, tgt2, mask2) is None


def test_relu_slot_rejected_leaves_nothing_in_the_gradient_arena(monkeypatch):
    """Whole model under a TrainEngine (its gradient arena is the sink), D = 512 / 1024 tokens / B = 2, train mode: the configuration of
    test_whole_model_round5_fusions_on_off.  (1) As it is: every hand-over that is offered is accepted, all three kinds are on the
    path.  (2) With a hook on Fc1SeqFn's sequence that returns a copy of its gradient, the ReLU slot is rejected and _fc1's gradients
    and the cls token's equal those of the _RELU_IN_LN_BWD = False step at that test's bars.  Two things have to hold for that: the
    bias gradient that layer 1's LayerNorm backward computed reaches the arena only on acceptance (else it is counted twice), and
    the f32 gradient that arrives, which lacks that LayerNorm's share on the ReLU rows (its ReLU form writes it to the bf16 tensor
    only), gets that share back (_ReluSlot.redo)."""
    import mirror_amd.models as M
    from mirror_amd import functional as Fn
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    cfg = dict(wsi_embed_dim=256, rna_embed_dim=96, embed_dim=512, wsi_num_tokens=1024, rna_encoder_depth=1, rna_num_heads=8,
               rna_mlp_ratio=4.0, style_mlp_hidden_dim=128, style_mlp_out_dim=64, style_latent_dim=32, num_prototypes=300)
    g = torch.Generator().manual_seed(15)
    wsi = torch.randn(2, 1024, 256, generator=g).cuda().to(bf16)
    rna = torch.randn(2, 96, generator=g).cuda()
    noise = {"wsi_mask": torch.rand(2, 1024, generator=g).cuda(), "rna_mask": torch.rand(2, 512, generator=g).cuda(),
             "wsi_eps": torch.randn(2, 32, generator=g).cuda(), "rna_eps": torch.randn(2, 32, generator=g).cuda()}
    keys = ("wsi_encoder._fc1.0.weight", "wsi_encoder._fc1.0.bias", "wsi_encoder.cls_token")

    def step():
        torch.manual_seed(0)
        model = M.mirror(**cfg).cuda().train()
        eng = TrainEngine(model, MIRRORLoss(), lr=0.0, precision="bf16", graph=False, seed=99, snapshot_grads=True)
        tap = []
        monkeypatch.setattr(Fn, "_handover_tap", tap)
        eng.step(wsi, rna, noise=noise)
        torch.cuda.synchronize()
        monkeypatch.setattr(Fn, "_handover_tap", None)
        at = {id(p): o for p, o in zip(eng.params, eng.offsets)}
        return tap, {k: eng.grad_snap[at[id(p)]:at[id(p)] + p.numel()].double().clone() for k, p in model.named_parameters() if k in keys}

    plain, _ = step()
    orig = Fn.fc1_seq

    def hooked(*a, **k):
        seq = orig(*a, **k)
        seq.register_hook(lambda g: g.clone())
        return seq
    monkeypatch.setattr(Fn, "fc1_seq", hooked)
    tap, got = step()
    monkeypatch.setattr(Fn, "_RELU_IN_LN_BWD", False)
    off, ref = step()
    assert set(got) == set(keys)
    figures = {k: (float(got[k] @ ref[k] / (got[k].norm() * ref[k].norm())), float(got[k].norm() / ref[k].norm())) for k in keys}
    print("rejected ReLU slot vs _RELU_IN_LN_BWD = False, (cosine, norm ratio):", figures)
    for k, (cos, ratio) in figures.items():
        assert cos >= 0.99995 and abs(ratio - 1.0) <= 1e-3, (k, cos, ratio)
    offered = sorted(w for w, what in plain if what == "offered")
    assert sorted(w for w, what in plain if what == "accepted") == offered and not [t for t in plain if t[1] == "rejected"], plain
    assert set(offered) == {"relu", "drop", "colsum"}, plain
    assert [t for t in tap if t[0] == "relu"] == [("relu", "offered"), ("relu", "rejected")], tap
    assert not [t for t in tap if t[0] != "relu" and t[1] == "rejected"], tap
    assert not [t for t in off if t[0] == "relu"], off


def test_relu_slot_with_a_gradient_edited_in_place_is_loud(monkeypatch):
    """A hook that edits the sequence's gradient in place: the LayerNorm's share of the ReLU rows never passed through it, so no
    fallback can be right (_ReluSlot) — the backward raises instead of returning _fc1 gradients of 2 * add + ln for 2 * (add + ln)."""
    import mirror_amd.models as M
    from mirror_amd import functional as Fn
    from mirror_amd.losses import MIRRORLoss
    cfg = dict(wsi_embed_dim=256, rna_embed_dim=96, embed_dim=512, wsi_num_tokens=1024, rna_encoder_depth=1, rna_num_heads=8,
               rna_mlp_ratio=4.0, style_mlp_hidden_dim=128, style_mlp_out_dim=64, style_latent_dim=32, num_prototypes=300)
    g = torch.Generator().manual_seed(15)
    wsi = torch.randn(2, 1024, 256, generator=g).cuda().to(bf16)
    rna = torch.randn(2, 96, generator=g).cuda()
    noise = {"wsi_mask": torch.rand(2, 1024, generator=g).cuda(), "rna_mask": torch.rand(2, 512, generator=g).cuda(),
             "wsi_eps": torch.randn(2, 32, generator=g).cuda(), "rna_eps": torch.randn(2, 32, generator=g).cuda()}
    orig = Fn.fc1_seq

    def hooked(*a, **k):
        seq = orig(*a, **k)
        seq.register_hook(lambda g: g.mul_(2))
        return seq
    monkeypatch.setattr(Fn, "fc1_seq", hooked)
    tap = []
    monkeypatch.setattr(Fn, "_handover_tap", tap)
    torch.manual_seed(0)
    model = M.mirror(**cfg).cuda().train()
    model.precision = "bf16"
    Fn.manual_seed(99)
    losses = MIRRORLoss()(*model(wsi, rna, noise=noise))
    with pytest.raises(Fn.K.MirrorHipError, match="edited in place"):
        losses[0].backward()
    torch.cuda.synchronize()
    assert [t for t in tap if t[0] == "relu"] == [("relu", "offered"), ("relu", "rejected")], tap
