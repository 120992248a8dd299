"""CPU: the acceptance rule of functional._Handover, alone, on toy autograd Functions (no kernel, no library call).

A backward node that writes a gradient tensor g may leave a by-product of g for the node whose backward receives g.  The receiver
may use it only when what it receives is g untouched: the same storage, shape and strides, at the version g had when it was offered,
with g kept alive by the slot in between.  The cases below are the ways autograd delivers something else: the sum with a second
consumer's gradient (out of place, and IN PLACE into g when nobody else holds it — the case a bare address comparison accepts), a hook
that returns a copy, a hook that edits g in place."""
import pytest
import torch

from mirror_amd import functional as Fn


class _P(torch.autograd.Function):
    """Producer: s = 1 * x; its backward claims and records (by-products or None, the gradient's values it received)."""

    @staticmethod
    def forward(ctx, x, slot, seen):
        ctx.slot, ctx.seen = slot, seen
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.seen.append((ctx.slot.claim(g), g.clone()))
        ctx.seen.append(ctx.slot.claim(g))      # a hand-over is consumed once
        return g, None, None


class _A(torch.autograd.Function):
    """Consumer that offers (its returned gradient 2 * dy, a marker)."""

    @staticmethod
    def forward(ctx, s, slot):
        ctx.slot = slot
        return s * 2.0

    @staticmethod
    def backward(ctx, dy):
        g = dy * 2.0
        ctx.slot.offer(g, "marker", 7)
        return g, None


class _B(torch.autograd.Function):
    """Consumer that offers nothing; its gradient is 3 * dy."""

    @staticmethod
    def forward(ctx, s):
        return s * 3.0

    @staticmethod
    def backward(ctx, dy):
        return dy * 3.0


def _run(order, hook=None):
    """order: the consumers of s in creation order.  Returns (first claim, gradient P received, second claim, tap, x.grad)."""
    x = torch.ones(4, requires_grad=True)
    slot, seen = Fn._Handover("toy"), []
    tap, Fn._handover_tap = Fn._handover_tap, []
    try:
        s = _P.apply(x, slot, seen)
        if hook is not None:
            s.register_hook(hook)
        outs = [_A.apply(s, slot) if c == "A" else _B.apply(s) for c in order]
        sum(o.sum() for o in outs).backward()
        rec = Fn._handover_tap
    finally:
        Fn._handover_tap = tap
    (first, g), second = seen
    return first, g, second, rec, x.grad


def test_single_consumer_is_accepted_once():
    first, g, second, tap, xg = _run("A")
    assert first == ("marker", 7) and second is None
    assert tap == [("toy", "offered"), ("toy", "accepted")]
    assert torch.equal(g, torch.full((4,), 2.0)) and torch.equal(xg, g)


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_second_consumer_is_rejected_and_the_producer_receives_the_sum(order):
    """"BA": A's backward runs first and its gradient waits in autograd's buffer, where B's would be added IN PLACE if the slot did not
    hold it — same address, other contents.  "AB": B's gradient is there first and the sum is another tensor."""
    first, g, second, tap, xg = _run(order)
    assert first is None and second is None
    assert tap == [("toy", "offered"), ("toy", "rejected")]
    assert torch.equal(g, torch.full((4,), 5.0)) and torch.equal(xg, g)


def test_hook_that_returns_a_copy_is_rejected():
    first, g, second, tap, _ = _run("A", hook=lambda g: g.clone())
    assert first is None and second is None and tap == [("toy", "offered"), ("toy", "rejected")]
    assert torch.equal(g, torch.full((4,), 2.0))


def test_hook_that_edits_in_place_is_rejected():
    first, g, second, tap, _ = _run("A", hook=lambda g: g.mul_(2))
    assert first is None and second is None and tap == [("toy", "offered"), ("toy", "rejected")]
    assert torch.equal(g, torch.full((4,), 4.0))


def test_another_view_of_the_same_storage_is_rejected_and_the_tap_is_off_by_default():
    assert Fn._handover_tap is None
    slot, g = Fn._Handover("toy"), torch.zeros(2, 6)
    slot.offer(g, 1)
    assert slot.claim(g.view(3, 4)) is None and slot.claim(g) is None      # cleared either way
    slot.offer(g, 1)
    assert slot.claim(g.t()) is None
    slot.offer(g, 1)
    assert slot.claim(g) == (1,)
