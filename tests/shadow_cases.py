"""The re-pointed-weight case of functional.shadow / shadow_t, shared by the GPU test and its CPU twin (which runs it with the
two kernels replaced by torch stand-ins)."""
import torch


def check_repointed_weights(dev):
    """`p.data = ...` (TrainEngine, ModelEmaV3.attach, model.to()) keeps the parameter object and its version counter and frees
    its block.  A second tensor on that block (made before the re-pointing: on it by construction) must get copies of its own
    contents, and the parameter copies of its new ones, for self-made and for kept copies."""
    from mirror_amd import functional as Fn
    bf = torch.bfloat16

    def full(v):
        return torch.full((64, 128), v, device=dev)

    def same(t, v, shape):
        return t.dtype == bf and tuple(t.shape) == shape and bool((t.float() == v).all())

    p = torch.nn.Parameter(full(1.5))
    assert same(Fn.shadow(p, Fn.BF16), 1.5, (64, 128)) and same(Fn.shadow_t(p, Fn.BF16), 1.5, (128, 64))
    w2 = p.data
    p.data = full(0.75)
    w2.data.fill_(-2.0)
    assert w2.data_ptr() != p.data_ptr() and w2._version == p._version == 0
    assert same(Fn.shadow(w2, Fn.BF16), -2.0, (64, 128)) and same(Fn.shadow_t(w2, Fn.BF16), -2.0, (128, 64))
    assert same(Fn.shadow(p, Fn.BF16), 0.75, (64, 128)) and same(Fn.shadow_t(p, Fn.BF16), 0.75, (128, 64))

    q = torch.nn.Parameter(full(3.0))
    kept, kept_t = torch.full((64, 128), 3.0, device=dev, dtype=bf), torch.full((128, 64), 3.0, device=dev, dtype=bf)
    Fn.register_shadow(q, kept)
    Fn.register_shadow_t(q, kept_t)
    assert Fn.shadow(q, Fn.BF16) is kept and Fn.shadow(q, Fn.BF16) is kept and Fn.shadow_t(q, Fn.BF16) is kept_t
    w3 = q.data
    q.data = full(0.25)
    w3.data.fill_(0.5)
    assert same(Fn.shadow(w3, Fn.BF16), 0.5, (64, 128)) and same(Fn.shadow_t(w3, Fn.BF16), 0.5, (128, 64))
    assert same(Fn.shadow(q, Fn.BF16), 0.25, (64, 128)) and same(Fn.shadow_t(q, Fn.BF16), 0.25, (128, 64))
    # a keeper that registers again (for the new block) is served again; None withdraws
    Fn.register_shadow(q, kept)
    assert Fn.shadow(q, Fn.BF16) is kept
    Fn.register_shadow(q, None)
    assert same(Fn.shadow(q, Fn.BF16), 0.25, (64, 128))
