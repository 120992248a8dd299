"""GPU: attn1's backward (mh_nys_attn1_bwd, one kernel) against an f64 restatement, held to the error of the two-kernel path it replaced.

That path (a dw2 / dk_l / delta1 kernel, then a dq kernel; removed since) multiplied the same bf16 operands into f32 accumulators and
rounded P1 / dS1 to bf16 between the products; at most the order of the sums and of the f32 atomics differs.  So the one-pass kernel
gets no tolerance of its own: its max error against f64 must stay within 1.5 x what the two-kernel path had on these inputs, per output
(BASE_ERR, recorded while that path could still be run)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mirror_amd import kernels as K  # noqa: E402

DEV = "cuda"
M, DH = 256, 64

# geometry: "c2" is what the flagship step runs per layer (B = 16, 8 heads, 4096 tokens + class token padded to 17 x 256 rows)
CASES = {"c2": dict(B=16, h=8, l=17, masked=False, seed=601), "masked": dict(B=2, h=2, l=3, masked=True, seed=602)}

# max |error| against f64 of the two-kernel path, measured on commit 2e89eac (the parent of the one-pass kernel, where that path was
# what the step ran) on an MI355X with this file's seeded inputs: profiles/r06_a_a1_bwd_errors_vs_f64_parent.txt
BASE_ERR = {
    "c2": {"dq": 3.353691e-02, "dw2": 1.949702e-02, "dk_l": 3.680489e-02, "delta1": 5.848020e-02},
    "masked": {"dq": 1.594493e-02, "dw2": 8.857098e-03, "dk_l": 2.309033e-02, "delta1": 2.913021e-02},
}
MARGIN = 1.5


def _inputs(B, h, l, masked, seed):
    gen = torch.Generator().manual_seed(seed)
    D, n_p, bf = h * DH, M * l, torch.bfloat16
    qkv = (torch.randn((B, n_p, 3 * D), generator=gen) * 1.5).to(bf)
    lm = (torch.randn((B, M, 2 * D), generator=gen) * 1.5).to(bf)
    w2 = torch.randn((B, h, M, DH), generator=gen).to(bf)
    dout = torch.randn((B, n_p, D), generator=gen).to(bf)
    kmask = None
    if masked:      # front padding + a ragged valid length per sample; landmark group j covers rows [j l, (j + 1) l)
        mrow = torch.zeros(B, n_p)
        for b in range(B):
            mrow[b, 5 + 40 * b:n_p - (17 + 100 * b)] = 1.0
        mlm = (mrow.reshape(B, M, l).sum(-1) > 0).float()
        assert float(mlm.min()) == 0.0 and float(mrow.min()) == 0.0
        kmask = (mrow.to(DEV), mlm.to(DEV))
    return tuple(t.to(DEV) for t in (qkv, lm, w2, dout)), kmask


def _reference(qkv, lm, w2, dout, kmask, h):
    """attn1's backward in f64 (on the device): P1 = softmax(scale q k_l^T), dP1 = dO w2^T, delta1 = sum_l P1 dP1,
    dS1 = P1 (dP1 - delta1) scale (zero at masked logits), dq = dS1 k_l, dk_l = dS1^T q, dw2 = P1^T dO."""
    B, n_p, D3 = qkv.shape
    D, scale = D3 // 3, DH ** -0.5

    def heads(t, which, parts):
        return t.double().view(B, t.shape[1], parts, h, DH)[:, :, which].permute(0, 2, 1, 3)

    q, kl, dO, w = heads(qkv, 0, 3), heads(lm, 1, 2), heads(dout, 0, 1), w2.double()
    s = scale * q @ kl.transpose(-1, -2)
    valid = None
    if kmask is not None:
        valid = kmask[0].bool()[:, None, :, None] & kmask[1].bool()[:, None, None, :]
        s = s.masked_fill(~valid, -torch.finfo(torch.float32).max)
    p = torch.softmax(s, -1)
    dp = dO @ w.transpose(-1, -2)
    delta = (p * dp).sum(-1)
    ds = p * (dp - delta[..., None]) * scale
    if valid is not None:
        ds = ds.masked_fill(~valid, 0.0)
    dq = (ds @ kl).permute(0, 2, 1, 3).reshape(B, n_p, D)
    dkl = (ds.transpose(-1, -2) @ q).permute(0, 2, 1, 3).reshape(B, M, D)
    return {"dq": dq, "dw2": p.transpose(-1, -2) @ dO, "dk_l": dkl, "delta1": delta}


def run_case(name):
    """The device outputs and the f64 reference for one geometry."""
    c = CASES[name]
    B, h, l = c["B"], c["h"], c["l"]
    (qkv, lm, w2, dout), kmask = _inputs(B, h, l, c["masked"], c["seed"])
    D, n_p, scale = h * DH, M * l, DH ** -0.5
    out = torch.empty((B, n_p, D), device=DEV, dtype=torch.bfloat16)
    o1 = torch.empty_like(out)
    lse1 = K.nys_attn1_fwd(qkv, lm, w2, out, h, scale, kmask=kmask, o1=o1)
    dqkv = torch.full_like(qkv, float("nan"))
    dw2 = torch.zeros((B, h, M, DH), device=DEV)
    dlm = torch.zeros((B, M, 2 * D), device=DEV)
    delta1 = torch.full((B, h, n_p), float("nan"), device=DEV)
    K.nys_attn1_bwd(qkv, lm, w2, dout, lse1, o1, delta1, dqkv, dw2, dlm, h, scale, kmask=kmask)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv[..., D:]).all()), "attn1's backward writes the q block of dqkv only"
    assert float(dlm[..., :D].abs().max()) == 0.0, "attn1's backward adds into the k_l half of dlm only"
    got = {"dq": dqkv[..., :D], "dw2": dw2, "dk_l": dlm[..., D:], "delta1": delta1}
    return got, _reference(qkv, lm, w2, dout, kmask, h), kmask


def max_errors(got, ref):
    return {k: float((got[k].double() - ref[k]).abs().max()) for k in ref}


@pytest.mark.parametrize("name", list(CASES))
def test_nys_attn1_bwd_one_pass(name):
    got, ref, kmask = run_case(name)
    err = max_errors(got, ref)
    for k in ref:
        print(f"{name} {k}: |ref| max {float(ref[k].abs().max()):.4e}  one-pass err {err[k]:.4e}  (two-kernel baseline {BASE_ERR[name][k]})")
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), k
        base = BASE_ERR[name][k]
        assert err[k] <= MARGIN * base, f"{name} {k}: one-pass max error {err[k]:.4e} > {MARGIN} x {base:.4e} (two-kernel path)"
    if kmask is not None:      # rows a key-padding mask removes get no gradient through sim1: exactly zero
        dead = kmask[0] == 0
        assert int(dead.sum()) > 0 and float(got["dq"][dead].abs().max()) == 0.0
