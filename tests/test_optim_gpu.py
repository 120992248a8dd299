"""GPU: the arena optimizer with weight decay (mh_optim_step) — each rule against torch.optim in float64 on a 10^6-element arena
with mixed decay groups, a hole and a clamped element; TrainEngine(opt=, weight_decay=, momentum=) against the same model under
torch.optim over timm's parameter groups (eager, clipping + accumulation, EMA, whole-step graph, two ranks, checkpoints)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CFG = dict(wsi_embed_dim=64, rna_embed_dim=48, embed_dim=64, wsi_num_tokens=60, rna_encoder_depth=1, rna_num_heads=8,
           style_mlp_hidden_dim=64, style_mlp_out_dim=32, style_latent_dim=16, num_prototypes=50)
CFG512 = dict(wsi_embed_dim=128, rna_embed_dim=96, embed_dim=512, wsi_num_tokens=1000, rna_encoder_depth=2, rna_num_heads=8,
              rna_mlp_ratio=4.0, style_mlp_hidden_dim=128, style_mlp_out_dim=64, style_latent_dim=32, num_prototypes=300)


# ====================================================================== 1. the kernel against torch.optim
N = 1_000_003                                    # not a multiple of 4: the scalar tail runs
# "parameters" (size, decay group), laid out like TrainEngine's arena: each starts on an 8-element block, padding stays zero
SEGS = [(300001, 1), (1, 0), (4099, 0), (250000, 1), (1000, 0), (444883, 2)]
GROUP_WD = [0.0, 0.05, 0.1]
CLAMP = (300008, 0.0, math.log(100.0))           # the one-element parameter (logit_scale)
HOLE = (302000, 420000)                          # 8-aligned; spans a no-decay parameter, its padding and part of a decaying one
GS, CLIP = 0.5, 0.5                              # grad_scale and the device clip factor: powers of two, exact in every precision
# max relative error of the kernel's update, as a multiple of the float32 torch.optim run's own (both against float64).
# SGD rounds where torch's float32 path rounds, up to FMA contraction: 2.  The Adam rules also read mh_adam's device step state, whose
# 1 - b2^t is formed in float32: b2^t ~ 1 is rounded to 2^-25, so the correction is off by up to 2^-25 / (t (1 - b2)) = 1.5e-5 at
# t = 2 and the step by half of that — about 60 ulp where torch (corrections in float64) spends a few.  The measure is a maximum
# over 10^6 elements and both runs reach it on elements whose three steps nearly cancel (|dp| just above the threshold), where the
# float32 run's error is its rounding of p (an ulp of p, ~ 2^-24 * 1e-2) and the kernel's adds ~ lr * 7e-6: a ratio near 10, not a
# few ulp's worth.  A float32 numpy restatement of the kernel's operation order gives 2.9 (adam_l2) and 6.3 (adamw) on this data;
# the Adam rules get 16.  Measured figures in the docstring of the test below.
MULT = {"adam": 16.0, "adamw": 16.0, "sgd": 2.0}


def _layout():
    offs, o = [], 0
    for n, _ in SEGS:
        offs.append(o)
        o += (n + 7) // 8 * 8
    assert offs[1] == CLAMP[0] and offs[-1] + SEGS[-1][0] == N
    return offs


def _data():
    offs = _layout()
    gen = torch.Generator().manual_seed(1234)
    live = torch.zeros(N, dtype=torch.bool)
    gmap = torch.zeros((N + 7) // 8, dtype=torch.uint8)
    for (n, grp), o in zip(SEGS, offs):
        live[o:o + n] = True
        gmap[o // 8:(o + n + 7) // 8] = grp
    p0 = torch.randn(N, generator=gen) * live
    p0[CLAMP[0]] = 7.0                           # leaves [0, ln 100] after the update
    gs = [torch.randn(N, generator=gen) * live for _ in range(3)]
    e0 = torch.randn(N, generator=gen) * live
    return offs, live, gmap, p0, gs, e0


def _torch_run(rule, mu, nesterov, lr, dtype, offs, p0, gs):
    ps = [p0[o:o + n].to(dtype).clone().requires_grad_() for (n, _), o in zip(SEGS, offs)]
    groups = [{"params": [p for p, (_, grp) in zip(ps, SEGS) if grp == k], "weight_decay": GROUP_WD[k]} for k in range(3)]
    if rule == "adam":
        opt = torch.optim.Adam(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    elif rule == "adamw":
        opt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    else:
        opt = torch.optim.SGD(groups, lr=lr, momentum=mu, nesterov=nesterov)
    for g in gs:
        for p, (n, _), o in zip(ps, SEGS, offs):
            p.grad = g[o:o + n].to(dtype) * (GS * CLIP)
        opt.step()
        with torch.no_grad():
            ps[1].clamp_(CLAMP[1], CLAMP[2])
    out = torch.zeros(N, dtype=dtype)
    for p, (n, _), o in zip(ps, SEGS, offs):
        out[o:o + n] = p.detach()
    return out


def _update_err(x, ref64, p0, live):
    """max over the elements that moved by more than 2^-10 of their value of |x - ref| / |ref - p0|, and how many those are."""
    dp = (ref64 - p0.double()).abs()
    sel = live & (dp > 2.0 ** -10 * p0.double().abs())
    return float(((x.double() - ref64).abs()[sel] / dp[sel]).max()), int(sel.sum())


def _ulp_close(got, want, a, b, k=4):
    """test_ema_gpu.py's tolerance: within k f32 ulps of the lerp's operands."""
    tol = k * 2.0 ** -23 * torch.maximum(a.abs(), b.abs()) + 1e-30
    bad = (got - want).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float((got - want).abs().max()))


def _kernel_run(cfg, lr, gmap, wdt, p0, gs, e0=None, ecfg=None, use_adam=False):
    """Three updates: one launch, two launches (the hole's range early, then the rest around it), one launch."""
    from mirror_amd import kernels as K
    p = p0.cuda()
    m = torch.zeros_like(p) if (cfg is None or cfg.rule != 2 or cfg.momentum != 0.0) else None
    v = torch.zeros_like(p) if (cfg is None or cfg.rule != 2) else None
    sh = torch.zeros(N, device="cuda", dtype=torch.bfloat16)
    e = None if e0 is None else e0.cuda()
    st = torch.tensor([0.0, 0.0, 0.0, lr, CLIP, 0.0], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    lo, hi = HOLE

    def cut(t, a, b):
        return None if t is None else t[a:b]

    def launch(g, a, b, **kw):
        if e is not None:
            kw.update(ema=e[a:b], ema_cfg=ecfg)
        if use_adam:
            K.adam(p[a:b], g[a:b], m[a:b], v[a:b], sh[a:b], lr, 0.9, 0.999, 1e-8, 1.0, 1.0, grad_scale=GS, dev_state=st, **kw)
        else:
            K.optim_step(p[a:b], g[a:b], cut(m, a, b), cut(v, a, b), sh[a:b], cfg, st, grad_scale=GS,
                         group_map=None if gmap is None else gmap[a // 8:], group_wd=wdt, **kw)
    traj = []
    for k, g in enumerate(gs):
        g = g.cuda()
        if k == 1:
            launch(g, lo, hi, tick="early")
            mid = [None if t is None else t.clone() for t in (p, m, v, sh.view(torch.int16), e)]
            launch(g, 0, N, clamp=CLAMP, counter=ctr, counter_add=5, tick=False, hole=HOLE)
            for t, t0 in zip((p, m, v, sh.view(torch.int16), e), mid):       # the hole is bit-untouched by the second launch
                assert t is None or torch.equal(t[lo:hi], t0[lo:hi])
            assert not torch.equal(p[:lo], mid[0][:lo]) and not torch.equal(p[hi:], mid[0][hi:])
        else:
            launch(g, 0, N, clamp=CLAMP, counter=ctr, counter_add=5)
        traj.append((p.clone(), None if e is None else e.clone()))
    torch.cuda.synchronize()
    assert int(ctr) == 15 and float(st[0]) == 3.0
    return p, m, v, sh, st, traj


RULES = {"adam_l2": ("adam", 0.0, False, 1e-2), "adamw": ("adamw", 0.0, False, 1e-2), "sgd_nesterov": ("sgd", 0.9, True, 5e-2),
         "sgd_momentum": ("sgd", 0.9, False, 5e-2), "sgd_plain": ("sgd", 0.0, False, 5e-2)}


@pytest.mark.parametrize("case", list(RULES))
def test_kernel_matches_torch_optim_in_float64(case):
    """Yardstick: the float32 torch.optim run's max relative update error against the float64 run; the kernel gets MULT[rule] times it.
    Measured on an MI355X (yardstick / kernel / ratio): adam_l2 1.131e-03 / 3.250e-03 / 2.87, adamw 2.445e-04 / 1.895e-03 / 7.75,
    sgd_nesterov 1.657e-04 / 1.327e-04 / 0.80, sgd_momentum 1.355e-04 / 1.355e-04 / 1.00, sgd_plain 1.369e-04 / 1.369e-04 / 1.00."""
    from mirror_amd._lib import EmaCfg, OptimCfg
    from mirror_amd.ema import ema_decay
    rule, mu, nesterov, lr = RULES[case]
    offs, live, gmap, p0, gs, e0 = _data()
    ref64 = _torch_run(rule, mu, nesterov, lr, torch.float64, offs, p0, gs)
    ref32 = _torch_run(rule, mu, nesterov, lr, torch.float32, offs, p0, gs)
    cfg = OptimCfg({"adam": 0, "adamw": 1, "sgd": 2}[rule], 0.9, 0.999, 1e-8, mu, int(nesterov))
    gmap_d, wdt = gmap.cuda(), torch.tensor(GROUP_WD).cuda()
    p, m, v, sh, st, first = _kernel_run(cfg, lr, gmap_d, wdt, p0, gs)
    yard, cnt = _update_err(ref32, ref64, p0, live)
    kern, _ = _update_err(p.cpu(), ref64, p0, live)
    print(f"\n[optim {case}] yardstick (torch f32 vs f64) {yard:.3e}  kernel vs f64 {kern:.3e}  ratio {kern / yard:.2f}  over {cnt} elements")
    assert cnt > 0.9 * int(live.sum()), "too few elements moved above rounding: the comparison would see little"
    assert kern <= MULT[rule] * yard, (kern, yard)
    # padding stays zero in every arena, the shadow is the rounded master, SGD never had a second moment
    pad = ~live.cuda()
    for t in (p, m, v):
        assert t is None or not bool(t[pad].any())
    assert torch.equal(sh.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
    assert float(first[0][0][CLAMP[0]]) == float(np.float32(CLAMP[2])), "7.0 is clamped to ln 100 behind the first update"
    assert CLAMP[1] <= float(p[CLAMP[0]]) <= float(np.float32(CLAMP[2]))
    assert (v is None) == (rule == "sgd") and (m is None) == (case == "sgd_plain")
    # with the EMA: the update itself is bit-identical, and the EMA is torch.lerp of each step's final value
    ecfg = EmaCfg(0.9, 0.0, 1.0, 2 / 3, 0, 0)
    p2, m2, v2, sh2, st2, traj = _kernel_run(cfg, lr, gmap_d, wdt, p0, gs, e0=e0, ecfg=ecfg)
    for a, b in ((p, p2), (m, m2), (v, v2), (sh.view(torch.int16), sh2.view(torch.int16)), (st, st2)):
        assert a is None or torch.equal(a, b)
    assert torch.equal(traj[0][1], traj[0][0]), "the first update (t = 1) copies the parameters"
    prev = traj[0][1]
    for t, (pt, et) in enumerate(traj[1:], start=2):
        w = float(np.float32(1.0 - ema_decay(t, 0.9)))
        _ulp_close(et, torch.lerp(prev, pt, w), prev, pt)
        prev = et


def test_rule_adam_without_decay_is_bit_identical_to_mh_adam():
    from mirror_amd._lib import OptimCfg
    offs, live, gmap, p0, gs, e0 = _data()
    cfg = OptimCfg(0, 0.9, 0.999, 1e-8, 0.0, 0)
    want = _kernel_run(None, 1e-2, None, None, p0, gs, use_adam=True)
    zeros = torch.zeros(3).cuda()
    for gm, wdt in ((None, None), (gmap.cuda(), zeros), (None, None)):       # no map; a map whose groups all have wd = 0; again
        got = _kernel_run(cfg, 1e-2, gm, wdt, p0, gs)
        for a, b in zip(want[:5], got[:5]):
            a, b = (a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.bfloat16 else (a, b)
            assert torch.equal(a, b)


# ====================================================================== 2. the engine against torch.optim over timm's groups
def _make(seed=0, cfg=CFG):
    import mirror_amd.models as M
    torch.manual_seed(seed)
    return M.mirror(**cfg).cuda().eval()       # eval: dropout off so runs are comparable


def _batch(b, seed, cfg=CFG):
    g = torch.Generator().manual_seed(seed)
    n, f, gd, d, lat = cfg["wsi_num_tokens"], cfg["wsi_embed_dim"], cfg["rna_embed_dim"], cfg["embed_dim"], cfg["style_latent_dim"]
    wsi, rna = torch.randn(b, n, f, generator=g), torch.randn(b, gd, generator=g)
    noise = {"wsi_mask": torch.rand(b, n, generator=g), "rna_mask": torch.rand(b, d, generator=g),
             "wsi_eps": torch.randn(b, lat, generator=g), "rna_eps": torch.randn(b, lat, generator=g)}
    return wsi.cuda(), rna.cuda(), {k: v.cuda() for k, v in noise.items()}


def _timm_groups(model, weight_decay):
    """timm.optim.param_groups_weight_decay, restated."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        (no_decay if param.ndim <= 1 or name.endswith(".bias") else decay).append(param)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def _torch_opt(kind, model, lr, wd):
    groups = _timm_groups(model, wd)
    if kind == "adamw":
        return torch.optim.AdamW(groups, lr=lr, weight_decay=0.0)
    if kind == "adam":
        return torch.optim.Adam(groups, lr=lr)
    return torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True)


def _ref_steps(kind, lr, wd, steps=3, ema=None):
    from mirror_amd.losses import MIRRORLoss
    ref = _make()
    ref.precision = "fp32"
    opt = _torch_opt(kind, ref, lr, wd)
    e = None if ema is None else ema(ref)
    for step in range(steps):
        wsi, rna, noise = _batch(4, 10 + step)
        with torch.no_grad():
            ref.prototypes.weight.copy_(torch.nn.functional.normalize(ref.prototypes.weight, dim=1))
        opt.zero_grad()
        MIRRORLoss()(*ref(wsi, rna, noise=noise))[0].backward()
        opt.step()
        with torch.no_grad():
            ref.logit_scale.clamp_(0, 4.6052)
        if e is not None:
            e.update(ref, step=step + 1)
    return ref, e


def _dist2(a, b):
    return sum(float((p.detach() - q.detach()).double().pow(2).sum()) for p, q in zip(a.parameters(), b.parameters()))


# (opt, lr, weight decay, must the decay show in the trajectory).  adamw at 0.05 is the reference template's own fine-tuning value: per
# element it moves lr * wd * |p| ~ 1e-6 beside Adam's lr = 1e-3, far inside the 5 % bound, so a second AdamW case has a decay large
# enough to show; L2 decay enters Adam's normalised step as wd * p against g; SGD's moves lr * wd * p a step beside lr * g, and
# gets 0.5 so that it shows whatever the gradient's size
ENGINE_CASES = [("adamw", 1e-3, 0.05, False), ("adamw", 1e-3, 5.0, True), ("adam", 1e-3, 0.05, True), ("sgd", 2e-2, 0.5, True)]


@pytest.mark.parametrize("kind,lr,wd,shows", ENGINE_CASES)
def test_engine_step_equals_autograd_plus_torch_optim(kind, lr, wd, shows):
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    init = _make()
    ref, _ = _ref_steps(kind, lr, wd)
    den = _dist2(ref, init)
    p0 = sum(float(p.detach().double().pow(2).sum()) for p in init.parameters())
    print(f"\n[engine {kind} wd={wd}] |p_ref - p0| = {den ** 0.5:.4e}, |p0| = {p0 ** 0.5:.4e}")
    assert den ** 0.5 > 1e-4 * p0 ** 0.5, "the torch trajectory is not well above f32 rounding (2^-24 |p0|)"
    if shows:      # torch against torch: the same run without decay lies outside the bound, so a lost or misgrouped decay fails below
        nowd, _ = _ref_steps(kind, lr, 0.0)
        gap = _dist2(nowd, ref)
        print(f"[engine {kind} wd={wd}] torch without decay is {gap ** 0.5 / den ** 0.5:.3f} of the trajectory away")
        assert gap ** 0.5 > 0.05 * den ** 0.5, (gap, den)
    model = _make()
    eng = TrainEngine(model, MIRRORLoss(), lr=lr, precision="fp32", opt=kind, weight_decay=wd)
    assert (eng.v is None) == (kind == "sgd")
    for step in range(3):
        wsi, rna, noise = _batch(4, 10 + step)
        eng.step(wsi, rna, noise=noise)
    num = _dist2(model, ref)
    print(f"[engine {kind} wd={wd}] |p - q| / |p - p0| = {num ** 0.5 / den ** 0.5:.4e}")
    assert num ** 0.5 < 0.05 * den ** 0.5, (num, den)


def test_filter_off_decays_every_parameter_and_momentum_zero_has_no_buffer():
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    ref = _make()
    ref.precision = "fp32"
    init = _make()
    opt = torch.optim.SGD(ref.parameters(), lr=2e-2, momentum=0.0, weight_decay=0.05)     # create_optimizer_v2 without the filter
    model = _make()
    eng = TrainEngine(model, MIRRORLoss(), lr=2e-2, precision="fp32", opt="momentum", momentum=0.0, weight_decay=0.05,
                      filter_bias_and_bn=False)
    assert eng.m is None and eng.v is None and int(eng._group_map.max()) == 0
    for step in range(3):
        wsi, rna, noise = _batch(4, 10 + step)
        with torch.no_grad():
            ref.prototypes.weight.copy_(torch.nn.functional.normalize(ref.prototypes.weight, dim=1))
        opt.zero_grad()
        MIRRORLoss()(*ref(wsi, rna, noise=noise))[0].backward()
        opt.step()
        with torch.no_grad():
            ref.logit_scale.clamp_(0, 4.6052)
        eng.step(wsi, rna, noise=noise)
    num, den = _dist2(model, ref), _dist2(ref, init)
    assert num ** 0.5 < 0.05 * den ** 0.5, (num, den)
    sd = eng.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1 and sd["param_groups"][0]["weight_decay"] == 0.05
    assert float(eng._state[0]) == 3.0, "SGD's tick still advances t"


def test_clip_and_accumulation_with_adamw_match_torch():
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    ref = _make()
    ref.precision = "fp32"
    model = _make()
    eng = TrainEngine(model, MIRRORLoss(), lr=1e-3, precision="fp32", clip_grad=0.05, accum_steps=2, opt="adamw", weight_decay=0.05)
    opt = _torch_opt("adamw", ref, 1e-3, 0.05)
    init = _make()
    for upd in range(2):
        with torch.no_grad():
            ref.prototypes.weight.copy_(torch.nn.functional.normalize(ref.prototypes.weight, dim=1))
        opt.zero_grad()
        for micro in range(2):
            wsi, rna, noise = _batch(2, 50 + 2 * upd + micro)
            (MIRRORLoss()(*ref(wsi, rna, noise=noise))[0] / 2).backward()
            eng.step(wsi, rna, noise=noise)
        gn = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        assert abs(float(eng._state[5]) - float(gn)) < 2e-3 * float(gn), (float(eng._state[5]), float(gn))
        opt.step()
        with torch.no_grad():
            ref.logit_scale.clamp_(0, 4.6052)
    assert float(eng._state[0]) == 2.0
    num, den = _dist2(model, ref), _dist2(ref, init)
    assert num ** 0.5 < 0.05 * den ** 0.5, (num, den)


def test_model_ema_with_sgd_follows_standalone_model_ema():
    from mirror_amd.ema import ModelEmaV3
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    ref, ref_ema = _ref_steps("sgd", 2e-2, 0.05, ema=lambda m: ModelEmaV3(m, decay=0.9, use_warmup=False))
    init = _make()
    model = _make()
    ema = ModelEmaV3(model, decay=0.9, use_warmup=False)
    eng = TrainEngine(model, MIRRORLoss(), lr=2e-2, precision="fp32", opt="sgd", weight_decay=0.05, model_ema=ema)
    for step in range(3):
        wsi, rna, noise = _batch(4, 10 + step)
        eng.step(wsi, rna, noise=noise)
        ema.update(model, step=step + 1)            # the reference's own call: a checked no-op
    num, den = _dist2(ema.module, ref_ema.module), _dist2(ref_ema.module, init)
    moved = _dist2(ref_ema.module, ref)
    assert den > 0 and moved > 0, "the EMA neither left the start nor lags the model: the test would see nothing"
    assert num ** 0.5 < 0.05 * den ** 0.5, (num, den)


def _traj_close(pa, pb, init, tol=0.05):
    num = float((pa - pb).double().pow(2).sum()) ** 0.5
    den = float((pa - init).double().pow(2).sum()) ** 0.5
    assert num < tol * den, (num, den)


def test_d512_graph_replay_of_an_adamw_step_matches_eager_launch(monkeypatch):
    """test_d512_graph_replay_matches_eager_launch with opt="adamw": losses, the last gradient arena and the trajectory, by its bounds.
    Both runs take the two-launch step: the early launch gets the group map cut to the RNA encoder's range."""
    import mirror_amd.models as M
    from mirror_amd import kernels as K
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    calls = []
    real = K.optim_step

    def counting(*a, **kw):
        calls.append((a[0].numel(), kw.get("tick"), kw.get("hole"), None if kw.get("group_map") is None else kw["group_map"].numel()))
        return real(*a, **kw)
    monkeypatch.setattr(K, "optim_step", counting)
    runs = []
    for graph in (True, False):
        torch.manual_seed(21)
        model = M.mirror(**CFG512, rna_proj_drop_rate=0.1).cuda().train()
        eng = TrainEngine(model, MIRRORLoss(), lr=1e-4, precision="bf16", graph=graph, seed=77, snapshot_grads=True, opt="adamw",
                          weight_decay=0.05)
        if not graph:
            eng._rna_branch_state = "off"
        init = eng.master.clone()
        wsi, rna, _ = _batch(4, 5, CFG512)
        wsi = wsi.to(torch.bfloat16)
        torch.manual_seed(123)
        losses = [[float(x) for x in eng.step(wsi, rna)] for _ in range(6)]
        assert (eng._graph is not None) == graph
        assert float(eng._state[0]) == 6.0
        lo, hi = eng._early_range
        assert (hi - lo, "early", None, (hi - lo) // 8) in calls and (eng.numel, False, (lo, hi), eng.numel // 8) in calls
        assert torch.equal(eng.shadow.view(torch.int16), eng.master.to(torch.bfloat16).view(torch.int16))
        runs.append((losses, eng.master.clone(), eng.grad_snap.clone(), init))
    (la, pa, ga, init), (lb, pb, gb, _) = runs
    for a, b in zip(la, lb):
        for x, y in zip(a, b):
            assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), (la, lb)
    assert float((ga - gb).norm()) <= 2e-2 * float(gb.norm())
    _traj_close(pa, pb, init)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mirror_amd.engine import TrainEngine
        from mirror_amd.losses import MIRRORLoss
        model = _make(seed=rank)                      # different init per rank: the engine broadcasts rank 0's
        eng = TrainEngine(model, MIRRORLoss(gather_distributed=True), lr=1e-3, precision="fp32", bucket_mb=0.05, opt="adamw",
                          weight_decay=0.05)
        assert len(eng.buckets) > 2
        wsi, rna, noise = _batch(8, 77)               # the global batch; each rank takes its half
        sl = slice(rank * 4, rank * 4 + 4)
        losses = None
        for _ in range(2):
            losses = eng.step(wsi[sl], rna[sl], noise={k: v[sl] for k, v in noise.items()})
        q.put((rank, eng.master.detach().cpu().numpy(), float(losses[1])))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_adamw_match_single_process_on_concatenated_batch():
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30300 + (os.getpid() % 300)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(res[0][1], res[1][1]), "ranks diverged"
    model = _make(seed=0)
    eng = TrainEngine(model, MIRRORLoss(), lr=1e-3, precision="fp32", opt="adamw", weight_decay=0.05)
    wsi, rna, noise = _batch(8, 77)
    for _ in range(2):
        losses = eng.step(wsi, rna, noise=noise)
    rel = (eng.master.cpu() - torch.from_numpy(res[0][1])).norm() / eng.master.cpu().norm()
    assert rel < 5e-3, rel
    assert abs(float(losses[1]) - 0.5 * (res[0][2] + res[1][2])) < 5e-3 * abs(float(losses[1]))


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_state_dict_round_trip_continues_the_run(kind):
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    lr = 1e-3 if kind == "adamw" else 2e-2
    model = _make()
    eng = TrainEngine(model, MIRRORLoss(), lr=lr, precision="fp32", graph=False, opt=kind, weight_decay=0.05)
    for i in range(2):
        eng.step(*_batch(4, 70 + i))
    sd = eng.state_dict()
    weights = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tail = _batch(4, 80)
    eng.step(*tail)
    model2 = _make(seed=5)
    eng2 = TrainEngine(model2, MIRRORLoss(), lr=0.5, precision="fp32", graph=False, opt=kind, weight_decay=0.05)
    model2.load_state_dict(weights)
    eng2.load_state_dict(sd)
    assert eng2.step_count == 2 and eng2.lr == lr and float(eng2._state[0]) == 2.0
    eng2.step(*tail)
    for (k, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), k
    # the dict has the matching torch.optim optimizer's shape: groups [no_decay, decay], indices running through them
    groups = _timm_groups(model, 0.05)
    opt = _torch_opt(kind, model, 0.123, 0.05)
    opt.load_state_dict(sd)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05] and opt.param_groups[0]["lr"] == lr
    flat = [p for g in groups for p in g["params"]]
    assert len(sd["state"]) == len(flat) == len(list(model.parameters()))
    key = "exp_avg" if kind == "adamw" else "momentum_buffer"
    for i, p in enumerate(flat):
        assert sd["state"][i][key].shape == p.shape and opt.state[p][key].shape == p.shape
        assert set(sd["state"][i]) == ({"step", "exp_avg", "exp_avg_sq"} if kind == "adamw" else {"momentum_buffer"})
    want = {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"} if kind == "adamw" else \
        {"lr", "momentum", "dampening", "weight_decay", "nesterov", "params"}
    assert all(set(g) == want for g in sd["param_groups"])
    # another rule's dict is refused
    other = TrainEngine(_make(), MIRRORLoss(), precision="fp32", opt="sgd" if kind == "adamw" else "adamw", weight_decay=0.05)
    with pytest.raises(ValueError, match="another rule"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError):
        TrainEngine(_make(), MIRRORLoss(), precision="fp32", opt=kind).load_state_dict(sd)       # one group, not two


def test_default_engine_dict_is_unchanged_and_unknown_modes_are_refused():
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    eng = TrainEngine(_make(), MIRRORLoss(), lr=1e-3, precision="fp32")
    from mirror_amd import _lib
    assert eng._opt_cfg.rule == _lib.OPT_ADAM and eng._group_map is None and eng._group_wd is None
    sd = eng.state_dict()
    (g,) = sd["param_groups"]
    assert list(g) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    assert g["weight_decay"] == 0 and isinstance(g["weight_decay"], int) and g["params"] == list(range(len(sd["state"])))
    assert set(sd) == {"state", "param_groups"}
    with pytest.raises(NotImplementedError, match="lion"):
        TrainEngine(_make(), MIRRORLoss(), precision="fp32", opt="lion")
    with pytest.raises(NotImplementedError):
        TrainEngine(_make(), MIRRORLoss(), precision="fp32", clip_grad=0.1, clip_mode="agc", opt="adamw")
    from mirror_amd.ema import ModelEmaV3
    m = _make()
    with pytest.raises(NotImplementedError):          # the fp8 policy still refuses the EMA, with the new rules too
        TrainEngine(m, MIRRORLoss(), precision="fp8", opt="adamw", weight_decay=0.05, model_ema=ModelEmaV3(m))
