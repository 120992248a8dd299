"""CPU: the arena optimizer's host side — the C ABI of mh_optim_step, timm's weight-decay grouping and the torch.optim state-dict
index order that TrainEngine.state_dict() speaks."""
import os
import re

import pytest
import torch

from mirror_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = dict(wsi_embed_dim=64, rna_embed_dim=48, embed_dim=64, wsi_num_tokens=60, rna_encoder_depth=1, rna_num_heads=8,
           style_mlp_hidden_dim=64, style_mlp_out_dim=32, style_latent_dim=16, num_prototypes=50)
CLS = dict(wsi_embed_dim=64, rna_embed_dim=48, embed_dim=64, num_classes=4, rna_encoder_depth=1, rna_num_heads=8)


def _timm_groups(model, weight_decay):
    """timm.optim.param_groups_weight_decay, restated (neither model defines no_weight_decay())."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if param.ndim <= 1 or name.endswith(".bias"):
            no_decay.append(param)
        else:
            decay.append(param)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def _models():
    import mirror_amd.models as M
    torch.manual_seed(0)
    return [M.mirror(**CFG), M.mirror_classifier(**CLS)]


def test_optim_entry_point_in_header_bindings_and_exports():
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"^int\s+mh_optim_step\s*\(([^;]*?)\)\s*;", flat, flags=re.M | re.S)
    assert m, "mh_optim_step is not declared"
    params = [" ".join(q.split()) for q in m.group(1).split(",")]
    assert params[-1] == "mh_stream s" and params[-2] == "const mh_ema_cfg* ema_cfg" and params[6] == "const mh_optim_cfg* opt"
    assert "mh_optim_step" in _lib.EXPORTS and len(_lib._SIGS["mh_optim_step"]) == len(params) - 1
    assert hasattr(_lib.load(), "mh_optim_step")
    # the header-vs-_SIGS check of the suite covers the new argument list
    from tests.test_host_cpu import test_binding_signatures_restate_the_header_argument_lists as check
    check()
    # OptimCfg restates mh_optim_cfg field by field
    end = flat.index("} mh_optim_cfg;")
    body = flat[flat.rindex("typedef struct {", 0, end):end].replace("typedef struct {", "")
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(" ", 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    assert [f[0] for f in fields] == [f[0] for f in _lib.OptimCfg._fields_]
    for (n, typ), (_, ct) in zip(fields, _lib.OptimCfg._fields_):
        assert ct.__name__ in {"int": ("c_int", "c_int32"), "float": ("c_float",)}[typ], (n, typ, ct)
    for name, val in (("MH_OPT_ADAM", _lib.OPT_ADAM), ("MH_OPT_ADAMW", _lib.OPT_ADAMW), ("MH_OPT_SGD", _lib.OPT_SGD)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name


def test_decay_groups_reproduce_timm_membership():
    from mirror_amd.engine import decay_groups
    for model in _models():
        want = _timm_groups(model, 0.05)
        got = decay_groups(model, 0.05)
        assert [wd for wd, _ in got] == [0.0, 0.05]
        for (_, members), grp in zip(got, want):
            assert [id(p) for _, p in members] == [id(p) for p in grp["params"]]
        no_decay, decay = ({n for n, _ in members} for _, members in got)
        names = dict(model.named_parameters())
        assert no_decay | decay == set(names) and not (no_decay & decay) and no_decay and decay
        for n, p in names.items():
            if n.endswith(".bias") or p.ndim <= 1:        # every bias, LayerNorm weight, logit_scale, and <= 1-D token
                assert n in no_decay, n
            else:
                assert n in decay and p.ndim >= 2, n
        ln = [n for n, mod in model.named_modules() if isinstance(mod, torch.nn.LayerNorm)]
        assert ln and all(f"{n}.weight" in no_decay and f"{n}.bias" in no_decay for n in ln)
        if "logit_scale" in names:
            assert "logit_scale" in no_decay
        # the filter off, or no decay: one group that carries the weight decay, as create_optimizer_v2 passes model.parameters()
        for wd, flt in ((0.05, False), (0.0, True)):
            one = decay_groups(model, wd, flt)
            assert len(one) == 1 and one[0][0] == wd and [id(p) for _, p in one[0][1]] == [id(p) for p in model.parameters()]
        # a frozen parameter is in no group, as in timm
        first = next(iter(model.parameters()))
        first.requires_grad_(False)
        assert all(id(p) != id(first) for _, members in decay_groups(model, 0.05) for _, p in members)
        first.requires_grad_(True)


def test_state_index_order_matches_torch_adamw_over_timm_groups():
    from mirror_amd.engine import decay_groups
    for model in _models():
        opt = torch.optim.AdamW(_timm_groups(model, 0.05), lr=1e-3, weight_decay=0.0)
        for p in model.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
        sd = opt.state_dict()
        groups = decay_groups(model, 0.05)
        i = 0
        for (wd, members), g in zip(groups, sd["param_groups"]):
            assert g["weight_decay"] == wd and g["params"] == list(range(i, i + len(members)))
            for _, p in members:
                assert sd["state"][i]["exp_avg"].shape == p.shape, i
                i += 1
        assert i == len(sd["state"]) == len(list(model.parameters()))


def test_engine_refuses_unknown_opt_before_touching_the_device():
    from mirror_amd.engine import TrainEngine
    model = torch.nn.Linear(4, 4)
    with pytest.raises(NotImplementedError, match="lamb"):
        TrainEngine(model, None, opt="lamb")
    with pytest.raises(ValueError, match="Nesterov"):
        TrainEngine(model, None, opt="sgd", momentum=0.0)
