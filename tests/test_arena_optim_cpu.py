"""CPU: the host side of mirror_amd.optim — the C ABI of mh_optim_groups and mh_gather_many, and what create_optimizer_v2 decides
before it touches the device (timm's grouping, frozen parameters, refused optimizers, refused CPU parameters)."""
import os
import re

import pytest
import torch

from mirror_amd import _lib
from tests.test_optim_cpu import CLS, _timm_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decl(name):
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % name, flat, flags=re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(q.split()) for q in m.group(1).split(",")]


def _classifier():
    import mirror_amd.models as M
    torch.manual_seed(0)
    return M.mirror_classifier(**CLS)


def test_new_entry_points_in_header_bindings_and_exports():
    step, groups, gather = _decl("mh_optim_step"), _decl("mh_optim_groups"), _decl("mh_gather_many")
    # mh_optim_groups is mh_optim_step plus the learning-rate table beside the decay table
    at = step.index("const float* group_wd")
    assert groups == step[:at + 1] + ["const float* group_lr"] + step[at + 1:]
    assert gather == ["float* arena", "const int64_t* table", "int nrows", "mh_stream s"]
    lib = _lib.load()
    for name, params in (("mh_optim_groups", groups), ("mh_gather_many", gather)):
        assert name in _lib.EXPORTS and name in _lib._SIGS and len(_lib._SIGS[name]) == len(params) - 1
        assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    assert re.search(r"#define MH_OPT_SKIP_GROUP %d\b" % _lib.OPT_SKIP_GROUP, header)
    from tests.test_host_cpu import test_binding_signatures_restate_the_header_argument_lists as check
    check()


def test_the_abi_generation_is_unchanged():
    assert _lib.load().mh_version() == 123 == _lib.ABI_VERSION


def test_create_optimizer_v2_groups_as_timm_and_skips_frozen_parameters():
    from mirror_amd.engine import decay_groups
    from mirror_amd.optim import param_groups_of
    model = _classifier()
    got = param_groups_of(model, 0.05)
    assert [g["weight_decay"] for g in got] == [0.0, 0.05]
    for g, (wd, members), want in zip(got, decay_groups(model, 0.05), _timm_groups(model, 0.05)):
        assert [id(p) for p in g["params"]] == [id(p) for _, p in members] == [id(p) for p in want["params"]]
    (one,) = param_groups_of(model, 0.05, filter_bias_and_bn=False)
    assert one["weight_decay"] == 0.05 and [id(p) for p in one["params"]] == [id(p) for p in model.parameters()]
    # the linear probe of train_subtyping.py:756-763: everything frozen but the head
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.head.parameters():
        p.requires_grad_(True)
    probe = param_groups_of(model, 0.05)
    assert [[id(p) for p in g["params"]] for g in probe] == [[id(model.head.bias)], [id(model.head.weight)]]


def test_create_optimizer_v2_refuses_other_optimizers_and_cpu_parameters():
    from mirror_amd.optim import ArenaOptimizer, create_optimizer_v2, dispatch_clip_grad
    model = _classifier()
    before = [p.data_ptr() for p in model.parameters()]
    with pytest.raises(NotImplementedError, match="lamb"):
        create_optimizer_v2(model, opt="lamb", lr=1e-3)
    for opt in ("adam", "adamw", "sgd", "nesterov", "momentum"):
        with pytest.raises(_lib.MirrorHipError, match="no CPU path"):
            create_optimizer_v2(model, opt=opt, lr=1e-3, weight_decay=0.05)
    with pytest.raises(_lib.MirrorHipError):
        ArenaOptimizer(list(model.parameters()), lr=1e-3)
    with pytest.raises(ValueError, match="Nesterov"):
        create_optimizer_v2(model, opt="sgd", lr=1e-3, momentum=0.0)
    # a refusal moves nothing: the parameters are where they were, without gradients
    assert [p.data_ptr() for p in model.parameters()] == before and all(p.grad is None for p in model.parameters())
    with pytest.raises(NotImplementedError):
        dispatch_clip_grad(model.parameters(), 1.0, mode="norm", norm_type=1.0)
    with pytest.raises(NotImplementedError):
        dispatch_clip_grad(model.parameters(), 1.0, mode="agc")
