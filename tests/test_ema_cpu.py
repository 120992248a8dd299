"""CPU: model EMA host logic — timm's decay rule, the C ABI of the two EMA entry points, EMA weights in checkpoints and
timm's choice of weights when loading one."""
import os
import re

import pytest
import torch

from mirror_amd import _lib
from mirror_amd.checkpoint import CheckpointSaver, load_checkpoint, select_state_dict
from mirror_amd.ema import ModelEmaV3, ema_decay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timm_rule(step, decay, min_decay, update_after_step, use_warmup, gamma, power):
    if step is None:
        return decay
    step = max(0, step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_warmup:
        d = 1 - (1 + step / gamma) ** -power
        return max(min(d, decay), min_decay)
    return decay


@pytest.mark.parametrize("use_warmup", [False, True])
@pytest.mark.parametrize("update_after_step", [0, 1, 5])
def test_get_decay_restates_timm(use_warmup, update_after_step):
    for decay, min_decay, gamma, power in ((0.9998, 0.0, 1.0, 2 / 3), (0.99, 0.5, 2.0, 0.75), (0.9, 0.95, 1.0, 2 / 3)):
        for step in [None] + list(range(0, 40)) + [100, 1000, 10 ** 5, 10 ** 7]:
            want = _timm_rule(step, decay, min_decay, update_after_step, use_warmup, gamma, power)
            got = ema_decay(step, decay, min_decay, update_after_step, use_warmup, gamma, power)
            assert got == want, (step, got, want)
            ema = ModelEmaV3.__new__(ModelEmaV3)       # the method, without the GPU state of a constructed one
            ema.decay, ema.min_decay, ema.update_after_step = decay, min_decay, update_after_step
            ema.use_warmup, ema.warmup_gamma, ema.warmup_power = use_warmup, gamma, power
            assert ema.get_decay(step) == want
    assert ema_decay(1, 0.9998) == 0.0 and ema_decay(1, 0.9998, use_warmup=True) == 0.0     # the first update copies
    assert ema_decay(2, 0.9998) == 0.9998


def test_ema_entry_points_in_header_bindings_and_exports():
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("mh_adam_ema", 24), ("mh_ema_update_many", 6)):
        m = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % name, flat, flags=re.M | re.S)
        assert m, name
        params = [" ".join(q.split()) for q in m.group(1).split(",")]
        assert params[-1] == "mh_stream s" and len(params) == n_args + 1, params
        assert params[-2] == "const mh_ema_cfg* cfg"
        assert len(_lib._SIGS[name]) == n_args and name in _lib.EXPORTS
    # mh_adam_ema = mh_adam's argument list + (ema, cfg)
    assert _lib._SIGS["mh_adam_ema"][:-2] == _lib._SIGS["mh_adam"]
    # EmaCfg restates mh_ema_cfg field by field
    end = flat.index("} mh_ema_cfg;")
    body = flat[flat.rindex("typedef struct {", 0, end):end]
    fields = []
    for decl in body.replace("typedef struct {", "").split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(" ", 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    ctype = {"double": "c_double", "int64_t": "c_long", "int": "c_int"}
    assert [f[0] for f in fields] == [f[0] for f in _lib.EmaCfg._fields_]
    for (n, typ), (_, ct) in zip(fields, _lib.EmaCfg._fields_):
        assert ct.__name__ in (ctype[typ], "c_int64", "c_int32", "c_longlong"), (n, typ, ct)


def test_model_ema_force_cpu_raises():
    with pytest.raises(NotImplementedError, match="CPU"):
        ModelEmaV3(torch.nn.Linear(4, 4), device="cpu")


class _Ema(torch.nn.Module):
    """Stands in for ModelEmaV3 (a GPU object): what the saver reads is state_dict(), keys `module.<name>`."""

    def __init__(self, m):
        super().__init__()
        self.module = m


def test_saver_writes_state_dict_ema_only_when_given(tmp_path):
    torch.manual_seed(0)
    model, shadow = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    plain = CheckpointSaver(model, checkpoint_dir=str(tmp_path / "a"))
    plain.save_checkpoint(0, metric=1.0)
    a = torch.load(tmp_path / "a" / "last.pth.tar")
    assert set(a) == {"epoch", "arch", "state_dict", "version", "metric"}
    saver = CheckpointSaver(model, checkpoint_dir=str(tmp_path / "b"), model_ema=_Ema(shadow))
    saver.save_checkpoint(0, metric=1.0)
    b = torch.load(tmp_path / "b" / "last.pth.tar")
    assert set(b) == set(a) | {"state_dict_ema"}
    assert sorted(b["state_dict_ema"]) == ["module.bias", "module.weight"]
    assert torch.equal(b["state_dict_ema"]["module.weight"], shadow.weight.detach())
    assert torch.equal(b["state_dict"]["weight"], model.weight.detach())
    # use_ema=True reloads the EMA weights, use_ema=False the model's
    fresh = torch.nn.Linear(3, 2)
    load_checkpoint(fresh, str(tmp_path / "b" / "last.pth.tar"), use_ema=True)
    assert torch.equal(fresh.weight, shadow.weight)
    load_checkpoint(fresh, str(tmp_path / "b" / "last.pth.tar"))
    assert torch.equal(fresh.weight, model.weight)


def test_load_checkpoint_picks_weights_in_timms_order():
    t = {k: torch.full((1,), float(i)) for i, k in enumerate(("sd_ema", "m_ema", "sd", "model", "bare"))}

    def w(x):
        return {"module.w": x}
    full = {"state_dict_ema": w(t["sd_ema"]), "model_ema": w(t["m_ema"]), "state_dict": w(t["sd"]), "model": w(t["model"])}
    assert select_state_dict(full, use_ema=True)["w"] is t["sd_ema"]
    assert select_state_dict(full, use_ema=False)["w"] is t["sd"]
    no_sde = dict(full, state_dict_ema=None)
    assert select_state_dict(no_sde, use_ema=True)["w"] is t["m_ema"]
    only_sd = {"state_dict": {"w": t["sd"]}, "epoch": 3}
    assert select_state_dict(only_sd, use_ema=True) == {"w": t["sd"]}
    assert select_state_dict({"model": w(t["model"])}, use_ema=True)["w"] is t["model"]
    assert select_state_dict({"module.w": t["bare"], "b": t["bare"]}, use_ema=True) == {"w": t["bare"], "b": t["bare"]}
