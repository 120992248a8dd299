"""CPU: mirror_amd.arena — the layout arithmetic (lay_out, span, group_bytes, range_of) on CPU tensors and the launch settings
rule_cfg builds.  Nothing here touches a device: a ParamArena under the fp32 policy only allocates and copies."""
import torch

from mirror_amd import _lib
from mirror_amd.arena import ALIGN, ParamArena, lay_out, pad, rule_cfg

SIZES = [1, 7, 8, 9, 2048, 33]
OFFSETS, TOTAL = [0, 8, 16, 24, 40, 2088], 2128
BLOCKS = [(0, 1), (1, 2), (2, 3), (3, 5), (5, 261), (261, 266)]          # the 9-element parameter owns 2 blocks, the 33-element one 5


def _arena():
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n)) for n in SIZES]
    before = [p.detach().clone() for p in params]
    return ParamArena(params, "adamw", True, "fp32", 1e-3), params, before


def test_lay_out_pads_every_tensor_to_the_block():
    assert ALIGN == 8 and [pad(n) for n in (0, 1, 8, 9)] == [0, 8, 8, 16]
    assert lay_out(SIZES) == (OFFSETS, TOTAL)
    assert lay_out([]) == ([], 0)


def test_arena_moves_the_parameters_and_zeroes_the_padding():
    pa, params, before = _arena()
    assert (pa.offsets, pa.numel) == (OFFSETS, TOTAL) and pa.master.numel() == pa.grad.numel() == pa.m.numel() == pa.v.numel() == TOTAL
    assert pa.bf is None and pa.shadow is None and pa.shadow_t is None and pa.t_params == []
    assert pa.off_of == {id(p): o for p, o in zip(params, OFFSETS)}
    covered = torch.zeros(TOTAL, dtype=torch.bool)
    for p, o, view, was in zip(params, OFFSETS, pa.grad_views, before):
        assert p.data_ptr() == pa.master.data_ptr() + 4 * o and view.data_ptr() == pa.grad.data_ptr() + 4 * o
        assert view.shape == p.shape and p.grad is None and torch.equal(p.detach(), was)
        covered[o:o + p.numel()] = True
    assert int((~covered).sum()) == TOTAL - sum(SIZES) and not bool(pa.master[~covered].any())
    assert pa.state.tolist() == [0.0, 0.0, 0.0, torch.tensor(1e-3).item(), 1.0, 0.0]


def test_group_bytes_write_exactly_the_blocks_of_each_parameter():
    pa, params, _ = _arena()
    assert [pa.span(p) for p in params] == BLOCKS
    groups = [0, 1, 0, 1, 0, 1]
    gmap = pa.group_bytes(groups)
    assert gmap.dtype == torch.uint8 and gmap.device.type == "cpu" and gmap.numel() == TOTAL // 8
    want = torch.zeros(TOTAL // 8, dtype=torch.uint8)
    for (a, b), gi in zip(BLOCKS, groups):
        want[a:b] = gi
    assert torch.equal(gmap, want)
    # every block has exactly one owner: the spans tile the map
    assert [a for a, _ in BLOCKS] + [TOTAL // 8] == [0] + [b for _, b in BLOCKS]
    # the skip value overwrites one parameter's span and nothing else
    first, end = pa.span(params[3])
    skipped = gmap.clone()
    skipped[first:end] = _lib.OPT_SKIP_GROUP
    assert (first, end) == (3, 5) and bool((skipped[3:5] == 255).all())
    assert torch.equal(skipped[:3], gmap[:3]) and torch.equal(skipped[5:], gmap[5:])


def test_range_of_a_run_of_parameters_includes_its_padding():
    pa, _, _ = _arena()
    assert pa.range_of(1, 3) == (8, 40)
    assert pa.range_of(0, 5) == (0, TOTAL) and pa.range_of(4, 4) == (40, 2088)


def test_set_step_writes_the_head_or_all_six():
    pa, _, _ = _arena()
    pa.state.copy_(torch.tensor([9.0, 9.0, 9.0, 9.0, 0.5, 3.0]))
    pa.set_step(2.0, 0.9, 0.999, 1e-2, keep_clip=True)
    head = torch.tensor([2.0, 1.0 - 0.9 ** 2.0, 1.0 - 0.999 ** 2.0, 1e-2])
    assert torch.equal(pa.state[:4], head) and pa.state[4:].tolist() == [0.5, 3.0]
    pa.set_step(2.0, 0.9, 0.999, 1e-2)
    assert torch.equal(pa.state[:4], head) and pa.state[4:].tolist() == [1.0, 0.0]


def test_sgd_allocates_no_second_moment_and_no_buffer_without_momentum():
    for momentum_buffer in (True, False):
        pa = ParamArena([torch.nn.Parameter(torch.ones(3))], "sgd", momentum_buffer, "fp32", 0.1)
        assert pa.v is None and (pa.m is not None) == momentum_buffer


def _fields(cfg):
    return [getattr(cfg, name) for name, _ in _lib.OptimCfg._fields_]


def test_rule_cfg_builds_what_the_two_constructors_built():
    f = lambda x: torch.tensor(x, dtype=torch.float32).item()          # the struct's fields are C floats
    # TrainEngine: every field from its arguments, whatever the rule
    for rule, code, nesterov in (("adam", _lib.OPT_ADAM, False), ("adamw", _lib.OPT_ADAMW, False), ("sgd", _lib.OPT_SGD, True)):
        want = _lib.OptimCfg(code, 0.9, 0.95, 1e-6, 0.8, int(nesterov))
        assert _fields(rule_cfg(rule, (0.9, 0.95), 1e-6, 0.8, nesterov)) == _fields(want) == [code, f(0.9), f(0.95), f(1e-6), f(0.8), int(nesterov)]
    # ArenaOptimizer: the fields of the other rules are zero
    assert _fields(rule_cfg("sgd", (0.0, 0.0), 0.0, 0.9, True)) == _fields(_lib.OptimCfg(_lib.OPT_SGD, 0.0, 0.0, 0.0, 0.9, 1))
    for rule, code in (("adam", _lib.OPT_ADAM), ("adamw", _lib.OPT_ADAMW)):
        assert _fields(rule_cfg(rule, (0.9, 0.999), 1e-8, 0.0, False)) == _fields(_lib.OptimCfg(code, 0.9, 0.999, 1e-8, 0.0, 0))
