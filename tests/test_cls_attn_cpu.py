"""CPU (no GPU): the slide-attention entry point is declared and exported, and every refusal of its wrappers carries a message."""
import os
import re

import pytest
import torch

from mirror_amd import _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from mirror_amd.explain import slide_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operands(n_p=512, m=256, dh=64, h=2, dtype=torch.bfloat16):
    D = h * dh
    return (torch.zeros(1, n_p, 3 * D, dtype=dtype), torch.zeros(1, m, 2 * D, dtype=dtype), torch.zeros(1, h, m, m), h, dh ** -0.5)


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    assert re.search(r"^int mh_nys_cls_attn\(", header, flags=re.M)
    assert "mh_nys_cls_attn" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "mh_nys_cls_attn")
    assert lib.mh_nys_cls_attn.argtypes[-1] is _lib.C.c_void_p and len(lib.mh_nys_cls_attn.argtypes) == 18


def test_cpu_tensors_are_refused():
    qkv, lm, z, h, scale = _operands()
    with pytest.raises(MirrorHipError, match="no CPU fallback"):
        K.nys_cls_attn(qkv, lm, z, h, scale, 0)


@pytest.mark.parametrize("cls_row", [-1, 512])
def test_cls_row_outside_the_sequence_is_refused(cls_row):
    qkv, lm, z, h, scale = _operands()
    with pytest.raises(MirrorHipError, match=r"cls_row=.* outside \[0, 512\)"):
        K.nys_cls_attn(qkv, lm, z, h, scale, cls_row)


def test_mrow_without_mlm_is_refused():
    qkv, lm, z, h, scale = _operands()
    with pytest.raises(MirrorHipError, match="mrow and mlm go together"):
        K.nys_cls_attn(qkv, lm, z, h, scale, 0, mrow=torch.ones(1, 512))
    with pytest.raises(MirrorHipError, match="mrow and mlm go together"):
        K.nys_cls_attn(qkv, lm, z, h, scale, 0, mlm=torch.ones(1, 256))


def test_unsupported_geometry_and_operands_are_refused():
    qkv, lm, z, h, scale = _operands(n_p=256, m=128, dh=32)
    with pytest.raises(MirrorHipError, match="built for"):
        K.nys_cls_attn(qkv, lm, z, h, scale, 0)
    qkv, lm, z, h, scale = _operands()
    with pytest.raises(MirrorHipError, match="z must be contiguous"):
        K.nys_cls_attn(qkv, lm, z, h, scale, 0, z_colmajor=True)            # the chain's layout is bf16
    with pytest.raises(MirrorHipError, match="one dtype"):
        K.nys_cls_attn(qkv, lm.float(), z, h, scale, 0)


def test_the_c_abi_refuses_before_it_launches():
    """MH_EINVAL with a message for what the kernel is not built for, checked on the host: no device is touched."""
    lib = _lib.load()
    P = 4096           # any 16-byte aligned non-null value: the checks below fail before a pointer is used

    def rc(B=1, h=2, n_p=512, m=256, dh=64, cls_row=0, mrow=None, mlm=None, zc=0, dt=_lib.MH_BF16):
        return lib.mh_nys_cls_attn(P, P, P, None, P, mrow, mlm, B, h, n_p, m, dh, cls_row, 0.125, 0, zc, dt, None)

    for kw, msg in (({"dh": 32, "m": 128, "n_p": 256}, "built for"), ({"cls_row": 512}, "cls_row=512 outside"), ({"cls_row": -1}, "cls_row=-1 outside"),
                    ({"mrow": P}, "mrow and mlm go together"), ({"n_p": 640}, "multiple of m"), ({"dt": 7}, "dt must be"),
                    ({"zc": 2}, "z_colmajor")):
        assert rc(**kw) == -1, kw
        assert msg in lib.mh_last_error().decode(), (kw, lib.mh_last_error())
    assert rc(B=0) == 0


def test_slide_attention_argument_refusals():
    with pytest.raises(ValueError, match="4 dims"):
        slide_attention(torch.zeros(2, 8, 10))
    with pytest.raises(ValueError, match="unknown reduce"):
        slide_attention(torch.zeros(2, 2, 8, 10), reduce="sum")
    with pytest.raises(ValueError, match="layer 2 outside"):
        slide_attention(torch.zeros(2, 2, 8, 10), layer=2)


def test_slide_attention_on_cpu_tensors():
    a = torch.arange(2 * 2 * 3 * 5, dtype=torch.float32).reshape(2, 2, 3, 5)
    out = slide_attention(a, layer=0, reduce="max")
    assert out.shape == (2, 5) and float(out.min()) == 0.0 and float(out.max()) == 1.0
    assert torch.equal(slide_attention(torch.ones(1, 1, 2, 4)), torch.zeros(1, 4))
