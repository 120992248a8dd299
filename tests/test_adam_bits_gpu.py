"""GPU: mh_adam and mh_adam_ema still give, bit for bit, what they gave while they had a device body of their own.  The fixture
(tests/golden/golden_adam_bits.npz, tools/make_golden_adam.py) holds the inputs and that build's results for three short cases:
the device step state, the same with the EMA, and host-side step constants; each with a hole, a clamped element and a scalar tail.
Every stored array must come out torch.equal: no element may differ."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.make_golden_adam import CASES, CLAMP_HI, N, replay  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_adam_bits.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.mark.parametrize("case", list(CASES))
def test_adam_reproduces_the_recorded_bits(z, case):
    want = {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(case + "/")}
    assert set(want) == {"p", "m", "v", "counter"} | ({"shadow", "state"} if case != "c" else set()) | ({"ema"} if case == "b" else set())
    got = replay(z, case)
    assert set(got) == set(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and torch.equal(got[k], w), (case, k, int((got[k] != w).sum()))
    # the fixture exercises what it is there for: the clamp bit, the counter ran, the tail and both sides of the hole moved
    p0 = torch.from_numpy(z["p0"])
    assert float(want["p"][CASES[case]]) == float(np.float32(CLAMP_HI)) and int(want["counter"]) == 15
    assert all(bool((want["p"][a:b] != p0[a:b]).all()) for a, b in ((0, 512), (512, 1024), (1024, 2048), (2048, N)))
