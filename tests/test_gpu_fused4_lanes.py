"""k_fused4's cross-lane halves at the smallest shapes where they can go wrong.

The kernel holds a lane's four columns as the stride-2 pairs (c0, c2) and (c1, c3).  Two of the
stencil's operand pairs straddle a lane -- (u2, next lane's u0) and (previous lane's u3, u1),
plus (u3, next lane's u1) at tap column class 0 -- and so do one term of the horizontal r2h
blend and one of the folded h2r: each is a DPP read of the neighbouring lane that must see 0 at
the wave's two ends and the right lane everywhere else.  The shapes put a raster edge, a window
edge or a lone lane at every such place:

  (1, 8, 4)    one owned lane: both neighbours are outside the raster
  (1, 8, 8)    two owned lanes: each has one neighbour inside
  (1, 9, 240)  one full window: lanes 2 and 61 are its edge lanes; odd height (a 3-step tail)
  (1, 8, 244)  a second window that owns one lane, its left neighbours all halo
  (2, 2 rows + 7, 484)  a downward band, an upward full band and a 7-row tail, three windows

Every width is accepted by both kernels as it stands (a multiple of 4, at least 4), so none had
to be moved to the next multiple of 4.  Each shape runs at both offsets: tap column class 1
(offset 0 at padding 1) and class 0 with its (u3, u5) pair.  Checks and tolerances are
tests/test_gpu_fused4.py's: bit-identical to the two-column kernel on downward bands, within
one bf16 step on upward ones, and within one bf16 rounding of the fp64 oracle chain."""
import numpy as np
import pytest
import torch

import fused_variants as FV

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi  # noqa: E402
from HyGrid.HexFrames import HexConv2d  # noqa: E402
from test_gpu_fused4 import DEV, _oracle, _run, _same  # noqa: E402


def _shapes():
    rows, own, _ = _abi.fused_layout(6)
    assert own == 240
    return [(1, 8, 4), (1, 8, 8), (1, 9, own), (1, 8, own + 4), (2, 2 * rows + 7, 2 * own + 4)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("idx", range(5))
def test_fused4_lane_edges(idx, off, monkeypatch):
    B, H, W = _shapes()[idx]
    torch.manual_seed(11 + off)
    conv = HexConv2d(3, 3, off, 2, padding=1, bias=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(H * 13 + W)
    # values in [-1, 1): signed, so a neighbour term that is dropped or taken from the wrong
    # lane is not hidden in a sum of like-signed terms
    x = (torch.rand((B, 3, H, W), generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
    y4 = _run(x, conv, off, monkeypatch, False)
    y2 = _run(x, conv, off, monkeypatch, True)
    _same(y4, y2)
    for b in range(B):
        ref = _oracle(x[b:b + 1], conv)[0]
        got = y4[b].double().cpu().numpy()
        tol = 2.0 ** -8 * np.abs(ref) + 1e-5 * np.abs(ref).max()
        bad = np.abs(got - ref) > tol
        assert not bad.any(), (f"image {b}: {int(bad.sum())} outputs beyond one bf16 rounding of "
                               "the oracle: " + FV.describe_first_bad(6, bad))
