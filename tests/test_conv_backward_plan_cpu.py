"""Which kernel each gradient of a HexConv2d layer runs on (hg_hexconv2d_backward_plan, host
only: nothing is launched and no device is needed).  d kernel / d bias of a dense radius-2,
stride-1, dilation-1 layer with f32 weights run on the matrix cores from 16 output channels, d
input from 16 input channels with constant padding (csrc/conv_mfma_bwd.hip); everything else,
and everything with HYGRID_CONV_BWD_MFMA=0, on the generic kernels (csrc/hexconv_bwd.hip)."""
import ctypes

import pytest
import torch

from HyGrid import _abi, ops

GEN, MFMA = _abi.HG_CONV_BWD_GENERIC, _abi.HG_CONV_BWD_MFMA
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16

# (x dtype, w dtype, B, C, O, h, w, radius, kwargs) -> (d input, d kernel)
TABLE = [
    ((BF16, F32, 4, 64, 64, 1080, 1920, 2, dict(padding=1)), (MFMA, MFMA)),
    ((F32, F32, 1, 64, 64, 20, 30, 2, dict(padding=0)), (MFMA, MFMA)),
    ((F16, F32, 1, 64, 64, 20, 30, 2, dict(padding=2)), (MFMA, MFMA)),
    ((BF16, F32, 4, 3, 64, 1080, 1920, 2, dict(padding=1)), (GEN, MFMA)),
    ((F32, F32, 2, 64, 3, 40, 50, 2, dict(padding=1)), (MFMA, GEN)),
    ((F32, F32, 2, 8, 8, 40, 50, 2, dict(padding=1)), (GEN, GEN)),
    ((F32, F32, 2, 16, 16, 40, 50, 2, dict(padding=1)), (MFMA, MFMA)),
    ((F32, F32, 2, 15, 15, 40, 50, 2, dict(padding=1)), (GEN, GEN)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, padding_mode="reflect")), (GEN, MFMA)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, padding_mode="replicate")), (GEN, MFMA)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, padding_mode="circular")), (GEN, MFMA)),
    ((F32, F32, 2, 64, 64, 40, 50, 3, dict(padding=1)), (GEN, GEN)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2)), (GEN, GEN)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, dilation=2)), (GEN, GEN)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, groups=2)), (GEN, GEN)),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=3)), (GEN, GEN)),
    ((F64, F64, 2, 64, 64, 40, 50, 2, dict(padding=1)), (GEN, GEN)),
    ((F32, F64, 2, 64, 64, 40, 50, 2, dict(padding=1)), (GEN, GEN)),
    ((torch.uint8, F32, 2, 64, 64, 40, 50, 2, dict(padding=1)), (GEN, GEN)),
    # past the forward's 32-bit-offset limit (C * h * w * 4 >= 2^31)
    ((BF16, F32, 1, 64, 64, 4096, 4096, 2, dict(padding=1)), (GEN, GEN)),
]


def _plan(row):
    *args, kw = row
    return ops.hexconv2d_backward_plan(*args, **kw)


@pytest.fixture
def switch_unset(monkeypatch):
    monkeypatch.delenv("HYGRID_CONV_BWD_MFMA", raising=False)


@pytest.mark.parametrize("row,want", TABLE)
def test_plan_domain_table(switch_unset, row, want):
    assert _plan(row) == want


@pytest.mark.parametrize("row,want", TABLE)
def test_plan_switch_selects_generic(monkeypatch, row, want):
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA", "0")
    assert _plan(row) == (GEN, GEN)
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA", "1")     # only "0" switches
    assert _plan(row) == want


def test_plan_error_codes_match_backward(switch_unset):
    """Bad arguments: the negative statuses hg_hexconv2d_backward reports before any launch."""
    L = _abi.lib()
    fake = ctypes.c_void_p(16)
    f32 = _abi.HG_F32
    dxk, dwk = ctypes.c_int(-7), ctypes.c_int(-7)

    def both(xd, wd, B, C, O_, h, w, r, s, p, d, g, pm):
        a = L.hg_hexconv2d_backward_plan(xd, wd, B, C, O_, h, w, r, s, p, d, g, pm,
                                         ctypes.byref(dxk), ctypes.byref(dwk))
        b = L.hg_hexconv2d_backward(fake, fake, fake, fake, fake, fake, xd, wd, B, C, O_, h, w,
                                    r, s, p, d, g, 0, pm, 0.0, None)
        assert a == b
        return a

    assert both(f32, f32, 1, 3, 4, 8, 8, 2, 1, 1, 1, 3, 0) == _abi.HG_EINVAL    # groups
    assert both(f32, f32, 1, 3, 3, 1, 1, 2, 1, 0, 1, 1, 0) == _abi.HG_ESHAPE    # too small
    assert both(f32, f32, 1, 3, 3, 8, 8, 2, 1, 1, 1, 1, 9) == _abi.HG_EINVAL    # pad mode
    assert both(f32, f32, 1, 3, 3, 2, 2, 2, 1, 2, 1, 1, 1) == _abi.HG_ESHAPE    # reflect pad
    assert both(f32, f32, 1, 3, 3, 8, 8, 0, 1, 1, 1, 1, 0) == _abi.HG_EINVAL    # radius
    assert both(f32, f32, -1, 3, 3, 8, 8, 2, 1, 1, 1, 1, 0) == _abi.HG_EINVAL   # batch
    assert both(f32, f32, 1, 3, 3, 40, 40, 8, 1, 1, 1, 1, 0) == _abi.HG_EUNSUP  # > 127 taps
    assert both(f32, _abi.HG_F16, 1, 3, 3, 8, 8, 2, 1, 1, 1, 1, 0) == _abi.HG_EDTYPE
    assert (dxk.value, dwk.value) == (-7, -7)           # untouched on error
    assert L.hg_hexconv2d_backward_plan(f32, f32, 1, 64, 64, 8, 8, 2, 1, 1, 1, 1, 0, None,
                                        ctypes.byref(dwk)) == _abi.HG_EINVAL
    with pytest.raises(ValueError):
        ops.hexconv2d_backward_plan(F32, F32, 1, 3, 4, 8, 8, 2, groups=3)
    with pytest.raises(ValueError):
        ops.hexconv2d_backward_plan(F32, F32, 1, 3, 3, 8, 8, 2, padding_mode="mirror")


def test_plan_empty_call_is_generic(switch_unset):
    assert ops.hexconv2d_backward_plan(F32, F32, 0, 64, 64, 40, 50, 2, padding=1) == (GEN, GEN)

