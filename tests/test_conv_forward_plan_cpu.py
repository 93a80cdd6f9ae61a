"""Which wide-channel forward kernel a HexConv2d layer gets (hg_hexconv2d_forward_plan, host
only: nothing is launched and no device is needed).  Dense radius-2, dilation-1 layers with f32
weights, O >= 16 and padding 0..2 run on the matrix cores at stride 1 and stride 2
(csrc/conv_mfma.hip): f32 / f16 inputs, and bf16 inputs whose pad value is no bf16, on the
f32-MFMA kernel; bf16 inputs on the split-weight bf16 kernel, staged by LDS-DMA at stride 1 when
the rows are dword-aligned (even width; the query answers for a 16-byte-aligned x) and through
registers otherwise and at stride 2.  Everything else is HG_CONV_FWD_OTHER (the streaming or
generic kernels)."""
import ctypes

import pytest
import torch

from HyGrid import _abi, ops

OTHER, MF32, MBF, MDMA = (_abi.HG_CONV_FWD_OTHER, _abi.HG_CONV_FWD_MFMA_F32,
                          _abi.HG_CONV_FWD_MFMA_BF16, _abi.HG_CONV_FWD_MFMA_BF16_DMA)
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
SWITCHES = ("HYGRID_CONV_MFMA", "HYGRID_CONV_MFMA_BF16", "HYGRID_CONV_DMA", "HYGRID_CONV_NT")


@pytest.fixture(autouse=True)
def switches_unset(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _plan(xd, wd, yd, B, C, O_, h, w, r=2, **kw):
    return ops.hexconv2d_forward_plan(xd, wd, yd, B, C, O_, h, w, r, **kw)


# (x, w, y dtypes, B, C, O, h, w, kwargs) -> kernel
STRIDE1 = [
    ((F32, F32, F32, 4, 64, 64, 1080, 1920, dict(padding=1)), MF32),
    ((F16, F32, F16, 1, 64, 64, 20, 30, dict(padding=0)), MF32),
    ((F32, F32, BF16, 1, 3, 64, 20, 30, dict(padding=2)), MF32),
    ((BF16, F32, BF16, 4, 64, 64, 1080, 1920, dict(padding=1)), MDMA),
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1)), MDMA),
    ((BF16, F32, F32, 1, 16, 16, 20, 31, dict(padding=1)), MBF),       # odd width
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1, padding_value=0.5)), MDMA),
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1, padding_value=0.3)), MF32),
    ((BF16, F32, F16, 1, 16, 16, 20, 30, dict(padding=1)), OTHER),     # no such dtype pair
    ((F32, F32, F32, 1, 64, 12, 20, 30, dict(padding=1)), OTHER),
    ((F32, F64, F32, 1, 64, 64, 20, 30, dict(padding=1)), OTHER),
    ((F64, F64, F64, 1, 64, 64, 20, 30, dict(padding=1)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=1, padding_mode="reflect")), MF32),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=3)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=1, groups=2)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=1, dilation=2)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(r=3, padding=1)), OTHER),
    ((torch.uint8, F32, F32, 1, 64, 64, 20, 30, dict(padding=1)), OTHER),
    # past the 32-bit-offset limit (C * h * w * 4 >= 2^31)
    ((BF16, F32, BF16, 1, 64, 64, 4096, 4096, dict(padding=1)), OTHER),
]
STRIDE2 = [
    ((F32, F32, F32, 4, 64, 128, 1080, 1920, dict(padding=1)), MF32),
    ((F16, F32, F16, 1, 64, 64, 20, 30, dict(padding=0)), MF32),
    ((F16, F32, F32, 1, 3, 64, 21, 131, dict(padding=2)), MF32),
    ((F32, F32, F16, 1, 16, 16, 3, 6, dict(padding=0)), MF32),
    ((BF16, F32, BF16, 4, 64, 128, 1080, 1920, dict(padding=1)), MBF),  # even width: never DMA
    ((BF16, F32, F32, 1, 16, 16, 20, 31, dict(padding=1)), MBF),        # odd width
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1, padding_value=0.5)), MBF),
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1, padding_value=0.3)), MF32),
    ((BF16, F32, F32, 1, 16, 16, 20, 30, dict(padding=1, padding_mode="circular")), MBF),
    ((F32, F32, F32, 1, 64, 8, 20, 30, dict(padding=1)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=1, groups=2)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=1, dilation=2)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(r=3, padding=1)), OTHER),
    ((F32, F32, F32, 1, 64, 64, 20, 30, dict(padding=3)), OTHER),
    ((F32, F64, F32, 1, 64, 64, 20, 30, dict(padding=1)), OTHER),
    ((BF16, F64, F32, 1, 64, 64, 20, 30, dict(padding=1)), OTHER),
]


@pytest.mark.parametrize("row,want", STRIDE1)
def test_stride1_routes(row, want):
    *args, kw = row
    assert _plan(*args, stride=1, **kw) == want
    assert _plan(*args, **kw) == want                    # stride defaults to 1


@pytest.mark.parametrize("row,want", STRIDE2)
def test_stride2_routes(row, want):
    *args, kw = row
    assert _plan(*args, stride=2, **kw) == want


@pytest.mark.parametrize("row,want", STRIDE1[:4] + STRIDE2[:5])
def test_stride3_and_up_is_other(row, want):
    *args, kw = row
    for s in (3, 4):
        assert _plan(*args, stride=s, **kw) == OTHER


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("stride", [1, 2])
def test_offset_does_not_route(stride, off):
    assert _plan(F32, F32, F32, 1, 16, 16, 9, 10, stride=stride, even_odd_offset=off) == MF32


@pytest.mark.parametrize("stride", [1, 2])
def test_switches(monkeypatch, stride):
    bf = (BF16, F32, BF16, 2, 32, 32, 40, 50)
    fl = (F32, F32, F32, 2, 32, 32, 40, 50)
    base = MDMA if stride == 1 else MBF
    assert _plan(*bf, stride=stride, padding=1) == base
    monkeypatch.setenv("HYGRID_CONV_DMA", "0")
    assert _plan(*bf, stride=stride, padding=1) == MBF
    monkeypatch.setenv("HYGRID_CONV_DMA", "1")           # only "0" switches
    assert _plan(*bf, stride=stride, padding=1) == base
    monkeypatch.setenv("HYGRID_CONV_MFMA_BF16", "0")
    assert _plan(*bf, stride=stride, padding=1) == MF32
    assert _plan(*fl, stride=stride, padding=1) == MF32
    monkeypatch.setenv("HYGRID_CONV_MFMA", "0")
    assert _plan(*bf, stride=stride, padding=1) == OTHER
    assert _plan(*fl, stride=stride, padding=1) == OTHER
    monkeypatch.setenv("HYGRID_CONV_MFMA", "1")
    monkeypatch.delenv("HYGRID_CONV_MFMA_BF16")
    assert _plan(*bf, stride=stride, padding=1) == base


def test_error_codes_match_forward():
    """Bad arguments: the negative statuses hg_hexconv2d reports before any launch (the call
    gets null buffers, which it looks at only after these checks)."""
    L = _abi.lib()
    f32 = _abi.HG_F32
    kk = ctypes.c_int(-7)

    def both(xd, wd, yd, B, C, O_, h, w, r, s, p, d, g, pm):
        a = L.hg_hexconv2d_forward_plan(xd, wd, yd, B, C, O_, h, w, r, s, p, d, g, 0, pm, 0.0,
                                        ctypes.byref(kk))
        b = L.hg_hexconv2d(None, None, None, None, xd, wd, yd, B, C, O_, h, w, r, s, p, d, g, 0,
                           pm, 0.0, None)
        assert a == b and a < 0
        return a

    for s in (1, 2):
        assert both(f32, f32, f32, 1, 3, 4, 8, 8, 2, s, 1, 1, 3, 0) == _abi.HG_EINVAL  # groups
        assert both(f32, f32, f32, 1, 64, 64, 3, 2, 2, s, 0, 1, 1, 0) == _abi.HG_ESHAPE  # small
        assert both(f32, f32, f32, 1, 3, 3, 8, 8, 2, s, 1, 1, 1, 9) == _abi.HG_EINVAL  # pad mode
        assert both(f32, f32, f32, 1, 3, 3, 2, 2, 2, s, 2, 1, 1, 1) == _abi.HG_ESHAPE  # reflect
        assert both(f32, f32, f32, 1, 3, 3, 8, 8, 0, s, 1, 1, 1, 0) == _abi.HG_EINVAL  # radius
        assert both(f32, f32, f32, -1, 3, 3, 8, 8, 2, s, 1, 1, 1, 0) == _abi.HG_EINVAL  # batch
        assert both(f32, f32, f32, 1, 3, 3, 40, 40, 8, s, 1, 1, 1, 0) == _abi.HG_EUNSUP  # taps
    assert both(f32, f32, f32, 1, 3, 3, 8, 8, 2, 0, 1, 1, 1, 0) == _abi.HG_EINVAL      # stride
    assert kk.value == -7                                # untouched on error
    # dtype errors: the call reports them once it has buffers; the query needs none
    assert L.hg_hexconv2d_forward_plan(f32, _abi.HG_F16, f32, 1, 64, 64, 8, 8, 2, 1, 1, 1, 1, 0,
                                       0, 0.0, ctypes.byref(kk)) == _abi.HG_EDTYPE
    assert L.hg_hexconv2d_forward_plan(f32, f32, _abi.HG_I32, 1, 64, 64, 8, 8, 2, 1, 1, 1, 1, 0,
                                       0, 0.0, ctypes.byref(kk)) == _abi.HG_EDTYPE
    assert L.hg_hexconv2d_forward_plan(f32, f32, f32, 1, 64, 64, 8, 8, 2, 1, 1, 1, 1, 0, 0, 0.0,
                                       None) == _abi.HG_EINVAL
    assert kk.value == -7
    with pytest.raises(ValueError):
        _plan(F32, F32, F32, 1, 3, 4, 8, 8, groups=3, stride=2)
    with pytest.raises(ValueError):
        _plan(F32, F32, F32, 1, 64, 64, 3, 2, stride=2)
    with pytest.raises(ValueError):
        _plan(F32, F32, F32, 1, 3, 3, 8, 8, padding_mode="mirror")


def test_empty_call_is_other():
    assert _plan(F32, F32, F32, 0, 64, 64, 40, 50, padding=1, stride=2) == OTHER


def test_smallest_stride2_layer_matches_out_shape():
    """(h, w) = (3, 6) is the smallest layer with an output at stride 2, pad 0: one row, two
    columns; one row or one column less has none."""
    assert ops.hexconv2d_out_shape(3, 6, 2, 2, 0, 1) == (1, 2)
    assert _plan(F32, F32, F32, 1, 16, 16, 3, 6, stride=2) == MF32
    with pytest.raises(ValueError):
        _plan(F32, F32, F32, 1, 16, 16, 2, 6, stride=2)
