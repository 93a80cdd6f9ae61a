"""Host side of the fused chain backward (hg_pipeline_r2h_conv_h2r_backward and its workspace
query): the domain and the argument checks, all of which return before any HIP call, so
none of this needs a device."""
import ctypes

from HyGrid import _abi

BF16, F32, U8 = _abi.HG_BF16, _abi.HG_F32, _abi.HG_U8


def workspace(x_dt=BF16, gy_dt=BF16, B=2, C=3, O=3, h=64, w=96, h1=None, w1=None, h2=None,
              w2=None, pad=1, groups=1, off=0, padv=0.0):
    h1 = h if h1 is None else h1
    w1 = w if w1 is None else w1
    h2 = h1 if h2 is None else h2
    w2 = w1 if w2 is None else w2
    return _abi.lib().hg_pipeline_r2h_conv_h2r_backward_workspace(
        x_dt, gy_dt, B, C, O, h, w, h1, w1, h2, w2, pad, groups, off, padv)


def test_workspace_is_a_positive_multiple_of_16_in_the_domain():
    for g in (1, 3):
        n = workspace(groups=g)
        assert n > 0 and n % 16 == 0, (g, n)


def test_workspace_unsupported_outside_the_domain():
    assert workspace(pad=0, h2=62, w2=94) == _abi.HG_EUNSUP
    assert workspace(pad=0) == _abi.HG_EUNSUP
    assert workspace(padv=0.3) == _abi.HG_EUNSUP
    assert workspace(h2=63) == _abi.HG_EUNSUP
    assert workspace(C=2, O=2) == _abi.HG_EUNSUP
    assert workspace(x_dt=U8) == _abi.HG_EUNSUP
    assert workspace(B=1, h=70, w=130, h1=71, w1=131, h2=70, w2=130) == _abi.HG_EUNSUP


def test_workspace_monotone_in_batch():
    sizes = [workspace(B=b, h=300, w=200) for b in (1, 2, 3, 8, 64)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


def backward(x, ws_bytes):
    fake = ctypes.c_void_p(256)
    return _abi.lib().hg_pipeline_r2h_conv_h2r_backward(
        x, fake, fake, fake, fake, fake, BF16, BF16, 2, 3, 3, 64, 96, 64, 96, 64, 96, 1, 1, 0,
        0.0, fake, ws_bytes, None)


def test_backward_argument_errors_before_any_launch():
    need = workspace()
    assert backward(None, need) < 0                       # NULL x
    assert backward(ctypes.c_void_p(256), need - 1) < 0   # workspace one byte short


def test_backward_tile_layout_query():
    rows, cols, band = _abi.fused_layout(9)
    assert rows > 0 and cols > 0 and band > 0
