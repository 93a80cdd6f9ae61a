"""GPU parity of the matrix-core HexConv2d backward (csrc/conv_mfma_bwd.hip): d kernel / d bias
on k_hexconv_bwd_weight_mfma (O >= 16) and d input on the forward f32-MFMA kernel run on the
adjoint geometry (C >= 16, constant padding), against the fp64 adjoint oracle
(oracle/hg_oracle.c or_hexconv2d_backward) and the generic kernels (HYGRID_CONV_BWD_MFMA=0).

Tolerances are those of tests/test_gpu_backward.py: fp32 sums in another order than the
oracle's -> rtol 1e-4, atol 1e-5 * max|ref|; a 16-bit d input is one rounding of the fp32 sum
(2^-8 bf16, 2^-11 f16, relative to max|ref|).  Every case first asserts through the plan query
which kernel it exercises.  Shapes are the smallest that reach each path: rows that are no
multiple of 4 (9, 33, 17, 11, 6), widths inside one 64-column tile, crossing one (70, 75) and
two (130), wo % 4 != 0 (scalar gy loads) and wo % 4 == 0 (16-B gy loads): wo = w - 2 + 2 *
padding, so every even width gives both across the three paddings and the odd widths (21, 75, 9)
only the scalar loads; partial channel chunks (1, 3, 13, 70) and partial output tiles (20, 33,
100)."""
import functools
import os

import numpy as np
import pytest
import torch

import placement as PL
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402
from HyGrid.HexFrames import HexConv2d  # noqa: E402

DEV = torch.device("cuda:0")
GEN, MFMA = _abi.HG_CONV_BWD_GENERIC, _abi.HG_CONV_BWD_MFMA
SWITCH = "HYGRID_CONV_BWD_MFMA"

DW_CASES = [  # (B, C, O, h, w)
    (2, 8, 16, 9, 10), (1, 16, 16, 33, 70), (1, 32, 64, 20, 130), (2, 3, 64, 17, 64),
    (1, 13, 20, 12, 21), (1, 24, 100, 11, 75), (1, 70, 33, 6, 9), (1, 1, 16, 9, 10)]
# the same list, C and O swapped where C < 16
DX_CASES = [(B, O_, C, h, w) if C < 16 else (B, C, O_, h, w) for (B, C, O_, h, w) in DW_CASES]


def _cfg(pad, off, mode="constant", pv=0.0):
    return dict(off=off, r=2, stride=1, pad=pad, dilation=1, groups=1, padding_mode=mode,
                padding_value=pv, out_dtype=None)


def _plan(x, k, cfg):
    B, C, h, w = x.shape
    return ops.hexconv2d_backward_plan(x.dtype, k.dtype, B, C, k.shape[0], h, w, 2,
                                       padding=cfg["pad"], padding_mode=cfg["padding_mode"])


def _with_env(name, value, fn, *args, **kw):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _generic(*args, **kw):
    return _with_env(SWITCH, "0", ops.hexconv2d_backward, *args, **kw)


@functools.lru_cache(maxsize=None)
def _data(case, pad, off, mode="constant", pv=0.0, dtype=torch.float32):
    """(x, kernel, bias, gy) on the host and the fp64 oracle's (dx, dk, db); computed once per
    key, shared by the tests, never modified."""
    B, C, O_, h, w = case
    g = torch.Generator().manual_seed(h * 131 + w * 7 + C + 3 * pad + off)
    x = (torch.rand((B, C, h, w), generator=g) - 0.5).to(dtype)
    k = (torch.rand((O_, C, 1, 7), generator=g) - 0.5) / np.sqrt(7 * C)
    b = torch.rand((O_,), generator=g) - 0.5
    ho, wo = O.hexconv2d_out_shape(h, w, 2, 1, pad, 1)
    gy = torch.randn((B, O_, ho, wo), generator=g)
    ref = O.hexconv2d_backward(x.double().numpy(), k.double().numpy(), gy.double().numpy(), off, 2,
                               1, pad, 1, 1, mode, pv)
    return (x, k, b, gy), ref


def _close(got, ref, rtol=1e-4):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    print("max abs err", np.abs(got - ref).max(), "max|ref|", np.abs(ref).max())
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 0.1 * max(np.abs(ref).max(), 1e-30))


def _dev(ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("case", DW_CASES)
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_dkernel_dbias_vs_oracle(case, pad, off):
    (x, k, b, gy), (_, rdk, rdb) = _data(case, pad, off)
    x, k, b, gy = _dev((x, k, b, gy))
    cfg = _cfg(pad, off)
    assert _plan(x, k, cfg)[1] == MFMA
    dx, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg, False, True, True)
    assert dx is None and dk.shape == k.shape
    _close(dk, rdk)
    _close(db, rdb)


@pytest.mark.parametrize("case", DX_CASES)
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_dinput_vs_oracle(case, pad, off):
    (x, k, b, gy), (rdx, _, _) = _data(case, pad, off)
    x, k, b, gy = _dev((x, k, b, gy))
    cfg = _cfg(pad, off)
    assert _plan(x, k, cfg)[0] == MFMA
    dx, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg, True, False, False)
    assert dk is None and db is None and dx.shape == x.shape
    _close(dx, rdx)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
def test_padding_modes_vs_oracle(mode):
    """d kernel on the MFMA kernel in every mode (the pad value 0.3 enters it through P);
    d input on it for constant padding only (the pad value does not reach it)."""
    pv = 0.3 if mode == "constant" else 0.0
    (x, k, b, gy), (rdx, rdk, rdb) = _data((1, 16, 32, 14, 40), 1, 0, mode, pv)
    x, k, b, gy = _dev((x, k, b, gy))
    cfg = _cfg(1, 0, mode, pv)
    assert _plan(x, k, cfg) == ((MFMA if mode == "constant" else GEN), MFMA)
    dx, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg)
    _close(dx, rdx)
    _close(dk, rdk)
    _close(db, rdb)


@pytest.mark.parametrize("dt,ulp", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_16bit_input(dt, ulp):
    """The oracle gets x's exact values; d input has x's dtype, one rounding of the fp32 sum."""
    (x, k, b, gy), (rdx, rdk, rdb) = _data((1, 32, 64, 20, 130), 1, 1, dtype=dt)
    x, k, b, gy = _dev((x, k, b, gy))
    cfg = _cfg(1, 1)
    assert _plan(x, k, cfg) == (MFMA, MFMA)
    dx, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg)
    assert dx.dtype == dt and dk.dtype == torch.float32
    got = dx.double().cpu().numpy()
    print("max abs err", np.abs(got - rdx).max(), "max|ref|", np.abs(rdx).max())
    np.testing.assert_allclose(got, rdx, rtol=ulp, atol=ulp * np.abs(rdx).max())
    _close(dk, rdk)
    _close(db, rdb)


def test_partial_requests_and_reproducibility():
    (x, k, b, gy), (rdx, rdk, rdb) = _data((1, 16, 16, 33, 70), 1, 0)
    x, k, b, gy = _dev((x, k, b, gy))
    cfg = _cfg(1, 0)
    assert _plan(x, k, cfg) == (MFMA, MFMA)
    dx, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg)
    _close(dx, rdx)
    _close(dk, rdk)
    _close(db, rdb)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for need in [(True, False, False), (False, True, False), (False, False, True),
                 (False, True, True)]:
        gx, gk, gb = ops.hexconv2d_backward(gy, x, k, b, cfg, *need)
        assert [g is not None for g in (gx, gk, gb)] == list(need)
        if gx is not None:
            assert torch.equal(bits(gx), bits(dx))
        if gk is not None:
            _close(gk, rdk)
            torch.testing.assert_close(gk, dk, rtol=1e-4, atol=1e-5 * float(dk.abs().max()))
        if gb is not None:
            _close(gb, rdb)
    # d input has no atomics: the same bits from run to run (and in the full call above)
    again = ops.hexconv2d_backward(gy, x, k, b, cfg, True, False, False)[0]
    assert torch.equal(bits(again), bits(dx))


@pytest.mark.parametrize("i", range(4))
def test_agrees_with_generic_kernels(i):
    for case, which in ((DW_CASES[i], 1), (DX_CASES[i], 0)):
        (x, k, b, gy), _ = _data(case, 1, 1)
        x, k, b, gy = _dev((x, k, b, gy))
        cfg = _cfg(1, 1)
        assert _plan(x, k, cfg)[which] == MFMA
        assert _with_env(SWITCH, "0", _plan, x, k, cfg) == (GEN, GEN)
        got = ops.hexconv2d_backward(gy, x, k, b, cfg)
        ref = _generic(gy, x, k, b, cfg)
        sel = (1, 2) if which else (0,)
        for j in sel:
            print("max abs diff", float((got[j] - ref[j]).abs().max()))
            torch.testing.assert_close(got[j], ref[j], rtol=1e-4,
                                       atol=1e-5 * float(ref[j].abs().max()))


def test_nonfinite_x_positions_match_generic():
    """NaN / Inf in x with finite gy, on a shape with wo % 64 != 0 and ho % 4 != 0: the edge
    tiles' masked pixels read the last row and column of x and must not contribute (both MFMA
    operands are zeroed there: 0 * Inf would be NaN)."""
    (x, k, b, gy), _ = _data((1, 16, 16, 33, 70), 1, 0)
    x, k, b, gy = _dev((x, k, b, gy))
    x = x.clone()
    x[0, 0, 0, 0] = float("nan")
    x[0, 1, :, -1] = float("inf")
    x[0, 2, -1, :] = float("-inf")
    x[0, 5, -1, -1] = float("inf")
    cfg = _cfg(1, 0)
    assert _plan(x, k, cfg)[1] == MFMA
    _, dk, db = ops.hexconv2d_backward(gy, x, k, b, cfg, False, True, True)
    _, rk, rb = _generic(gy, x, k, b, cfg, False, True, True)
    assert torch.equal(torch.isnan(dk), torch.isnan(rk))
    assert torch.equal(torch.isinf(dk), torch.isinf(rk))
    assert torch.equal(dk[torch.isinf(rk)], rk[torch.isinf(rk)])
    fin = torch.isfinite(rk)
    assert int(fin.sum()) >= 16 * 10 * 7 and int((~fin).sum()) > 0
    torch.testing.assert_close(dk[fin], rk[fin], rtol=1e-4, atol=1e-5 * float(rk[fin].abs().max()))
    assert bool(torch.isfinite(db).all())
    torch.testing.assert_close(db, rb, rtol=1e-4, atol=1e-5 * float(rb.abs().max()))


def test_nonfinite_gy_positions_match_generic():
    (x, k, b, gy), _ = _data((1, 16, 16, 33, 70), 1, 0)
    x, k, b, gy = _dev((x, k, b, gy))
    gy = gy.clone()
    gy[0, 3, 0, 0] = float("inf")
    gy[0, 4, -1, -1] = float("-inf")
    gy[0, 7, 16, 63] = float("inf")
    gy[0, 9, 16, 64] = float("-inf")
    cfg = _cfg(1, 0)
    assert _plan(x, k, cfg)[0] == MFMA
    dx = ops.hexconv2d_backward(gy, x, k, b, cfg, True, False, False)[0]
    rx = _generic(gy, x, k, b, cfg, True, False, False)[0]
    assert torch.equal(torch.isnan(dx), torch.isnan(rx))
    assert torch.equal(torch.isinf(dx), torch.isinf(rx))
    assert torch.equal(dx[torch.isinf(rx)], rx[torch.isinf(rx)])
    fin = torch.isfinite(rx)
    assert int((~fin).sum()) > 0
    torch.testing.assert_close(dx[fin], rx[fin], rtol=1e-4, atol=1e-5 * float(rx[fin].abs().max()))


@pytest.mark.parametrize("case,pad", [((1, 16, 16, 33, 70), 1), ((2, 16, 16, 17, 64), 1),
                                      ((1, 24, 100, 11, 75), 0)])
@pytest.mark.parametrize("off_out", [0, 1])
@pytest.mark.parametrize("off_in", [0, 1])
def test_placement_inside_guard_arenas(monkeypatch, case, pad, off_out, off_in):
    """d input, d kernel and d bias allocated inside sentinel arenas at element offsets 0 / 1,
    x and gy placed at offsets 0 / 1 with NaN guards around them (offset 1 takes gy off its
    16-B alignment: the scalar gy loads; (2, 16, 16, 17, 64) has wo % 4 == 0, so offset 0 there
    is the vector path).  No guard byte changes, every result element is written, and no guard
    NaN reaches a gradient."""
    (x, k, b, gy), (rdx, rdk, rdb) = _data(case, pad, 0)
    k, b = _dev((k, b))
    xv, xa = PL.place(x, DEV, off_in)
    gv, ga = PL.place(gy, DEV, off_in)
    cfg = _cfg(pad, 0)
    assert _plan(xv, k, cfg) == (MFMA, MFMA)
    with PL.placed(monkeypatch, off_out, min_dim=1) as rec:
        dx, dk, db = ops.hexconv2d_backward(gv, xv, k, b, cfg)
    assert len(rec.arenas) == 3
    assert rec.arena_of(dx) is not None and rec.arena_of(db) is not None
    PL.guards_intact(xa, xv, "x ")
    PL.guards_intact(ga, gv, "gy ")
    for t in (dx, dk, db):
        assert PL.sentinel_count(t) == 0
        assert bool(torch.isfinite(t).all())
    _close(dx, rdx)
    _close(dk, rdk)
    _close(db, rdb)


def test_autograd_hexconv2d_end_to_end():
    torch.manual_seed(7)
    m = HexConv2d(16, 32, 1, 2, padding=1, bias=True).to(DEV)
    x = torch.rand((2, 16, 31, 45), device=DEV, requires_grad=True)
    assert ops.hexconv2d_backward_plan(x.dtype, m.kernel.dtype, 2, 16, 32, 31, 45, 2,
                                       padding=1) == (MFMA, MFMA)
    y = m(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    dx, dk, db = O.hexconv2d_backward(
        x.detach().double().cpu().numpy(), m.kernel.detach().double().cpu().numpy(),
        gy.double().cpu().numpy(), 1, 2, 1, 1)
    _close(x.grad, dx)
    _close(m.kernel.grad, dk)
    _close(m.bias.grad, db)


def test_autograd_hexconvmodule_fused_epilogue_end_to_end():
    """conv + eval BatchNorm + ReLU in one launch; its backward carries gy through the
    activation mask and the BN scale (HexModules._HexConvEpilogueFn.backward) into
    hg_hexconv2d_backward."""
    from HyGrid.HexModules import HexConvModule
    torch.manual_seed(3)
    m = HexConvModule(16, 32, 1, 2, padding=1, bias=True, norm_cfg=dict(type="BN"),
                      act_cfg=dict(type="ReLU")).to(DEV).eval()
    with torch.no_grad():
        m.norm.running_mean.uniform_(-0.2, 0.2)
        m.norm.running_var.uniform_(0.5, 1.5)
        m.norm.weight.uniform_(0.5, 1.5)
    for prm in m.norm.parameters():                      # a frozen BN: the fused epilogue
        prm.requires_grad_(False)
    x = torch.rand((2, 16, 31, 45), device=DEV, requires_grad=True)
    assert m._epilogue_plan(x, True, True) is not None
    assert ops.hexconv2d_backward_plan(x.dtype, m.conv.kernel.dtype, 2, 16, 32, 31, 45, 2,
                                       padding=1) == (MFMA, MFMA)
    y = m(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    scale = (m.norm.weight / torch.sqrt(m.norm.running_var + m.norm.eps)).detach()
    g = gy * (y.detach() > 0).to(gy.dtype) * scale.view(1, -1, 1, 1)
    dx, dk, db = O.hexconv2d_backward(
        x.detach().double().cpu().numpy(), m.conv.kernel.detach().double().cpu().numpy(),
        g.double().cpu().numpy(), 1, 2, 1, 1)
    _close(x.grad, dx)
    _close(m.conv.kernel.grad, dk)
    _close(m.conv.bias.grad, db)
