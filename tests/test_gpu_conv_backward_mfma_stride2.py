"""GPU parity of the stride-2 training routes: d kernel / d bias on k_hexconv_bwd_weight_mfma_s2
(hg_hexconv2d_weight_grad, csrc/conv_mfma_bwd.hip) and d input as the transposed layer's forward
on gy (k_hexconvt_s2), both through ops.hexconv2d_grads, against the fp64 adjoint oracle
(oracle.hexconv2d_backward with stride 2) and the generic kernels (HYGRID_CONV_BWD_MFMA_S2=0,
HYGRID_CONVT_MFMA=0).

Tolerances are those of tests/test_gpu_conv_backward_mfma.py: fp32-exact products summed in
another order than the oracle's -> rtol 1e-4, atol 1e-5 * max|ref|; a 16-bit d input is one
rounding of the fp32 sum (2^-8 bf16, 2^-11 f16, relative to max|ref|).  Every case first asserts
through the plan queries which kernels it exercises.  The shapes (tests/conv_bwd_s2_cases.py) are
the smallest that reach each path; tests/test_conv_backward_mfma_stride2_index_cpu.py walks every
one of them on the host first."""
import os

import numpy as np
import pytest
import torch

import conv_bwd_s2_cases as CS
import placement as PL
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402
from HyGrid.HexFrames import HexConv2d, HexConvTranspose2d  # noqa: E402

DEV = torch.device("cuda:0")
S2, GEN = _abi.HG_CONV_WGRAD_MFMA_S2, _abi.HG_CONV_WGRAD_GENERIC
SW_DK, SW_DX = "HYGRID_CONV_BWD_MFMA_S2", "HYGRID_CONVT_MFMA"


def _cfg(case):
    B, C, O_, h, w, pad, off, mode, pv = case
    return dict(off=off, r=2, stride=2, pad=pad, dilation=1, groups=1, padding_mode=mode,
                padding_value=pv, out_dtype=None)


def _plan(case, x_dtype=torch.float32):
    B, C, O_, h, w, pad, off, mode, pv = case
    return ops.hexconv2d_training_plan(x_dtype, torch.float32, B, C, O_, h, w, 2, 2, pad, 1, 1,
                                       off, mode)


def _with_env(names, fn, *args, **kw):
    old = {n: os.environ.get(n) for n in names}
    os.environ.update({n: "0" for n in names})
    try:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


def _close(got, ref, rtol=1e-4):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    print("max abs err", np.abs(got - ref).max(), "max|ref|", np.abs(ref).max())
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 0.1 * max(np.abs(ref).max(), 1e-30))


def _dev(arrs, x_dtype=torch.float32):
    x, k, b, gy = (torch.from_numpy(np.array(a)).to(DEV) for a in arrs)
    return x.to(x_dtype), k, b, gy


def _check_all(case, want_plan):
    arrs, (rdx, rdk, rdb) = CS.data(case)
    x, k, b, gy = _dev(arrs)
    assert _plan(case) == want_plan
    dx, dk, db = ops.hexconv2d_grads(gy, x, k, b, _cfg(case))
    assert dx.shape == x.shape and dk.shape == k.shape and db.shape == b.shape
    _close(dk, rdk)
    _close(db, rdb)
    _close(dx, rdx)
    return (x, k, b, gy), (dx, dk, db)


# ---- 1. guard bands ---------------------------------------------------------------------------------
@pytest.mark.parametrize("off_out", [0, 1])
@pytest.mark.parametrize("off_in", [0, 1])
def test_placement_inside_guard_arenas(monkeypatch, off_out, off_in):
    """hg_hexconv2d_weight_grad's two destinations inside sentinel arenas at element offsets
    0 / 1, x and gy placed at offsets 0 / 1 with NaN guards around them (offset 1 takes gy off
    its 16-B alignment).  No guard byte changes, every element of d kernel and d bias is written,
    and no guard NaN reaches a gradient; then each destination alone."""
    case = (2, 16, 16) + CS.SMALL + (1, 1, "constant", 0.0)
    arrs, (_, rdk, rdb) = CS.data(case)
    x, k, b, gy = _dev(arrs)
    xv, xa = PL.place(x, DEV, off_in)
    gv, ga = PL.place(gy, DEV, off_in)
    cfg = _cfg(case)
    assert _plan(case)[1] == S2
    for need in [(True, True), (True, False), (False, True)]:
        with PL.placed(monkeypatch, off_out, min_dim=1) as rec:
            dk, db = ops.hexconv2d_weight_grad(gv, xv, k, b, cfg, *need)
        torch.cuda.synchronize()
        assert len(rec.arenas) == sum(need)
        rec.check("weight_grad ")
        PL.guards_intact(xa, xv, "x ")
        PL.guards_intact(ga, gv, "gy ")
        assert [t is not None for t in (dk, db)] == list(need)
        for t, ref in ((dk, rdk), (db, rdb)):
            if t is not None:
                assert rec.arena_of(t) is not None
                assert PL.sentinel_count(t) == 0 and bool(torch.isfinite(t).all())
                _close(t, ref)


# ---- 2. every (offset, padding) pair on one tile with every edge ------------------------------------
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_offsets_and_paddings_vs_oracle(off, pad):
    _check_all((2, 16, 16) + CS.SMALL + (pad, off, "constant", 0.0), ("convt_s2", S2))


# ---- 3. column tiles and both gy load paths -----------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1])
def test_column_tiles_and_gy_load_paths(i):
    h, w = CS.column_cases(ops.hexconv2d_out_shape)[i]
    assert (h, w) == CS.column_cases(O.hexconv2d_out_shape)[i]
    ho, wo = ops.hexconv2d_out_shape(h, w, 2, 2, 1, 1)
    assert h == 11 and wo > 64 and (wo % 4 != 0 if i == 0 else wo % 4 == 0)
    _check_all((1, 16, 16, h, w, 1, 1, "constant", 0.0), ("convt_s2", S2))


# ---- 4. row tiles and more than one slice ---------------------------------------------------------------
def test_row_tiles_and_slices():
    h, w = CS.slice_case(ops.hexconv2d_out_shape)
    ho, wo = ops.hexconv2d_out_shape(h, w, 2, 2, 1, 1)
    assert (ho, wo) == (20, 65) and 2 * ((ho + 3) // 4) * ((wo + 63) // 64) >= 16
    _check_all((2, 16, 16, h, w, 1, 0, "constant", 0.0), ("convt_s2", S2))


# ---- 5. channel remainders -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,O_", CS.CHANNELS)
def test_channel_remainders(C, O_):
    _check_all((2, C, O_) + CS.SMALL + (1, 1, "constant", 0.0),
               ("convt_s2" if C >= 16 else "generic", S2))


# ---- 6. input dtypes, padding modes, pad value -----------------------------------------------------------
@pytest.mark.parametrize("dt,ulp", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11),
                                    (torch.float32, None)])
def test_input_dtypes(dt, ulp):
    """The oracle gets x's exact values; d input has x's dtype, one rounding of the fp32 sum."""
    case = (2, 16, 16) + CS.SMALL + (1, 1, "constant", 0.0)
    arrs, (rdx, rdk, rdb) = CS.data(case, str(dt).split(".")[1])
    x, k, b, gy = _dev(arrs, dt)
    assert _plan(case, dt) == ("convt_s2", S2)
    dx, dk, db = ops.hexconv2d_grads(gy, x, k, b, _cfg(case))
    assert dx.dtype == dt and dk.dtype == torch.float32 and db.dtype == torch.float32
    _close(dk, rdk)
    _close(db, rdb)
    if ulp is None:
        _close(dx, rdx)
    else:
        got = dx.double().cpu().numpy()
        print("max abs err", np.abs(got - rdx).max(), "max|ref|", np.abs(rdx).max())
        np.testing.assert_allclose(got, rdx, rtol=ulp, atol=ulp * np.abs(rdx).max())


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
def test_padding_modes(mode):
    """d kernel on the matrix cores in every mode; d input of these is planned generic."""
    _check_all((2, 16, 16) + CS.SMALL + (2, 1, mode, 0.0), ("generic", S2))


def test_constant_pad_value_reaches_dkernel_only():
    case = (2, 16, 16) + CS.SMALL + (1, 0, "constant", 0.5)
    _, (dx, dk, db) = _check_all(case, ("convt_s2", S2))
    zero = case[:8] + (0.0,)
    arrs, _ = CS.data(case)
    x, k, b, gy = _dev(arrs)
    dx0, dk0, db0 = ops.hexconv2d_grads(gy, x, k, b, _cfg(zero))
    assert torch.equal(dx0, dx)                          # d input: no atomics, the same bits
    torch.testing.assert_close(db0, db, rtol=1e-4, atol=1e-5 * float(db.abs().max()))
    rdk, rdk0 = CS.data(case)[1][1], CS.data(zero)[1][1]
    _close(dk0, rdk0)
    assert np.abs(rdk - rdk0).max() > 1e-2 * np.abs(rdk).max()     # far above the tolerance


# ---- the generic kernels under the switches ----------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 16, 16) + CS.SMALL + (1, 1, "constant", 0.0),
                                  (2, 20, 24) + CS.SMALL + (1, 1, "constant", 0.0),
                                  (2, 16, 16) + CS.SMALL + (2, 1, "reflect", 0.0)], ids=str)
def test_agrees_with_generic_kernels(case):
    arrs, _ = CS.data(case)
    x, k, b, gy = _dev(arrs)
    cfg = _cfg(case)
    assert _plan(case)[1] == S2
    assert _with_env((SW_DK, SW_DX), _plan, case) == ("generic", GEN)
    got = ops.hexconv2d_grads(gy, x, k, b, cfg)
    ref = _with_env((SW_DK, SW_DX), ops.hexconv2d_grads, gy, x, k, b, cfg)
    old = ops.hexconv2d_backward(gy, x, k, b, cfg)       # hg_hexconv2d_backward: generic at stride 2
    for j in range(3):
        print("max abs diff", float((got[j] - ref[j]).abs().max()))
        torch.testing.assert_close(got[j], ref[j], rtol=1e-4, atol=1e-5 * float(ref[j].abs().max()))
        torch.testing.assert_close(ref[j], old[j], rtol=1e-4, atol=1e-5 * float(old[j].abs().max()))


# ---- 7. Inf where no tap reaches ---------------------------------------------------------------------------
def test_inf_where_no_tap_reaches():
    """Padding 0 and a size whose last row / columns no tap reads: +Inf there and nowhere else.
    The edge tiles stage those samples and mask them (both MFMA operands), and d input there is
    0: all three gradients are finite and match the oracle."""
    (h, w), hole = CS.untapped_case()
    case = (1, 16, 16, h, w, 0, 0, "constant", 0.0)
    arrs, (rdx, rdk, rdb) = CS.data(case)
    x, k, b, gy = _dev(arrs)
    if hole.any():
        assert int(hole.sum()) >= w                      # at least the last row
    x = x.clone()
    x[:, :, torch.from_numpy(hole).to(DEV)] = float("inf")
    assert int(torch.isinf(x).sum()) == 16 * int(hole.sum())
    assert _plan(case) == ("convt_s2", S2)
    dx, dk, db = ops.hexconv2d_grads(gy, x, k, b, _cfg(case))
    for t in (dx, dk, db):
        assert bool(torch.isfinite(t).all())
    _close(dk, rdk)
    _close(db, rdb)
    _close(dx, rdx)
    assert bool((dx[:, :, torch.from_numpy(hole).to(DEV)] == 0).all())


# ---- 8. autograd through the modules ------------------------------------------------------------------------
def _module_refs(m, x, gy, off):
    return O.hexconv2d_backward(
        x.detach().double().cpu().numpy(), m.kernel.detach().double().cpu().numpy(),
        gy.double().cpu().numpy(), off, 2, 2, 1)


def test_autograd_hexconv2d():
    torch.manual_seed(7)
    m = HexConv2d(16, 32, 1, 2, stride=2, padding=1, bias=True).to(DEV)
    h, w = CS.SMALL
    assert ops.hexconv2d_training_plan(torch.float32, torch.float32, 2, 16, 32, h, w, 2, 2, 1, 1, 1,
                                       1, "constant") == ("convt_s2", S2)
    x = torch.rand((2, 16, h, w), device=DEV, requires_grad=True)
    y = m(x)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    y.backward(gy)
    rdx, rdk, rdb = _module_refs(m, x, gy, 1)
    _close(x.grad, rdx)
    _close(m.kernel.grad, rdk)
    _close(m.bias.grad, rdb)
    # each gradient requested alone
    for which in ("x", "kernel", "bias"):
        for p in m.parameters():
            p.requires_grad_(False)
            p.grad = None
        xx = x.detach().clone().requires_grad_(which == "x")
        if which != "x":
            getattr(m, which).requires_grad_(True)
        m(xx).backward(gy)
        got = xx.grad if which == "x" else getattr(m, which).grad
        others = [t.grad for t in (xx, m.kernel, m.bias) if t.grad is not None]
        assert len(others) == 1 and got is not None
        _close(got, dict(x=rdx, kernel=rdk, bias=rdb)[which])
    torch.manual_seed(7)
    nb = HexConv2d(16, 32, 1, 2, stride=2, padding=1, bias=False).to(DEV)
    xx = x.detach().clone().requires_grad_(True)
    nb(xx).backward(gy)
    assert nb.bias is None
    rdx, rdk, _ = _module_refs(nb, xx, gy, 1)
    _close(xx.grad, rdx)
    _close(nb.kernel.grad, rdk)


def test_autograd_hexconv_transpose2d_dkernel():
    """y = A^T x: d kernel is A's d kernel with the roles swapped (A's input is gy, A's gradient
    is x), at stride 2 on k_hexconv_bwd_weight_mfma_s2."""
    torch.manual_seed(5)
    m = HexConvTranspose2d(32, 16, 1, 2, stride=2, padding=1).to(DEV)
    x = torch.rand((2, 32, 7, 11), device=DEV, requires_grad=True)
    y = m(x)
    h, w = y.shape[2:]
    with torch.no_grad():
        assert ops.hexconv2d_out_shape(h, w, 2, 2, 1, 1) == (7, 11)
        # the adjoint conv A: 16 -> 32 channels on (h, w)
        assert ops.hexconv2d_training_plan(torch.float32, torch.float32, 2, 16, 32, h, w, 2, 2, 1,
                                           1, 1, 1, "constant")[1] == S2
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y.backward(gy)
    _, rdk, _ = O.hexconv2d_backward(gy.double().cpu().numpy(),
                                     m.kernel.detach().double().cpu().numpy(),
                                     x.detach().double().cpu().numpy(), 1, 2, 2, 1)
    _close(m.kernel.grad, rdk)
    _close(m.bias.grad, gy.double().sum((0, 2, 3)).cpu().numpy())
