"""GPU parity of the fused chain backward (hg_pipeline_r2h_conv_h2r_backward) against the fp64
oracle composition

    u = rect_to_hex(x);  gz = hex_to_rect_backward(gy)
    (du, dk, db) = hexconv2d_backward(u, k, gz);  dx = rect_to_hex_backward(du)

Inputs x, gy ~ U[0, 1): every entry of dK is then within 20 % of the largest, so the relative
tolerance tests every weight.  Tolerances: the project's gradient tolerance
(tests/test_gpu_backward.py: rtol 1e-4, atol 1e-5 max|ref|); a 16-bit dx within one rounding of
its dtype (tests/test_gpu_pipeline.py::one_rounding: 2^-8 |ref| + 1e-5 max|ref| per element)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402
from HyGrid.HexFrames import HexConv2d  # noqa: E402
from HyGrid.pipeline import rect_hex_conv_rect  # noqa: E402

DEV = torch.device("cuda:0")
TR, TC, BAND = _abi.fused_layout(9)   # tile rows, tile columns, tiles per weight-pass band


def grad_close(got, ref, what):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    atol = 1e-5 * max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref)
    print(f"{what}: max err {err.max():.3e}, max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=atol, err_msg=what)


def one_rounding(got, ref, what, ulp=2.0 ** -8):
    got = np.asarray(got, np.float64)
    tol = ulp * np.abs(ref) + 1e-5 * np.abs(ref).max()
    bad = np.abs(got - ref) > tol
    print(f"{what}: max err {np.abs(got - ref).max():.3e}, max|ref| {np.abs(ref).max():.3e}")
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} beyond one rounding of the "
                           f"oracle (worst excess {float((np.abs(got - ref) - tol).max()):.3e})")


def oracle_backward(x, k, gy, off, groups, pad=1, hex_size=None):
    """fp64 (dx, dk, db) of the chain for numpy x, k, gy."""
    H, W = x.shape[-2:]
    hs = hex_size or (H, W)
    u = O.rect_to_hex(x, hs)
    ho, wo = O.hexconv2d_out_shape(hs[0], hs[1], 2, 1, pad, 1)
    gz = O.hex_to_rect_backward(gy, (ho, wo))
    du, dk, db = O.hexconv2d_backward(u, k, gz, off, 2, padding=pad, groups=groups)
    return O.rect_to_hex_backward(du, (H, W)), dk, db


@functools.lru_cache(maxsize=None)
def case_data(B, C, H, W, off, groups, x_dt=torch.float32, gy_dt=torch.float32):
    """Seeded inputs (rounded to their dtypes), the conv and the oracle's gradients; shared by
    the tests of one shape and left unchanged."""
    torch.manual_seed(11)
    conv = HexConv2d(C, C, off, 2, padding=1, groups=groups, bias=True).to(DEV)
    g = torch.Generator().manual_seed(1000 * H + W)
    x = torch.rand((B, C, H, W), generator=g).to(x_dt)
    gy = torch.rand((B, C, H, W), generator=g).to(gy_dt)
    ref = oracle_backward(x.double().numpy(), conv.kernel.detach().double().cpu().numpy(),
                          gy.double().numpy(), off, groups)
    return conv, x.to(DEV), gy.to(DEV), ref


def fused_backward(conv, x, gy, **kw):
    out = ops.pipeline_r2h_conv_h2r_backward(gy, x, conv.kernel, None, None, conv.pad, conv.groups,
                                             int(conv.even_odd_offset),
                                             float(conv.padding_value), **kw)
    assert out is not None, "the fused backward should cover this call"
    return out


FP32_CASES = [
    (2, 3, 9, 8, 0, 1),                              # smaller than a tile
    (1, 3, 37, 54, 1, 1),
    (2, 3, 20, 34, 0, 3),                            # depthwise
    (2, 1, 33, 70, 1, 1),
    (1, 3, 3 * TR + 5, 3 * TC + 11, 0, 1),           # > 3 x 3 tiles, odd width
    (1, 3, TR * BAND + 2 * TR + 3, 3 * TC + 10, 1, 1),   # two weight-pass bands
]


@pytest.mark.parametrize("case", FP32_CASES)
def test_fp32_vs_oracle(case):
    conv, x, gy, (rdx, rdk, rdb) = case_data(*case)
    dx, dk, db = fused_backward(conv, x, gy)
    assert dx.dtype == torch.float32 and dk.dtype == torch.float32 and db.dtype == torch.float32
    grad_close(dk.cpu().numpy(), rdk, "dk")
    grad_close(db.cpu().numpy(), rdb, "db")
    grad_close(dx.cpu().numpy(), rdx, "dx")          # per element, edges included


@pytest.mark.parametrize("x_dt, gy_dt", [(torch.bfloat16, torch.bfloat16),
                                         (torch.bfloat16, torch.float32),
                                         (torch.float16, torch.float16),
                                         (torch.float32, torch.bfloat16)])
def test_dtypes(x_dt, gy_dt):
    conv, x, gy, (rdx, rdk, rdb) = case_data(2, 3, 40, 66, 0, 1, x_dt, gy_dt)
    dx, dk, db = fused_backward(conv, x, gy)
    assert dx.dtype == x_dt and dk.dtype == torch.float32 and db.dtype == torch.float32
    grad_close(dk.cpu().numpy(), rdk, "dk")
    grad_close(db.cpu().numpy(), rdb, "db")
    if x_dt == torch.float32:
        grad_close(dx.cpu().numpy(), rdx, "dx")
    else:
        # bf16: 2^-8 as in test_gpu_pipeline.py (twice the half-ulp bound 2^-9); f16 alike: 2^-10
        one_rounding(dx.double().cpu().numpy(), rdx, "dx",
                     ulp=2.0 ** -8 if x_dt == torch.bfloat16 else 2.0 ** -10)


def test_requested_gradients_only():
    conv, x, gy, _ = case_data(1, 3, 37, 54, 1, 1)
    dx, dk, db = fused_backward(conv, x, gy)
    dx2, dk2, db2 = fused_backward(conv, x, gy, need_x=False)
    assert dx is not None and dx2 is None
    assert torch.equal(dk, dk2) and torch.equal(db, db2)
    dx3, dk3, db3 = fused_backward(conv, x, gy, need_k=False, need_b=False)
    assert dk3 is None and db3 is None and torch.equal(dx3, dx)
    # a conv without a bias: autograd asks for no d bias
    torch.manual_seed(5)
    nb = HexConv2d(3, 3, 1, 2, padding=1, bias=False).to(DEV).train()
    assert nb.bias is None
    y = rect_hex_conv_rect(x, nb)
    assert type(y.grad_fn).__name__.startswith("_FusedChainFn")
    y.backward(gy)
    _, rdk, _ = oracle_backward(x.double().cpu().numpy(), nb.kernel.detach().double().cpu().numpy(),
                                gy.double().cpu().numpy(), 1, 1)
    grad_close(nb.kernel.grad.cpu().numpy(), rdk, "dk (no bias)")
    _, _, db4 = fused_backward(nb, x, gy, need_b=False)
    assert db4 is None


def test_reproducible_bitwise():
    conv, x, gy, _ = case_data(1, 3, 3 * TR + 5, 3 * TC + 11, 0, 1)
    a = fused_backward(conv, x, gy)
    b = fused_backward(conv, x, gy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("x_grad", [False, True])
def test_autograd(monkeypatch, x_grad):
    conv, x, gy, (rdx, rdk, rdb) = case_data(2, 3, 40, 66, 0, 1)
    conv.train()
    calls = []
    real = ops.rect_to_hex
    monkeypatch.setattr(ops, "rect_to_hex", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    conv.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(x_grad)
    y = rect_hex_conv_rect(xx, conv)
    assert type(y.grad_fn).__name__.startswith("_FusedChainFn")
    assert not calls, "the operator chain ran"
    with torch.no_grad():
        y0 = rect_hex_conv_rect(x, conv)
    assert torch.equal(y.detach(), y0)
    y.backward(gy)
    assert not calls
    gk, gb = conv.kernel.grad.clone(), conv.bias.grad.clone()
    assert gk.shape == conv.kernel.shape and gk.dtype == conv.kernel.dtype
    grad_close(gk.cpu().numpy(), rdk, "kernel.grad")
    grad_close(gb.cpu().numpy(), rdb, "bias.grad")
    if x_grad:
        grad_close(xx.grad.cpu().numpy(), rdx, "x.grad")
    else:
        assert xx.grad is None
    # the operator chain's autograd (fused=False), same tolerance
    conv.zero_grad(set_to_none=True)
    x2 = x.clone().requires_grad_(x_grad)
    y2 = rect_hex_conv_rect(x2, conv, fused=False)
    assert calls, "fused=False keeps the operator chain"
    y2.backward(gy)
    grad_close(gk.cpu().numpy(), conv.kernel.grad.double().cpu().numpy(), "kernel.grad vs operators")
    grad_close(gb.cpu().numpy(), conv.bias.grad.double().cpu().numpy(), "bias.grad vs operators")
    if x_grad:
        grad_close(xx.grad.cpu().numpy(), x2.grad.double().cpu().numpy(), "x.grad vs operators")
    conv.zero_grad(set_to_none=True)


@pytest.mark.parametrize("pad, hex_size, shape", [(0, None, (1, 3, 24, 40)),
                                                  (1, (71, 131), (1, 3, 70, 130))])
def test_fallback_through_the_operators(pad, hex_size, shape):
    """Outside the fused backward's domain autograd still runs, through the three operators."""
    torch.manual_seed(7)
    conv = HexConv2d(3, 3, 0, 2, padding=pad, bias=True).to(DEV).train()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(shape, generator=g)
    H, W = shape[-2:]
    hs = hex_size or (H, W)
    ho, wo = O.hexconv2d_out_shape(hs[0], hs[1], 2, 1, pad, 1)
    rect = (H, W) if hex_size else None
    xx = x.to(DEV).requires_grad_(True)
    y = rect_hex_conv_rect(xx, conv, hex_size=hex_size, rect_size=rect)
    assert not type(y.grad_fn).__name__.startswith("_FusedChainFn")
    gy = torch.rand(tuple(y.shape), generator=g)
    y.backward(gy.to(DEV))
    k = conv.kernel.detach().double().cpu().numpy()
    u = O.rect_to_hex(x.double().numpy(), hs)
    gz = O.hex_to_rect_backward(gy.double().numpy(), (ho, wo))
    du, rdk, rdb = O.hexconv2d_backward(u, k, gz, 0, 2, padding=pad)
    rdx = O.rect_to_hex_backward(du, (H, W))
    grad_close(conv.kernel.grad.cpu().numpy(), rdk, "kernel.grad")
    grad_close(conv.bias.grad.cpu().numpy(), rdb, "bias.grad")
    grad_close(xx.grad.cpu().numpy(), rdx, "x.grad")


def test_one_real_size_bf16():
    """(1, 3, 1080, 1920) bf16: dk / db against the oracle, dx on 8 seeded rows."""
    conv, x, gy, (rdx, rdk, rdb) = case_data(1, 3, 1080, 1920, 0, 1, torch.bfloat16, torch.bfloat16)
    dx, dk, db = fused_backward(conv, x, gy)
    grad_close(dk.cpu().numpy(), rdk, "dk")
    grad_close(db.cpu().numpy(), rdb, "db")
    rows = np.sort(np.random.default_rng(4).choice(1080, 8, replace=False))
    one_rounding(dx[:, :, rows].double().cpu().numpy(), rdx[:, :, rows], "dx rows")
