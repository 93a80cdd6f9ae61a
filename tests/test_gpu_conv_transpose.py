"""GPU parity of HexConvTranspose2d (csrc/conv_transpose_mfma.hip, k_hexconvt_s2): the stride-2
transposed hex convolution on the f32 matrix cores, against the fp64 oracle's adjoint
(y - bias = hexconv2d_backward's d input of the adjoint conv for gy = x) and against the layer's
other route (HYGRID_CONVT_MFMA=0: the generic gather + bias add).

Tolerances are those of tests/test_gpu_backward.py: fp32 sums in another order than the oracle's
-> rtol 1e-4, atol 1e-5 * max|ref|; a 16-bit output is one rounding of the fp32 sum (2^-8 bf16,
2^-11 f16, relative to max|ref|).  The sums have at most 2 * in_channels terms.  Every case first
asserts its route through the plan.  Shapes (tests/conv_transpose_cases.py) are the smallest that
reach each path: all four valid output sizes of every input, rows that are no multiple of 4,
output widths inside one 128-column tile and crossing one (130 / 131) and two (258 / 259), even
widths (paired stores) and odd ones (scalar stores), partial K chunks and partial M tiles.
The guard-arena tests come first."""
import os

import numpy as np
import pytest
import torch

import conv_transpose_cases as CT
import placement as PL
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402
from HyGrid.HexFrames import HexConv2d, HexConvTranspose2d  # noqa: E402

DEV = torch.device("cuda:0")
ADJ, MFMA = _abi.HG_CONVT_ADJOINT, _abi.HG_CONVT_MFMA_S2
SWITCH = "HYGRID_CONVT_MFMA"
CASES = CT.gpu_cases()
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


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


def _plan(case, x_dtype=torch.float32, y_dtype=torch.float32):
    B, ci, co, hin, win, p, h, w, off = case
    return ops.hexconv_transpose2d_plan(x_dtype, torch.float32, y_dtype, B, ci, co, hin, win, h, w,
                                        2, 2, p, 1, 1, off)


def _run(case, x, k, b, out_dtype=torch.float32):
    B, ci, co, hin, win, p, h, w, off = case
    y = ops.hexconv_transpose2d(x, k, b, off, 2, 2, p, 1, 1, (h, w), out_dtype)
    assert y.shape == (B, co, h, w) and y.dtype == out_dtype
    return y


def _dev(case, x_dtype="float32"):
    (x, k, b), ref = CT.data(case, x_dtype)
    x = torch.from_numpy(x).to(getattr(torch, x_dtype)).to(DEV)
    return x, torch.from_numpy(k).to(DEV), torch.from_numpy(b).to(DEV), ref


def _close(got, ref, rtol=1e-4, atol_rel=None):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    m = max(np.abs(ref).max(), 1e-30)
    print("max abs err", np.abs(got - ref).max(), "max|ref|", m)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=(rtol * 0.1 if atol_rel is None else atol_rel) * m)


def _with_bias(ref, b):
    return ref + np.asarray(b, np.float64).reshape(1, -1, 1, 1)


# ---- guard arenas (first) -------------------------------------------------------------------------
GUARD = [c for c in CASES if (c[3], c[4]) in ((17, 35), (3, 33), (1, 2))][::3]


@pytest.mark.parametrize("case", GUARD, ids=str)
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("off_out", [0, 1])
@pytest.mark.parametrize("off_in", [0, 1])
def test_placement_inside_guard_arenas(monkeypatch, case, out_dtype, off_out, off_in):
    """x placed at element offset 0 / 1 between NaN guards, y allocated inside a sentinel arena at
    offset 0 / 1 (offset 1 takes y off its pair alignment: the scalar stores), for every output
    dtype.  No guard byte changes, every element of y is written (the untapped ones too), and no
    guard NaN reaches y."""
    monkeypatch.delenv(SWITCH, raising=False)
    x, k, b, ref = _dev(case)
    xv, xa = PL.place(x, DEV, off_in)
    assert _plan(case, x.dtype, out_dtype) == MFMA
    with PL.placed(monkeypatch, off_out) as rec:
        y = _run(case, xv, k, b, out_dtype)
    assert len(rec.arenas) == 1 and rec.arena_of(y) is not None
    PL.guards_intact(xa, xv, "x ")
    assert PL.sentinel_count(y) == 0
    assert bool(torch.isfinite(y).all())
    ulp = ULP.get(out_dtype)
    if ulp is None:
        _close(y, _with_bias(ref, b.cpu()))
    else:
        _close(y, _with_bias(ref, b.cpu()), rtol=ulp, atol_rel=ulp)


def test_guard_cases_cover_both_store_paths():
    assert {c[7] % 2 for c in GUARD} == {0, 1} and len(GUARD) >= 4


# ---- against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
def test_vs_oracle(case, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    x, k, b, ref = _dev(case)
    assert _plan(case) == MFMA
    _close(_run(case, x, k, b), _with_bias(ref, b.cpu()))
    _close(_run(case, x, k, None), ref)


@pytest.mark.parametrize("case", CASES[3::5], ids=str)
@pytest.mark.parametrize("xdt", ["bfloat16", "float16"])
def test_16bit_inputs_and_outputs(case, xdt, monkeypatch):
    """The oracle gets x's exact values; a 16-bit y is one rounding of the fp32 sum."""
    monkeypatch.delenv(SWITCH, raising=False)
    x, k, b, ref = _dev(case, xdt)
    assert x.dtype == getattr(torch, xdt)
    want = _with_bias(ref, b.cpu())
    for ydt in (torch.float32, torch.bfloat16, torch.float16):
        assert _plan(case, x.dtype, ydt) == MFMA
        y = _run(case, x, k, b, ydt)
        if ydt == torch.float32:
            _close(y, want)
        else:
            _close(y, want, rtol=ULP[ydt], atol_rel=ULP[ydt])


@pytest.mark.parametrize("case", CASES[::4], ids=str)
def test_agrees_with_adjoint_route(case, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    x, k, b, ref = _dev(case)
    assert _plan(case) == MFMA and _with_env(SWITCH, "0", _plan, case) == ADJ
    got = _run(case, x, k, b)
    other = _with_env(SWITCH, "0", _run, case, x, k, b)
    _close(other, _with_bias(ref, b.cpu()))
    print("max abs diff", float((got - other).abs().max()))
    torch.testing.assert_close(got, other, rtol=1e-4, atol=1e-5 * float(other.abs().max()))


def test_adjoint_route_outside_the_domain_and_dtypes(monkeypatch):
    """out_channels 15 and stride 1 take the adjoint route (stride 1: the MFMA d input); bf16 x
    and a bf16 result are converted around it."""
    monkeypatch.delenv(SWITCH, raising=False)
    g = torch.Generator().manual_seed(5)
    for (ci, co, s, hin, win, p, off) in [(20, 15, 2, 9, 11, 1, 1), (16, 24, 1, 12, 30, 1, 0),
                                          (6, 4, 3, 5, 7, 0, 1)]:
        h, w = ops.hexconv_transpose2d_out_shape(hin, win, 2, s, p, 1)
        x = (torch.rand((2, ci, hin, win), generator=g) - 0.5).bfloat16()
        k = (torch.rand((ci, co, 1, 7), generator=g) - 0.5) / 4
        b = torch.rand((co,), generator=g) - 0.5
        assert ops.hexconv_transpose2d_plan(x.dtype, k.dtype, torch.bfloat16, 2, ci, co, hin, win,
                                            h, w, 2, s, p, 1, 1, off) == ADJ
        ref = CT.oracle_adjoint(x.double().numpy(), k.double().numpy(), h, w, off, p, 2, s)
        ref = _with_bias(ref, b)
        y = ops.hexconv_transpose2d(x.to(DEV), k.to(DEV), b.to(DEV), off, 2, s, p, 1, 1, None,
                                    torch.float32)
        _close(y, ref)
        y = ops.hexconv_transpose2d(x.to(DEV), k.to(DEV), b.to(DEV), off, 2, s, p, 1, 1, None,
                                    torch.bfloat16)
        assert y.dtype == torch.bfloat16
        _close(y, ref, rtol=2.0 ** -8, atol_rel=2.0 ** -8)


def test_bit_identical_runs(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    for case in (CASES[17], CASES[30]):
        x, k, b, _ = _dev(case)
        assert _plan(case) == MFMA
        a = _run(case, x, k, b)
        c = _run(case, x, k, b)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("off", [0, 1])
def test_nonfinite_x_positions_match_adjoint_route(off, monkeypatch):
    """NaN / +-Inf in x on a shape with h % 4 != 0 and w % 64 != 0, including x's last row and
    column and a tile's last column: a zero-weight shortcut for absent taps (0 * Inf = NaN) or an
    unmasked edge operand would move the masks."""
    monkeypatch.delenv(SWITCH, raising=False)
    case = (1, 16, 16, 17, 65, 1, 33, 131, off)
    x, k, b, _ = _dev(case)
    x = x.clone()
    x[0, 0, 0, 0] = float("nan")
    x[0, 1, :, -1] = float("inf")
    x[0, 2, -1, :] = float("-inf")
    x[0, 5, -1, -1] = float("inf")
    x[0, 7, 8, 63] = float("inf")
    x[0, 9, 9, 64] = float("-inf")
    x[0, 11, 3, 31] = float("nan")
    assert _plan(case) == MFMA
    y = _run(case, x, k, b)
    r = _with_env(SWITCH, "0", _run, case, x, k, b)
    assert torch.equal(torch.isnan(y), torch.isnan(r))
    assert torch.equal(torch.isinf(y), torch.isinf(r))
    assert torch.equal(y[torch.isinf(r)], r[torch.isinf(r)])
    fin = torch.isfinite(r)
    assert int((~fin).sum()) > 0 and int(fin.sum()) >= 16 * 17
    torch.testing.assert_close(y[fin], r[fin], rtol=1e-4, atol=1e-5 * float(r[fin].abs().max()))


@pytest.mark.parametrize("case", [CASES[18], CASES[27], CASES[41]], ids=str)
def test_adjoint_identity_with_the_stride2_forward(case, monkeypatch):
    """<conv(u), x> = <u, convT(x) - bias> with the library's own stride-2 forward."""
    monkeypatch.delenv(SWITCH, raising=False)
    B, ci, co, hin, win, p, h, w, off = case
    x, k, b, _ = _dev(case)
    u = torch.randn((B, co, h, w), generator=torch.Generator().manual_seed(3)).to(DEV)
    assert _plan(case) == MFMA
    cu = ops.hexconv2d(u, k, None, off, 2, 2, p, out_dtype=torch.float32)
    assert cu.shape == x.shape
    yt = _run(case, x, k, b) - b.view(1, -1, 1, 1)
    lhs = float((cu.double() * x.double()).sum())
    rhs = float((u.double() * yt.double()).sum())
    print("lhs", lhs, "rhs", rhs)
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs)


# ---- autograd ---------------------------------------------------------------------------------------
def _oracle_grads(x, kernel, gy, off, p):
    """d x = the adjoint conv of gy; d kernel = its d kernel with the roles swapped; d bias."""
    xn, kn, gn = (t.detach().double().cpu().numpy() for t in (x, kernel, gy))
    dx = O.hexconv2d(gn, kn, None, off, 2, 2, p)
    dk = O.hexconv2d_backward(gn, kn, xn, off, 2, 2, p)[1]
    return dx, dk, gn.sum((0, 2, 3))


def test_autograd_layer_end_to_end(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    torch.manual_seed(7)
    m = HexConvTranspose2d(16, 32, 1, 2, stride=2, padding=1).to(DEV)
    x = torch.rand((2, 16, 9, 21), device=DEV, requires_grad=True)
    assert ops.hexconv_transpose2d_plan(x.dtype, m.kernel.dtype, torch.float32, 2, 16, 32, 9, 21,
                                        18, 42, 2, 2, 1) == MFMA
    y = m(x)
    assert y.shape == (2, 32, 18, 42)
    gy = torch.randn_like(y)
    y.backward(gy)
    dx, dk, db = _oracle_grads(x, m.kernel, gy, 1, 1)
    _close(x.grad, dx)
    _close(m.kernel.grad, dk)
    _close(m.bias.grad, db)


def test_autograd_hexconvmodule_end_to_end(monkeypatch):
    """The layer inside a HexConvModule with training BatchNorm + ReLU (the unfused path)."""
    monkeypatch.delenv(SWITCH, raising=False)
    from HyGrid.HexModules import HexConvModule
    torch.manual_seed(3)
    m = HexConvModule(16, 32, 0, 2, stride=2, padding=1, bias=True, norm_cfg=dict(type="BN"),
                      act_cfg=dict(type="ReLU"), conv_cfg=dict(type="HexConvTranspose2d")).to(DEV)
    m.train()
    x = torch.rand((2, 16, 9, 21), device=DEV, requires_grad=True)
    assert m._epilogue_plan(x, True, True) is None
    seen = {}

    def keep(mod, inp, out):
        out.retain_grad()
        seen["y"] = out

    hook = m.conv.register_forward_hook(keep)
    z = m(x)
    hook.remove()
    assert z.shape == (2, 32, 18, 42) and bool((z >= 0).all())
    z.backward(torch.randn_like(z))
    gy = seen["y"].grad
    assert gy is not None and float(gy.abs().max()) > 0
    dx, dk, db = _oracle_grads(x, m.conv.kernel, gy, 0, 1)
    _close(x.grad, dx)
    _close(m.conv.kernel.grad, dk)
    # Training BatchNorm removes each channel's mean, so d bias is 0 in exact arithmetic: the
    # oracle's value is its own fp64 rounding (~1e-5 here) and max|ref| says nothing about the
    # size of the 2 * 18 * 42 terms that cancel.  The fp32 sum's error scales with sum |gy|
    # per channel, so that is what the 1e-5 is taken relative to.
    terms = float(gy.detach().abs().sum((0, 2, 3)).max())
    got = m.conv.bias.grad.double().cpu().numpy()
    print("d bias: max abs err", np.abs(got - db).max(), "max sum|gy|", terms)
    np.testing.assert_allclose(got, db, rtol=1e-4, atol=1e-5 * terms)


def test_encoder_decoder_round_trip(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    torch.manual_seed(1)
    down = HexConv2d(16, 32, 0, 2, stride=2, padding=1).to(DEV)
    up = HexConvTranspose2d(32, 16, 0, 2, stride=2, padding=1).to(DEV)
    with torch.no_grad():
        x = torch.rand((1, 16, 34, 70), device=DEV)
        assert up(down(x)).shape == x.shape
        x = torch.rand((1, 16, 33, 71), device=DEV)
        mid = down(x)
        assert up(mid).shape == (1, 16, 34, 70)
        assert up(mid, output_size=x.shape).shape == x.shape
        with pytest.raises(ValueError):
            up(mid, output_size=(32, 71))
