"""GPU parity of the stride-2 wide-channel HexConv2d kernels (csrc/conv_mfma.hip:
k_hexconv_mfma_s2 on v_mfma_f32_16x16x4_f32 and k_hexconv_mfma_bf16_s2, the register-staged
three-part weight split on v_mfma_f32_16x16x32_bf16; dense radius 2, dilation 1, O >= 16) against
the fp64 oracle at the north-star fp32 tolerance (rtol 1e-5, atol 1e-5 * max|ref|: the contraction
length 7 C is the stride-1 layer's) and against the generic kernel (HYGRID_CONV_MFMA=0) for 16-bit
outputs and the fused HexConvModule epilogue.

Every test first asserts through ops.hexconv2d_forward_plan that its layer runs the kernel it
names.  Shapes: the smallest legal layer (3 x 6 -> 1 x 2), rows that are no multiple of the 4-row
tile, one / two / three 64-column tiles with second tiles of 1 or 2 columns, channel counts that are
no multiple of the chunk (1, 3, 5, 13, 70) or of the 16-channel tile (20, 33, 40, 100), O <= 32 (two
tiles per workgroup) and O > 32 (four).  The tile's index arithmetic is checked on the host by
tests/test_conv_mfma_stride2_index_cpu.py."""
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
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
OTHER, MF32, MBF, MDMA = (_abi.HG_CONV_FWD_OTHER, _abi.HG_CONV_FWD_MFMA_F32,
                          _abi.HG_CONV_FWD_MFMA_BF16, _abi.HG_CONV_FWD_MFMA_BF16_DMA)
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 1e-5}

CASES = [  # (B, C, O, h, w)
    (1, 16, 16, 3, 6), (2, 8, 16, 9, 10), (1, 16, 16, 33, 70), (1, 32, 64, 20, 140),
    (1, 13, 20, 12, 21), (1, 24, 100, 11, 75), (1, 70, 33, 6, 9), (2, 3, 64, 21, 131),
    (1, 1, 16, 9, 10), (1, 5, 40, 14, 33), (1, 16, 32, 19, 264)]
# (ho, wo) at pad 0 / 1 / 2, from the CPU oracle
OUT_SHAPES = {(3, 6): ((1, 2), (2, 3), (3, 4)), (9, 10): ((4, 4), (5, 5), (6, 6)),
              (33, 70): ((16, 34), (17, 35), (18, 36)), (20, 140): ((9, 69), (10, 70), (11, 71)),
              (21, 131): ((10, 64), (11, 65), (12, 66))}


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


def _generic(fn, *args, **kw):
    return _with_env("HYGRID_CONV_MFMA", "0", fn, *args, **kw)


def _weights(O_, C, seed):
    """As tests/test_gpu_conv_mfma.py::_weights."""
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / np.sqrt(7 * C)
    k = ((torch.rand((O_, C, 1, 7), generator=g) * 2 - 1) * bound).to(DEV)
    b = ((torch.rand((O_,), generator=g) * 2 - 1) * bound).to(DEV)
    return k, b


def _bf16_input(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(shape, generator=g, device=DEV) - 0.5).to(BF16)


def _plan(x, k, out_dtype, pad, off=0, mode="constant", pv=0.0):
    B, C, h, w = x.shape
    return ops.hexconv2d_forward_plan(x.dtype, k.dtype, out_dtype, B, C, k.shape[0], h, w, 2,
                                      stride=2, padding=pad, even_odd_offset=off,
                                      padding_mode=mode, padding_value=pv)


def _oracle(x, k, b, off, pad, mode="constant", pv=0.0):
    return O.hexconv2d(x.double().cpu().numpy(), k.cpu().double().numpy(),
                       b.cpu().double().numpy(), off, 2, stride=2, padding=pad,
                       padding_mode=mode, padding_value=pv)


def _close_to_oracle(y, ref):
    y = y.cpu().numpy()
    scale = max(np.abs(ref).max(), 1e-30)
    print("max abs err", np.abs(y - ref).max(), "max|ref|", scale)
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, rtol=1e-5, atol=1e-5 * scale)


def test_table_out_shapes():
    for (h, w), shapes in OUT_SHAPES.items():
        for pad, want in enumerate(shapes):
            assert ops.hexconv2d_out_shape(h, w, 2, 2, pad, 1) == want
    assert [ops.hexconv2d_out_shape(19, 264, 2, 2, p, 1)[1] for p in (0, 1, 2)] == [131, 132, 133]
    assert ops.hexconv2d_out_shape(30, 74, 2, 2, 0, 1)[1] == 36
    assert ops.hexconv2d_out_shape(30, 74, 2, 2, 1, 1)[1] == 37


# ---- guard bands (run before any other GPU run of new kernels) ------------------------------

@pytest.mark.parametrize("dt,nbytes", [(F32, 4), (F32, 8), (F32, 16),
                                       (BF16, 2), (BF16, 4), (BF16, 8), (BF16, 16)])
@pytest.mark.parametrize("case,pad", [((1, 32, 64, 20, 140), 1), ((2, 3, 64, 21, 131), 0)])
def test_guard_bands(monkeypatch, case, pad, dt, nbytes):
    """x, kernel and bias inside NaN-guarded arenas, y allocated inside a sentinel arena whose
    view starts 2 (16-bit only) / 4 / 8 / 16 bytes past a 256-B boundary: no guard byte changes,
    the sources keep their bits, every output element is written, and the output is bit-identical
    to the run on fresh tensors (no guard NaN reaches a sum, the store path does not depend on
    the base alignment)."""
    es = torch.empty((), dtype=dt).element_size()
    B, C, O_, h, w = case
    k, b = _weights(O_, C, h + w)
    g = torch.Generator(device=DEV).manual_seed(w + pad)
    x = (torch.rand((B, C, h, w), generator=g, device=DEV) - 0.5).to(dt)
    assert _plan(x, k, dt, pad) == (MF32 if dt == F32 else MBF)
    fresh = ops.hexconv2d(x, k, b, 0, 2, stride=2, padding=pad, out_dtype=dt)
    torch.cuda.synchronize()
    xv, xa = PL.place(x, DEV, nbytes // es)
    kv, ka = PL.place(k, DEV, 1)
    bv, ba = PL.place(b, DEV, 1)
    with PL.placed(monkeypatch, nbytes // es) as rec:
        y = ops.hexconv2d(xv, kv, bv, 0, 2, stride=2, padding=pad, out_dtype=dt)
    assert len(rec.arenas) == 1 and rec.arena_of(y) is not None
    assert (y.data_ptr() % 256) == nbytes
    for a, v, t, what in ((xa, xv, x, "x "), (ka, kv, k, "kernel "), (ba, bv, b, "bias ")):
        PL.guards_intact(a, v, what)
        assert torch.equal(v.view(torch.int16 if es == 2 and what == "x " else torch.int32),
                           t.view(torch.int16 if es == 2 and what == "x " else torch.int32))
    assert PL.sentinel_count(y) == 0
    it = torch.int16 if es == 2 else torch.int32
    assert torch.equal(y.view(it), fresh.view(it))


# ---- parity against the fp64 oracle -----------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_s2_fp32_vs_oracle(case, pad, off):
    B, C, O_, h, w = case
    k, b = _weights(O_, C, h * 13 + w + pad)
    rng = np.random.default_rng(h + w * 3 + off)
    x = torch.from_numpy(rng.random((B, C, h, w)).astype(np.float32) - 0.5).to(DEV)
    assert _plan(x, k, F32, pad, off) == MF32
    y = ops.hexconv2d(x, k, b, off, 2, stride=2, padding=pad, out_dtype=F32)
    _close_to_oracle(y, _oracle(x, k, b, off, pad))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_s2_bf16_vs_oracle(case, pad, off):
    """bf16 input (exact in fp64), fp32 output, on the split-weight kernel."""
    B, C, O_, h, w = case
    k, b = _weights(O_, C, h * 13 + w + pad)
    x = _bf16_input((B, C, h, w), h + w * 3 + off)
    assert _plan(x, k, F32, pad, off) == MBF
    y = ops.hexconv2d(x, k, b, off, 2, stride=2, padding=pad, out_dtype=F32)
    _close_to_oracle(y, _oracle(x, k, b, off, pad))


@functools.lru_cache(maxsize=None)
def _pad_mode_data(dt):
    B, C, O_, h, w = 1, 16, 32, 14, 40
    k, b = _weights(O_, C, 7)
    if dt == BF16:
        x = _bf16_input((B, C, h, w), 5)
    else:
        x = torch.from_numpy(np.random.default_rng(5).random((B, C, h, w)).astype(np.float32)).to(DEV)
    return x, k, b


@pytest.mark.parametrize("mode,pv", [("constant", 0.3), ("constant", 0.5), ("reflect", 0.0),
                                     ("replicate", 0.0), ("circular", 0.0)])
@pytest.mark.parametrize("pad", [1, 2])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_s2_pad_modes_vs_oracle(dt, pad, mode, pv):
    """Every padding mode on both kernels; a pad value that is no bf16 (0.3) sends a bf16 input
    to the f32 kernel, and the plan says so; 0.5 stays on the bf16 kernel."""
    x, k, b = _pad_mode_data(dt)
    want = MF32 if (dt == F32 or pv == 0.3) else MBF
    assert _plan(x, k, F32, pad, 0, mode, pv) == want
    y = ops.hexconv2d(x, k, b, 0, 2, stride=2, padding=pad, padding_mode=mode, padding_value=pv,
                      out_dtype=F32)
    _close_to_oracle(y, _oracle(x, k, b, 0, pad, mode, pv))


# ---- 16-bit outputs and the fused epilogue against the generic kernel ---------------------

@pytest.mark.parametrize("dt_in,dt_out", [(BF16, BF16), (BF16, F32), (F16, F16), (F32, BF16)])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("with_epi", [False, True])
def test_s2_16bit_vs_generic(dt_in, dt_out, pad, with_epi):
    """wo = 36 (pad 0: the 8-byte column stores of 16-bit outputs) and 37 (pad 1: their scalar
    stores), plain and with the BN-affine + LeakyReLU epilogue, within one unit of the output
    dtype of the generic kernel."""
    B, C, O_, h, w = 2, 32, 48, 30, 74
    k, b = _weights(O_, C, 3)
    g = torch.Generator(device=DEV).manual_seed(9)
    x = (torch.rand((B, C, h, w), generator=g, device=DEV) - 0.5).to(dt_in)
    epi = None
    if with_epi:
        scale = torch.rand((O_,), generator=g, device=DEV) + 0.5
        shift = torch.rand((O_,), generator=g, device=DEV) - 0.5
        epi = (scale, shift, 2, 0.1)          # hg_act 2: LeakyReLU
    assert _plan(x, k, dt_out, pad) == (MBF if dt_in == BF16 else MF32)
    y = ops.hexconv2d(x, k, b, 0, 2, stride=2, padding=pad, out_dtype=dt_out, epilogue=epi)
    ref = _generic(ops.hexconv2d, x, k, b, 0, 2, stride=2, padding=pad, out_dtype=dt_out,
                   epilogue=epi)
    assert y.shape == ref.shape and y.shape[-1] == 36 + pad
    sc = float(ref.float().abs().max())
    torch.testing.assert_close(y.float(), ref.float(), rtol=ULP[dt_out], atol=ULP[dt_out] * sc)


@pytest.mark.parametrize("act", ["ReLU", "LeakyReLU", "Sigmoid"])
def test_s2_hexconvmodule_epilogue_vs_generic(act):
    """HexConvModule's fused conv + eval BatchNorm + activation on the stride-2 kernel."""
    from HyGrid.HexModules import HexConvModule
    torch.manual_seed(2)
    m = HexConvModule(16, 32, 0, 2, stride=2, padding=1, norm_cfg=dict(type="BN"),
                      act_cfg=dict(type=act)).to(DEV).eval()
    assert ops.hexconv2d_forward_plan(F32, F32, F32, 2, 16, 32, 24, 50, 2, stride=2,
                                      padding=1) == MF32
    with torch.no_grad():
        m.norm.running_mean.uniform_(-0.2, 0.2)
        m.norm.running_var.uniform_(0.5, 1.5)
        x = torch.rand((2, 16, 24, 50), device=DEV)
        y = m(x)
        ref = _generic(m, x)
    assert y.shape == (2, 32) + ops.hexconv2d_out_shape(24, 50, 2, 2, 1, 1)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))


# ---- non-finite inputs --------------------------------------------------------------------------

NF_CASE, NF_PAD, NF_OFF = (1, 16, 16, 20, 70), 0, 0
NF_POS = [(3, 0, 0, float("nan")), (7, 19, 69, float("inf")), (9, 10, 30, float("-inf"))]


def _plant(x):
    for c, i, j, v in NF_POS:
        x[0, c, i, j] = v
    return x


def test_s2_some_planted_positions_are_never_read():
    """At stride 2 some input samples are read by no tap: of the three planted positions (a
    corner, the last row and column, an interior sample) the oracle reads at least one and skips
    at least one, so the tests below check both that a non-finite value spreads exactly as far as
    in the generic kernel and that an unread one reaches no output."""
    _, _, _, h, w = NF_CASE
    read = []
    for _, i, j, _ in NF_POS:
        x = np.zeros((1, 1, h, w))
        x[0, 0, i, j] = np.nan
        y = O.hexconv2d(x, np.ones((1, 1, 1, 7)), np.zeros(1), NF_OFF, 2, stride=2, padding=NF_PAD)
        read.append(bool(np.isnan(y).any()))
    assert any(read) and not all(read), read


def test_s2_nonfinite_positions_match_generic_f32():
    B, C, O_, h, w = NF_CASE
    k, b = _weights(O_, C, 4)
    x = _plant(torch.rand((B, C, h, w), device=DEV))
    assert _plan(x, k, F32, NF_PAD, NF_OFF) == MF32
    y = ops.hexconv2d(x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    ref = _generic(ops.hexconv2d, x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    assert bool(torch.isnan(ref).any()) or bool(torch.isinf(ref).any())
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.equal(torch.isinf(y), torch.isinf(ref))


def test_s2_nonfinite_positions_match_generic_bf16():
    """The relaxed rule of test_mfma_bf16_nan_positions_match_generic: the same non-finite
    positions; an infinite input times a weight part that is exactly 0 is NaN where one fp32
    product is +-Inf."""
    B, C, O_, h, w = NF_CASE
    k, b = _weights(O_, C, 4)
    x = _plant(_bf16_input((B, C, h, w), 8))
    assert _plan(x, k, F32, NF_PAD, NF_OFF) == MBF
    y = ops.hexconv2d(x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    ref = _generic(ops.hexconv2d, x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    assert bool((~torch.isfinite(ref)).any())
    assert torch.equal(~torch.isfinite(y), ~torch.isfinite(ref))
    assert torch.equal(torch.isnan(ref) & ~torch.isnan(y), torch.zeros_like(y, dtype=torch.bool))
    fin = torch.isfinite(ref)
    torch.testing.assert_close(y[fin], ref[fin], rtol=1e-5, atol=1e-5 * float(ref[fin].abs().max()))


def test_s2_bf16_exact_weights_keep_inf():
    """test_mfma_bf16_exact_weights_keep_inf at stride 2: bf16-exact weights run one part's MFMAs
    on the kernel's own weight split, so an infinite input times a weight stays +-Inf as in the
    generic kernel: the same NaN and Inf positions and signs, finite outputs within 1e-5."""
    B, C, O_, h, w = NF_CASE
    g = torch.Generator().manual_seed(21)
    k = (torch.randint(-4, 5, (O_, C, 1, 7), generator=g).float() / 8.0).to(DEV)
    b = (torch.randint(-4, 5, (O_,), generator=g).float() / 4.0).to(DEV)
    x = _plant(_bf16_input((B, C, h, w), 9))
    assert _plan(x, k, F32, NF_PAD, NF_OFF) == MBF
    y = ops.hexconv2d(x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    ref = _generic(ops.hexconv2d, x, k, b, NF_OFF, 2, stride=2, padding=NF_PAD, out_dtype=F32)
    assert bool(torch.isinf(ref).any())                   # a planted Inf is read
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.equal(torch.isinf(y), torch.isinf(ref))
    assert torch.equal(y[torch.isinf(ref)], ref[torch.isinf(ref)])
    fin = torch.isfinite(ref)
    torch.testing.assert_close(y[fin], ref[fin], rtol=1e-5, atol=1e-5 * float(ref[fin].abs().max()))


def test_s2_bf16_mixed_exact_and_split_chunks():
    """C = 16: the chunk of channels 0-7 has bf16-exact weights (one part's MFMAs), the chunk of
    channels 8-15 random ones (all three parts), in one accumulation; finite inputs, 1e-5 against
    the generic kernel."""
    B, C, O_, h, w = 1, 16, 16, 14, 40
    k, b = _weights(O_, C, 33)
    g = torch.Generator().manual_seed(34)
    k[:, :8] = (torch.randint(-4, 5, (O_, 8, 1, 7), generator=g).float() / 8.0).to(DEV)
    x = _bf16_input((B, C, h, w), 35)
    assert _plan(x, k, F32, 1) == MBF
    y = ops.hexconv2d(x, k, b, 0, 2, stride=2, padding=1, out_dtype=F32)
    ref = _generic(ops.hexconv2d, x, k, b, 0, 2, stride=2, padding=1, out_dtype=F32)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))


# ---- training: MFMA forward, generic backward ---------------------------------------------------

def test_s2_autograd_forward_mfma_backward_generic():
    """A strided layer trains as matrix-core forward plus generic backward; gradients against
    the fp64 adjoint oracle at the tolerances of tests/test_gpu_conv_backward_mfma.py (rtol 1e-4,
    atol 1e-5 * max|ref|)."""
    torch.manual_seed(7)
    m = HexConv2d(16, 16, 1, 2, stride=2, padding=1, bias=True).to(DEV)
    x = torch.rand((2, 16, 13, 22), device=DEV, requires_grad=True)
    assert ops.hexconv2d_forward_plan(F32, F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1,
                                      even_odd_offset=1) == MF32
    gen = _abi.HG_CONV_BWD_GENERIC
    assert ops.hexconv2d_backward_plan(F32, F32, 2, 16, 16, 13, 22, 2, stride=2,
                                       padding=1) == (gen, gen)
    y = m(x)
    ref = O.hexconv2d(x.detach().double().cpu().numpy(), m.kernel.detach().double().cpu().numpy(),
                      m.bias.detach().double().cpu().numpy(), 1, 2, stride=2, padding=1)
    _close_to_oracle(y.detach(), ref)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    y.backward(gy)
    dx, dk, db = O.hexconv2d_backward(
        x.detach().double().cpu().numpy(), m.kernel.detach().double().cpu().numpy(),
        gy.double().cpu().numpy(), 1, 2, 2, 1)
    for got, want in ((x.grad, dx), (m.kernel.grad, dk), (m.bias.grad, db)):
        got = got.detach().double().cpu().numpy().reshape(want.shape)
        print("max abs err", np.abs(got - want).max(), "max|ref|", np.abs(want).max())
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * max(np.abs(want).max(), 1e-30))
