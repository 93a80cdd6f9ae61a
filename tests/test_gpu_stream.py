"""GPU parity of the row-streaming resample kernels (csrc/resample_stream.hip).

hg_rect_to_hex / hg_hex_to_rect route near-identity lattices (same-size resamples) to
k_r2h_stream / k_h2r_stream.  Those evaluate the general kernels' fp32 expressions in
the same order, so they are asserted BIT-IDENTICAL to the general LDS kernels
(selected with HYGRID_STREAM=0 and HYGRID_DOWN=0, read on every call: with the first alone a
same-size hex -> rect runs k_tri_up and a tiny 16-bit rect -> hex k_r2h_down), NaN/Inf
positions included, and within the north_star tolerance (rtol 1e-5, atol 1e-5*max|ref|; 16-bit
outputs one rounding of max|ref|) of the fp64 oracle (oracle/hg_oracle.c, pinned to
geometry_np.py:191-519 by tests/golden).  Every comparison first asserts, through the host-only
dispatch query, which kernel each side runs.
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only with -m gpu
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402

DEV = torch.device("cuda:0")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


GENERAL_ENV = {"HYGRID_STREAM": "0", "HYGRID_DOWN": "0"}
OP = {"rect_to_hex": _abi.HG_OP_RECT_TO_HEX, "hex_to_rect": _abi.HG_OP_HEX_TO_RECT}


def _with_env(env, fn, *args, **kw):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        out = fn(*args, **kw)
        if isinstance(out, torch.Tensor):
            torch.cuda.synchronize()
        return out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _kernel(op, x, size, out_dtype=None, env=None):
    """The kernel ops.<op>(x, size, out_dtype=...) runs under the switches env."""
    planes = x.numel() // (x.shape[-2] * x.shape[-1])
    od = x.dtype if out_dtype is None else out_dtype
    return _with_env(env or {}, _abi.resample_kernel, OP[op], _abi.dtype_code(x.dtype),
                     _abi.dtype_code(od), planes, x.shape[-2], x.shape[-1], size[0], size[1])


def _general(fn, x, size, **kw):
    """The call on the general kernel (asserted to be the one that runs)."""
    assert _kernel(fn.__name__, x, size, kw.get("out_dtype"), GENERAL_ENV) == _abi.HG_KERNEL_GENERAL
    return _with_env(GENERAL_ENV, fn, x, size, **kw)


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)
    nbad = int((ia != ib).sum().item())
    assert nbad == 0, f"{nbad} elements differ from the general kernel"


def _close(y, ref, rtol=1e-5):
    y = np.asarray(y, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    np.testing.assert_allclose(y, ref, rtol=rtol, atol=rtol * scale)


def _close_for(y, ref):
    """fp32 outputs: _close; 16-bit outputs: one rounding of max|ref| (tests/test_gpu_down.py)."""
    got = y.double().cpu().numpy()
    ref = ref.reshape(got.shape)
    if y.dtype == torch.float32:
        _close(got, ref)
    else:
        ulp = 2.0 ** (-8 if y.dtype == torch.bfloat16 else -11)
        assert np.abs(got - ref).max() <= ulp * max(np.abs(ref).max(), 1e-30)


# (h, w, h1, w1): same-size, ragged widths (not a multiple of the 256-column window),
# odd heights, band edges (128-row bands), and near-identity r2h with h1 != h
SHAPES_R2H = [(7, 8, 7, 8), (16, 20, 16, 20), (33, 260, 33, 260), (129, 516, 129, 516),
              (130, 1000, 130, 1000), (255, 256, 255, 256), (64, 300, 65, 300),
              (90, 512, 91, 516), (90, 512, 91, 512), (90, 516, 91, 516)]


def _r2h_kernel(shape, pair):
    """The kernel a SHAPES_R2H call really gets: a wider output (w1 != w) is no near identity
    and stays on the general kernel; the 7 x 8 raster with a 16-bit input is taken by
    k_r2h_down, which is tried first (its 16-byte chunk holds the whole row)."""
    if shape == (90, 512, 91, 516):
        return _abi.HG_KERNEL_GENERAL
    if shape == (7, 8, 7, 8) and pair[0] in ("bf16", "f16"):
        return _abi.HG_KERNEL_DOWN
    return _abi.HG_KERNEL_STREAM

SHAPES_H2R = [(7, 8), (16, 20), (33, 260), (129, 516), (130, 1000), (255, 256), (2, 4)]
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32"),
         ("f32", "bf16"), ("f32", "f16")]


@pytest.mark.parametrize("shape", SHAPES_R2H)
@pytest.mark.parametrize("pair", PAIRS)
def test_r2h_stream_bit_identical_to_general(shape, pair):
    h, w, h1, w1 = shape
    g = torch.Generator(device=DEV).manual_seed(h * 1000 + w)
    x = torch.rand((3, 2, h, w), generator=g, device=DEV).to(DT[pair[0]])
    want = _r2h_kernel(shape, pair)
    assert _kernel("rect_to_hex", x, (h1, w1), DT[pair[1]]) == want
    y = ops.rect_to_hex(x, (h1, w1), out_dtype=DT[pair[1]])
    ref = _general(ops.rect_to_hex, x, (h1, w1), out_dtype=DT[pair[1]])
    _same_bits(y, ref)
    if want == _abi.HG_KERNEL_DOWN:
        # the streaming kernel as well (HYGRID_DOWN=0 alone)
        env = {"HYGRID_DOWN": "0"}
        assert _kernel("rect_to_hex", x, (h1, w1), DT[pair[1]], env) == _abi.HG_KERNEL_STREAM
        _same_bits(_with_env(env, ops.rect_to_hex, x, (h1, w1), out_dtype=DT[pair[1]]), ref)
    if want != _abi.HG_KERNEL_STREAM:
        # the bit-identity above compares these shapes with (nearly) themselves: the oracle too
        _close_for(y[2], O.rect_to_hex(x[2].double().cpu().numpy(), (h1, w1), 1))


@pytest.mark.parametrize("shape", SHAPES_H2R)
@pytest.mark.parametrize("pair", PAIRS)
def test_h2r_stream_bit_identical_to_general(shape, pair):
    h, w = shape
    g = torch.Generator(device=DEV).manual_seed(h * 1000 + w + 1)
    x = torch.rand((2, 3, h, w), generator=g, device=DEV).to(DT[pair[0]])
    assert _kernel("hex_to_rect", x, (h, w), DT[pair[1]]) == _abi.HG_KERNEL_STREAM
    y = ops.hex_to_rect(x, (h, w), out_dtype=DT[pair[1]])
    ref = _general(ops.hex_to_rect, x, (h, w), out_dtype=DT[pair[1]])
    _same_bits(y, ref)


@pytest.mark.parametrize("op", ["rect_to_hex", "hex_to_rect"])
def test_stream_nan_inf_positions_match_general(op):
    h, w = 40, 264
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand((2, h, w), generator=g, device=DEV)
    x[0, 5, 17] = float("nan")
    x[0, 0, 0] = float("inf")
    x[1, h - 1, w - 1] = float("-inf")
    x[1, 20, 255] = float("nan")      # window edge column
    x[1, 21, 256] = float("nan")
    fn = getattr(ops, op)
    assert _kernel(op, x, (h, w)) == _abi.HG_KERNEL_STREAM
    y = fn(x, (h, w))
    ref = _general(fn, x, (h, w))
    _same_bits(y, ref)


@pytest.mark.parametrize("shape", [(33, 260, 33, 260), (64, 300, 65, 300), (129, 516, 129, 516)])
def test_r2h_stream_vs_oracle(shape):
    h, w, h1, w1 = shape
    rng = np.random.default_rng(h + w)
    x = rng.random((2, h, w), dtype=np.float64).astype(np.float32)
    assert _kernel("rect_to_hex", torch.from_numpy(x), (h1, w1)) == _abi.HG_KERNEL_STREAM
    y = ops.rect_to_hex(torch.from_numpy(x).to(DEV), (h1, w1)).cpu().numpy()
    ref = O.rect_to_hex(x.astype(np.float64), (h1, w1), 1)
    _close(y, ref)


@pytest.mark.parametrize("shape", [(33, 260), (129, 516), (255, 256)])
def test_h2r_stream_vs_oracle(shape):
    h, w = shape
    rng = np.random.default_rng(h * w)
    x = rng.random((2, h, w), dtype=np.float64).astype(np.float32)
    assert _kernel("hex_to_rect", torch.from_numpy(x), (h, w)) == _abi.HG_KERNEL_STREAM
    y = ops.hex_to_rect(torch.from_numpy(x).to(DEV), (h, w)).cpu().numpy()
    ref = O.hex_to_rect(x.astype(np.float64), (h, w), 1)
    _close(y, ref)


def test_stream_at_4k_matches_general():
    """BASELINE size (4K, 2 images x 3 channels, bf16) through both kernels."""
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand((2, 3, 2160, 3840), generator=g, device=DEV, dtype=torch.bfloat16)
    assert _kernel("rect_to_hex", x, (2160, 3840)) == _abi.HG_KERNEL_STREAM
    assert _kernel("hex_to_rect", x, (2160, 3840)) == _abi.HG_KERNEL_STREAM
    u = ops.rect_to_hex(x, (2160, 3840))
    _same_bits(u, _general(ops.rect_to_hex, x, (2160, 3840)))
    r = ops.hex_to_rect(u, (2160, 3840))
    _same_bits(r, _general(ops.hex_to_rect, u, (2160, 3840)))
