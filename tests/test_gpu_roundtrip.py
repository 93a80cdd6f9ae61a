"""BASELINE config 2: the rect -> hex -> rect round trip (geometry_np.rect_to_hex_resample,
geometry_np.py:358-519, then hex_to_rect_resample, :191-356) as one pass of the fused kernel
(hg_pipeline_r2h_h2r, fused_kernel.h MD 2) against the fp64 oracle chain and the two GPU
resamplers.  fp32: rtol 1e-5 (north_star); 16-bit outputs: one output rounding of the fp32
result (the hex image stays fp32 on chip where the operator chain may store it rounded)."""
import numpy as np
import pytest
import torch

import fused_variants as FV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import ops  # noqa: E402
from HyGrid.pipeline import rect_hex_rect  # noqa: E402

DEV = torch.device("cuda:0")


def oracle_roundtrip(x):
    xd = x.double().cpu().numpy()
    H, W = xd.shape[-2:]
    planes = xd.reshape(-1, H, W)
    hx = O.rect_to_hex(planes, (H, W), 1)
    return O.hex_to_rect(hx, (H, W), 1).reshape(xd.shape)


# the list lives in tests/fused_variants.py: tests/test_fused_variants_cpu.py pins that it
# reaches every loop variant of k_fused MD 2
@pytest.mark.parametrize("shape", FV.roundtrip_shapes())
def test_roundtrip_fp32_vs_oracle(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g).to(DEV)
    y = ops.pipeline_r2h_h2r(x)
    assert y is not None and y.shape == x.shape and y.dtype == torch.float32
    ref = oracle_roundtrip(x)
    scale = np.abs(ref).max()
    got = y.double().cpu().numpy()
    msg = FV.describe_first_bad(2, ~(np.abs(got - ref) <= 1e-5 * scale + 1e-5 * np.abs(ref)))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * scale, err_msg=msg)


def test_roundtrip_1080p_fp32_full_image_vs_oracle():
    """One full config-2 image (3 x 1080 x 1920 fp32) through the fused round trip."""
    g = torch.Generator().manual_seed(12)
    x = torch.rand((1, 3, 1080, 1920), generator=g).to(DEV)
    y = rect_hex_rect(x)
    ref = oracle_roundtrip(x)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(y.double().cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * scale)


@pytest.mark.parametrize("dt,out", [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                                    (torch.bfloat16, torch.float32)])
def test_roundtrip_16bit_vs_fp32_chain(dt, out):
    g = torch.Generator().manual_seed(4)
    x = torch.rand((2, 3, 96, 200), generator=g).to(DEV).to(dt)
    y = ops.pipeline_r2h_h2r(x, out_dtype=out)
    assert y is not None and y.dtype == out
    ref = ops.hex_to_rect(ops.rect_to_hex(x.float(), out_dtype=torch.float32),
                          out_dtype=torch.float32)
    ulp = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 1e-5}[out]
    scale = float(ref.abs().max())
    torch.testing.assert_close(y.float(), ref, rtol=ulp, atol=ulp * scale)


def test_roundtrip_matches_two_gpu_resamplers_batched():
    """Fused vs the two streaming resamplers on a 4-D fp32 batch (same fp32 arithmetic up to
    the order of the h2r terms)."""
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.rand((4, 3, 270, 480), generator=g, device=DEV)
    y = rect_hex_rect(x)
    ref = rect_hex_rect(x, fused=False)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)


def test_roundtrip_unsupported_geometry_falls_back():
    """Odd width or a resized hex lattice: the fused entry declines, rect_hex_rect runs the
    two resamplers and still matches the oracle."""
    g = torch.Generator().manual_seed(2)
    x = torch.rand((1, 2, 40, 63), generator=g).to(DEV)
    assert ops.pipeline_r2h_h2r(x) is None
    y = rect_hex_rect(x)
    ref = oracle_roundtrip(x)
    np.testing.assert_allclose(y.double().cpu().numpy(), ref, rtol=1e-5,
                               atol=1e-5 * np.abs(ref).max())
    assert ops.pipeline_r2h_h2r(x[..., :62], hex_size=(30, 62)) is None


def test_roundtrip_nonfinite_inputs_stay_local():
    """A NaN stays local: the fused kernel evaluates fixed tap sets (a zero-weight tap still
    multiplies, 0 x NaN = NaN; the same-size h2r's zero-weight third vertex is not read), so
    which outputs within 3 samples turn NaN can differ from the reference; every output
    farther away is finite and matches the oracle (as for the fused
    pipeline)."""
    g = torch.Generator().manual_seed(6)
    x = torch.rand((1, 1, 64, 128), generator=g)
    x[0, 0, 30, 70] = float("nan")
    y = ops.pipeline_r2h_h2r(x.to(DEV)).cpu()
    ref = torch.from_numpy(oracle_roundtrip(x))
    assert bool(torch.isnan(y[0, 0, 30, 70]))
    far = torch.ones_like(y, dtype=torch.bool)
    far[..., 27:34, 67:74] = False
    assert bool(torch.isfinite(y[far]).all())
    torch.testing.assert_close(y[far].double(), ref[far], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("md", [2])
def test_roundtrip_nonfinite_at_band_and_window_edges(md, monkeypatch):
    """Band / window edges of the kernel that runs (md 2: k_fused MD 2; round 5's opt-in
    four-column rt4.hip was removed in round 6), from hg_fused_layout (not hard-coded):
    non-finite inputs on the last row of a band and the first of the next, on the last owned
    column of a window and the first of the next; everything farther than 3 samples stays
    finite and matches the oracle, and every planted point reaches the output next to it."""
    from HyGrid import _abi
    rows, own, _ = _abi.fused_layout(md)
    H, W = 2 * rows + 10, 2 * own + 12
    g = torch.Generator().manual_seed(7)
    x = torch.rand((2, 1, H, W), generator=g)
    vals = [float("nan"), float("inf"), float("-inf")]
    er = [r for k in (1, 2) for r in (k * rows - 1, k * rows) if r < H]
    ec = [q for k in (1, 2) for q in (k * own - 1, k * own) if q < W]
    pts = [(i % 2, r, ec[i % len(ec)]) for i, r in enumerate(er)]
    for i, (p, r, q) in enumerate(pts):
        x[p, 0, r, q] = vals[i % 3]
    y = ops.pipeline_r2h_h2r(x.to(DEV))
    assert y is not None
    y = y.cpu()
    ref = torch.from_numpy(oracle_roundtrip(x))
    far = torch.ones_like(y, dtype=torch.bool)
    for p, r, q in pts:
        far[p, :, max(r - 3, 0):r + 4, max(q - 3, 0):q + 4] = False
        assert not bool(torch.isfinite(y[p, :, max(r - 3, 0):r + 4, max(q - 3, 0):q + 4]).all())
    assert bool(torch.isfinite(y[far]).all())
    torch.testing.assert_close(y[far].double(), ref[far], rtol=1e-5, atol=1e-5)
