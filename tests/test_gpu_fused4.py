"""GPU parity of the four-column variant of the fused rect->hex->HexConv2d->hex->rect kernel
(csrc/fused4.hip, k_fused4: bf16 in and out, C = O = 3, widths a multiple of 4 -- the
headline's launch).  It evaluates the two-column kernel's (k_fused MD 0) products and sums per
output in the same order (vertical and horizontal r2h blends, the 7 packed taps per conv row in
tap order, the folded h2r), so on the bands it walks downwards its bf16 output is asserted
BIT-IDENTICAL to the two-column kernel (HYGRID_FUSED4=0), NaN / Inf included, at band and window
edges placed from hg_fused_layout(6); and within one bf16 rounding of the fp64 oracle chain.
Round 6: odd full bands walk upwards (F4_REV, shared halo rows read together), where a conv row
sums its below taps before its above taps: the same products in another order, so those rows
are asserted within one bf16 step of the two-column kernel instead (and the oracle check holds
for every row)."""
import numpy as np
import pytest
import torch

import fused_variants as FV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi, ops  # noqa: E402
from HyGrid.HexFrames import HexConv2d  # noqa: E402

DEV = torch.device("cuda:0")


def _run(x, conv, off, monkeypatch, two_col):
    if two_col:
        monkeypatch.setenv("HYGRID_FUSED4", "0")
    else:
        monkeypatch.delenv("HYGRID_FUSED4", raising=False)
    with torch.no_grad():
        y = ops.pipeline_r2h_conv_h2r(x, conv.kernel, conv.bias, None, None, 1, 1, off, 0.0,
                                      torch.bfloat16)
    torch.cuda.synchronize()
    monkeypatch.delenv("HYGRID_FUSED4", raising=False)
    assert y is not None
    return y


def _oracle(x, conv):
    h = O.rect_to_hex(x.double().cpu().numpy(), None, 1)
    c = O.hexconv2d(h, conv.kernel.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(),
                    int(conv.even_odd_offset), 2, padding=1)
    return O.hex_to_rect(c, None, 1)


def _up_rows(H):
    """Rows of the bands k_fused4 walks upwards: odd bands of the full band length (the rule
    is restated once, in tests/fused_variants.py)."""
    return torch.from_numpy(FV.up_rows(6, H))


def _same(a, b, mask=None):
    """Bit-identical outside the upward bands; within one bf16 step inside them (the same
    products summed in another order can tip a rounding).  mask: (H, W) outputs to compare."""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16
    H, W = a.shape[-2:]
    up = _up_rows(H).to(a.device)[:, None].expand(H, W)
    sel = torch.ones((H, W), dtype=torch.bool, device=a.device) if mask is None else mask
    fwd, rev = (sel & ~up).expand_as(a), (sel & up).expand_as(a)
    diff = (a.view(torch.int16) != b.view(torch.int16)) & fwd
    nbad = int(diff.sum().item())
    assert nbad == 0, (f"{nbad} outputs of downward bands differ from the two-column kernel: "
                       + _where(diff))
    if bool(rev.any()):
        fa, fb = a[rev].float(), b[rev].float()
        assert torch.equal(torch.isnan(fa), torch.isnan(fb)), \
            _where(rev & (torch.isnan(a) != torch.isnan(b)))
        fin = torch.isfinite(fb)
        assert torch.equal(fa[~fin & ~torch.isnan(fb)], fb[~fin & ~torch.isnan(fb)]), \
            _where(rev & torch.isinf(b) & (a != b))
        d = (fa[fin] - fb[fin]).abs()
        tol = 2.0 ** -7 * torch.maximum(fa[fin].abs(), fb[fin].abs()) + 1e-6
        if not bool((d <= tol).all()):
            af, bf = a.float(), b.float()
            over = rev & torch.isfinite(bf) & ~((af - bf).abs() <= 2.0 ** -7 * torch.maximum(af.abs(), bf.abs()) + 1e-6)
            raise AssertionError(f"{int((d > tol).sum())} outputs of upward bands beyond one bf16 step: "
                                 + _where(over))


def _where(bad):
    """The first bad output and the loop variant that made it (tests/fused_variants.py)."""
    return FV.describe_first_bad(6, bad.cpu().numpy())


def test_layout():
    rows, own, halo = _abi.fused_layout(6)
    assert rows % 6 == 0 and own == 240 and halo == 8


# (B, H, W): one window / band, band and window edges, several of each, the full 4K width;
# then the shapes whose last band ends on steps 5 and 3 of a block and whose bands and windows
# run every (cd, rc) loop downwards and upwards (tests/fused_variants.py, pinned by
# tests/test_fused_variants_cpu.py)
SHAPES = FV.fused4_shapes()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused4_bit_identical_to_two_column_and_vs_oracle(shape, off, monkeypatch):
    B, H, W = shape
    torch.manual_seed(3 + off)
    conv = HexConv2d(3, 3, off, 2, padding=1, bias=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(H * 7 + W)
    x = torch.rand((B, 3, H, W), generator=g, device=DEV).to(torch.bfloat16)
    y4 = _run(x, conv, off, monkeypatch, False)
    y2 = _run(x, conv, off, monkeypatch, True)
    _same(y4, y2)
    # What pins this kernel at the north_star's 1e-5 is the agreement above: the two-column
    # kernel is oracle-checked at 1e-5 in fp32 (tests/test_gpu_pipeline.py).  Against the fp64
    # oracle directly, each bf16 output is one rounding of an fp32 value within ~1e-6 of the
    # oracle's: per element |got - ref| <= 2^-8 |ref| (half an ulp is 2^-9 |ref| at most; the
    # fp32 error may tip a near-tie to the other neighbour) plus an absolute floor for values
    # near zero, where the fp32 cancellation error is relative to the terms, not the sum.
    ref = _oracle(x[B - 1:B], conv)[0]
    got = y4[B - 1].double().cpu().numpy()
    tol = 2.0 ** -8 * np.abs(ref) + 1e-5 * np.abs(ref).max()
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (f"{int(bad.sum())} outputs beyond one bf16 rounding of the oracle: "
                           + FV.describe_first_bad(6, bad))


@pytest.mark.parametrize("off", [0, 1])
def test_fused4_nonfinite_at_band_and_window_edges(off, monkeypatch):
    """Inf / NaN on the four-column kernel's band edges (last row of a band, first of the
    next) and window edges (last owned column of a window, first of the next), the raster's
    corners and edges."""
    _nonfinite_at_edges(14, off, monkeypatch)


@pytest.mark.parametrize("off", [0, 1])
def test_fused4_nonfinite_at_edges_odd_tail(off, monkeypatch):
    """The same on an odd height whose last band ends on step 3 of a block (2 rows + 15)."""
    _nonfinite_at_edges(15, off, monkeypatch)


def _nonfinite_at_edges(extra, off, monkeypatch):
    rows, own, _ = _abi.fused_layout(6)
    H, W = 2 * rows + extra, 2 * own + 16
    torch.manual_seed(5)
    conv = HexConv2d(3, 3, off, 2, padding=1, bias=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.rand((1, 3, H, W), generator=g, device=DEV).to(torch.bfloat16)
    vals = [float("inf"), float("-inf"), float("nan")]
    pts = [(0, 0, 0), (1, H - 1, W - 1), (2, 0, W - 1), (0, H - 1, 0), (1, 5, 1), (2, 7, W - 2)]
    for k in (1, 2):
        for r in (k * rows - 1, k * rows):
            for q in (own - 1, own, 2 * own - 1, 2 * own):
                if r < H and q < W:
                    pts.append((len(pts) % 3, r, q))
    for i, (c, r, q) in enumerate(pts):
        x[0, c, r, q] = vals[i % 3]
    y4 = _run(x, conv, off, monkeypatch, False)
    y2 = _run(x, conv, off, monkeypatch, True)
    # every output farther than 3 rows / columns from a planted value is finite and agrees with
    # the two-column kernel's (_same); near one, a zero-weight tap of a window's column class may
    # carry the non-finite value differently (a 240-column window's class can differ from its
    # two 120-column windows': DESIGN.md section 3), but the value reaches the output near it
    near = torch.zeros((H, W), dtype=torch.bool)
    for _, r, q in pts:
        near[max(r - 3, 0):r + 4, max(q - 3, 0):q + 4] = True
    far = ~near.to(DEV)
    assert torch.isfinite(y4[0][:, far].float()).all()
    _same(y4, y2, far)
    for _, r, q in pts:
        assert not torch.isfinite(y4[0, :, max(r - 3, 0):r + 4, max(q - 3, 0):q + 4].float()).all()
