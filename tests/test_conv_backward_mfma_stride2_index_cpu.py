"""The stride-2 backward routes, restated on the host and checked against the fp64 oracle before
anything runs on a GPU.

  * d kernel / d bias: k_hexconv_bwd_weight_mfma_s2's tile walk (csrc/conv_mfma_bwd.hip) in NumPy,
    conv_bwd_s2_cases.kernel_walk, with the tile constants read from the sources: the host's
    slices, cs_stage_p's rows 2 r0 .. 2 r0 + 8 and column-parity planes under every padding rule,
    the staged row 2 (r0 + wv) + dy_t - 2 r0 and the plane / slot of column 2 q + dk_t(par) per
    (c, t) pair, both operands masked outside the output, the constant-1 slot.  Every index must
    stay inside the staged chunk and inside the slots that were written, and the sums must equal
    oracle.hexconv2d_backward(..., stride=2, ...) for every shape of the GPU test, at both chunk
    sizes (4 and 8 channels), up to fp64 summation order.
  * d input: hexconv_transpose2d's definition (the class tap table k_hexconvt_s2 is launched
    with, ops.hexconv_transpose2d_taps) applied to gy with the layer's own kernel equals the
    oracle's d input for the routed (offset, padding, size) cases."""
import numpy as np
import pytest

import conv_bwd_s2_cases as CS
import conv_transpose_cases as CT
from HyGrid import ops
from oracle import oracle as O

SHAPES = CS.all_shapes()
# resident workgroups per CU the host sizes the grid for (cmb_s2_wgs), by chunk and tile count
WGS = {4: {2: 5, 4: 4}, 8: {2: 3, 4: 2}}


def _close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12 * max(np.abs(ref).max(), 1e-30))


def test_committed_chunk_is_one_of_the_restated():
    K = CS.constants()
    assert K["CMB_S2_CC"] in WGS and K["CS_CST"] % 32 == 16
    assert K["CMB_S2_MIN_O"] >= 16
    src = open(CS.CSRC + "/conv_mfma_bwd.hip").read()
    assert "(nt == 2 ? 3 : 2) : (nt == 2 ? 5 : 4)" in src      # WGS above is cmb_s2_wgs


@pytest.mark.parametrize("case", SHAPES, ids=str)
@pytest.mark.parametrize("cc", [4, 8])
def test_tile_walk_matches_oracle(case, cc):
    (x, k, b, gy), (_, rdk, rdb) = CS.data(case)
    B, C, O_, h, w, pad, off, mode, pv = case
    nt = 2 if O_ <= 32 else 4
    dk, db, wgs = CS.kernel_walk(x.astype(np.float64), gy.astype(np.float64), off, pad, mode, pv,
                                 cc, WGS[cc][nt])
    _close(dk, rdk.reshape(dk.shape))
    _close(db, rdb)
    assert wgs >= -(-C // cc) * -(-O_ // (16 * nt))


def test_the_table_holds_every_mechanism():
    """More than one slice; wo > 64 with both gy load paths; ho no multiple of 4; every padding
    mode; partial chunks and output tiles."""
    K = CS.constants()
    h, w = CS.slice_case(O.hexconv2d_out_shape)
    ho, wo = O.hexconv2d_out_shape(h, w, 2, 2, 1, 1)
    assert (ho, wo) == (20, 65) and 2 * 5 * 2 // K["CMB_MIN_TILES"] >= 2
    x, gy = np.zeros((2, 16, h, w)), np.zeros((2, 16, ho, wo))
    assert CS.kernel_walk(x, gy, 0, 1, "constant", 0.0, 4, 5)[2] == 2 * 4      # 2 slices x 4 chunks
    wos = [O.hexconv2d_out_shape(h_, w_, 2, 2, 1, 1)[1] for (h_, w_) in
           CS.column_cases(O.hexconv2d_out_shape)]
    assert wos[0] > 64 and wos[0] % 4 != 0 and wos[1] > 64 and wos[1] % 4 == 0
    assert {c[7] for c in SHAPES} == {"constant", "reflect", "replicate", "circular"}
    assert {(c[5], c[6]) for c in SHAPES} >= {(p, o) for p in (0, 1, 2) for o in (0, 1)}
    assert any(O.hexconv2d_out_shape(c[3], c[4], 2, 2, c[5], 1)[0] % 4 for c in SHAPES)


def test_inf_where_no_tap_reaches_stays_out_of_the_sums():
    """Padding 0: the samples no tap reads exist, hold +Inf, and the walk's edge tiles (which
    stage them) still sum finite values equal to the oracle's: both operands are masked."""
    (h, w), hole = CS.untapped_case()
    assert hole.any() and hole[-1].all()
    case = (1, 16, 16, h, w, 0, 0, "constant", 0.0)
    (x, k, b, gy), (rdx, rdk, rdb) = CS.data(case)
    xi = x.astype(np.float64)
    xi[:, :, hole] = np.inf
    dk, db, _ = CS.kernel_walk(xi, gy.astype(np.float64), 0, 0, "constant", 0.0, 4, 5)
    assert np.isfinite(dk).all()
    _close(dk, rdk.reshape(dk.shape))
    _close(db, rdb)
    assert (rdx[:, :, hole] == 0).all()


@pytest.mark.parametrize("case", [c for c in SHAPES if c[7] == "constant" and c[1] >= 16], ids=str)
def test_transposed_layer_on_gy_is_the_oracles_dinput(case):
    (x, k, b, gy), (rdx, _, _) = CS.data(case)
    B, C, O_, h, w, pad, off, mode, pv = case
    T = [[ops.hexconv_transpose2d_taps(off, pad, rc, cc) for cc in (0, 1)] for rc in range(4)]
    assert ops.hexconv_transpose2d_out_shape(gy.shape[2], gy.shape[3], 2, 2, pad, 1, (h, w)) == (h, w)
    got = CT.from_taps(T, gy, k.reshape(O_, C, 7), h, w)
    _close(got, rdx)
