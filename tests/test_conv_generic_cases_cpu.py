"""The case table of the generic HexConv2d kernels (tests/conv_generic_cases.py) reaches what it
says it reaches, checked without a device from the library's host-only plan query
(hg_hexconv2d_generic_plan): every case lies in the regions it is filed under, the table as a
whole hits every region, every case is refused by the streaming and the MFMA kernel through the
condition it names, and the plan itself agrees with an independent restatement of the tap
geometry and the LDS budget.

The cib values this pins (input channels staged per pass, 56 KiB budget, 16 x 128 tiles):
    stride 1, dilation 1: radius 1: 6, radius 2-3: 5, radius 4-5: 4 (f32); 3, 2, 2 (f64)
    stride 1, dilation 2: radius 1: 6, radius 2: 5, 3: 4, 4: 3, 5: 3 or 2 by row parity (f32);
                          3, 2, 2, 1, 1 (f64)
    stride 2: 1 (f32), direct kernel (f64);  stride 3: direct kernel."""
import numpy as np
import pytest

import conv_generic_cases as CG
from HyGrid import _abi

TR, TC = 16, 128                  # k_hexconv's output tile (hexconv.hip CV_TR, CV_TC)
LDS_BUDGET, TAP_TABLE = 56 * 1024, 3 * 128 * 4      # CV_LDS_BUDGET, the three int[CV_MAXK] tables


# ---- the table --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CG.CASES, ids=repr)
def test_case_lies_in_its_regions(case):
    P = case.plan()
    assert case.regions, "a case is filed under at least one region"
    for region in case.regions:
        assert CG.REGIONS[region](case, P), f"{case.name} is not in {region}: plan {P}"
    cg, og = case.cg, case.og
    ho, wo = case.out_shape()
    if P["direct"]:
        assert (P["cib"], P["ocb"], P["bc"]) == (0, 1, 1)
        total = case.B * case.O * ho * wo
        assert P["tiles"] == -(-total // 256)
    else:
        assert 1 <= P["cib"] <= cg
        assert P["ocb"] == (4 if og % 4 == 0 or og > 4 else og)
        assert P["tiles"] == -(-ho // TR) * -(-wo // TC)
        nchunk = min(max(1, min(-(-2048 // P["tiles"]), case.B)), 65535)
        assert P["bc"] == -(-case.B // nchunk)
    # the spatial size does what the table's docstring says
    if case.spatial == "tiles":
        assert not P["direct"] and P["bc"] == 1
        assert -(-ho // TR) >= 2 and -(-wo // TC) >= 2 and ho % TR and wo % TC, (ho, wo)
        assert 17 <= ho <= 35 and 130 <= wo <= 140
    elif case.spatial == "one":
        assert not P["direct"] and P["tiles"] == 1 and ho < TR and wo < TC
        assert P["bc"] >= 2 and case.B % P["bc"], "several images per workgroup, a short last one"
    else:
        assert case.spatial == "blocks" and P["direct"]
        assert P["tiles"] >= 2 and (case.B * case.O * ho * wo) % 256, "a partial last block"


def test_every_region_has_a_case():
    hit = {}
    for case in CG.CASES:
        P = case.plan()
        for region in case.regions:
            assert region in CG.REGIONS, f"{case.name}: unknown region {region}"
            if CG.REGIONS[region](case, P):
                hit.setdefault(region, []).append(case.name)
    missing = sorted(set(CG.REGIONS) - set(hit))
    assert not missing, f"regions without a case: {missing}"
    # both row-parity offsets on the chunked kernel, on the direct kernel and in the batch loop
    for spatial in ("tiles", "one", "blocks"):
        assert {c.off for c in CG.CASES if c.spatial == spatial} == {0, 1}, spatial
    # both chunk shapes with both weight types
    multi = [(c, c.plan()) for c in CG.CASES if c.spatial == "tiles"]
    for w_dt in (CG.F32, CG.F64):
        assert any(c.w_dt == w_dt and c.cg % P["cib"] == 0 and P["cib"] < c.cg for c, P in multi)
        assert any(c.w_dt == w_dt and c.cg % P["cib"] != 0 and P["cib"] < c.cg for c, P in multi)
    # more than two chunks somewhere: a stale tile between chunks is not hidden by symmetry
    assert any(-(-c.cg // P["cib"]) >= 3 and c.cg % P["cib"] for c, P in multi)


def stream_takes(c):
    """hexconv.hip, hg_hexconv2d_epilogue: the register-streaming kernel's condition."""
    return (c.r == 2 and c.s == 1 and c.d == 1 and c.mode == "constant" and c.w_dt == CG.F32
            and c.C <= 3 and c.O <= 3)


def mfma_takes(c):
    """hexconv.hip (f32 weights only) and conv_mfma.hip, conv_mfma_try: the MFMA kernel's."""
    return (c.w_dt == CG.F32 and not c.mfma_off and c.r == 2 and c.s == 1 and c.d == 1
            and c.g == 1 and c.O >= 16 and 0 <= c.p <= 2)


@pytest.mark.parametrize("case", CG.CASES, ids=repr)
def test_case_is_refused_by_the_other_kernels(case):
    assert CG.REFUSALS["stream"][case.stream](case), f"{case.name}: stream not refused by {case.stream}"
    assert CG.REFUSALS["mfma"][case.mfma](case), f"{case.name}: mfma not refused by {case.mfma}"
    assert not stream_takes(case) and not mfma_takes(case)
    # the switch is set only where the layer is a dense radius-2 O >= 16 layer on purpose
    if case.mfma_off:
        assert case.mfma == "env" and case.w_dt == CG.F32 and case.r == 2 and case.s == 1 \
            and case.d == 1 and case.g == 1 and case.O >= 16 and case.p <= 2
    else:
        assert case.mfma != "env"


def test_backward_lists_name_cases():
    assert len(CG.BACKWARD) >= 6 and set(CG.BACKWARD) <= set(CG.BY_NAME)
    by = [CG.BY_NAME[n] for n in CG.BACKWARD]
    assert any(c.g == 4 and c.C == 24 and c.O == 28 for c in by)
    assert any(c.g == c.C == c.O == 24 for c in by)
    assert any(c.s == 2 and c.C == 8 and c.O == 8 for c in by)
    assert any(c.r == 3 and c.C == 13 and c.O == 6 for c in by)
    assert any(c.g == 1 and c.C == 37 and c.O == 12 for c in by)
    assert any(c.mode == "reflect" and c.p == 2 for c in by)
    assert any(c.w_dt == CG.F64 for c in by)
    assert all(c.x_dt in (CG.F32, CG.F64) and c.epi is None for c in by)
    needs = {(nx, nk, nb) for _, nx, nk, nb in CG.BACKWARD_PARTIAL}
    assert (True, False, False) in needs and (False, True, False) in needs
    assert {n for n, *_ in CG.BACKWARD_PARTIAL} <= set(CG.BY_NAME)


# ---- the plan against an independent restatement ----------------------------------------------
def tap_geom(r, s, d, op):
    """hexconv_geom.h tap_geom: (dy, dk at even output rows, dk at odd output rows) per tap."""
    taps = []
    for ii in range(2 * r - 1):
        tt = abs(ii - r + 1)
        for m in range(2 * r - 1 - tt):
            col = tt * d + 2 * d * m
            dk = []
            for par in (0, 1):
                y = par * s + ii * d
                L = ((y & 1) + op) & 1
                dk.append((1 + par * s + col - L) >> 1)
            taps.append((ii * d, dk[0], dk[1]))
    return taps


def footprint(r, s, d, op, esz):
    """(nPr, pitch, cib) of one tile: rows and padded columns of the padded image that a
    16 x 128 output tile reads, and how many channels of it fit in the LDS budget (0: none)."""
    taps = tap_geom(r, s, d, op)
    assert len(taps) == 3 * r * r - 3 * r + 1
    mink = min(min(a, b) for _, a, b in taps)
    maxk = max(max(a, b) for _, a, b in taps)
    maxdy = max(dy for dy, _, _ in taps)
    nPr = s * (TR - 1) + maxdy + 1
    pitch = (s * (TC - 1) + (maxk - mink) + 1 + 3) & ~3
    per = nPr * pitch * esz
    return nPr, pitch, (LDS_BUDGET - TAP_TABLE) // per if per + TAP_TABLE <= LDS_BUDGET else 0


@pytest.mark.parametrize("w_dt", [CG.F32, CG.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
def test_plan_matches_restated_footprint(r, s, d, w_dt):
    esz = 8 if w_dt == CG.F64 else 4
    code = _abi.dtype_code(w_dt)
    for p, off in [(0, 0), (0, 1), (1, 0), (2, 1)]:
        _, _, cib = footprint(r, s, d, (off + p) & 1, esz)
        # wide enough per group that the budget, not the layer, bounds cib; a narrower layer
        # stages all its channels at once
        for cg, groups in [(64, 1), (7, 3), (2, 1)]:
            P = _abi.hexconv2d_generic_plan(code, 3, cg * groups, 5 * groups, 70, 300, r, s, p, d,
                                            groups, off)
            assert P["direct"] == (cib == 0), (p, off, cg, P)
            assert P["cib"] == min(cg, cib), (p, off, cg, P)


def test_cib_table():
    """The values in this file's docstring, from the restatement (the plan equals it: above)."""
    def cibs(r, s, d, esz):
        return {footprint(r, s, d, op, esz)[2] for op in (0, 1)}

    assert [cibs(r, 1, 1, 4) for r in (1, 2, 3, 4, 5)] == [{6}, {5}, {5}, {4}, {4}]
    assert [cibs(r, 1, 1, 8) for r in (1, 2, 3, 4, 5)] == [{3}, {2}, {2}, {2}, {2}]
    assert [cibs(r, 1, 2, 4) for r in (1, 2, 3, 4, 5)] == [{6}, {5}, {4}, {3}, {2, 3}]
    assert [cibs(r, 1, 2, 8) for r in (1, 2, 3, 4, 5)] == [{3}, {2}, {2}, {1}, {1}]
    for r in (1, 2, 3, 4, 5):
        for d in (1, 2):
            assert cibs(r, 2, d, 4) == {1} and cibs(r, 2, d, 8) == {0}
            assert cibs(r, 3, d, 4) == {0} and cibs(r, 3, d, 8) == {0}
    # radius 2, the most common layer: 18 rows x 132 columns per channel
    assert footprint(2, 1, 1, 0, 4)[:2] == (18, 132) and footprint(2, 2, 1, 1, 4)[:2] == (33, 260)


def test_plan_query_validates_like_the_launch():
    f32 = _abi.dtype_code(CG.F32)
    with pytest.raises(ValueError):      # groups must divide the channels
        _abi.hexconv2d_generic_plan(f32, 1, 3, 4, 8, 8, 2, 1, 1, 1, 3, 0)
    with pytest.raises(ValueError):      # input too small
        _abi.hexconv2d_generic_plan(f32, 1, 3, 3, 1, 1, 2, 1, 0, 1, 1, 0)
    with pytest.raises(ValueError):      # weights are f32 or f64
        _abi.hexconv2d_generic_plan(_abi.dtype_code(CG.BF16), 1, 3, 3, 8, 8, 2)
    with pytest.raises(ValueError):      # more taps than the kernels' tables hold (radius <= 7)
        _abi.hexconv2d_generic_plan(f32, 1, 1, 1, 40, 40, 8)
    # an empty call launches nothing
    assert _abi.hexconv2d_generic_plan(f32, 0, 3, 3, 8, 8, 2) == dict(direct=False, cib=0, ocb=0,
                                                                     bc=0, tiles=0)
    # null out-parameters
    assert _abi.lib().hg_hexconv2d_generic_plan(f32, 1, 3, 3, 8, 8, 2, 1, 0, 1, 1, 0, None, None,
                                                None, None, None) == _abi.HG_EINVAL


def test_oracle_side_of_the_table_is_small():
    """The fp64 references stay cheap: multiply-adds of all oracle calls, forward and backward
    (three passes' worth), bounded so the GPU file's CPU side is seconds, not minutes."""
    def macs(c):
        ho, wo = c.out_shape()
        return c.B * c.O * ho * wo * c.cg * c.K

    total = sum(macs(c) for c in CG.CASES) + 3 * sum(macs(CG.BY_NAME[n]) for n in CG.BACKWARD)
    assert total < 1.5e9, total
    assert all(np.prod((c.B, max(c.C, c.O)) + c.out_shape()) < 2 ** 22 for c in CG.CASES)
