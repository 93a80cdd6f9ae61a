"""Coverage pin of the fused streaming kernels' loop variants (no device needed): the shapes the
GPU parity tests run (tests/fused_variants.py), put through the CPU mirror of the kernels'
variant selection, reach every loop class in every direction, every tail length, every block
bucket and every window fill -- separately for both tap column classes (OP) and, for the two
conv modes, for every channel configuration the dispatchers instantiate.  A retune of a band
length or a window that moves a shape off a variant fails here instead of silently dropping
the variant from the suite."""
import numpy as np
import pytest

import fused_variants as FV
from oracle import oracle as O


def _need(have, want, what):
    missing = sorted(set(want) - set(have), key=str)
    assert not missing, f"{what}: no test shape reaches {missing}"


def _check_factors(md, waves, what):
    """Every loop x direction, every tail of a downward band, every reachable block bucket
    (k_fused), every window fill."""
    rows = FV.layout(md)[0]
    _need({(w.loop, w.direction) for w in waves},
          [(lp, d) for lp in FV.loops(md) for d in FV.directions(md)], f"{what} loop x direction")
    # a band of fewer than `rows` rows is the last one and walks down: tails 0 .. 5 all exist
    _need({w.tail for w in waves if w.direction == "down"}, range(FV.STEP_BLOCK), f"{what} tail")
    if md != 6:
        _need({w.bucket for w in waves}, {FV.bucket_of(n) for n in range(1, rows + 1)},
              f"{what} block bucket")
    _need({w.fill for w in waves}, FV.FILLS, f"{what} window fill")


def _check_classes(md, waves, what):
    _need({(w.loop, w.direction) for w in waves},
          [(lp, d) for lp in FV.loops(md) for d in FV.directions(md)], f"{what} loop x direction")


def _md6(shapes):
    return [w for _, H, W in shapes for w in FV.census(6, H, W)]


def _md0(cases, op, chan=None):
    return [w for _, c, H, W, off, g in cases
            if FV.op_of(off) == op and (chan is None or (c, c, g) == chan)
            for w in FV.census(0, H, W)]


def _md1(cases, chan=None):
    return [w for _, c, o, g, H, W in cases if chan is None or (c, o, g) == chan
            for w in FV.census(1, H, W)]


def _md2(shapes):
    return [w for _, _, H, W in shapes for w in FV.census(2, H, W)]


def test_layouts_fit_the_census():
    for md in FV.MODES:
        rows, own, halo, width = FV.layout(md)
        assert rows % FV.STEP_BLOCK == 0 and rows > 0 and own > 0 and halo > 0
        assert width == 64 * width_per_lane(md)


def width_per_lane(md):
    return 4 if md == 6 else 2


def test_lattice_matches_the_oracle_maps():
    """The mirror's fp64 lattice is the oracle's (itself pinned to the reference's maps)."""
    for h, w in ((37, 52), (185, 500), (2, 4)):
        m = O.r2h_maps(h, w, h, w)
        i_n, i_f = FV.r2h_rows(h, h)
        j_n, j_f = FV.r2h_cols(w, w)
        assert np.array_equal(m["i_n"], np.broadcast_to(i_n[:, None], (h, w)))
        assert np.array_equal(m["j_n"], np.broadcast_to(j_n[None, :], (h, w)))
        assert np.array_equal(m["i_f"], np.broadcast_to(i_f[:, None], (h, w)))
        assert np.array_equal(m["j_f"], np.broadcast_to(j_f[None, :], (h, w)))


def test_census_records_one_wave_per_band_and_window():
    rows, own, _, _ = FV.layout(6)
    waves = FV.census(6, 2 * rows + 3, 5 * own)
    assert len(waves) == 3 * 8                        # 5 windows run as 2 groups of 4 waves
    assert [w.n for w in waves if w.win == 0] == [rows, rows, 3]
    assert [w.direction for w in waves if w.win == 0] == ["down", "up", "down"]
    assert [w.fill for w in waves if w.band == 0] == ["full"] * 5 + ["empty"] * 3
    assert waves[0].loop == "generic"                 # row 0 blends downwards: band 0 is mixed
    up = FV.up_rows(6, 2 * rows + 3)
    assert up.sum() == rows and up[rows] and up[2 * rows - 1] and not up[2 * rows]
    assert all(w.direction == "down" for w in FV.census(0, 300, 500))


def test_shapes_fit_the_kernels_and_stay_small():
    for _, H, W in FV.fused4_shapes():
        assert W % 4 == 0
    for _, _, H, W, _, _ in FV.md0_cases():
        assert W % 2 == 0 and H <= 300 and W <= 1000
    for _, _, _, _, H, W in FV.fconv_cases():
        assert W % 2 == 0
    for B, H, W in FV.fused4_new_shapes():
        assert B <= 2 and H <= 300 and W <= 1000
    for B, _, _, _, H, W in FV.fconv_new_cases():
        assert B <= 2 and H <= 300 and W <= 1000


@pytest.mark.parametrize("op", [0, 1])
def test_fused4_shapes_reach_every_variant(op):
    # test_gpu_fused4.py runs every shape at both offsets, so OP 0 and OP 1 see the same waves
    _check_factors(6, _md6(FV.fused4_shapes()), f"k_fused4 OP {op}")


@pytest.mark.parametrize("op", [0, 1])
def test_md0_cases_reach_every_variant(op):
    cases = FV.md0_cases()
    _check_factors(0, _md0(cases, op), f"k_fused MD 0 OP {op}")
    for chan in FV.CHANNELS:
        _check_classes(0, _md0(cases, op, chan), f"k_fused MD 0 OP {op} C/O/G {chan}")


@pytest.mark.parametrize("op", [0, 1])
def test_fconv_cases_reach_every_variant(op):
    # test_gpu_fused_conv.py runs every case at both offsets
    cases = FV.fconv_cases()
    _check_factors(1, _md1(cases), f"k_fused MD 1 OP {op}")
    for chan in FV.CHANNELS:
        _check_classes(1, _md1(cases, chan), f"k_fused MD 1 OP {op} C/O/G {chan}")


def test_roundtrip_shapes_reach_every_variant():
    _check_factors(2, _md2(FV.roundtrip_shapes()), "k_fused MD 2")


def test_every_new_shape_is_needed():
    """Each shape this census added carries a variant nothing else in its list reaches."""
    def fails(fn, *a):
        try:
            fn(*a)
        except AssertionError:
            return True
        return False

    s6 = FV.fused4_shapes()
    for s in FV.fused4_new_shapes():
        assert fails(_check_factors, 6, _md6([t for t in s6 if t != s]), "k_fused4"), s
    c0 = FV.md0_cases()
    for s in c0:
        rest = [t for t in c0 if t != s]
        op, chan = FV.op_of(s[4]), (s[1], s[1], s[5])
        assert (fails(_check_factors, 0, _md0(rest, op), "MD 0") or
                fails(_check_classes, 0, _md0(rest, op, chan), "MD 0")), s
    c1 = FV.fconv_cases()
    for s in FV.fconv_new_cases():
        rest = [t for t in c1 if t != s]
        assert (fails(_check_factors, 1, _md1(rest), "MD 1") or
                fails(_check_classes, 1, _md1(rest, s[1:4]), "MD 1")), s


def test_describe_first_bad_names_the_loop():
    rows, own, _, _ = FV.layout(6)
    H, W = 6 * rows + 5, 2 * own + 20
    bad = np.zeros((1, 3, H, W), bool)
    assert FV.describe_first_bad(6, bad) == ""
    bad[0, 1, H - 2, own + 1] = True
    msg = FV.describe_first_bad(6, bad)
    assert "band 6" in msg and "tail 5" in msg and "window 1" in msg and "down" in msg
