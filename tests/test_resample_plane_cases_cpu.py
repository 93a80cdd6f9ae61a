"""The case table of the resamplers' plane loops (tests/resample_plane_cases.py) reaches what it
says it reaches, checked without a device from the library's host-only plan query
(hg_resample_plan, computed by the host functions the launches themselves call): every case is
routed to its family's kernel and lies in the regions it is filed under, every region has a case
for every kernel instantiation it applies to, every case's plan is pinned, and the plan's kernel
equals hg_resample_kernel over the table and over the shape lists of the four older GPU files."""
import json
import os

import pytest
import torch

import resample_plane_cases as RP
from HyGrid import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = json.load(open(os.path.join(HERE, "golden", "resample_plane_plans.json")))


@pytest.mark.parametrize("case", RP.CASES, ids=repr)
def test_case_lies_in_its_regions(case):
    P = case.plan()
    assert P["kernel"] == RP.FAMILY_KERNEL[case.family], f"{case.name}: plan {P}"
    assert case.regions, "a case is filed under at least one region"
    for region in case.regions:
        assert RP.REGIONS[region](case, P), f"{case.name} is not in {region}: plan {P}"
    # the plan is consistent with itself
    assert P["chunks"] == -(-case.planes // P["pc"]) and (P["chunks"] - 1) * P["pc"] < case.planes
    if case.family in ("tri_up", "hexdown"):
        rb, wc = P["band_rows"], P["window_cols"]
        assert P["units"] == -(-case.h1 // rb) * -(-case.w1 // wc) * P["chunks"]
        assert P["launched"] == (P["units"] if P["wave_per_unit"] else min(P["units"], 4096))
        assert P["pdp"] == (3 if case.family == "tri_up" else 1 if P["DB"] == 16 else 2)
    if case.family == "hexdown":
        assert P["P"] == (1 if P["DB"] == 16 else 2) and P["K"] in (4, P["P"])
        assert P["nout"] == P["window_cols"] and (P["K"] == 4) == (P["nout"] > 64 * P["P"])
        assert P["DB"] == (4 if case.align or case.env.get("HYGRID_UP") == "0" else 16)
    if case.family in ("general", "nearest", "backward"):
        assert P["units"] == P["launched"] == P["chunks"], "one tile: a workgroup per chunk"
    if case.family in ("r2h_stream", "h2r_stream", "r2h_down"):
        nwin, nband = -(-case.w1 // P["window_cols"]), -(-case.h1 // P["band_rows"])
        assert P["launched"] == case.planes * nband * -(-nwin // 4), "no workgroup past the planes"
    # the general-kernel reference of the bit-identity comparison is the general kernel
    if case.family in RP.GENERAL_SWITCH:
        G = case.plan(dict(case.env, **RP.GENERAL_SWITCH[case.family]))
        assert G["kernel"] == (RP.GENERAL if case.interp else RP.NEAR_K)
    es = lambda dt: torch.empty((), dtype=dt).element_size()                       # noqa: E731
    nbytes = case.planes * (case.h * case.w * es(case.in_dt) + case.h1 * case.w1 * es(case.out_dt))
    assert nbytes <= 10 << 20, "source + result: a few MB"


def required():
    """instantiation -> regions it must reach."""
    need = {}
    for K in ("Knat", "K1"):
        for i in ("bf16", "f16", "f32"):
            for o in ("bf16", "f16", "f32"):
                need[("k_tri_up", "linear", i, o, K)] = RP.CHUNK_REGIONS[3] + RP.GRID_REGIONS["tri_up"]
        for e in ("1B", "2B", "4B"):
            need[("k_tri_up", "nearest", e, K)] = RP.CHUNK_REGIONS[3] + RP.GRID_REGIONS["tri_up"]
    for i in ("bf16", "f16"):
        for o in ("bf16", "f16", "f32"):
            for db, pdp in (("DB16", 1), ("DB4", 2)):
                for K in ("K4", "KP"):
                    for sep in ("SEP", "shared"):
                        need[("k_hexresize_down", i, o, db, K, sep)] = \
                            RP.CHUNK_REGIONS[pdp] + RP.GRID_REGIONS["hexdown"]
    for fam in ("general", "nearest", "backward"):
        need[(fam,)] = ("wg_pc=2", "wg_pc=3")
    need[("general",)] += ("direct",)
    for fam in ("r2h_stream", "h2r_stream", "r2h_down"):
        need[(fam,)] = ("blocks%8",)
    return need


def reached(cases):
    hit = {}
    for c in cases:
        P = c.plan()
        for region in c.regions:
            assert region in RP.REGIONS, f"{c.name}: unknown region {region}"
            if RP.REGIONS[region](c, P):
                hit.setdefault((c.inst(P), region), []).append(c.name)
    return hit


def missing(cases):
    hit = reached(cases)
    return sorted((inst, r) for inst, regions in required().items() for r in regions
                  if (inst, r) not in hit)


def test_every_region_has_a_case_for_every_instantiation():
    assert not missing(RP.CASES)
    hit = reached(RP.CASES)
    # the regions that need one case, not one per instantiation
    for fam, region in (("tri_up", "two_units_per_wave"), ("hexdown", "two_units_per_wave"),
                        ("hexdown", "upw")):
        assert any(r == region and c[0].startswith("k_" + fam[:3]) for c, r in hit), (fam, region)
    # linear and nearest k_tri_up both stride
    two = [RP.BY_NAME[n] for (i, r), ns in hit.items() if r == "two_units_per_wave" for n in ns]
    assert {c.interp for c in two if c.family == "tri_up"} == {RP.LINEAR, RP.NEAREST}
    # DB = 4 both ways: a source 4 bytes off, an up-lattice under HYGRID_UP=0 on both ops
    db4 = [c for c in RP.CASES if c.family == "hexdown" and c.plan()["DB"] == 4]
    assert any(c.align == 4 for c in db4)
    assert {c.op for c in db4 if c.env.get("HYGRID_UP") == "0"} == {RP.H2R, RP.RESIZE}
    # both ops on k_tri_up; f32 and f64, linear and nearest, every op on the backward
    assert {c.op for c in RP.CASES if c.family == "tri_up"} == {RP.H2R, RP.RESIZE}
    bw = {(c.op, c.in_dt, c.interp) for c in RP.CASES if c.family == "backward"}
    assert len(bw) == 12
    assert all(c.name in RP.BY_NAME for c in map(RP.BY_NAME.get, RP.PLACED)) and len(RP.PLACED) >= 4


def test_removing_the_last_case_of_a_region_is_noticed():
    """Without the only case of (k_tri_up linear bf16 -> f16 at K = 1, tail=2) the check fails,
    and it names that hole."""
    inst, region = ("k_tri_up", "linear", "bf16", "f16", "K1"), "tail=2"
    names = reached(RP.CASES)[(inst, region)]
    assert len(names) == 1
    assert missing([c for c in RP.CASES if c.name != names[0]]) == [(inst, region)]


FIELDS = ("kernel", "K", "pc", "chunks", "units")


@pytest.mark.parametrize("case", RP.CASES, ids=repr)
def test_plan_is_pinned(case):
    P = case.plan()
    assert case.name in PINNED, "a new case: pin its plan in tests/golden/resample_plane_plans.json"
    assert [P[f] for f in FIELDS] == PINNED[case.name], f"{case.name}: plan {P}"


def test_no_stale_pins():
    assert set(PINNED) == set(RP.BY_NAME)


# ---- hg_resample_plan's kernel == hg_resample_kernel ------------------------------------------
def older_shape_lists():
    """(op, in, out, planes, h, w, h1, w1, interp, env) over the shape lists of
    tests/test_gpu_stream.py, test_gpu_down.py, test_gpu_triup.py and test_gpu_hexdown.py
    (restated: those modules need a device to import)."""
    c = _abi.dtype_code
    f = {"f32": RP.F32, "bf16": RP.BF16, "f16": RP.F16}
    stream_r2h = [(7, 8, 7, 8), (8, 8, 8, 8), (16, 20, 16, 20), (33, 260, 33, 260),
                  (129, 516, 129, 516), (130, 1000, 130, 1000), (255, 256, 255, 256),
                  (64, 300, 65, 300), (90, 512, 91, 516), (90, 512, 91, 512), (90, 516, 91, 516)]
    stream_h2r = [(7, 8), (16, 20), (33, 260), (129, 516), (130, 1000), (255, 256), (2, 4)]
    pairs = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32"),
             ("f32", "bf16"), ("f32", "f16")]
    for i, o in pairs:
        for s in stream_r2h:
            yield (RP.R2H, c(f[i]), c(f[o]), 6) + s + (RP.LINEAR,)
        for h, w in stream_h2r:
            yield (RP.H2R, c(f[i]), c(f[o]), 6, h, w, h, w, RP.LINEAR)
    down = [(4, 8), (9, 22), (17, 40), (64, 66), (65, 130), (100, 1000), (256, 256), (512, 683),
            (130, 2050), (2160, 3840)]
    for h, w in down:
        yield (RP.R2H, c(RP.U8), c(RP.U8), 6, h, w, h // 2, w // 2, RP.NEAREST)
        for i in (RP.BF16, RP.F16, RP.I16):
            yield (RP.R2H, c(i), c(i), 2, h, w, h // 2, w // 2, RP.NEAREST)
        for i in (RP.BF16, RP.F16):
            for o in (RP.BF16, RP.F16, RP.F32):
                yield (RP.R2H, c(i), c(o), 6, h, w, h // 2, w // 2, RP.LINEAR)
    yield (RP.R2H, c(RP.BF16), c(RP.BF16), 6, 512, 683, 256, 341, RP.LINEAR)
    up = [(2, 2, 4, 4), (5, 10, 10, 19), (8, 12, 16, 23), (17, 40, 34, 80), (32, 34, 65, 67),
          (60, 100, 120, 200), (100, 1000, 200, 2000), (135, 240, 270, 480), (64, 128, 96, 192),
          (33, 260, 65, 520), (40, 96, 41, 97), (1080, 1920, 2160, 3840)]
    for op in (RP.H2R, RP.RESIZE):
        for s in up:
            for i in (RP.BF16, RP.F16, RP.F32):
                for o in (RP.BF16, RP.F16, RP.F32):
                    yield (op, c(i), c(o), 6) + s + (RP.LINEAR,)
            for e in (RP.U8, RP.BF16, RP.I32):
                yield (op, c(e), c(e), 6) + s + (RP.NEAREST,)
    hexdown = [(4, 4), (6, 10), (9, 22), (17, 40), (33, 124), (35, 126), (64, 66), (65, 130),
               (100, 1000), (128, 250), (256, 256), (270, 480), (540, 960), (4320, 7680)]
    strong = [(256, 1024, 64, 256), (256, 1024, 32, 128), (512, 2048, 32, 128), (130, 520, 26, 104),
              (64, 66, 4, 4), (33, 125, 16, 62)]
    for i in (RP.BF16, RP.F16):
        for o in (RP.BF16, RP.F16, RP.F32, RP.F64):
            for h, w in hexdown:
                yield (RP.RESIZE, c(i), c(o), 6, h, w, h // 2, w // 2, RP.LINEAR)
            for s in strong:
                yield (RP.RESIZE, c(i), c(o), 6) + s + (RP.LINEAR,)


SWITCHES = [{}, {"HYGRID_DOWN": "0"}, {"HYGRID_STREAM": "0"}, {"HYGRID_UP": "0"}]


def test_plan_kernel_equals_resample_kernel():
    n = 0
    calls = list(older_shape_lists()) + [
        (c.op, _abi.dtype_code(c.in_dt), _abi.dtype_code(c.out_dt), c.planes, c.h, c.w, c.h1, c.w1,
         c.interp) for c in RP.CASES if not c.backward]
    for env in SWITCHES:
        with RP.environ(env):
            for a in calls:
                k = _abi.lib().hg_resample_kernel(*a)
                if k < 0:
                    with pytest.raises(ValueError):
                        _abi.resample_plan(*a)
                    continue
                assert _abi.resample_plan(*a)["kernel"] == k, (a, env)
                n += 1
    assert n > 4000


def test_vacuous_shapes_of_the_older_files_route_where_the_issue_found_them():
    k = _abi.resample_kernel
    bf, f16, f32, u8 = (_abi.dtype_code(d) for d in (RP.BF16, RP.F16, RP.F32, RP.U8))
    for i, o in ((f32, f32), (bf, bf), (f16, f16), (bf, f32), (f16, f32), (f32, bf), (f32, f16)):
        assert k(RP.R2H, i, o, 6, 90, 512, 91, 516) == _abi.HG_KERNEL_GENERAL
        assert k(RP.R2H, i, o, 6, 90, 512, 91, 512) == _abi.HG_KERNEL_STREAM
        assert k(RP.R2H, i, o, 6, 90, 516, 91, 516) == _abi.HG_KERNEL_STREAM
        want = _abi.HG_KERNEL_DOWN if i in (bf, f16) else _abi.HG_KERNEL_STREAM
        assert k(RP.R2H, i, o, 6, 7, 8, 7, 8) == want and k(RP.R2H, i, o, 6, 8, 8, 8, 8) == want
    assert k(RP.R2H, u8, u8, 6, 4, 8, 2, 4, _abi.HG_NEAREST) == _abi.HG_KERNEL_NEAREST


def test_plan_query_validates_like_the_call():
    f32 = _abi.dtype_code(RP.F32)
    with pytest.raises(ValueError):
        _abi.resample_plan(7, f32, f32, 1, 8, 8, 8, 8)                       # no such op
    with pytest.raises(ValueError):
        _abi.resample_plan(RP.R2H, f32, _abi.HG_I32, 1, 8, 8, 8, 8)          # linear into ints
    with pytest.raises(ValueError):
        _abi.resample_plan(RP.R2H, _abi.HG_U8, f32, 1, 8, 8, 8, 8, RP.NEAREST)
    with pytest.raises(ValueError):
        _abi.resample_plan(RP.R2H, _abi.HG_F16, f32, 1, 8, 8, 8, 8, backward=True)
    with pytest.raises(ValueError):
        _abi.resample_plan(RP.R2H, f32, f32, 1, 8, 8, 8, 8, src_align=-1)
    assert _abi.lib().hg_resample_plan(RP.R2H, f32, f32, 1, 8, 8, 8, 8, 1, 0, 0, None) == _abi.HG_EINVAL
    # an empty call launches nothing: the kernel alone
    E = _abi.resample_plan(RP.H2R, f32, f32, 0, 8, 12, 5, 7)
    assert E["kernel"] == _abi.HG_KERNEL_GENERAL and E["pc"] == E["units"] == E["launched"] == 0
    # a 4-byte-aligned source: 4-byte pieces, narrower windows
    a = _abi.resample_plan(RP.RESIZE, _abi.HG_F16, _abi.HG_F16, 6, 96, 512, 48, 256)
    b = _abi.resample_plan(RP.RESIZE, _abi.HG_F16, _abi.HG_F16, 6, 96, 512, 48, 256, src_align=4)
    assert (a["DB"], b["DB"]) == (16, 4) and b["nout"] < a["nout"]
    # a 2-byte-aligned one: no LDS-DMA, the general kernel
    g = _abi.resample_plan(RP.RESIZE, _abi.HG_F16, _abi.HG_F16, 6, 96, 512, 48, 256, src_align=2)
    assert g["kernel"] == _abi.HG_KERNEL_GENERAL and g["lds"] == 1
