"""The case table of the pooling kernels (tests/pool_window_cases.py) reaches what it says it
reaches, checked without a device:

  (a) every case's route is the one the library's own query reports (hg_hex_pool2d_route, the
      host function that routes both real launches), every case lies in the regions it is filed
      under, and every region has a case for every method and type it claims;
  (b) the tied inputs are tied: in a tied region at least half of the windows of the integer
      planes hold their extreme twice or more (a condition on the inputs);
  (c) the checker of the GPU test is right on this kind of data: oracle.hex_pool2d /
      hex_pool2d_backward against torch's own autograd over a gather restatement of the
      operation, on every float64 case and all three methods: max / min exact, forward and
      backward; average within tests/test_gpu_pool.py's float64 bounds."""
import numpy as np
import pytest
import torch

import pool_window_cases as PW
from HyGrid import _abi
from oracle import oracle as O


# ---- (a) routes and regions -------------------------------------------------------------------
@pytest.mark.parametrize("case", PW.CASES, ids=repr)
def test_case_lies_in_its_regions(case):
    route = case.route()
    assert route == case.route(backward=True), "forward and backward share one threshold"
    assert route == (PW.LARGE if case.n >= 512 else PW.SMALL), (case.name, case.n, route)
    assert case.regions, "a case is filed under at least one region"
    for region in case.regions:
        assert PW.REGIONS[region](case, route), f"{case.name} is not in {region} (route {route})"
    assert 1 <= case.n <= PW.N_MAX, "an f16 count stays exact"
    x = PW.inputs(case)
    assert tuple(x.shape) == case.shape and x.numel() <= 1 << 16, "a tiny input"
    assert torch.equal(x.to(case.dtype).double().nan_to_num(7.0), x.nan_to_num(7.0)), \
        "the input holds values of its type"


def reached(cases):
    hit = {}
    for c in cases:
        route = c.route()
        for region in c.regions:
            assert region in PW.REGIONS, f"{c.name}: unknown region {region}"
            if PW.REGIONS[region](c, route):
                hit.setdefault((region, c.method, c.dtype), []).append(c.name)
    return hit


def missing(cases):
    hit = reached(cases)
    return sorted((region, m, PW.DT_NAME[dt]) for region, (methods, dtypes) in PW.CLAIMS.items()
                  for m in methods for dt in dtypes if (region, m, dt) not in hit)


def test_every_region_has_a_case_for_every_method_and_type():
    assert set(PW.CLAIMS) == set(PW.REGIONS)
    assert not missing(PW.CASES)
    # every data class on both routes, the threshold from both sides
    for region in ("small_n511", "large_n512", "large_n513", "large_n527", "large_n576",
                   "large_n600", "large_row", "large_const_pad", "large_reflect", "large_replicate",
                   "large_circular", "large_ext_zero", "large_ext_nan", "small_overlap",
                   "large_overlap"):
        assert region in PW.REGIONS
    for name in PW.DATA_REGIONS:
        assert f"small_{name}" in PW.REGIONS and f"large_{name}" in PW.REGIONS


def test_removing_the_last_case_of_a_region_is_noticed():
    """Without the only case of (large_n576, min, bf16) the check fails, and it names the hole."""
    key = ("large_n576", "min", PW.BF16)
    names = reached(PW.CASES)[key]
    assert len(names) == 1
    assert missing([c for c in PW.CASES if c.name != names[0]]) == [("large_n576", "min", "bf16")]


def test_route_query():
    assert _abi.hex_pool2d_route(1, 511) == _abi.HG_POOL_SMALL == PW.SMALL
    assert _abi.hex_pool2d_route(1, 512) == _abi.HG_POOL_LARGE == PW.LARGE
    assert _abi.hex_pool2d_route(16, 32, backward=True) == _abi.HG_POOL_LARGE
    assert _abi.hex_pool2d_route(23, 22, backward=True) == _abi.HG_POOL_SMALL
    assert _abi.hex_pool2d_route(0, 0) == _abi.HG_POOL_SMALL
    assert _abi.hex_pool2d_route(2 ** 31 - 1, 2 ** 31 - 1) == _abi.HG_POOL_LARGE    # no int overflow
    with pytest.raises(ValueError):
        _abi.hex_pool2d_route(-1, 4)
    assert _abi.lib().hg_hex_pool2d_route(3, -2, 0) == _abi.HG_EINVAL


# ---- (b) the tied data are tied ----------------------------------------------------------------
TIED_CASES = [c for c in PW.CASES if set(c.regions) & set(PW.TIED) and c.method != "average"
              and c.dtype == PW.F64]      # (the inputs are the same in every type)


@pytest.mark.parametrize("case", TIED_CASES, ids=repr)
def test_tied_inputs_are_tied(case):
    share = PW.tie_share(case)
    assert share >= 0.5, f"{case.name}: only {share:.2f} of the integer planes' windows are tied"
    # and the special planes are tied throughout (a constant pad value can be a window's only
    # extreme, so only where nothing is padded)
    if case.args[7] == 0:
        assert PW.tie_share(case, ("constant", "all_nan", "signed_zeros")) == 1.0


@pytest.mark.parametrize("case", [c for c in TIED_CASES if c.n >= 512], ids=repr)
def test_large_tied_inputs_need_the_trees_index_rule(case):
    """In every large tied case some window's first extreme sits in a higher thread of the LDS
    tree than a later one: only the merge's smaller-index rule finds it."""
    assert PW.tree_order_matters(case), case.name


def test_controls_are_tie_free():
    for c in PW.CASES:
        if c.data == "free" and c.method != "average":
            assert PW.tie_share(c, ("free",)) == 0.0, c.name


def test_const_planes_separate_a_rounded_count_from_an_exact_one():
    """The constant planes' values: at 257 and 527 valid elements a bf16 mean with the count
    rounded to bf16 differs from one with the exact count; at 511 and 513 no bf16 sum can show
    the difference (pool_window_cases.py, CONST_VALUES)."""
    def bf(v):
        return torch.as_tensor(v, dtype=torch.float64).to(torch.bfloat16).double()

    differs = {}
    for nv, values in PW.CONST_VALUES.items():
        for v in values:
            assert bf(v) == v and torch.tensor(v).to(torch.float16).double() == v
            s = bf(v * nv)
            differs.setdefault(nv, []).append(bool(bf(s / bf(float(nv))) != bf(s / nv)))
    assert all(differs[257]) and differs[527] == [False, True]
    assert not any(differs[511]) and not any(differs[513])
    assert [float(bf(float(n))) for n in (257, 511, 513, 527)] == [256.0, 512.0, 512.0, 528.0]


# ---- (c) the oracle against torch autograd on the table's own data -----------------------------
F64_CASES = [c for c in PW.CASES if c.dtype == PW.F64]


@pytest.mark.parametrize("case", F64_CASES, ids=repr)
def test_oracle_agrees_with_torch_autograd(case):
    x = case.raster(PW.inputs(case))
    gy = case.out(PW.grad_output(case))
    xt = x.clone().requires_grad_(True)
    yt = PW.pool_torch(xt, case.args)
    yt.backward(gy)
    y = O.hex_pool2d(x.numpy(), *case.args)
    dx = O.hex_pool2d_backward(x.numpy(), gy.numpy(), *case.args)
    if case.method == "average":
        np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-13, atol=1e-13)
    else:
        np.testing.assert_array_equal(y, yt.detach().numpy())
        np.testing.assert_array_equal(dx, xt.grad.numpy())
        assert np.array_equal(np.isnan(y), np.isnan(yt.detach().numpy()))


def test_all_three_methods_are_validated_on_every_float64_geometry():
    seen = {(c.geom, c.data, c.method) for c in F64_CASES}
    for geom in PW.GEOMS:
        for m in PW.METHODS:
            assert (geom, "mixed", m) in seen
