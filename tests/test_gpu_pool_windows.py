"""GPU: the pooling kernels (csrc/pool.hip) on tied, quantised and large-window inputs: the case
table of tests/pool_window_cases.py (tests/test_pool_window_cases_cpu.py shows on the CPU that the
table reaches what it claims and that the oracle agrees with torch autograd on this data).

Every case asserts the kernel pair it ran on (hg_hex_pool2d_route) and goes through the public
modules.  Inputs hold values every one of the four types represents exactly.

max / min, forward and backward: EXACT against the fp64 oracle in every type.  The upstream
gradient holds whole numbers in -8..8, so every partial sum is exact in float32 in any order
(atomics, overlapping windows), dx survives its rounding to a 16-bit type, and a gradient sent
to the second of two tied elements is an error of a whole number.

average, f64 / f32: against the oracle at tests/test_gpu_pool.py::test_pool_random_vs_oracle's
bounds (forward 1e-14 / 2e-6, gradient 1e-13 / 1e-5, rtol = atol).

average, bf16 / f16, forward: against a model of the reference's arithmetic (model_average).  The
reference's average_pooling builds the count and the sum as tensors of the input type T and
divides them, so with round_T the rounding to T:
        y = round_T( round_T(sum of the non-NaN values) / round_T(their count) ),  NaN for count 0
(pool.hip's pool_result; the fp64 oracle does not model the rounded count).  The sum is taken in
float64 here: the kernels accumulate in f32 / f64 and the reference in T's own accumulation
order, which the bound covers.  The bound is test_pool_random_vs_oracle's, 1.6e-2 for bf16 and
2e-3 for f16 (rtol = atol).  These are LOOSE against the effect under test: a count of 527 that
bf16 rounds to 528 moves the mean by 0.19 %, a count of 257 rounded to 256 by 0.39 %.  So on
the constant planes ("const" data: value v on n_valid elements of a plane's one window, NaN on
the rest; n_valid 257, 511, 513 and 527) the result must EQUAL the model's in every type: 1 for
v = 1, and at n_valid 527 and 257 values at which an unrounded count gives another bf16 number
(at 511 and 513 no bf16 sum can show the difference, tests/pool_window_cases.py CONST_VALUES).
The gradient of a 16-bit average is round_T(round_T(gy) / round_T(count)) per non-NaN element
(the reference divides tensors of type T); checked exactly on the constant planes, and against
the oracle at test_pool_random_vs_oracle's gradient bounds (3e-2 / 4e-3) elsewhere.

Every window holds at most 2048 elements, so an f16 count is exact and nothing overflows.  (An
f16 count above 65504 overflows in the reference as well: faithful, and out of scope here.)

Batch independence: planes of a case equal their single-plane calls bit for bit (forward; the
max / min backward as well), on both routes."""
import functools

import numpy as np
import pytest
import torch

import pool_window_cases as PW
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import _abi  # noqa: E402

DEV = torch.device("cuda:0")
Y_TOL = {PW.F64: 1e-14, PW.F32: 2e-6, PW.BF16: 1.6e-2, PW.F16: 2e-3}     # test_pool_random_vs_oracle
G_TOL = {PW.F64: 1e-13, PW.F32: 1e-5, PW.BF16: 3e-2, PW.F16: 4e-3}
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
WORST = {}      # (region, "y" | "dx") -> worst |err| / tolerance of the average cases


def _round(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()


@functools.lru_cache(maxsize=None)
def _reference(geom, data, method):
    """(x, gy, oracle forward, oracle backward) of a (geometry, data, method): the inputs are
    the same in every type, so one reference serves the four of them.  Left unchanged."""
    case = PW.Case(geom, data, method, PW.F64, ())
    x, gy = PW.inputs(case), PW.grad_output(case)
    xo, go = case.raster(x).numpy(), case.out(gy).numpy()
    return x, gy, O.hex_pool2d(xo, *case.args), O.hex_pool2d_backward(xo, go, *case.args)


def model_average(case, x, gy):
    """(y, dx) of the reference's arithmetic in case.dtype (module docstring), as float64."""
    T = case.dtype
    g = PW.gather(case.raster(x), case.args)
    nan = g.isnan()
    with np.errstate(invalid="ignore", divide="ignore"):
        count = _round((~nan).sum(-1).double().numpy(), T)
        total = _round(torch.where(nan, torch.zeros_like(g), g).sum(-1).numpy(), T)
        y = _round(total / count, T)
        gs = _round(_round(case.out(gy).numpy(), T) / count, T)
    y[count == 0] = np.nan
    gs[count == 0] = 0.0
    # every non-NaN element of a window receives the window's gs (summed in float64: exact
    # where an element lies in one window, as on the constant planes)
    xr = case.raster(x).clone().requires_grad_(True)
    gr = PW.gather(xr, case.args)
    torch.where(gr.isnan(), torch.zeros_like(gr), gr).mul(torch.from_numpy(gs).unsqueeze(-1)).sum().backward()
    return y, torch.where(case.raster(x).isnan(), torch.zeros_like(xr.grad), xr.grad).numpy()


def _ratio(got, ref, tol):
    """Worst |got - ref| / (tol + tol |ref|) over the finite references; the rest must match
    as NaN / infinity (assert_allclose's own rule)."""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / (tol + tol * np.abs(ref[fin]))).max())


def _record(case, what, ratio):
    for region in case.regions:
        WORST[(region, what)] = max(WORST.get((region, what), 0.0), ratio)


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()]).cpu()


def _run(case, x):
    """(y, dx) on the device for the input x (float64 CPU values of case.dtype)."""
    xr = x.to(case.dtype).to(DEV).requires_grad_(True)
    y = case.apply(xr)
    return xr, y


@pytest.mark.parametrize("case", PW.CASES, ids=repr)
def test_case(case):
    route = case.route()
    assert route == case.route(backward=True) == (PW.LARGE if case.n >= 512 else PW.SMALL)
    assert all(r.startswith(("small_", "large_")) and r.startswith("small_") == (route == PW.SMALL)
               for r in case.regions), "the case ran on the kernels its regions name"
    x, gy, yref, dref = _reference(case.geom, case.data, case.method)
    xr, y = _run(case, x)
    assert y.dtype == case.dtype
    y.backward(gy.to(case.dtype).to(DEV))
    torch.cuda.synchronize()
    assert xr.grad.dtype == case.dtype
    got = case.out(y.detach()).double().cpu().numpy()
    dx = case.raster(xr.grad).double().cpu().numpy()
    if case.method != "average":
        np.testing.assert_array_equal(got, yref)                       # exact in every type
        np.testing.assert_array_equal(dx, dref)
        return
    sixteen = case.dtype in (PW.BF16, PW.F16)
    if sixteen or case.data == "const":
        ymodel, dmodel = model_average(case, x, gy)
    yr = _ratio(got, ymodel if sixteen else yref, Y_TOL[case.dtype])
    dr = _ratio(dx, dref, G_TOL[case.dtype])
    print(f"{case.name}: route {route} forward |err|/tol {yr:.3g} gradient |err|/tol {dr:.3g}")
    _record(case, "y", yr)
    _record(case, "dx", dr)
    assert yr <= 1.0, f"{case.name}: forward {yr:.3g} x the tolerance {Y_TOL[case.dtype]}"
    assert dr <= 1.0, f"{case.name}: gradient {dr:.3g} x the tolerance {G_TOL[case.dtype]}"
    if case.data == "const":
        # the constant planes: the reference's arithmetic to the bit, in every type
        np.testing.assert_array_equal(got, ymodel)
        np.testing.assert_array_equal(dx, dmodel)
        cp = PW.const_planes(case.n)
        ones = [p for p in range(got.size) if cp[p % len(cp)][0] == 1.0]
        assert ones and (got.reshape(-1)[ones] == 1.0).all(), "T(T(n) / T(n)) = 1"


def _planes(case):
    a, b = case.lead
    n = a * b
    return sorted({0, n - 1, 2, sum(map(ord, case.name)) % n})


@pytest.mark.parametrize("case", [c for c in PW.CASES if c.data != "const"], ids=repr)
def test_plane_equals_its_single_plane_call(case):
    x, gy, _, _ = _reference(case.geom, case.data, case.method)
    xr, y = _run(case, x)
    exact_bwd = case.method != "average"        # float atomics of an average: order-dependent
    if exact_bwd:
        y.backward(gy.to(case.dtype).to(DEV))
    b = case.lead[1]
    for p in _planes(case):
        i, j = divmod(p, b)
        x1r, y1 = _run(case, x[i:i + 1, j:j + 1])
        assert torch.equal(_bits(y1.detach()).reshape(-1), _bits(y.detach()[i:i + 1, j:j + 1]).reshape(-1)), \
            f"{case.name}: plane {p} differs from its single-plane call"
        if exact_bwd:
            y1.backward(gy[i:i + 1, j:j + 1].to(case.dtype).to(DEV))
            assert torch.equal(_bits(x1r.grad).reshape(-1), _bits(xr.grad[i:i + 1, j:j + 1]).reshape(-1)), \
                f"{case.name}: plane {p}'s gradient differs from its single-plane call"


def test_route_query_is_host_only():
    """hg_hex_pool2d_route takes no pointer and no stream: nothing to launch or to write."""
    assert _abi.lib().hg_hex_pool2d_route(16, 32, 0) == _abi.HG_POOL_LARGE
    assert _abi.lib().hg_hex_pool2d_route(1, 511, 1) == _abi.HG_POOL_SMALL


def test_zz_report():
    """Prints the worst |err| / tolerance per region of the average cases (run with -s); the
    max / min cases are exact."""
    if not WORST:
        return
    print("\nregion: worst |err| / tolerance, average forward, gradient (max / min: exact)")
    for region in sorted({r for r, _ in WORST}):
        print(f"  {region:28s} {WORST.get((region, 'y'), 0.0):8.3g} {WORST.get((region, 'dx'), 0.0):8.3g}")
    assert max(WORST.values()) <= 1.0
