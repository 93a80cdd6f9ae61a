"""The guard-band harness (tests/placement.py) and its case table (tests/placement_cases.py),
checked without a device:

  * the harness detects what it claims to: a store one element before a view, one element after
    it, an interior element never written; a well-behaved op passes;
  * completeness: every hg_* export of include/hygrid.h with a destination pointer is covered by
    a case or exempt with a written reason, and every resample / pyramid kernel route is reached;
  * every tensor a case places gets at least 4 KiB and two rows of guard on each side;
  * each case's shape takes the kernel its entry names (the library's host-side queries)."""
import os
import re

import pytest
import torch

import placement as P
import placement_cases as PC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hygrid.h")
DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.uint8, torch.int32]


# ---- the harness ------------------------------------------------------------------------------
def _good_op(dst):
    dst.copy_(torch.arange(dst.numel(), dtype=torch.float32).view(dst.shape).to(dst.dtype) % 100)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_well_behaved_op_passes(dtype, offset):
    view, flat = P.arena((3, 5, 7), dtype, "cpu", offset)
    es = flat.element_size()
    assert view.is_contiguous() and view.shape == (3, 5, 7)
    assert (view.data_ptr() - flat.data_ptr()) % P.BASE_ALIGN == (offset * es) % P.BASE_ALIGN
    assert P.sentinel_count(view) == view.numel()          # the interior starts as sentinel too
    _good_op(view)
    assert P.guards_intact(flat, view)
    assert P.sentinel_count(view) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_one_element_before_the_view_is_caught(dtype):
    view, flat = P.arena((4, 6), dtype, "cpu", 2)
    es = flat.element_size()
    _good_op(view)
    start = (view.data_ptr() - flat.data_ptr()) // es
    flat[start - 1] = 1
    with pytest.raises(AssertionError, match=rf"before the view: first at -{es}, last at -1 "):
        P.guards_intact(flat, view)


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_one_element_after_the_view_is_caught(dtype):
    view, flat = P.arena((4, 6), dtype, "cpu", 1)
    es = flat.element_size()
    _good_op(view)
    start = (view.data_ptr() - flat.data_ptr()) // es
    flat[start + view.numel()] = 1
    with pytest.raises(AssertionError, match=rf"after the view: first at \+0, last at \+{es - 1} "):
        P.guards_intact(flat, view)


def test_single_damaged_byte_far_out_is_caught_and_located():
    view, flat = P.arena((4, 6), torch.float32, "cpu")
    _good_op(view)
    lead, trail = P.guard_gaps(flat, view)
    raw = flat.view(torch.uint8)
    raw[0] ^= 0xFF                       # the first byte of the arena
    raw[-1] ^= 0x01                      # the last one
    with pytest.raises(AssertionError) as e:
        P.guards_intact(flat, view)
    assert f"first at -{lead}, last at -{lead}" in str(e.value)
    assert f"first at +{trail - 1}, last at +{trail - 1}" in str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_interior_element_is_caught(dtype):
    view, flat = P.arena((4, 6), dtype, "cpu", 1)
    keep = view[2, 3].clone()
    _good_op(view)
    view[2, 3] = keep                    # the op skipped one element
    assert P.guards_intact(flat, view)
    assert P.sentinel_count(view) == 1
    assert P.sentinel_mask(view).nonzero().tolist() == [[2, 3]]
    if dtype.is_floating_point:          # and it reads as a NaN in the result
        assert torch.isnan(view.float()).sum() == 1


def test_guard_nan_reaches_arithmetic_even_with_weight_zero():
    view, flat = P.arena((8,), torch.float32, "cpu", guard_elems=None)
    view.fill_(1.0)
    start = (view.data_ptr() - flat.data_ptr()) // 4
    assert torch.isnan(0.0 * flat[start - 1] + view[0])


def test_guard_floor_is_enforced():
    with pytest.raises(ValueError):
        P.arena((4, 6), torch.float32, "cpu", guard_elems=16)


# ---- placed(): the allocation routing -----------------------------------------------------------
def test_placed_routes_result_allocations_and_checks_guards(monkeypatch):
    with P.placed(monkeypatch, 3, device_types=("cpu",)) as rec:
        a = torch.empty((4, 5), dtype=torch.float32, device="cpu")
        b = torch.zeros(2, 3, dtype=torch.int32, device="cpu")
        c = torch.empty_like(a)
        d = torch.empty(7, dtype=torch.float32, device="cpu")          # 1-D: passes through
        e = torch.empty((4, 5), dtype=torch.float32, device="cpu", requires_grad=True)
        a.fill_(1)
        c.fill_(2)
    assert len(rec.arenas) == 3
    assert all(rec.arena_of(t) is not None for t in (a, b, c))
    assert rec.arena_of(d) is None and rec.arena_of(e) is None
    flat, view = rec.arena_of(a)
    assert (view.data_ptr() - flat.data_ptr()) // 4 == P.default_guard_elems((4, 5), torch.float32) + 3
    assert int(b.sum()) == 0 and P.sentinel_count(b) == 0              # zeros are zeros
    assert torch.empty is P._EMPTY and torch.zeros is P._ZEROS         # restored on exit
    assert torch.empty_like is P._EMPTY_LIKE


def test_placed_offset_function_and_min_dim(monkeypatch):
    off = lambda dtype, ndim: 0 if ndim < 2 else 16 // torch.empty((), dtype=dtype).element_size()  # noqa: E731
    with P.placed(monkeypatch, off, device_types=("cpu",), min_dim=1) as rec:
        ws = torch.empty(100, dtype=torch.uint8, device="cpu")
        y = torch.empty((2, 3), dtype=torch.bfloat16, device="cpu")
        ws.fill_(0)
        y.fill_(0)
    (fa, va), (fb, vb) = rec.arenas
    assert (va.data_ptr() - fa.data_ptr()) % 256 == 0
    assert (vb.data_ptr() - fb.data_ptr()) % 256 == 16


def test_placed_fails_an_op_that_overruns(monkeypatch):
    def bad_op():
        y = torch.empty((4, 6), dtype=torch.float32, device="cpu")
        y.fill_(0)
        flat, view = rec.arena_of(y)
        start = (view.data_ptr() - flat.data_ptr()) // 4
        flat[start + view.numel()] = 0          # one element past the end
        return y

    with pytest.raises(AssertionError, match=r"after the view: first at \+0, last at \+3 "):
        with P.placed(monkeypatch, 1, device_types=("cpu",)) as rec:
            bad_op()
    assert torch.empty is P._EMPTY


# ---- the case table ---------------------------------------------------------------------------
def exports_with_destination():
    """hg_* functions of the header with a pointer the library writes through: any pointer
    parameter that is not const-qualified data, the stream handle aside."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(hg_\w+)\s*\(([^)]*)\)", src):
        dests = []
        for p in params.split(","):
            p = " ".join(p.split())
            if "*" not in p or p.startswith("const "):
                continue
            if p.split()[-1].lstrip("*") == "stream":
                continue
            dests.append(p)
        out[name] = dests
    return out


def test_header_parse_sees_the_known_destinations():
    ex = exports_with_destination()
    assert ex["hg_rect_to_hex"] == ["void* dst"]
    assert ex["hg_hexconv2d_backward"] == ["void* dx", "void* dkernel", "void* dbias"]
    assert ex["hg_hex_pyramid_chain"] == ["void* const* ys", "void* workspace"]
    assert ex["hg_resample_kernel"] == [] and ex["hg_abi_version"] == []
    from HyGrid import _abi
    assert set(ex) == set(_abi.SIGNATURES)


def test_every_export_with_a_destination_is_covered_or_exempt():
    ex = exports_with_destination()
    need = {n for n, d in ex.items() if d}
    covered = {e for c in PC.CASES for e in c.exports}
    assert covered <= need, f"cases name exports without a destination: {sorted(covered - need)}"
    assert set(PC.EXEMPT) <= need and not set(PC.EXEMPT) & covered
    assert all(len(reason) > 20 for reason in PC.EXEMPT.values())
    left_out = need - covered - set(PC.EXEMPT)
    assert not left_out, f"exports left out without a reason: {sorted(left_out)}"


def test_every_kernel_route_is_reached():
    """The queries say which kernel a shape runs: all five resample routes for the ops that
    have them, all four pyramid level kernels."""
    routes = {}
    for c in PC.CASES:
        if c.route is not None:
            want = c.route()[0]
            routes.setdefault(c.exports[-1], set()).update(want if isinstance(want, tuple) else (want,))
    assert routes["hg_rect_to_hex"] == {PC.GENERAL, PC.NEAREST, PC.STREAM, PC.DOWN}
    assert routes["hg_hex_to_rect"] == {PC.GENERAL, PC.NEAREST, PC.STREAM, PC.UP}
    assert routes["hg_hexresize"] == {PC.GENERAL, PC.DOWN, PC.UP}
    assert routes["hg_hex_pyramid_level"] == {PC.PYR_FUSED, PC.PYR_FUSED_SHORT, PC.PYR_STREAM,
                                              PC.PYR_LDS}


@pytest.mark.parametrize("case", PC.CASES, ids=repr)
def test_case_guards_routes_and_citation(case, monkeypatch):
    # at least 4 KiB and two rows of sentinel on each side of every placed tensor
    tensors = case.placed_tensors()
    assert tensors, "a case places at least its destination"
    for shape, dtype in tensors:
        for off in (0, 1):
            view, flat = P.arena(shape, dtype, "cpu", off)
            es = flat.element_size()
            lead, trail = P.guard_gaps(flat, view)
            floor = max(4096, 2 * shape[-1] * es)
            assert lead >= floor and trail >= floor, (shape, dtype, lead, trail)
    # the outputs line up with the comparisons
    assert len(case.outs) == len(case.cmp)
    assert all(i < len(case.outs) for i in case.atomic)
    # the shape runs the kernel the entry names
    if case.route is not None:
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        want, got = case.route()
        assert got in want if isinstance(want, tuple) else got == want, (want, got)
    # the sibling whose tolerance the case borrows exists
    path, test = case.sibling.split("::")
    assert re.search(rf"^def {test}\(", open(os.path.join(ROOT, path)).read(), flags=re.M), case.sibling


def test_every_source_has_batch_two():
    for c in PC.CASES:
        inp = c.inputs()
        for k in c.placed:
            assert inp[k].shape[0] >= 2 or c.name == "chain_bwd_two_weight_bands", (c.name, k)
