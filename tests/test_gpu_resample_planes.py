"""GPU parity of the resamplers' plane loops: the case table of tests/resample_plane_cases.py
(many tiny planes, pc forced through the launch switches; tests/test_resample_plane_cases_cpu.py
proves on the host which loop each case reaches).

Per case, with different random data in every plane:
  * every plane against the fp64 oracle (oracle/hg_oracle.c, pinned to the reference by
    tests/golden) at the tolerance the kernel's own parity file uses: nearest exactly; fp32
    outputs rtol 1e-5 with atol 1e-5 max|ref|; bf16 / f16 outputs max|err| <= 2^-8 / 2^-11 max|ref|
    (one output rounding); the backward 1e-12 (f64) / 1e-5 (f32) likewise;
  * bit-identical to the general kernels (HYGRID_DOWN=0 / HYGRID_STREAM=0);
  * bit-identical to single-plane calls on a sample of planes (first, last, both sides of a chunk
    boundary, the ragged chunk);
  * NaN / Inf planted in the last plane of a chunk and the first of the next reach exactly the
    outputs they reach in the general kernel (forward) and stay in their planes;
  * for one ragged-chunk case per instantiation family, the output placed between guard bands
    (tests/placement.py): guards intact, no element left unwritten.
A mismatch here is a finding about a counted wait or a chunk bound, not noise: the kernels are
deterministic."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only with -m gpu
    pytest.skip("needs a HIP device", allow_module_level=True)

import placement as PL  # noqa: E402
import resample_plane_cases as RP  # noqa: E402
from HyGrid import _abi, ops  # noqa: E402

DEV = torch.device("cuda:0")
ORACLE = {RP.R2H: (O.rect_to_hex, O.rect_to_hex_backward), RP.H2R: (O.hex_to_rect, O.hex_to_rect_backward),
          RP.RESIZE: (O.hexresize, O.hexresize_backward)}
WORST = {}          # family -> worst |err| / tolerance, printed per test (pytest -s / -rA)


def _device_source(c):
    """The case's source on the device, c.align bytes past a 16-byte boundary."""
    x = RP.inputs(c)
    if not c.align:
        return x.to(DEV)
    es = x.element_size()
    assert c.align % es == 0
    flat = torch.empty(x.numel() + c.align // es, dtype=x.dtype, device=DEV)
    v = flat[c.align // es:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == c.align
    return v


def _run(c, x, env=None):
    fn = getattr(ops, RP.OP_NAME[c.op])
    with RP.environ(c.env if env is None else env):
        y = fn(x, (c.h1, c.w1), interp=c.interp, out_dtype=c.out_dt)
        torch.cuda.synchronize()
    return y


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype
    bad = (_bits(a) != _bits(b)).flatten(1).any(dim=1)
    assert not bool(bad.any()), f"planes {torch.nonzero(bad).view(-1).tolist()[:16]} differ from {what}"


def _ratio(c, got, ref, interp, dt):
    """worst |err| / tolerance over all planes (<= 1 passes), at the sibling file's tolerance."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64).reshape(got.shape)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    if interp == RP.NEAREST and not c.backward:
        return 0.0 if np.array_equal(got, ref) else np.inf
    if dt in (RP.BF16, RP.F16):
        return float(err.max() / ((2.0 ** -8 if dt == RP.BF16 else 2.0 ** -11) * scale))
    tol = 1e-12 if dt == RP.F64 else 1e-5
    return float((err / (tol * scale + tol * np.abs(ref))).max())


def _note(c, r):
    WORST[c.family] = max(WORST.get(c.family, 0.0), r)
    print(f"{c.name}: worst |err| / tolerance {r:.3f} (family {c.family}: {WORST[c.family]:.3f})")


FORWARD = [c for c in RP.CASES if not c.backward]
BACKWARD = [c for c in RP.CASES if c.backward]


@pytest.mark.parametrize("case", FORWARD, ids=repr)
def test_forward_planes(case):
    c, P = case, case.plan()
    assert P["kernel"] == RP.FAMILY_KERNEL[c.family], P
    x = _device_source(c)
    y = _run(c, x)
    assert y.shape == (c.planes, c.h1, c.w1) and y.dtype == c.out_dt
    # every plane against the oracle
    ref = ORACLE[c.op][0](x.double().cpu().numpy(), (c.h1, c.w1), c.interp)
    r = _ratio(c, y.double().cpu().numpy(), ref, c.interp, c.out_dt)
    _note(c, r)
    assert r <= 1.0, f"{c.name}: |err| / tolerance {r}"
    # the general kernel
    if c.family in RP.GENERAL_SWITCH:
        genv = dict(c.env, **RP.GENERAL_SWITCH[c.family])
        assert c.plan(genv)["kernel"] in (RP.GENERAL, RP.NEAR_K)
        _same_bits(y, _run(c, x, genv), "the general kernel")
    # single-plane calls
    sample = RP.sample_planes(c, P)
    assert {0, c.planes - 1} <= set(sample)
    for p in sample:
        one = _run(c, x[p:p + 1], {})
        assert bool((_bits(one[0]) == _bits(y[p])).all()), f"plane {p} differs from its single-plane call"
    # NaN / Inf in the last plane of a chunk and the first plane of the next
    if c.in_dt.is_floating_point and c.planes > P["pc"]:
        x2 = x.clone() if not c.align else _device_source(c)
        pa, pb = P["pc"] - 1, P["pc"]
        last0 = (P["chunks"] - 1) * P["pc"]
        x2[pa, 0, 0] = float("nan")
        x2[pa, c.h - 1, c.w - 1] = float("inf")
        x2[pb, c.h // 2, c.w // 2] = float("nan")
        x2[pb, 0, c.w - 1] = float("-inf")
        x2[last0, c.h - 1, 0] = float("nan")
        y2 = _run(c, x2)
        touched = sorted({pa, pb, last0})
        if c.family in RP.GENERAL_SWITCH:
            _same_bits(y2, _run(c, x2, dict(c.env, **RP.GENERAL_SWITCH[c.family])),
                       "the general kernel (non-finite inputs)")
        else:
            for p in touched:
                one = _run(c, x2[p:p + 1], {})
                assert bool((_bits(one[0]) == _bits(y2[p])).all()), f"non-finite plane {p}"
        ref2 = ORACLE[c.op][0](x2[touched].double().cpu().numpy(), (c.h1, c.w1), c.interp)
        got2 = y2[touched].double().cpu().numpy()
        assert np.array_equal(np.isfinite(got2), np.isfinite(ref2.reshape(got2.shape))), \
            "non-finite outputs are not where the oracle has them"
        keep = torch.ones(c.planes, dtype=torch.bool, device=DEV)
        keep[touched] = False
        _same_bits(y2[keep], y[keep], "the run without NaN / Inf (other planes)")


@pytest.mark.parametrize("case", BACKWARD, ids=repr)
def test_backward_planes(case):
    c, P = case, case.plan()
    assert P["kernel"] == RP.BACKWARD and P["pc"] in (2, 3) and c.planes % P["pc"]
    gy = RP.inputs(c).to(DEV)
    dx = torch.empty((c.planes, c.h, c.w), dtype=c.in_dt, device=DEV)
    st = _abi.lib().hg_resample_backward(c.op, _abi.ptr(gy), _abi.ptr(dx), _abi.dtype_code(c.in_dt),
                                         c.planes, c.h, c.w, c.h1, c.w1, c.interp, _abi.stream_of(gy))
    _abi.check(st, "hg_resample_backward")
    torch.cuda.synchronize()
    ref = ORACLE[c.op][1](gy.double().cpu().numpy(), (c.h, c.w), c.interp)
    r = _ratio(c, dx.double().cpu().numpy(), ref, c.interp, c.in_dt)
    _note(c, r)
    assert r <= 1.0, f"{c.name}: |err| / tolerance {r}"


@pytest.mark.parametrize("name", RP.PLACED)
def test_ragged_chunk_output_between_guards(name, monkeypatch):
    c = RP.BY_NAME[name]
    P = c.plan()
    assert P["chunks"] >= 2 and c.planes % P["pc"], "a ragged last chunk"
    x = _device_source(c)
    want = _run(c, x)
    for offset in (0, 1):
        with PL.placed(monkeypatch, offset) as rec:
            y = _run(c, x)
        assert rec.arena_of(y) is not None, "the result was not placed"
        # (the integer sentinel byte 0xA5 is also a value the random u8 data holds: as many as
        # the unplaced result has; the float sentinel is a NaN payload no result has)
        legit = 0 if c.out_dt.is_floating_point else PL.sentinel_count(want)
        assert PL.sentinel_count(y) == legit, "output elements never written"
        _same_bits(y, want, f"the unplaced run (offset {offset})")


def test_plan_query_launches_nothing():
    """hg_resample_plan is host-only: its answer slot is host memory and no stream is involved."""
    out = (ctypes.c_int * len(_abi.RESAMPLE_PLAN_FIELDS))()
    assert _abi.lib().hg_resample_plan(RP.H2R, _abi.HG_BF16, _abi.HG_BF16, 96, 8, 12, 16, 24, 1,
                                       0, 0, out) == 0
    assert out[0] == _abi.HG_KERNEL_UP
