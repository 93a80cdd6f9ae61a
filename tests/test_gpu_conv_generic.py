"""GPU parity of the generic HexConv2d kernels (csrc/hexconv.hip: k_hexconv with its
channel-chunk, output-channel-block and batch loops; k_hexconv_direct) at wide channels, against
the fp64 oracle (oracle/hg_oracle.c) on the inputs as rounded to their dtypes.

The cases are tests/conv_generic_cases.py; tests/test_conv_generic_cases_cpu.py pins without a
device that each one reaches the loop it is filed under and that no other kernel takes it.

Tolerances are the project's own, per (weight, output) dtype:
    f32 weights, f32 output   rtol 1e-5, atol 1e-5 max|ref|   (tests/test_gpu_parity.py::close)
    bf16 / f16 output         2^-8 / 2^-11 the same way
    f64 weights, f64 output   rtol 1e-12, atol 1e-12 max|ref|
    gradients                 rtol 1e-4, atol 1e-5 max|ref|   (tests/test_gpu_backward.py::close);
                              f64 weights: d x 1e-12, d kernel / d bias 1e-10
                              (test_backward_bf16_input_and_fp64_kernel)
Each comparison prints its worst error as a fraction of the tolerance (pytest -s shows it)."""
import functools
import os

import numpy as np
import pytest
import torch

import conv_generic_cases as CG

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import ops  # noqa: E402

DEV = torch.device("cuda:0")
OUT_TOL = {CG.F32: 1e-5, CG.BF16: 2.0 ** -8, CG.F16: 2.0 ** -11, CG.F64: 1e-12}


def close(got, ref, rtol, what, atol_rel=None):
    """assert_allclose(rtol, atol = atol_rel max|ref|), atol_rel = rtol unless given; prints the
    worst |err| / (atol + rtol |ref|)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = (rtol if atol_rel is None else atol_rel) * max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    ratio = float((err / (atol + rtol * np.abs(ref))).max())
    print(f"{what}: worst |err| / tolerance {ratio:.3f} (max err {err.max():.3e}, "
          f"max|ref| {np.abs(ref).max():.3e}, rtol {rtol:.1e})")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)


class _env:
    """The A/B switches of a case around a call (tests/test_gpu_conv_mfma.py::_generic)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _dev(t):
    return None if t is None else t.to(DEV)


def run_forward(case, t, x=None):
    x = _dev(t["x"]) if x is None else x
    epi = None
    if case.epi is not None:
        epi = (_dev(t["scale"]), _dev(t["shift"]), case.epi[2], case.epi[3])
    with _env(case.env()):
        return ops.hexconv2d(x, _dev(t["k"]), _dev(t["b"]), case.off, case.r, case.s, case.p,
                             case.d, case.g, case.mode, case.pv, out_dtype=case.y_dt, epilogue=epi)


@functools.lru_cache(maxsize=None)
def forward_data(name):
    """(inputs, fp64 reference) of a case, computed once and left unchanged."""
    case = CG.BY_NAME[name]
    t = case.inputs()
    ref = CG.reference(case, t)
    ref.setflags(write=False)
    return t, ref


@pytest.mark.parametrize("case", CG.CASES, ids=repr)
def test_forward_vs_oracle(case):
    t, ref = forward_data(case.name)
    y = run_forward(case, t)
    assert y.dtype == case.y_dt and tuple(y.shape) == ref.shape
    if case.w_dt == CG.F64:
        assert case.y_dt == CG.F64, "f64 weights are compared at the f64 tolerance"
    close(y.double().cpu().numpy(), ref, OUT_TOL[case.y_dt], f"{case.name} [{'+'.join(case.regions)}]")


@pytest.mark.parametrize("case", [c for c in CG.CASES if c.spatial == "one"], ids=repr)
def test_batch_loop_images_bit_identical_to_single_calls(case):
    """Image b of the batched call (several images per workgroup, tile re-staged per image)
    equals the one-image call on image b bit for bit: the first image, one in the middle of a
    workgroup's range and the last one, which sits in the short last workgroup."""
    P = case.plan()
    bc = P["bc"]
    assert bc >= 2 and case.B % bc
    t, _ = forward_data(case.name)
    x = _dev(t["x"])
    y = run_forward(case, t)
    mid = (case.B // (2 * bc)) * bc + bc // 2      # not the first image of its workgroup
    assert mid % bc != 0 and 0 < mid < case.B - 1
    for b in (0, mid, case.B - 1):
        one = run_forward(case, t, x[b:b + 1].contiguous())
        assert torch.equal(y[b:b + 1], one), f"{case.name}: image {b} (workgroup {b // bc}, bc {bc})"


# ---- backward ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backward_data(name):
    case = CG.BY_NAME[name]
    t = case.inputs(positive=True)
    ref = CG.reference_backward(case, t)
    for r in ref:
        r.setflags(write=False)
    return t, ref


def grads_close(case, got, ref, what):
    for g, r, part in zip(got, ref, ("dx", "dkernel", "dbias")):
        if g is None:
            continue
        g = g.double().cpu().numpy().reshape(r.shape)
        if case.w_dt == CG.F64:
            tol = 1e-12 if part == "dx" else 1e-10
            close(g, r, tol, f"{what} {part}")
        else:
            close(g, r, 1e-4, f"{what} {part}", atol_rel=1e-5)


@pytest.mark.parametrize("name", CG.BACKWARD)
def test_backward_vs_oracle(name):
    case = CG.BY_NAME[name]
    t, ref = backward_data(name)
    got = ops.hexconv2d_backward(_dev(t["gy"]), _dev(t["x"]), _dev(t["k"]), _dev(t["b"]), case.cfg())
    assert all(g is not None for g in got)
    assert got[0].dtype == case.x_dt and got[1].shape == t["k"].shape
    grads_close(case, got, ref, name)


@pytest.mark.parametrize("name,need_x,need_k,need_b", CG.BACKWARD_PARTIAL)
def test_backward_partial_requests(name, need_x, need_k, need_b):
    case = CG.BY_NAME[name]
    t, ref = backward_data(name)
    got = ops.hexconv2d_backward(_dev(t["gy"]), _dev(t["x"]), _dev(t["k"]), _dev(t["b"]), case.cfg(),
                                 need_x=need_x, need_k=need_k, need_b=need_b)
    assert [g is not None for g in got] == [need_x, need_k, need_b]
    grads_close(case, got, ref, f"{name} need={int(need_x)}{int(need_k)}{int(need_b)}")
