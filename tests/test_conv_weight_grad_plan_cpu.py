"""hg_hexconv2d_weight_grad_plan and ops.hexconv2d_training_plan (host only: nothing is launched
and no device is needed), and include/hygrid_train.h against the library.

d kernel / d bias of a dense radius-2, dilation-1 layer with f32 weights run on the matrix cores:
at stride 2 from S2_MIN_O output channels on k_hexconv_bwd_weight_mfma_s2 (switch
HYGRID_CONV_BWD_MFMA_S2=0), at stride 1 where hg_hexconv2d_backward_plan says so (switch
HYGRID_CONV_BWD_MFMA=0); everything else on the generic kernels.  d input of a stride-2 layer with
constant padding and 16 input channels or more is the transposed layer's forward ("convt_s2",
switch HYGRID_CONVT_MFMA=0)."""
import ctypes
import os
import re

import pytest
import torch

import conv_bwd_s2_cases as CS
from conftest import ROOT
from HyGrid import _abi, ops

HEADER = os.path.join(ROOT, "include", "hygrid_train.h")
GEN, MFMA, S2 = _abi.HG_CONV_WGRAD_GENERIC, _abi.HG_CONV_WGRAD_MFMA, _abi.HG_CONV_WGRAD_MFMA_S2
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
S2_MIN_O = 16            # CMB_S2_MIN_O: the stride-2 threshold
SWITCHES = ("HYGRID_CONV_BWD_MFMA", "HYGRID_CONV_BWD_MFMA_S2", "HYGRID_CONVT_MFMA")

# (x dtype, w dtype, B, C, O, h, w, radius, kwargs) -> kernel
TABLE = [((xd, F32, 2, C, O_, 40, 50, 2, dict(padding=1, stride=2)), S2)
         for O_ in (S2_MIN_O, 64) for C in (3, 16, 64) for xd in (F32, BF16)]
TABLE += [
    ((F16, F32, 4, 64, 128, 1080, 1920, 2, dict(padding=0, stride=2)), S2),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=2, stride=2, padding_mode="reflect")), S2),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2, padding_mode="circular")), S2),
    ((F32, F32, 2, 64, S2_MIN_O - 1, 40, 50, 2, dict(padding=1, stride=2)), GEN),
    ((F32, F32, 2, 64, 64, 40, 50, 3, dict(padding=1, stride=2)), GEN),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2, dilation=2)), GEN),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2, groups=2)), GEN),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=3, stride=2)), GEN),
    ((F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=3)), GEN),
    ((F64, F64, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2)), GEN),
    ((F32, F64, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2)), GEN),
    ((torch.uint8, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, stride=2)), GEN),
    # past the forward's 32-bit-offset limit (C * h * w * 4 >= 2^31)
    ((BF16, F32, 1, 64, 64, 4096, 4096, 2, dict(padding=1, stride=2)), GEN),
]
# stride 1: hexconv2d_backward_plan's d kernel answer
STRIDE1 = [
    (BF16, F32, 4, 64, 64, 1080, 1920, 2, dict(padding=1)),
    (F32, F32, 2, 64, 3, 40, 50, 2, dict(padding=1)),
    (F32, F32, 2, 16, 16, 40, 50, 2, dict(padding=1)),
    (F32, F32, 2, 15, 15, 40, 50, 2, dict(padding=1)),
    (F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, padding_mode="reflect")),
    (F32, F32, 2, 64, 64, 40, 50, 3, dict(padding=1)),
    (F32, F32, 2, 64, 64, 40, 50, 2, dict(padding=1, groups=2)),
    (F32, F64, 2, 64, 64, 40, 50, 2, dict(padding=1)),
    (BF16, F32, 1, 64, 64, 4096, 4096, 2, dict(padding=1)),
]


def _plan(row):
    *args, kw = row
    return ops.hexconv2d_weight_grad_plan(*args, **kw)


@pytest.fixture
def switches_unset(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


@pytest.mark.parametrize("row,want", TABLE)
def test_plan_domain_table(switches_unset, row, want):
    assert _plan(row) == want


@pytest.mark.parametrize("row", STRIDE1)
def test_plan_stride_1_is_the_backward_plans_dkernel(switches_unset, monkeypatch, row):
    *args, kw = row
    want = {_abi.HG_CONV_BWD_GENERIC: GEN, _abi.HG_CONV_BWD_MFMA: MFMA}
    assert _plan(row) == want[ops.hexconv2d_backward_plan(*args, **kw)[1]]
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA", "0")
    assert _plan(row) == GEN
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA", "1")
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA_S2", "0")          # not stride 1's switch
    assert _plan(row) == want[ops.hexconv2d_backward_plan(*args, **kw)[1]]
    assert MFMA in {_plan(r) for r in STRIDE1}


@pytest.mark.parametrize("row,want", TABLE)
def test_plan_switches(switches_unset, monkeypatch, row, want):
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA_S2", "0")
    assert _plan(row) == GEN
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA_S2", "1")          # only "0" switches
    assert _plan(row) == want
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA_S2", "")
    assert _plan(row) == want
    monkeypatch.delenv("HYGRID_CONV_BWD_MFMA_S2")
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA", "0")             # stride 1's switch alone
    assert _plan(row) == want


def test_plan_error_codes_match_backward(switches_unset):
    """The bad arguments of test_conv_backward_plan_cpu.py::test_plan_error_codes_match_backward:
    the plan, hg_hexconv2d_weight_grad and hg_hexconv2d_backward give each the same status."""
    L = _abi.lib()
    fake = ctypes.c_void_p(16)
    f32 = _abi.HG_F32
    kern = ctypes.c_int(-7)

    def all3(xd, wd, B, C, O_, h, w, r, s, p, d, g, pm):
        a = L.hg_hexconv2d_weight_grad_plan(xd, wd, B, C, O_, h, w, r, s, p, d, g, pm,
                                            ctypes.byref(kern))
        b = L.hg_hexconv2d_weight_grad(fake, fake, fake, fake, xd, wd, B, C, O_, h, w, r, s, p, d,
                                       g, 0, pm, 0.0, None)
        c = L.hg_hexconv2d_backward(fake, fake, fake, fake, fake, fake, xd, wd, B, C, O_, h, w,
                                    r, s, p, d, g, 0, pm, 0.0, None)
        assert a == b == c
        return a

    for s in (1, 2):
        assert all3(f32, f32, 1, 3, 4, 8, 8, 2, s, 1, 1, 3, 0) == _abi.HG_EINVAL    # groups
        assert all3(f32, f32, 1, 3, 3, 1, 1, 2, s, 0, 1, 1, 0) == _abi.HG_ESHAPE    # too small
        assert all3(f32, f32, 1, 3, 3, 8, 8, 2, s, 1, 1, 1, 9) == _abi.HG_EINVAL    # pad mode
        assert all3(f32, f32, 1, 3, 3, 2, 2, 2, s, 2, 1, 1, 1) == _abi.HG_ESHAPE    # reflect pad
        assert all3(f32, f32, 1, 3, 3, 8, 8, 0, s, 1, 1, 1, 0) == _abi.HG_EINVAL    # radius
        assert all3(f32, f32, -1, 3, 3, 8, 8, 2, s, 1, 1, 1, 0) == _abi.HG_EINVAL   # batch
        assert all3(f32, f32, 1, 3, 3, 40, 40, 8, s, 1, 1, 1, 0) == _abi.HG_EUNSUP  # > 127 taps
        assert all3(f32, _abi.HG_F16, 1, 3, 3, 8, 8, 2, s, 1, 1, 1, 0) == _abi.HG_EDTYPE
    assert kern.value == -7                              # untouched on error
    assert L.hg_hexconv2d_weight_grad_plan(f32, f32, 1, 64, 64, 8, 8, 2, 2, 1, 1, 1, 0,
                                           None) == _abi.HG_EINVAL
    assert L.hg_hexconv2d_weight_grad_plan(99, f32, 1, 64, 64, 8, 8, 2, 2, 1, 1, 1, 0,
                                           ctypes.byref(kern)) == _abi.HG_EDTYPE
    # missing sources, and nothing asked for
    assert L.hg_hexconv2d_weight_grad(fake, None, fake, fake, f32, f32, 1, 64, 64, 8, 8, 2, 2, 1, 1,
                                      1, 0, 0, 0.0, None) == _abi.HG_EINVAL
    assert L.hg_hexconv2d_weight_grad(None, fake, fake, fake, f32, f32, 1, 64, 64, 8, 8, 2, 2, 1, 1,
                                      1, 0, 0, 0.0, None) == _abi.HG_EINVAL
    assert L.hg_hexconv2d_weight_grad(fake, fake, None, None, f32, f32, 1, 64, 64, 8, 8, 2, 2, 1, 1,
                                      1, 0, 0, 0.0, None) == _abi.HG_OK
    with pytest.raises(ValueError):
        ops.hexconv2d_weight_grad_plan(F32, F32, 1, 3, 4, 8, 8, 2, groups=3)
    with pytest.raises(ValueError):
        ops.hexconv2d_training_plan(F32, F32, 1, 3, 3, 8, 8, 2, padding_mode="mirror")


def test_plan_empty_call_is_generic(switches_unset):
    assert ops.hexconv2d_weight_grad_plan(F32, F32, 0, 64, 64, 40, 50, 2, stride=2, padding=1) == GEN
    assert ops.hexconv2d_training_plan(F32, F32, 0, 64, 64, 40, 50, 2, stride=2,
                                       padding=1) == ("generic", GEN)
    # nothing requested from an empty batch: success, nothing launched
    assert _abi.lib().hg_hexconv2d_weight_grad(None, None, None, None, _abi.HG_F32, _abi.HG_F32, 0,
                                               64, 64, 40, 50, 2, 2, 1, 1, 1, 0, 0, 0.0, None) == 0


def test_training_plan_rows(switches_unset, monkeypatch):
    tp = ops.hexconv2d_training_plan
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1, even_odd_offset=1) == ("convt_s2", S2)
    assert tp(BF16, F32, 4, 64, 128, 1080, 1920, 2, stride=2, padding=1) == ("convt_s2", S2)
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1,
              padding_mode="reflect") == ("generic", S2)
    assert tp(F32, F32, 2, 3, 16, 13, 22, 2, stride=2, padding=1) == ("generic", S2)
    assert tp(F32, F32, 2, 15, S2_MIN_O - 1, 13, 22, 2, stride=2, padding=1) == ("generic", GEN)
    assert tp(F32, F64, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == ("generic", GEN)
    assert tp(torch.uint8, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == ("generic", GEN)
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, padding=1) == ("mfma", MFMA)
    assert tp(F32, F32, 2, 3, 16, 13, 22, 2, padding=1) == ("generic", MFMA)
    monkeypatch.setenv("HYGRID_CONVT_MFMA", "0")
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == ("generic", S2)
    monkeypatch.setenv("HYGRID_CONV_BWD_MFMA_S2", "0")
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == ("generic", GEN)
    monkeypatch.delenv("HYGRID_CONVT_MFMA")
    assert tp(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == ("convt_s2", GEN)
    # hg_hexconv2d_backward's own plan keeps stride 2 generic
    g = _abi.HG_CONV_BWD_GENERIC
    assert ops.hexconv2d_backward_plan(F32, F32, 2, 16, 16, 13, 22, 2, stride=2, padding=1) == (g, g)


def test_threshold_constant_is_the_sources():
    assert CS.constants()["CMB_S2_MIN_O"] == S2_MIN_O


# ---- the header -----------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hg_\w+)\s*\(", src)))


def test_train_header_exports_and_signatures():
    names = _declared()
    assert names == sorted(_abi.TRAIN_SIGNATURES) and len(names) == 2
    assert not set(names) & set(_abi.SIGNATURES) and not set(names) & set(_abi.LAYER_SIGNATURES)
    L = _abi.lib()
    for n in names:
        fn = getattr(L, n)
        assert fn.argtypes == _abi.TRAIN_SIGNATURES[n][0] and fn.restype is _abi.TRAIN_SIGNATURES[n][1]
    text = open(HEADER).read()
    assert '#include "hygrid.h"' in text and "part three" in text
    # the same contract text as hygrid.h
    contract = re.search(r"Contract \(all entry points\):.*?renders either kind\.",
                         open(os.path.join(ROOT, "include", "hygrid.h")).read(), flags=re.S).group(0)
    assert contract in text
    for e, v in (("HG_CONV_WGRAD_GENERIC", GEN), ("HG_CONV_WGRAD_MFMA", MFMA),
                 ("HG_CONV_WGRAD_MFMA_S2", S2)):
        assert re.search(rf"\b{e} = {v}\b", text)
    # the kernel-source digest covers the new header
    from HyGrid._digest import kernel_source_digest
    assert kernel_source_digest() != kernel_source_digest(train_header=os.devnull + ".absent")


def test_every_device_writing_export_has_a_guard_band_case(monkeypatch):
    import test_placement_cpu as TP
    monkeypatch.setattr(TP, "HEADER", HEADER)
    ex = TP.exports_with_destination()
    assert set(ex) == set(_abi.TRAIN_SIGNATURES)
    need = {n for n, d in ex.items() if d}
    assert need == {"hg_hexconv2d_weight_grad"}
    assert ex["hg_hexconv2d_weight_grad"] == ["void* dkernel", "void* dbias"]
    assert set(CS.GUARD_CASES) == need
    for n, where in CS.GUARD_CASES.items():
        path, test = where.split("::")
        src = open(os.path.join(ROOT, path)).read()
        body = re.search(rf"^def {test}\(.*?(?=^def |\Z)", src, flags=re.M | re.S)
        assert body, where
        assert "PL.placed(" in body.group(0) and "PL.place(" in body.group(0)
        assert "guards_intact" in body.group(0) and "sentinel_count" in body.group(0)
