"""HexConvTranspose2d without a device: the index check that comes before any GPU run.

  * the class tap table k_hexconvt_s2 is launched with (hg_hexconv_transpose2d_taps), turned into
    the layer in NumPy, equals the fp64 oracle's adjoint for every shape of the GPU test, both
    offsets and paddings 0..2, at fp64 rounding;
  * the output-size rule, the plan table and its error statuses (equal to the call's);
  * hg_hexconv2d_backward_plan still keeps stride 2 on the generic kernels;
  * include/hygrid_layers.h against the library, _abi.LAYER_SIGNATURES and the guard-band cases;
  * the module: state-dict alias, registry, seeded init."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conv_transpose_cases as CT
from conftest import ROOT
from HyGrid import _abi, ops
from HyGrid.HexFrames import HexConv2d, HexConvTranspose2d
from oracle import oracle as O

HEADER = os.path.join(ROOT, "include", "hygrid_layers.h")
ADJ, MFMA = _abi.HG_CONVT_ADJOINT, _abi.HG_CONVT_MFMA_S2
F16, BF16, F32, F64, I32 = _abi.HG_F16, _abi.HG_BF16, _abi.HG_F32, _abi.HG_F64, _abi.HG_I32


# ---- the tap table ----------------------------------------------------------------------------
def _taps(off, p):
    return [[ops.hexconv_transpose2d_taps(off, p, rc, cc) for cc in (0, 1)] for rc in range(4)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_class_structure(off, p):
    """One or two taps per class, 7/4 on average; rows of even iy + p take one tap from each of
    two x rows, rows of odd iy + p two or one taps of one x row, alternating by column; three
    staged x rows and x columns b - 1 .. b + 1 hold everything."""
    T = _taps(off, p)
    n = [[len(T[rc][cc]) for cc in (0, 1)] for rc in range(4)]
    assert sum(map(sum, n)) == 14 and all(v in (1, 2) for row in n for v in row)
    for rc in range(4):
        rows = [{ro for (_, ro, _) in T[rc][cc]} for cc in (0, 1)]
        if (rc + p) % 2 == 0:
            assert n[rc] == [2, 2] and all(len(r) == 2 for r in rows)
        else:
            assert sorted(n[rc]) == [1, 2] and all(len(r) == 1 for r in rows)
    rofs = [ro for rc in range(4) for cc in (0, 1) for (_, ro, _) in T[rc][cc]]
    qofs = [q for rc in range(4) for cc in (0, 1) for (_, _, q) in T[rc][cc]]
    assert max(rofs) - min(rofs) <= 2 and min(qofs) >= -1 and max(qofs) <= 1
    taps = sorted(t for rc in range(4) for cc in (0, 1) for (t, _, _) in T[rc][cc])
    assert taps == sorted(list(range(7)) * 2)            # every tap in exactly two classes


@pytest.mark.parametrize("shape", CT.SHAPES, ids=str)
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_tap_table_rebuilds_the_oracle_adjoint(shape, off, p):
    hin, win, _ = shape
    rng = np.random.default_rng(hin * 100 + win + 7 * off + p)
    x = rng.standard_normal((2, 3, hin, win))
    k = rng.standard_normal((3, 2, 7))
    T = _taps(off, p)
    sizes = CT.valid_sizes(hin, win, p)
    for (h, w) in sizes:
        if h < 1 or w < 1:
            continue
        assert O.hexconv2d_out_shape(h, w, 2, 2, p, 1) == (hin, win)
        ref = CT.oracle_adjoint(x, k.reshape(3, 2, 1, 7), h, w, off, p)
        got = CT.from_taps(T, x, k, h, w)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    # untapped positions exist at p = 0: the last row / columns of the larger sizes
    if p == 0:
        h, w = sizes[-1]
        ones = CT.from_taps(T, np.ones((1, 1, hin, win)), np.ones((1, 1, 7)), h, w)
        assert (ones[0, 0, -1] == 0).all() and (ones == 0).sum() > 0


def test_taps_argument_errors():
    L = _abi.lib()
    out = (ctypes.c_int * 7)()
    assert L.hg_hexconv_transpose2d_taps(0, 1, 4, 0, out) == _abi.HG_EINVAL
    assert L.hg_hexconv_transpose2d_taps(0, 1, 0, 2, out) == _abi.HG_EINVAL
    assert L.hg_hexconv_transpose2d_taps(0, 1, 0, 0, None) == _abi.HG_EINVAL
    assert L.hg_hexconv_transpose2d_taps(0, 3, 0, 0, out) == _abi.HG_EUNSUP


# ---- the output-size rule -----------------------------------------------------------------------
@pytest.mark.parametrize("p", [0, 1, 2])
def test_output_size_rule(p):
    for h in range(3, 21):
        for w in range(6, 25):
            try:
                hin, win = O.hexconv2d_out_shape(h, w, 2, 2, p, 1)
            except ValueError:
                continue
            if hin < 1 or win < 1:
                continue
            assert ops.hexconv_transpose2d_out_shape(hin, win, 2, 2, p, 1, (h, w)) == (h, w)
            valid = CT.valid_sizes(hin, win, p)
            assert (h, w) in valid
            d = ops.hexconv_transpose2d_out_shape(hin, win, 2, 2, p, 1)
            assert d in valid and d == (2 * hin + 2 - 2 * p, 2 * win + 2 - 2 * p)
            if p == 1:
                assert d == (2 * hin, 2 * win)
            hs, ws = sorted({v[0] for v in valid}), sorted({v[1] for v in valid})
            for bad in [(hs[0] - 1, ws[0]), (hs[-1] + 1, ws[0]), (hs[0], ws[0] - 1),
                        (hs[0], ws[-1] + 1)]:
                with pytest.raises(ValueError):
                    ops.hexconv_transpose2d_out_shape(hin, win, 2, 2, p, 1, bad)


def test_output_size_rule_other_strides():
    """Stride 1 has one valid size; stride 3 three per axis; the default is (max h, min w)."""
    for (r, s, p, d) in [(2, 1, 1, 1), (2, 3, 1, 1), (3, 2, 0, 1), (2, 2, 2, 2)]:
        for (h, w) in [(12, 17), (13, 18), (20, 31)]:
            hin, win = O.hexconv2d_out_shape(h, w, r, s, p, d)
            hs = [a for a in range(1, 80)
                  if _shape_or_none(a, w, r, s, p, d) and _shape_or_none(a, w, r, s, p, d)[0] == hin]
            ws = [b for b in range(max(1, w - 10), w + 10)
                  if _shape_or_none(h, b, r, s, p, d) and _shape_or_none(h, b, r, s, p, d)[1] == win]
            assert ops.hexconv_transpose2d_out_shape(hin, win, r, s, p, d) == (max(hs), min(ws))
            assert ops.hexconv_transpose2d_out_shape(hin, win, r, s, p, d, (h, w)) == (h, w)


def _shape_or_none(h, w, r, s, p, d):
    try:
        return O.hexconv2d_out_shape(h, w, r, s, p, d)
    except ValueError:
        return None


# ---- the plan ---------------------------------------------------------------------------------
def _plan_raw(xd=F32, wd=F32, yd=F32, B=1, ci=32, co=16, hw=(34, 70), r=2, s=2, p=1, d=1, g=1,
              size=None):
    h, w = hw
    hin, win = size if size is not None else O.hexconv2d_out_shape(h, w, r, s, p, d)
    k = ctypes.c_int(-7)
    st = _abi.lib().hg_hexconv_transpose2d_plan(xd, wd, yd, B, ci, co, hin, win, h, w, r, s, p, d,
                                                g, 0, ctypes.byref(k))
    return st, k.value


def _call_raw(xd=F32, wd=F32, yd=F32, B=1, ci=32, co=16, hw=(34, 70), r=2, s=2, p=1, d=1, g=1,
              size=None):
    """The call's status for arguments it rejects before any launch (fake pointers)."""
    h, w = hw
    hin, win = size if size is not None else O.hexconv2d_out_shape(h, w, r, s, p, d)
    fake = ctypes.c_void_p(256)
    return _abi.lib().hg_hexconv_transpose2d(fake, fake, None, fake, xd, wd, yd, B, ci, co, hin,
                                             win, h, w, r, s, p, d, g, 0, None)


def test_plan_table(monkeypatch):
    monkeypatch.delenv("HYGRID_CONVT_MFMA", raising=False)
    for xd in (BF16, F16, F32):
        for yd in (BF16, F16, F32):
            for p in (0, 1, 2):
                assert _plan_raw(xd=xd, yd=yd, p=p) == (0, MFMA)
    assert _plan_raw(ci=1, co=16) == (0, MFMA) and _plan_raw(ci=100, co=24, B=3) == (0, MFMA)
    assert _plan_raw(hw=(4, 7), p=0) == (0, MFMA)                    # the smallest layer
    outside = [dict(co=15), dict(r=3), dict(s=1), dict(s=3), dict(d=2, hw=(36, 74)),
               dict(g=2), dict(p=3), dict(wd=F64), dict(xd=F64), dict(yd=F64),
               dict(hw=(8192, 4096))]                                # 16 x 8192 x 4096 x 4 B = 2 GiB
    for kw in outside:
        assert _plan_raw(**kw) == (0, ADJ), kw
    assert _plan_raw(hw=(8190, 4096)) == (0, MFMA)                   # just inside the limit
    monkeypatch.setenv("HYGRID_CONVT_MFMA", "0")
    assert _plan_raw() == (0, ADJ)
    assert ops.hexconv_transpose2d_plan(torch.bfloat16, torch.float32, torch.float32, 2, 8, 16,
                                        17, 35, 34, 70, 2, 2, 1) == ADJ
    monkeypatch.setenv("HYGRID_CONVT_MFMA", "1")
    assert _plan_raw() == (0, MFMA)


def test_plan_errors_equal_the_calls(monkeypatch):
    monkeypatch.delenv("HYGRID_CONVT_MFMA", raising=False)
    bad = [(dict(g=3), _abi.HG_EINVAL),                              # groups divide neither count
           (dict(g=0), _abi.HG_EINVAL),
           (dict(size=(17, 36)), _abi.HG_ESHAPE),                    # (34, 70) maps onto (17, 35)
           (dict(size=(16, 35)), _abi.HG_ESHAPE),
           (dict(hw=(0, 70), size=(1, 35)), _abi.HG_ESHAPE),         # too small for the kernel
           (dict(s=0, size=(17, 35)), _abi.HG_EINVAL),
           (dict(wd=F16), _abi.HG_EDTYPE), (dict(xd=I32), _abi.HG_EDTYPE),
           (dict(yd=_abi.HG_U8), _abi.HG_EDTYPE)]
    for kw, want in bad:
        st, k = _plan_raw(**kw)
        assert st == want and k == -7, (kw, st, k)                   # the answer slot is left alone
        assert _call_raw(**kw) == want, kw
    assert _abi.lib().hg_hexconv_transpose2d_plan(F32, F32, F32, 1, 32, 16, 17, 35, 34, 70, 2, 2, 1,
                                                  1, 1, 0, None) == _abi.HG_EINVAL
    # the adjoint route's equal-dtype rule is the call's alone (ops converts after asking)
    assert _plan_raw(xd=BF16, s=1, hw=(34, 70)) == (0, ADJ)
    assert _call_raw(xd=BF16, s=1, hw=(34, 70)) == _abi.HG_EDTYPE
    assert _call_raw(yd=BF16, co=15) == _abi.HG_EDTYPE
    # an empty batch: success, nothing launched, on either route
    assert _call_raw(B=0) == 0 and _call_raw(B=0, s=1) == 0


def test_conv_backward_plan_keeps_stride_2_generic():
    gen = _abi.HG_CONV_BWD_GENERIC
    for (C, O_) in [(16, 16), (64, 128), (128, 64)]:
        assert ops.hexconv2d_backward_plan(torch.float32, torch.float32, 2, C, O_, 34, 70, 2,
                                           stride=2, padding=1) == (gen, gen)


# ---- the header -----------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hg_\w+)\s*\(", src)))


def test_layers_header_exports_and_signatures():
    names = _declared()
    assert names == sorted(_abi.LAYER_SIGNATURES) and len(names) == 3
    assert not set(names) & set(_abi.SIGNATURES)
    L = _abi.lib()
    for n in names:
        fn = getattr(L, n)
        assert fn.argtypes == _abi.LAYER_SIGNATURES[n][0] and fn.restype is _abi.LAYER_SIGNATURES[n][1]
    text = open(HEADER).read()
    assert '#include "hygrid.h"' in text
    # the same contract text as hygrid.h
    contract = re.search(r"Contract \(all entry points\):.*?renders either kind\.",
                         open(os.path.join(ROOT, "include", "hygrid.h")).read(), flags=re.S).group(0)
    assert contract in text
    # the kernel-source digest covers the new header
    from HyGrid._digest import kernel_source_digest
    assert kernel_source_digest() != kernel_source_digest(layers_header=os.devnull + ".absent")


def test_every_device_writing_export_has_a_guard_band_case(monkeypatch):
    import test_placement_cpu as TP
    monkeypatch.setattr(TP, "HEADER", HEADER)
    ex = TP.exports_with_destination()
    assert set(ex) == set(_abi.LAYER_SIGNATURES)
    need = {n for n, d in ex.items() if d}
    assert need == {"hg_hexconv_transpose2d"} and ex["hg_hexconv_transpose2d"] == ["void* y"]
    assert set(CT.GUARD_CASES) == need
    for n, where in CT.GUARD_CASES.items():
        path, test = where.split("::")
        src = open(os.path.join(ROOT, path)).read()
        body = re.search(rf"^def {test}\(.*?(?=^def |\Z)", src, flags=re.M | re.S)
        assert body, where
        assert "PL.placed(" in body.group(0) and "PL.place(" in body.group(0)
        assert "guards_intact" in body.group(0) and "sentinel_count" in body.group(0)


# ---- the module -----------------------------------------------------------------------------------
def test_module_parameters_and_seeded_init():
    torch.manual_seed(11)
    t = HexConvTranspose2d(24, 24, 1, 2, stride=2, padding=1)
    torch.manual_seed(11)
    a = HexConv2d(24, 24, 1, 2, stride=2, padding=1)          # the adjoint conv: out -> in
    assert t.kernel.shape == (24, 24, 1, 7) and t.bias.shape == (24,)
    assert torch.equal(t.kernel, a.kernel) and torch.equal(t.bias, a.bias)
    torch.manual_seed(5)
    t = HexConvTranspose2d(16, 32, 0, 2, stride=2, groups=2, bias=False)
    torch.manual_seed(5)
    a = HexConv2d(32, 16, 0, 2, stride=2, groups=2, bias=False)
    assert t.kernel.shape == (16, 16, 1, 7) and t.bias is None
    assert torch.equal(t.kernel, a.kernel)
    assert t.in_even_odd_offset == a.out_even_odd_offset == 0
    with pytest.raises(ValueError):
        HexConvTranspose2d(16, 30, 0, 2, groups=4)
    assert t.output_shape(17, 35) == (36, 72) and t.output_shape(17, 35, (35, 73)) == (35, 73)
    with pytest.raises(ValueError):
        t.output_shape(17, 35, (34, 72))


def test_state_dict_weight_alias():
    t = HexConvTranspose2d(8, 16, 0, 2, stride=2, padding=1)
    sd = {"weight": torch.full((8, 16, 1, 7), 0.25), "bias": torch.full((16,), -1.0)}
    t.load_state_dict(sd)
    assert float(t.kernel.detach().min()) == float(t.kernel.detach().max()) == 0.25
    assert float(t.bias.detach()[3]) == -1.0
    assert set(t.state_dict()) == {"kernel", "bias"}


def test_registry_builds_the_layer():
    from HyGrid import HexFrames
    from HyGrid.HexModules import CONV_LAYERS, HexConvModule, build_hexconv_layer
    assert "HexConvTranspose2d" in CONV_LAYERS and "HexConvTranspose2d" in HexFrames.__all__
    m = build_hexconv_layer(dict(type="HexConvTranspose2d"), 16, 32, 1, 2, stride=2, padding=1)
    assert type(m) is HexConvTranspose2d and (m.in_channels, m.out_channels) == (16, 32)
    blk = HexConvModule(16, 32, 0, 2, stride=2, padding=1, conv_cfg=dict(type="HexConvTranspose2d"),
                        norm_cfg=dict(type="BN"))
    assert type(blk.conv) is HexConvTranspose2d and blk.conv.bias is None
    assert blk.norm.num_features == 32
    assert blk._epilogue_plan(torch.zeros(1, 16, 4, 4), True, True) is None   # the unfused path
