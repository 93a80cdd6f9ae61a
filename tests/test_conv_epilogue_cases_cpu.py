"""The quantised epilogue table (tests/conv_epilogue_cases.py) does what it says, checked
without a device: every case reaches the kernel it is filed under (from the library's own
queries hg_hexconv2d_forward_plan and hg_hexconv2d_generic_plan and the stream kernel's
conditions restated from csrc/hexconv.hip and csrc/conv_stream.hip), its pre-activations sit on
the thresholds often enough, every reference value is exact in f32; and the fp64 reference of
the epilogue and of its derivative equals torch.nn's activations and their autograd."""
import numpy as np
import pytest
import torch

import conv_epilogue_cases as CE
from HyGrid import _abi, ops
from oracle import oracle as O

OTHER, MF32, MBF, MDMA = (_abi.HG_CONV_FWD_OTHER, _abi.HG_CONV_FWD_MFMA_F32,
                          _abi.HG_CONV_FWD_MFMA_BF16, _abi.HG_CONV_FWD_MFMA_BF16_DMA)
SWITCHES = ("HYGRID_CONV_MFMA", "HYGRID_CONV_MFMA_BF16", "HYGRID_CONV_DMA", "HYGRID_CONV_NT",
            "HYGRID_FCONV")
TR, TC = 16, 128                  # k_hexconv's output tile (hexconv.hip CV_TR, CV_TC)


@pytest.fixture(autouse=True)
def switches_unset(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


# ---- routes -----------------------------------------------------------------------------------
def stream_takes(c):
    """hexconv.hip, hg_hexconv2d_epilogue: the register-streaming kernel's condition
    (tests/test_conv_generic_cases_cpu.py), and conv_stream.hip, launch_conv_stream /
    cs_channels: paddings 0..2, the three channel layouts and the six dtype pairs it has kernels
    for.  An epilogue keeps the call off the two-column kernel (fused_conv.hip, fused_conv_try
    returns HG_EUNSUP for one), so what runs is k_hexconv_stream."""
    pairs = {(CE.BF16, CE.BF16), (CE.BF16, CE.F32), (CE.F16, CE.F16), (CE.F16, CE.F32),
             (CE.F32, CE.F32), (CE.F32, CE.BF16)}
    return (c.r == 2 and c.s == 1 and c.d == 1 and c.mode == "constant" and c.w_dt == CE.F32
            and c.C <= 3 and c.O <= 3 and 0 <= c.p <= 2
            and (c.C, c.O, c.g) in {(3, 3, 1), (3, 3, 3), (1, 1, 1)}
            and (c.x_dt, c.y_dt) in pairs)


def forward_plan(c):
    return ops.hexconv2d_forward_plan(c.x_dt, c.w_dt, c.y_dt, c.B, c.C, c.O, c.h, c.w, c.r,
                                      stride=c.s, padding=c.p, dilation=c.d, groups=c.g,
                                      even_odd_offset=c.off, padding_mode=c.mode,
                                      padding_value=c.pv)


def generic_plan(c):
    return _abi.hexconv2d_generic_plan(_abi.dtype_code(c.w_dt), c.B, c.C, c.O, c.h, c.w, c.r, c.s,
                                       c.p, c.d, c.g, c.off)


MFMA_ROUTE = {"mfma_f32": (MF32, 1), "mfma_bf16": (MBF, 1), "mfma_bf16_dma": (MDMA, 1),
              "mfma_f32_s2": (MF32, 2), "mfma_bf16_s2": (MBF, 2)}


@pytest.mark.parametrize("case", CE.CASES, ids=repr)
def test_case_reaches_its_kernel(case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    ho, wo = case.out_shape()
    if case.route == "stream":
        assert stream_takes(case) and forward_plan(case) == OTHER
        # two column windows, the second one ragged (64 lanes less the halo own 61 or 62 columns)
        assert (case.h, case.w) == (9, 70) and 62 < wo < 2 * 61
        return
    assert not stream_takes(case)
    if case.route in MFMA_ROUTE:
        kern, stride = MFMA_ROUTE[case.route]
        assert forward_plan(case) == kern and case.s == stride
        return
    assert forward_plan(case) == OTHER
    P = generic_plan(case)
    if case.route == "direct":
        assert P["direct"] and case.s == 3 and case.g == 2
        assert P["tiles"] >= 2 and (case.B * case.O * ho * wo) % 256, "a partial last block"
    else:
        assert case.route == "lds" and not P["direct"]
        assert P["ocb"] == case.ocb and P["cib"] >= 1 and P["bc"] == 1
        assert P["tiles"] == 1 and ho < TR and wo < TC, "one ragged tile"


def test_table_covers_the_routes_of_the_issue():
    by = {}
    for c in CE.CASES:
        by.setdefault(c.route, []).append(c)
    assert set(by) == set(CE.ROUTES)
    # stream: every (channel layout, padding, offset) instantiation; every dtype pair on every
    # layout and at every padding
    st = by["stream"]
    assert {(c.C, c.O, c.g, c.p, c.off) for c in st} == {
        (C, O_, g, p, off) for C, O_, g in [(3, 3, 1), (3, 3, 3), (1, 1, 1)] for p in (0, 1, 2)
        for off in (0, 1)}
    pairs = {(CE.F32, CE.F32), (CE.F32, CE.BF16), (CE.BF16, CE.BF16), (CE.F16, CE.F32)}
    for C, O_, g in [(3, 3, 1), (3, 3, 3), (1, 1, 1)]:
        assert {(c.x_dt, c.y_dt) for c in st if (c.C, c.O, c.g) == (C, O_, g)} == pairs
    for p in (0, 1, 2):
        assert {(c.x_dt, c.y_dt) for c in st if c.p == p} == pairs
    # k_hexconv: og 1 / 2 / 3 and OCB 4 with a remainder behind a group offset-free 7 -> 5;
    # radius 3 (the non-K7 template); f64 weights with f64 output
    lds = by["lds"]
    assert {c.ocb for c in lds} == {1, 2, 3, 4}
    assert any(c.C == c.O == c.g == 6 for c in lds)
    assert any(c.og == 2 and c.g == 2 for c in lds) and any(c.og == 3 and c.g == 2 for c in lds)
    assert any((c.C, c.O, c.g, c.ocb) == (7, 5, 1, 4) and c.O % 4 for c in lds)
    assert any(c.r == 3 for c in lds)
    assert any(c.w_dt == CE.F64 and c.y_dt == CE.F64 for c in lds)
    # f32 MFMA: 16 -> 32, 16 -> 80 (four channel tiles of 16 x nt = 64, the last with o >= O
    # lanes), the f16 column store with and without its scalar tail
    mf = by["mfma_f32"]
    assert any((c.C, c.O, c.x_dt, c.y_dt) == (16, 32, CE.F32, CE.F32) for c in mf)
    assert any((c.C, c.O, c.x_dt, c.y_dt) == (16, 80, CE.F32, CE.F32) for c in mf)
    f16 = [c for c in mf if (c.x_dt, c.y_dt) == (CE.F16, CE.F16)]
    assert {c.out_shape()[1] % 4 == 0 for c in f16} == {True, False}
    # bf16 kernels: each with bf16 and f32 output; register-staged by odd width and by the switch
    for route in ("mfma_bf16", "mfma_bf16_dma"):
        assert {c.y_dt for c in by[route]} == {CE.BF16, CE.F32}
        assert all(c.x_dt == CE.BF16 for c in by[route])
    assert any(c.w % 2 and not c.env for c in by["mfma_bf16"])
    assert any(c.w % 2 == 0 and c.env == {"HYGRID_CONV_DMA": "0"} for c in by["mfma_bf16"])
    assert all(c.w % 2 == 0 and not c.env for c in by["mfma_bf16_dma"])
    # stride 2: 16 -> 16, f32 -> f32 and bf16 -> bf16, padding 0 and 1
    assert {(c.x_dt, c.y_dt, c.p) for c in by["mfma_f32_s2"]} == {(CE.F32, CE.F32, 0), (CE.F32, CE.F32, 1)}
    assert {(c.x_dt, c.y_dt, c.p) for c in by["mfma_bf16_s2"]} == {(CE.BF16, CE.BF16, 0),
                                                                 (CE.BF16, CE.BF16, 1)}
    assert all((c.C, c.O) == (16, 16) for c in by["mfma_f32_s2"] + by["mfma_bf16_s2"])
    # both row parities on every route but the one-case direct kernel
    for route, cs in by.items():
        if route != "direct":
            assert {c.off for c in cs} == {0, 1}, route
    # a non-finite case per route
    assert {CE.BY_NAME[n].route for n in CE.NONFINITE} == set(CE.ROUTES)


# ---- conditions and exactness -----------------------------------------------------------------
@pytest.mark.parametrize("case", CE.CASES, ids=repr)
def test_case_is_quantised_and_sits_on_the_thresholds(case):
    t, v = CE.data(case.name)
    x, k, b = (t[n].double() for n in ("x", "k", "b"))
    for a, bound in ((x, 4), (k, 2), (b, 3)):
        assert torch.equal(a, a.round()) and float(a.abs().max()) <= bound
    # exact in the 16-bit input types too (the bf16 kernels split the weights into bf16 parts)
    for dt in (CE.BF16, CE.F16):
        assert torch.equal(x.to(dt).double(), x) and torch.equal(k.to(dt).double(), k)
    scale, shift = t["scale"].double(), t["shift"].double()
    mant, _ = np.frexp(scale.numpy())
    assert np.all(np.abs(mant) == 0.5), "scale is +- a power of two"
    assert len(set(scale.tolist())) == case.O, "distinct across channels"
    assert bool((scale < 0).any())
    assert torch.equal(shift * 4, (shift * 4).round()), "shift is a multiple of 1/4"
    assert v.shape == (case.B, case.O) + case.out_shape()
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() < 2 ** 11
    pre = CE.preact(case.name)
    n0, n6 = int((pre == 0).sum()), int((pre == 6).sum())
    print(f"{case.name}: {pre.size} outputs, {n0} pre-activations exactly 0, {n6} exactly 6")
    assert n0 >= 8 and n6 >= 8
    assert (pre < 0).any() and ((pre > 0) & (pre < 6)).any() and (pre > 6).any()
    # every value the kernels form, and every reference value, is exact in f32
    sc, sf = CE.affine(t, CE.NONE)
    for a in (v * sc[None, :, None, None], pre):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    for _, act, slope in CE.EXACT_ACTS:
        ref = CE.expected(case.name, act, slope)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), (act, slope)
    # Sigmoid / Tanh: the squashed pre-activation is exact as well and half of it is in (-4, 4)
    sq = CE.preact(case.name, CE.SIGMOID)
    assert np.array_equal(sq, pre * CE.SQUASH)
    assert np.array_equal(sq.astype(np.float32).astype(np.float64), sq)
    assert (np.abs(sq) < 4).mean() >= 0.5


@pytest.mark.parametrize("name", CE.NONFINITE)
def test_nonfinite_points_lie_apart(name):
    c = CE.BY_NAME[name]
    pts = CE.nonfinite_points(c)
    assert {np.isnan(v) or v for _, _, v in pts} == {True, float("inf"), float("-inf")}
    for i, (r0, c0, _) in enumerate(pts):
        assert 0 <= r0 < c.h and 0 <= c0 < c.w
        for r1, c1, _ in pts[i + 1:]:
            assert abs(r0 - r1) >= 3 * c.s or abs(c0 - c1) >= 4 * c.s + 1, (name, r0, c0, r1, c1)
    rows, cols = {r for r, _, _ in pts}, {q for _, q, _ in pts}
    assert {0, c.h - 1} <= rows and {0, c.w - 1} <= cols            # borders
    assert any(0 < r < c.h - 1 and 0 < q < c.w - 1 for r, q, _ in pts)   # interior
    if c.route == "stream":
        assert 61 in cols, "the last column the first window owns"
    # what the activations get to see, by the oracle: ReLU / ReLU6 a NaN, ReLU6 +inf, ReLU -inf
    t, _ = CE.data(name)
    v = O.hexconv2d(CE.nonfinite_input(c, t).double().numpy(), t["k"].double().numpy(),
                    t["b"].double().numpy(), c.off, c.r, c.s, c.p, c.d, c.g, c.mode, c.pv)
    pre = CE.epilogue_ref(v, *CE.affine(t, CE.NONE), CE.NONE)
    assert np.isnan(pre).any() and (pre == np.inf).any() and (pre == -np.inf).any()
    assert np.isfinite(pre).mean() > 0.9


@pytest.mark.parametrize("layer", list(CE.MODULE_LAYERS))
def test_module_layers(layer):
    d = CE.module_data(layer)
    C, O_, g, p, h, w = CE.MODULE_LAYERS[layer]
    scale, shift, gy = d["scale"].numpy(), d["shift"].numpy(), d["gy"].numpy()
    assert (scale < 0).any()
    pre = CE.epilogue_ref(d["v"], scale, shift, CE.NONE)
    at0, at6 = pre == 0, pre == 6
    assert at0.sum() >= 8 and at6.sum() >= 8
    assert np.all(gy[at0] != 0) and np.all(gy[at6] != 0), "`>` against `>=` changes the gradient"
    assert np.array_equal(gy, np.round(gy)) and np.abs(gy).max() == 4
    # the gradient sums are exact in f32: multiples of 2^-3 below 2^17
    for _, act, slope in CE.EXACT_ACTS:
        gr = gy * CE.act_grad_ref(pre, act, slope) * scale[None, :, None, None]
        for a in O.hexconv2d_backward(d["x"].numpy(), d["k"].numpy(), gr, 0, 2, 1, p, 1, g):
            assert np.array_equal(a * 8, np.round(a * 8)) and np.abs(a).max() < 2 ** 17
    # routes: the forward kernel, and the matrix-core backward of the wide layer
    plan = ops.hexconv2d_forward_plan(CE.F32, CE.F32, CE.F32, CE.MODULE_B, C, O_, h, w, 2, padding=p,
                                      groups=g)
    assert plan == (MF32 if layer == "mfma" else OTHER)
    bwd = ops.hexconv2d_backward_plan(CE.F32, CE.F32, CE.MODULE_B, C, O_, h, w, 2, padding=p, groups=g)
    want = _abi.HG_CONV_BWD_MFMA if layer == "mfma" else _abi.HG_CONV_BWD_GENERIC
    assert bwd == (want, want)


# ---- the reference against torch --------------------------------------------------------------
EDGE = [-np.inf, -7.5, -1.0, -0.0, 0.0, 0.25, 6.0, 7.0, np.inf, np.nan]
TORCH_ACTS = [
    (CE.RELU, 0.0, lambda: torch.nn.ReLU()),
    (CE.RELU6, 0.0, lambda: torch.nn.ReLU6()),
    (CE.LEAKY, 0.25, lambda: torch.nn.LeakyReLU(0.25)),
    (CE.LEAKY, 0.0, lambda: torch.nn.LeakyReLU(0.0)),
    (CE.LEAKY, 2.0, lambda: torch.nn.LeakyReLU(2.0)),
    (CE.SIGMOID, 0.0, lambda: torch.nn.Sigmoid()),
    (CE.TANH, 0.0, lambda: torch.nn.Tanh()),
]


def _same_bits(a, b):
    """Equal NaN positions, equal bit patterns (the sign of zero included) elsewhere."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize("act,slope,make", TORCH_ACTS,
                         ids=["relu", "relu6", "leaky0.25", "leaky0", "leaky2", "sigmoid", "tanh"])
def test_reference_equals_torch(act, slope, make):
    gen = torch.Generator().manual_seed(5)
    v = torch.cat([torch.tensor(EDGE, dtype=torch.float64),
                   (torch.rand(200, generator=gen, dtype=torch.float64) - 0.5) * 24])
    x = v.clone().requires_grad_(True)
    y = make()(x)
    y.backward(torch.ones_like(y))
    ref = CE.epilogue_ref(v.numpy(), None, None, act, slope)
    gref = CE.act_grad_ref(v.numpy(), act, slope)
    if act in (CE.SIGMOID, CE.TANH):
        yt = y.detach().numpy()
        assert np.array_equal(np.isnan(ref), np.isnan(yt))
        np.testing.assert_allclose(ref, yt, rtol=1e-15, atol=0)
        # the derivative is torch's formula on its own rounded output y (y (1 - y), 1 - y^2),
        # which cancels in the tails: two outputs that agree to rtol 1e-15 give derivatives that
        # differ by |d formula / d y| 1e-15 |y| (at v = 7, 1 - y^2 = 3.3e-6 moves by 1e-11 of
        # itself when tanh differs in its last bit), so that much is allowed on top of rtol 1e-15
        gt = x.grad.numpy()
        assert np.array_equal(np.isnan(gref), np.isnan(gt))
        ok = ~np.isnan(gt)
        dgdy = np.abs(1 - 2 * yt) if act == CE.SIGMOID else 2 * np.abs(yt)
        bound = 1e-15 * np.abs(gt[ok]) + dgdy[ok] * 1e-15 * np.abs(yt[ok])
        assert np.all(np.abs(gref[ok] - gt[ok]) <= bound)
    else:
        assert _same_bits(ref, y.detach().numpy()), (ref[:len(EDGE)], y[:len(EDGE)])
        assert _same_bits(gref, x.grad.numpy()), (gref[:len(EDGE)], x.grad[:len(EDGE)])
    assert np.isnan(ref[len(EDGE) - 1]), "NaN propagates through every activation"


def test_affine_of_the_reference():
    v = np.arange(24, dtype=np.float64).reshape(1, 3, 2, 4) - 10
    sc, sf = np.array([2.0, -0.5, 1.0]), np.array([0.25, 0.0, -6.0])
    want = v * sc[None, :, None, None] + sf[None, :, None, None]
    assert np.array_equal(CE.epilogue_ref(v, sc, sf, CE.NONE), want)
    assert np.array_equal(CE.epilogue_ref(v, None, sf, CE.RELU6), np.clip(v + sf[None, :, None, None], 0, 6))
    assert np.array_equal(CE.epilogue_ref(v, sc, None, CE.LEAKY, 2.0),
                          np.where(v * sc[None, :, None, None] > 0, v * sc[None, :, None, None],
                                   2 * v * sc[None, :, None, None]))
    assert np.array_equal(CE.act_grad_ref(np.array([-1.0, 0.0, 3.0, 6.0, 7.0]), CE.RELU6),
                          [0, 0, 1, 0, 0])
    with pytest.raises(ValueError):
        CE.epilogue_ref(v, None, None, 6)
