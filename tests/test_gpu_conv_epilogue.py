"""GPU: the fused HexConv2d epilogue act(scale[o] * v + shift[o]) (hg_hexconv2d_epilogue, epi_apply
in csrc/common.h) at every store site that calls it, against the fp64 statement of it in
tests/conv_epilogue_cases.py, and HexConvModule's fused path with its Python backward
(_HexConvEpilogueFn / _act_grad) against the oracle's adjoint.

The cases are quantised (tests/conv_epilogue_cases.py; tests/test_conv_epilogue_cases_cpu.py pins
without a device that each reaches its kernel, is exact in f32 and has pre-activations exactly
on 0 and on 6), so None / ReLU / ReLU6 / LeakyReLU are compared with torch.equal against the
reference rounded once to the output dtype.  Sigmoid / Tanh are compared at the project's output
tolerances (tests/test_gpu_conv_generic.py::OUT_TOL), all of which goes to the device's exp /
tanh; each comparison prints its worst error as a fraction of the tolerance (pytest -s), recorded
in profiles/conv_epilogue_cases.txt.

Non-finite inputs: the epilogue call is compared with the reference applied to the same kernel's
own plain f32 output, which factors out where the conv itself puts NaN / inf."""
import os

import numpy as np
import pytest
import torch

import conv_epilogue_cases as CE

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from HyGrid import HexModules as HM  # noqa: E402
from HyGrid import ops  # noqa: E402
from oracle import oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
OUT_TOL = {CE.F32: 1e-5, CE.BF16: 2.0 ** -8, CE.F16: 2.0 ** -11, CE.F64: 1e-12}
ALL_ACTS = CE.EXACT_ACTS + CE.SMOOTH_ACTS
ACT_IDS = [a[0] for a in ALL_ACTS]


def close(got, ref, rtol, what, atol_rel=None):
    """assert_allclose(rtol, atol = atol_rel max|ref|), atol_rel = rtol unless given; prints the
    worst |err| / (atol + rtol |ref|) (tests/test_gpu_conv_generic.py::close)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = (rtol if atol_rel is None else atol_rel) * max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    ratio = float((err / (atol + rtol * np.abs(ref))).max()) if err.size else 0.0
    print(f"{what}: worst |err| / tolerance {ratio:.3f} (max err {err.max():.3e}, "
          f"max|ref| {np.abs(ref).max():.3e}, rtol {rtol:.1e})")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)


class _env:
    """A/B switches around a call (tests/test_gpu_conv_generic.py::_env)."""

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


def _t(a, dt=CE.F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def run(case, t, epi, x=None, out_dtype=None, env=None):
    """hg_hexconv2d_epilogue (hg_hexconv2d when epi is None) on the case's layer."""
    x = t["x"].to(DEV) if x is None else x
    with _env(case.env if env is None else env):
        return ops.hexconv2d(x, t["k"].to(DEV), t["b"].to(DEV), case.off, case.r, case.s, case.p,
                             case.d, case.g, case.mode, case.pv,
                             out_dtype=case.y_dt if out_dtype is None else out_dtype, epilogue=epi)


def device_epilogue(case, t, act, slope):
    sc, sf = CE.affine(t, act)
    return (_t(sc, case.w_dt).to(DEV), _t(sf, case.w_dt).to(DEV), act, slope)


def first_bad(got, want, pre):
    """The first (b, o, row, col) where got != want, with both values and whether the
    pre-activation there was 0, 6 or neither."""
    bad = torch.nonzero(~((got == want) | (got.isnan() & want.isnan())))
    if len(bad) == 0:
        return "no element differs"
    i = tuple(int(j) for j in bad[0])
    p = float(pre[i])
    where = "exactly 0" if p == 0 else "exactly 6" if p == 6 else "neither 0 nor 6"
    return (f"{len(bad)} of {got.numel()} differ, first at (b, o, row, col) = {i}: got "
            f"{float(got[i])!r}, want {float(want[i])!r}, pre-activation {p!r} ({where})")


# ---- forward, every case x every activation ---------------------------------------------------
@pytest.mark.parametrize("act_id,act,slope", CE.EXACT_ACTS, ids=[a[0] for a in CE.EXACT_ACTS])
@pytest.mark.parametrize("case", CE.CASES, ids=repr)
def test_forward_bit_exact(case, act_id, act, slope):
    t, _ = CE.data(case.name)
    want = _t(CE.expected(case.name, act, slope), case.y_dt)      # rounded once, to nearest even
    y = run(case, t, device_epilogue(case, t, act, slope)).cpu()
    assert y.dtype == case.y_dt and y.shape == want.shape
    assert torch.equal(y, want), f"{case.name} {act_id}: " + first_bad(y, want, CE.preact(case.name))


@pytest.mark.parametrize("act_id,act,slope", CE.SMOOTH_ACTS, ids=[a[0] for a in CE.SMOOTH_ACTS])
@pytest.mark.parametrize("case", CE.CASES, ids=repr)
def test_forward_sigmoid_tanh(case, act_id, act, slope):
    t, _ = CE.data(case.name)
    ref = CE.expected(case.name, act, slope)
    y = run(case, t, device_epilogue(case, t, act, slope))
    assert y.dtype == case.y_dt
    close(y.double().cpu().numpy(), ref, OUT_TOL[case.y_dt], f"{case.name} [{case.route}] {act_id}")


# ---- non-finite inputs ------------------------------------------------------------------------
@pytest.mark.parametrize("act_id,act,slope", ALL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("name", CE.NONFINITE)
def test_nonfinite(name, act_id, act, slope):
    case = CE.BY_NAME[name]
    t, _ = CE.data(name)
    x = CE.nonfinite_input(case, t).to(DEV)
    # the same kernel without an epilogue, f32 out (the stream layers off the two-column kernel,
    # which an epilogue call never takes)
    plain_env = dict(case.env, HYGRID_FCONV="0") if case.route == "stream" else case.env
    y0 = run(case, t, None, x=x, out_dtype=CE.F32, env=plain_env).double().cpu().numpy()
    sc, sf = CE.affine(t, act)
    pre = CE.epilogue_ref(y0, sc, sf, CE.NONE)
    assert np.isnan(pre).any() and (pre == np.inf).any() and (pre == -np.inf).any(), \
        "ReLU / ReLU6 see NaN, ReLU6 sees +inf, ReLU sees -inf"
    assert np.isfinite(pre).mean() > 0.5
    ref = CE.activation_ref(pre, act, slope)
    y = run(case, t, device_epilogue(case, t, act, slope), x=x, out_dtype=CE.F32)
    got = y.double().cpu().numpy()
    what = f"{name} [{case.route}] {act_id}"
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), \
        f"{what}: NaN at {int(nan_g.sum())} outputs, reference at {int(nan_r.sum())}; first " \
        f"difference at {tuple(np.argwhere(nan_g != nan_r)[0])}"
    assert np.array_equal(np.isinf(got), np.isinf(ref)), f"{what}: inf positions"
    inf = np.isinf(ref)
    assert np.array_equal(np.sign(got[inf]), np.sign(ref[inf])), f"{what}: inf signs"
    fin = np.isfinite(ref)
    if act in (CE.SIGMOID, CE.TANH):
        close(got[fin], ref[fin], OUT_TOL[CE.F32], what)
    else:
        want = ref.astype(np.float32).astype(np.float64)
        assert np.array_equal(got[fin], want[fin]), f"{what}: " + first_bad(
            torch.from_numpy(np.where(fin, got, 0.0)), torch.from_numpy(np.where(fin, want, 0.0)), pre)


# ---- HexConvModule's fused path ---------------------------------------------------------------
ACT_CFG = {"affine": None, "relu": dict(type="ReLU"), "relu6": dict(type="ReLU6"),
           "leaky0.25": dict(type="LeakyReLU", negative_slope=0.25),
           "leaky0": dict(type="LeakyReLU", negative_slope=0.0),
           "leaky2": dict(type="LeakyReLU", negative_slope=2.0),
           "sigmoid": dict(type="Sigmoid"), "tanh": dict(type="Tanh")}


def make_module(layer, act_id, act, *, bias="auto", norm=True, padding_mode="zeros"):
    """An eval HexConvModule on the layer's quantised tensors whose frozen BatchNorm folds to
    exactly the layer's (scale, shift), times SQUASH for the smooth activations: eps 0, running
    variance 1 or 4, weight scale sqrt(var) (negative where scale is), running mean a whole
    number mm and bias shift + mm scale."""
    d = CE.module_data(layer)
    C, O_, g, p, h, w = CE.MODULE_LAYERS[layer]
    m = HM.HexConvModule(C, O_, 0, 2, padding=p, groups=g, bias=bias,
                         norm_cfg=dict(type="BN") if norm else None, act_cfg=ACT_CFG[act_id],
                         padding_mode=padding_mode).to(DEV).eval()
    q = CE.SQUASH if act in (CE.SIGMOID, CE.TANH) else 1.0
    scale, shift = d["scale"] * q, d["shift"] * q
    with torch.no_grad():
        m.conv.kernel.copy_(d["k"])
        if m.conv.bias is not None:
            m.conv.bias.copy_(d["b"])
        if norm:
            bn = m.norm
            bn.eps = 0.0
            o = torch.arange(O_, dtype=CE.F64)
            var, mm = 1.0 + 3.0 * (o % 2), (o % 5) - 2
            bn.running_var.copy_(var)
            bn.running_mean.copy_(mm)
            bn.weight.copy_(scale * var.sqrt())
            bn.bias.copy_(shift + mm * scale)
    for prm in m.parameters():
        prm.requires_grad_(False)
    m.conv.kernel.requires_grad_(True)
    if m.conv.bias is not None:
        m.conv.bias.requires_grad_(True)
    return m, scale.numpy(), shift.numpy()


@pytest.mark.parametrize("act_id,act,slope", ALL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("layer", list(CE.MODULE_LAYERS))
def test_module_forward_backward(layer, act_id, act, slope):
    """conv + bias -> frozen eval BN -> act through the fused Function, forward and the three
    gradients, against epilogue_ref and the oracle's adjoint on gy act'(v) scale."""
    d = CE.module_data(layer)
    m, scale, shift = make_module(layer, act_id, act, bias=True)
    x = d["x"].float().to(DEV).requires_grad_(True)
    assert m._epilogue_plan(x, True, True) is not None
    y = m(x)
    y.backward(d["gy"].float().to(DEV))
    pre = CE.epilogue_ref(d["v"], scale, shift, CE.NONE)
    ref = CE.activation_ref(pre, act, slope)
    g = d["gy"].numpy() * CE.act_grad_ref(pre, act, slope) * scale[None, :, None, None]
    grads = O.hexconv2d_backward(d["x"].numpy(), d["k"].numpy(), g, 0, 2, 1, d["p"], 1, d["g"])
    got = (x.grad, m.conv.kernel.grad, m.conv.bias.grad)
    what = f"module {layer} {act_id}"
    if act in (CE.SIGMOID, CE.TANH):
        close(y.detach().double().cpu().numpy(), ref, OUT_TOL[CE.F32], what)
        for a, r, part in zip(got, grads, ("dx", "dkernel", "dbias")):
            close(a.double().cpu().numpy().reshape(r.shape), r, 1e-4, f"{what} {part}", atol_rel=1e-5)
        return
    yc = y.detach().cpu()
    assert torch.equal(yc, _t(ref, CE.F32)), f"{what}: " + first_bad(yc, _t(ref, CE.F32), pre)
    for a, r, part in zip(got, grads, ("dx", "dkernel", "dbias")):
        a = a.double().cpu().reshape(r.shape)
        assert torch.equal(a, _t(r)), f"{what} {part}: max |err| {float((a - _t(r)).abs().max())}"


def _module_forward_ref(d, scale, shift, act, slope, x=None, bias=True, pad=None):
    x = d["x"].numpy() if x is None else x
    v = O.hexconv2d(x, d["k"].numpy(), d["b"].numpy() if bias else None, 0, 2, 1,
                    d["p"] if pad is None else pad, 1, d["g"], "constant", 0.0)
    return CE.epilogue_ref(v, scale, shift, act, slope)


@pytest.mark.parametrize("flag", ["bias_and_bn", "no_bias_bn", "activate_false", "norm_false",
                                  "reflect", "input_3d"])
def test_module_flags_reach_the_fused_path(flag):
    """The module's flags and layouts on the fused path, forward, bit for bit (LeakyReLU 0.25 on
    the generic layer; eval BN with negative weights throughout)."""
    layer, act_id, act, slope = "generic", "leaky0.25", CE.LEAKY, 0.25
    d = CE.module_data(layer)
    bias = "auto" if flag == "no_bias_bn" else True
    m, scale, shift = make_module(layer, act_id, act, bias=bias,
                                  padding_mode="reflect" if flag == "reflect" else "zeros")
    assert (m.conv.bias is None) == (flag == "no_bias_bn") and bool((m.norm.weight < 0).any())
    x = d["x"].float().to(DEV)
    activate, norm = flag != "activate_false", flag != "norm_false"
    if flag == "input_3d":
        x = x[0]
    with torch.no_grad():
        assert m._epilogue_plan(x, activate, norm) is not None
        y = m(x, activate=activate, norm=norm).cpu()
    xn = d["x"].numpy()[:1] if flag == "input_3d" else d["x"].numpy()
    pad = None
    if flag == "reflect":      # the explicit padding layer (nn.ReflectionPad2d), then an unpadded conv
        assert m.with_explicit_padding and m.conv.pad == 0
        xn = np.pad(xn, ((0, 0), (0, 0), (d["p"],) * 2, (d["p"],) * 2), mode="reflect")
        pad = 0
    ref = _module_forward_ref(d, scale if norm else None, shift if norm else None,
                              act if activate else CE.NONE, slope, x=xn,
                              bias=flag != "no_bias_bn", pad=pad)
    want = _t(ref, CE.F32)
    assert y.shape == want.shape
    pre = _module_forward_ref(d, scale if norm else None, shift if norm else None, CE.NONE, 0.0,
                              x=xn, bias=flag != "no_bias_bn", pad=pad)
    assert torch.equal(y, want), f"{flag}: " + first_bad(y, want, pre)
