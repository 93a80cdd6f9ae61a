"""The fused HexConv2d epilogue, act(scale[o] * v + shift[o]) (hg_hexconv2d_epilogue; epi_apply
in csrc/common.h, called from the store of every forward conv kernel), stated once in NumPy fp64
together with its derivative, and a table of quantised layers on which the pre-activation is
exact on every kernel, so that the piecewise-linear activations can be compared bit for bit.

Shared by tests/test_gpu_conv_epilogue.py (runs the table on the device),
tests/test_conv_epilogue_cases_cpu.py (checks without a device that every case reaches the kernel
it is filed under, meets the threshold conditions below and is exact in f32, and pins the two
reference functions to torch.nn and its autograd) and tests/conv_generic_cases.py::reference.

Quantisation.  Inputs are whole numbers in -4..4, weights in -2..2, the bias in -3..3; scale[o]
is +-2^k with the (sign, k) pairs distinct across the channels of a layer (k runs over
ceil(O / 2) consecutive exponents around 0, so both signs of every exponent are used before one
repeats); shift[o] = m max(1/4, 2^k) with m a whole number in -3..3, a multiple of 1/4.  Every
partial sum of the conv is a whole number below 2^11 in magnitude (C <= 16, K <= 19), exact in
f32 in any order; the inputs and weights are exact in bf16 and f16, so the split-weight bf16
MFMA kernels are exact too; scale * v is exact (a power of two) and scale * v + shift is
(v + m) 2^k for k >= -2 and a multiple of 2^k below 2^(k + 24) otherwise.  LeakyReLU slopes are
0.25, 0 and 2.0.  The result of None / ReLU / ReLU6 / LeakyReLU must therefore equal the fp64
reference rounded once to the output dtype.

Conditions on every case (asserted on the CPU): at least 8 pre-activations exactly 0, at least 8
exactly 6, and elements in each of v < 0, 0 < v < 6, v > 6.  For Sigmoid / Tanh the scale and
the shift are multiplied by SQUASH = 1/32 (still exact), which brings at least half of the
pre-activations into (-4, 4).

Not a conftest and not a test: imported like tests/conv_generic_cases.py."""
import functools
import zlib

import numpy as np
import torch

from oracle import oracle as O

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NONE, RELU, LEAKY, RELU6, SIGMOID, TANH = range(6)          # enum hg_act
SQUASH = 1.0 / 32

# (id, act, slope): compared bit for bit / at the output tolerance
EXACT_ACTS = [("affine", NONE, 0.0), ("relu", RELU, 0.0), ("relu6", RELU6, 0.0),
              ("leaky0.25", LEAKY, 0.25), ("leaky0", LEAKY, 0.0), ("leaky2", LEAKY, 2.0)]
SMOOTH_ACTS = [("sigmoid", SIGMOID, 0.0), ("tanh", TANH, 0.0)]


# ---- the epilogue and its derivative, torch's rules -------------------------------------------
def _per_channel(a, ndim):
    a = np.asarray(a, np.float64)
    return a.reshape((1, -1) + (1,) * (ndim - 2)) if a.ndim == 1 and ndim >= 2 else a


def activation_ref(v, act, slope=0.0):
    """act(v) in fp64 as torch computes it: ReLU is clamp_min(v, 0) and ReLU6 clamp(v, 0, 6),
    both of which keep NaN (and -0.0); LeakyReLU is v > 0 ? v : v * slope (NaN stays NaN,
    -inf * 0 is NaN); Sigmoid and Tanh in fp64."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if act == NONE:
            return v.copy()
        if act == RELU:
            return np.where(v < 0, 0.0, v)
        if act == RELU6:
            return np.where(v < 0, 0.0, np.where(v > 6, 6.0, v))
        if act == LEAKY:
            return np.where(v > 0, v, v * slope)
        if act == SIGMOID:
            return 1.0 / (1.0 + np.exp(-v))
        if act == TANH:
            return np.tanh(v)
    raise ValueError(f"unknown hg_act {act}")


def epilogue_ref(v, scale, shift, act, slope=0.0):
    """act(scale[o] * v + shift[o]) in fp64; v is (B, O, ...) (or any array with scalar scale /
    shift), scale / shift are (O,) arrays or None."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if scale is not None:
            v = v * _per_channel(scale, v.ndim)
        if shift is not None:
            v = v + _per_channel(shift, v.ndim)
    return activation_ref(v, act, slope)


def act_grad_ref(v, act, slope=0.0):
    """d act / d pre-activation in fp64 from the pre-activation v, as torch's backward formulas
    give it: ReLU v > 0, ReLU6 0 < v < 6, LeakyReLU v > 0 ? 1 : slope, Sigmoid s (1 - s), Tanh
    1 - t^2.  At NaN: torch's threshold_backward tests `v <= 0`, so ReLU passes the gradient (1);
    ReLU6 gives 0 and LeakyReLU the slope; Sigmoid and Tanh give NaN."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if act == NONE:
            return np.ones_like(v)
        if act == RELU:
            return np.where(v <= 0, 0.0, 1.0)
        if act == RELU6:
            return np.where((v > 0) & (v < 6), 1.0, 0.0)
        if act == LEAKY:
            return np.where(v > 0, 1.0, float(slope))
        if act == SIGMOID:
            s = 1.0 / (1.0 + np.exp(-v))
            return s * (1.0 - s)
        if act == TANH:
            t = np.tanh(v)
            return 1.0 - t * t
    raise ValueError(f"unknown hg_act {act}")


# ---- quantised data ---------------------------------------------------------------------------
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64).double()


def quantised_affine(gen, n, exps=None):
    """(scale, shift) fp64 tensors of n channels: scale +-2^k, the (sign, k) pairs distinct (k
    over ceil(n / 2) consecutive exponents around 0, or drawn from exps, then not distinct);
    shift m max(1/4, 2^k), m in -3..3.  One channel: scale -1."""
    if exps is None:
        ne = -(-n // 2)
        pairs = [(sg, k) for k in range(-(ne // 2), ne - ne // 2) for sg in (1.0, -1.0)]
        order = torch.randperm(len(pairs), generator=gen).tolist()[:n]
        pairs = [pairs[i] for i in order]
        if n == 1:
            pairs = [(-1.0, 0)]
    else:
        ks = torch.randint(0, len(exps), (n,), generator=gen).tolist()
        sg = torch.randint(0, 2, (n,), generator=gen).tolist()
        pairs = [(1.0 if s else -1.0, exps[k]) for s, k in zip(sg, ks)]
        pairs[0] = (-1.0, pairs[0][1])                       # a negative one always
    m = _ints(gen, (n,), -3, 3)
    scale = torch.tensor([sg * 2.0 ** k for sg, k in pairs], dtype=F64)
    unit = torch.tensor([max(0.25, 2.0 ** k) for _, k in pairs], dtype=F64)
    return scale, m * unit


ROUTES = ("stream", "lds", "direct", "mfma_f32", "mfma_bf16", "mfma_bf16_dma", "mfma_f32_s2",
          "mfma_bf16_s2")


class Case:
    """One layer: x (B, C, h, w) of x_dt, kernel (O, C/g, 1, K) of w_dt, y of y_dt; radius r,
    stride s, constant zero padding p, groups g, row-parity offset off; route: the kernel it is
    filed under (ROUTES); env: the A/B switches the call runs under; ocb: the k_hexconv
    instantiation an "lds" case names."""

    def __init__(self, name, route, B, C, O_, h, w, *, r=2, s=1, p=1, g=1, off=0, x_dt=F32,
                 y_dt=F32, w_dt=F32, env=None, ocb=None):
        assert route in ROUTES
        self.name, self.route = name, route
        self.B, self.C, self.O, self.h, self.w = B, C, O_, h, w
        self.r, self.s, self.p, self.g, self.off = r, s, p, g, off
        self.d, self.mode, self.pv = 1, "constant", 0.0
        self.x_dt, self.y_dt, self.w_dt = x_dt, y_dt, w_dt
        self.env = dict(env or {})
        self.ocb = ocb
        self.cg, self.og = C // g, O_ // g
        self.K = 3 * r * r - 3 * r + 1

    def __repr__(self):
        return self.name

    def out_shape(self):
        return O.hexconv2d_out_shape(self.h, self.w, self.r, self.s, self.p, self.d)

    def inputs(self):
        """Seeded CPU tensors x, k, b, scale, shift (module docstring), in their dtypes."""
        gen = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        x = _ints(gen, (self.B, self.C, self.h, self.w), -4, 4).to(self.x_dt)
        k = _ints(gen, (self.O, self.cg, 1, self.K), -2, 2).to(self.w_dt)
        b = _ints(gen, (self.O,), -3, 3).to(self.w_dt)
        scale, shift = quantised_affine(gen, self.O)
        return dict(x=x, k=k, b=b, scale=scale.to(self.w_dt), shift=shift.to(self.w_dt))


def _np(t):
    return None if t is None else t.double().numpy()


@functools.lru_cache(maxsize=None)
def data(name):
    """(inputs, fp64 conv + bias output) of a case, computed once and left unchanged."""
    c = BY_NAME[name]
    t = c.inputs()
    v = O.hexconv2d(_np(t["x"]), _np(t["k"]), _np(t["b"]), c.off, c.r, c.s, c.p, c.d, c.g, c.mode,
                    c.pv)
    v.setflags(write=False)
    return t, v


def affine(t, act):
    """(scale, shift) fp64 arrays the call gets for this activation: times SQUASH for the smooth
    ones."""
    q = SQUASH if act in (SIGMOID, TANH) else 1.0
    return _np(t["scale"]) * q, _np(t["shift"]) * q


def preact(name, act=NONE):
    t, v = data(name)
    return epilogue_ref(v, *affine(t, act), NONE)


def expected(name, act, slope):
    """fp64 reference of the epilogue call."""
    t, v = data(name)
    return epilogue_ref(v, *affine(t, act), act, slope)


CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- k_hexconv_stream: 9 x 70 input, two column windows with a ragged second one --------------
# every (channels, padding, offset) instantiation, the dtype pairs dealt round over them so that
# each pair meets each channel layout and each padding
_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F32)]
_n = 0
for _C, _O, _g in [(3, 3, 1), (3, 3, 3), (1, 1, 1)]:
    for _p in (0, 1, 2):
        for _off in (0, 1):
            _x, _y = _PAIRS[(_n + _n // 6) % 4]
            _n += 1
            add(f"stream_{_C}_{_O}_g{_g}_p{_p}_off{_off}", "stream", 2, _C, _O, 9, 70, p=_p, g=_g,
                off=_off, x_dt=_x, y_dt=_y)

# ---- k_hexconv: one ragged tile per case, each OCB instantiation -------------------------------
add("lds_depthwise6", "lds", 2, 6, 6, 10, 40, g=6, ocb=1)
add("lds_12_4_g2", "lds", 2, 12, 4, 10, 40, g=2, off=1, ocb=2)
add("lds_14_6_g2", "lds", 2, 14, 6, 10, 40, g=2, p=0, ocb=3)
add("lds_7_5", "lds", 2, 7, 5, 10, 40, off=1, ocb=4)
add("lds_7_5_f16", "lds", 2, 7, 5, 11, 37, p=2, x_dt=F16, y_dt=F16, ocb=4)
add("lds_7_5_bf16", "lds", 2, 7, 5, 11, 37, p=0, off=1, y_dt=BF16, ocb=4)
add("lds_8_8_g2_r3", "lds", 2, 8, 8, 10, 40, r=3, p=2, g=2, ocb=4)
add("lds_5_6_f64", "lds", 2, 5, 6, 10, 40, off=1, x_dt=F64, y_dt=F64, w_dt=F64, ocb=4)

# ---- k_hexconv_direct --------------------------------------------------------------------------
add("direct_6_4_s3_g2", "direct", 2, 6, 4, 59, 149, s=3, g=2)

# ---- f32 matrix-core kernel, stride 1 ----------------------------------------------------------
add("mfma_16_32", "mfma_f32", 2, 16, 32, 12, 40)
add("mfma_16_80", "mfma_f32", 1, 16, 80, 11, 39, off=1)       # four channel tiles, o >= O lanes
add("mfma_f16_cols_vec", "mfma_f32", 2, 16, 32, 12, 40, x_dt=F16, y_dt=F16)          # wo % 4 == 0
add("mfma_f16_cols_tail", "mfma_f32", 2, 16, 32, 12, 39, p=2, off=1, x_dt=F16, y_dt=F16)

# ---- bf16 matrix-core kernels: register-staged (odd width or HYGRID_CONV_DMA=0) and LDS-DMA ----
add("mfma_bf16_odd", "mfma_bf16", 2, 16, 32, 12, 39, x_dt=BF16, y_dt=BF16)
add("mfma_bf16_dma_off_f32", "mfma_bf16", 2, 16, 32, 12, 40, p=0, off=1, x_dt=BF16, y_dt=F32,
    env={"HYGRID_CONV_DMA": "0"})
add("mfma_bf16_dma", "mfma_bf16_dma", 2, 16, 32, 12, 40, off=1, x_dt=BF16, y_dt=BF16)
add("mfma_bf16_dma_f32", "mfma_bf16_dma", 2, 16, 32, 12, 38, p=2, x_dt=BF16, y_dt=F32)

# ---- stride-2 matrix-core kernels --------------------------------------------------------------
add("mfma_s2_f32_p0", "mfma_f32_s2", 2, 16, 16, 25, 81, s=2, p=0)
add("mfma_s2_f32_p1", "mfma_f32_s2", 2, 16, 16, 24, 78, s=2, p=1, off=1)
add("mfma_s2_bf16_p0", "mfma_bf16_s2", 2, 16, 16, 24, 80, s=2, p=0, off=1, x_dt=BF16, y_dt=BF16)
add("mfma_s2_bf16_p1", "mfma_bf16_s2", 2, 16, 16, 23, 79, s=2, p=1, x_dt=BF16, y_dt=BF16)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"

# ---- non-finite inputs: one case per kernel family ---------------------------------------------
NONFINITE = ["stream_3_3_g1_p1_off0", "stream_3_3_g3_p2_off1", "lds_7_5", "direct_6_4_s3_g2",
             "mfma_16_32", "mfma_bf16_odd", "mfma_bf16_dma_f32", "mfma_s2_f32_p1",
             "mfma_s2_bf16_p0"]


def nonfinite_points(c):
    """[(row, col, value)] of the input: NaN in the interior, +inf in the first and the last
    corner, -inf on the right border and at the column where the stream kernel's first window
    ends (61 / 62 owned columns), NaN on the top border; rows and columns far enough apart (the
    taps span 3 rows x 4 columns, times the stride) that each reaches outputs of its own."""
    h, w = c.h, c.w
    nan, inf = float("nan"), float("inf")
    edge = 61 if c.route == "stream" else (w // 4) * 3
    return [(h // 2, w // 4, nan), (0, 0, inf), (h - 1, w - 1, inf), (h // 2, w - 1, -inf),
            (h // 2, edge, -inf), (0, w // 2, nan)]


def nonfinite_input(c, t):
    """The case's x with nonfinite_points written into it: NaN into every channel, +-inf into
    channel 0 alone, so that an output sees one infinite product (+inf, -inf, or NaN at a zero
    weight) and not inf - inf."""
    x = t["x"].clone()
    for r, q, val in nonfinite_points(c):
        if val != val:
            x[:, :, r, q] = val
        else:
            x[:, 0, r, q] = val
    return x


# ---- HexConvModule layers (tests/test_gpu_conv_epilogue.py, module level) ----------------------
# name -> (C, O, groups, padding, h, w): a stream layer, a generic one, an MFMA one whose
# backward takes the matrix-core d input / d kernel kernels
MODULE_LAYERS = {"stream": (3, 3, 1, 1, 9, 70), "generic": (7, 5, 1, 1, 10, 40),
                 "mfma": (16, 32, 1, 1, 12, 40)}
MODULE_B = 2
MODULE_EXPS = (-1, 0, 1)


@functools.lru_cache(maxsize=None)
def module_data(layer):
    """Quantised tensors of a module layer: x, k, b, scale, shift and a whole-number upstream
    gradient gy in -4..4 that is non-zero wherever the pre-activation is exactly 0 or 6; and v,
    the fp64 conv + bias output.  scale is +-2^k with k in MODULE_EXPS (not distinct), so that
    with the slopes 0.25 and 2.0 every gradient sum is a multiple of 2^-3 below 2^17: exact in
    f32 in any order."""
    C, O_, g, p, h, w = MODULE_LAYERS[layer]
    gen = torch.Generator().manual_seed(zlib.crc32(("module_" + layer).encode()))
    x = _ints(gen, (MODULE_B, C, h, w), -4, 4)
    k = _ints(gen, (O_, C // g, 1, 7), -2, 2)
    b = _ints(gen, (O_,), -3, 3)
    scale, shift = quantised_affine(gen, O_, MODULE_EXPS)
    v = O.hexconv2d(x.numpy(), k.numpy(), b.numpy(), 0, 2, 1, p, 1, g, "constant", 0.0)
    gy = _ints(gen, v.shape, -4, 4)
    pre = epilogue_ref(v, scale.numpy(), shift.numpy(), NONE)
    at = torch.from_numpy((pre == 0) | (pre == 6))
    gy = torch.where(at & (gy == 0), torch.full_like(gy, 3.0), gy)
    v.setflags(write=False)
    return dict(x=x, k=k, b=b, scale=scale, shift=shift, gy=gy, v=v, p=p, g=g)
