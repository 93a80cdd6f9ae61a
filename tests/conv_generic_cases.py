"""The case table of the generic HexConv2d kernels (csrc/hexconv.hip: k_hexconv, the LDS kernel
with its channel-chunk, output-channel-block and batch loops, and k_hexconv_direct, the gather
fallback), shared by tests/test_gpu_conv_generic.py (which runs it against the fp64 oracle) and
tests/test_conv_generic_cases_cpu.py (which checks without a device, from the library's own plan
query hg_hexconv2d_generic_plan, that every case lies in the region it is filed under and that
the table as a whole reaches every region).

hg_hexconv2d tries two other kernels before the generic ones.  Every case here is refused by
both through one of their documented conditions, named per case:
  stream  (hexconv.hip, hg_hexconv2d_epilogue): taken only at radius 2, stride 1, dilation 1,
          constant padding, f32 weights, C <= 3 and O <= 3;
  mfma    (conv_mfma.hip, conv_mfma_try): taken only at groups 1, radius 2, stride 1,
          dilation 1, O >= 16, padding <= 2, f32 weights, and not with HYGRID_CONV_MFMA=0.
A case names the condition it relies on as (kernel, reason), reasons from REFUSALS below.

The table holds no cib / bc / tile numbers: a region is a predicate on the plan the library
reports (REGIONS), so a change of the LDS budget or the tile size fails the CPU test instead of
silently un-covering a loop.

Spatial sizes: 19-35 output rows x 130-140 output columns, i.e. 2 x 2 or 3 x 2 tiles of 16 x 128
with ragged last ones ("tiles"); one tile of about 5 x 6 for the batch-loop cases ("one"); the
direct kernel has no tiles, its cases are a few 256-sample blocks with a partial last one
("blocks").

Not a conftest and not a test: imported like tests/placement_cases.py."""
import zlib

import numpy as np
import torch

from conv_epilogue_cases import epilogue_ref
from oracle import oracle as O

BF16, F16, F32, F64, U8 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.uint8
NONE, RELU, LEAKY, RELU6, SIGMOID, TANH = range(6)          # enum hg_act

# reason -> predicate(case): the condition under which the kernel returns HG_EUNSUP / is skipped
REFUSALS = {
    "stream": {
        "C>3": lambda c: c.C > 3,
        "O>3": lambda c: c.O > 3,
        "radius": lambda c: c.r != 2,
        "stride": lambda c: c.s != 1,
        "dilation": lambda c: c.d != 1,
        "pad_mode": lambda c: c.mode != "constant",
        "f64": lambda c: c.w_dt == F64,
    },
    "mfma": {
        "groups": lambda c: c.g != 1,
        "radius": lambda c: c.r != 2,
        "stride": lambda c: c.s != 1,
        "dilation": lambda c: c.d != 1,
        "O<16": lambda c: c.O < 16,
        "f64": lambda c: c.w_dt == F64,
        "env": lambda c: c.mfma_off,
    },
}


class Case:
    """One layer and call: x (B, C, h, w) of x_dt, kernel (O, C/g, 1, K) of w_dt, y of y_dt;
    radius r, stride s, padding p (mode, pv), dilation d, groups g, row-parity offset off;
    bias: whether the call passes one; epi: None or (scale?, shift?, act, slope) — which of the
    per-channel affine terms hg_hexconv2d_epilogue gets, and the activation; mfma_off: run
    under HYGRID_CONV_MFMA=0; spatial: "tiles" / "one" / "blocks" (module docstring); regions:
    the REGIONS entries the case is filed under; stream / mfma: why those kernels refuse it."""

    def __init__(self, name, regions, B, C, O_, h, w, *, stream, mfma, r=2, s=1, p=1, d=1, g=1,
                 off=0, mode="constant", pv=0.0, w_dt=F32, x_dt=F32, y_dt=None, bias=True,
                 epi=None, mfma_off=False, spatial="tiles"):
        self.name, self.regions = name, tuple(regions)
        self.B, self.C, self.O, self.h, self.w = B, C, O_, h, w
        self.r, self.s, self.p, self.d, self.g, self.off = r, s, p, d, g, off
        self.mode, self.pv, self.w_dt, self.x_dt = mode, pv, w_dt, x_dt
        self.y_dt = w_dt if y_dt is None else y_dt
        self.bias, self.epi, self.mfma_off, self.spatial = bias, epi, mfma_off, spatial
        self.stream, self.mfma = stream, mfma
        self.cg, self.og = C // g, O_ // g
        self.K = 3 * r * r - 3 * r + 1

    def __repr__(self):
        return self.name

    def out_shape(self):
        return O.hexconv2d_out_shape(self.h, self.w, self.r, self.s, self.p, self.d)

    def plan(self):
        """The library's plan for this layer (hg_hexconv2d_generic_plan; nothing is launched)."""
        from HyGrid import _abi
        return _abi.hexconv2d_generic_plan(_abi.dtype_code(self.w_dt), self.B, self.C, self.O,
                                           self.h, self.w, self.r, self.s, self.p, self.d, self.g,
                                           self.off)

    def env(self):
        return {"HYGRID_CONV_MFMA": "0"} if self.mfma_off else {}

    def cfg(self):
        """The cfg dict of ops.hexconv2d_backward."""
        return dict(off=self.off, r=self.r, stride=self.s, pad=self.p, dilation=self.d,
                    groups=self.g, padding_mode=self.mode, padding_value=self.pv, out_dtype=None)

    def inputs(self, positive=False):
        """Seeded CPU tensors: x in [-0.5, 0.5) rounded to x_dt (u8: 0..255), weights and bias
        bounded by 1/sqrt(K cg) (tests/test_gpu_conv_mfma.py::_weights), the epilogue's scale in
        [0.5, 1.5) and shift in [-0.5, 0.5).  positive: x in [0, 1) and, as "gy", an upstream
        gradient in [0, 1) (tests/test_gpu_pipeline_backward.py: no d-kernel entry near 0)."""
        gen = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        shape = (self.B, self.C, self.h, self.w)
        if self.x_dt == U8:
            x = torch.randint(0, 256, shape, generator=gen, dtype=U8)
        else:
            x = (torch.rand(shape, generator=gen, dtype=F64) - (0.0 if positive else 0.5)).to(self.x_dt)
        bound = 1.0 / np.sqrt(self.K * self.cg)
        k = ((torch.rand((self.O, self.cg, 1, self.K), generator=gen, dtype=F64) * 2 - 1) * bound)
        b = ((torch.rand((self.O,), generator=gen, dtype=F64) * 2 - 1) * bound)
        t = dict(x=x, k=k.to(self.w_dt), b=b.to(self.w_dt) if self.bias else None)
        if self.epi is not None:
            sc = (torch.rand((self.O,), generator=gen, dtype=F64) + 0.5).to(self.w_dt)
            sf = (torch.rand((self.O,), generator=gen, dtype=F64) - 0.5).to(self.w_dt)
            t["scale"] = sc if self.epi[0] else None
            t["shift"] = sf if self.epi[1] else None
        if positive:
            ho, wo = self.out_shape()
            t["gy"] = torch.rand((self.B, self.O, ho, wo), generator=gen, dtype=F64).to(self.w_dt)
        return t


def _np(t):
    return None if t is None else t.double().numpy()


def reference(case, t):
    """fp64: the oracle conv on the inputs as rounded to their dtypes, then the affine and the
    activation in NumPy (tests/conv_epilogue_cases.py::epilogue_ref, every hg_act)."""
    y = O.hexconv2d(_np(t["x"]), _np(t["k"]), _np(t["b"]), case.off, case.r, case.s, case.p,
                    case.d, case.g, case.mode, case.pv)
    if case.epi is not None:
        _, _, act, slope = case.epi
        y = epilogue_ref(y, _np(t["scale"]), _np(t["shift"]), act, slope)
    return y


def reference_backward(case, t):
    """fp64 (dx, dkernel, dbias) of the oracle's adjoint for t = case.inputs(positive=True)."""
    return O.hexconv2d_backward(_np(t["x"]), _np(t["k"]), _np(t["gy"]), case.off, case.r, case.s,
                                case.p, case.d, case.g, case.mode, case.pv)


# ---- regions: predicates on (case, plan) ------------------------------------------------------
def _lds(c, P):
    return not P["direct"]


def _multi(c, P):
    return _lds(c, P) and 0 < P["cib"] < c.cg


def _exact(c, P):
    return _multi(c, P) and c.cg % P["cib"] == 0


def _ragged(c, P):
    return _multi(c, P) and c.cg % P["cib"] != 0


def _dense_r2(c):
    return c.r == 2 and c.s == 1 and c.d == 1 and c.g == 1


def _plain(c):
    """f32 in, f32 weights, f32 out, no epilogue: the region is about the loops alone."""
    return c.x_dt == F32 and c.w_dt == F32 and c.y_dt == F32 and c.epi is None


def _batch(c, P, B):
    return (c.B == B and _lds(c, P) and P["tiles"] == 1 and P["bc"] >= 2 and c.B % P["bc"] != 0
            and c.spatial == "one")


def _epi(c, scale, shift):
    return c.epi is not None and bool(c.epi[0]) == scale and bool(c.epi[1]) == shift


REGIONS = {
    # multi-chunk k_hexconv: cg an exact multiple of cib, and cg leaving a ragged last chunk
    "r2_f32_exact": lambda c, P: _exact(c, P) and c.r == 2 and c.s == 1 and c.d == 1 and c.w_dt == F32,
    "r2_f32_ragged": lambda c, P: _ragged(c, P) and c.r == 2 and c.s == 1 and c.d == 1 and c.w_dt == F32,
    "r2_f64_exact": lambda c, P: _exact(c, P) and c.r == 2 and c.s == 1 and c.d == 1 and c.w_dt == F64,
    "r2_f64_ragged": lambda c, P: _ragged(c, P) and c.r == 2 and c.s == 1 and c.d == 1 and c.w_dt == F64,
    "r3_exact": lambda c, P: _exact(c, P) and c.r == 3 and c.s == 1 and c.d == 1,
    "r3_ragged": lambda c, P: _ragged(c, P) and c.r == 3 and c.s == 1 and c.d == 1,
    "d2_exact": lambda c, P: _exact(c, P) and c.d == 2 and c.s == 1,
    "d2_ragged": lambda c, P: _ragged(c, P) and c.d == 2 and c.s == 1,
    "r4_exact": lambda c, P: _exact(c, P) and c.r == 4 and c.s == 1 and c.d == 1,
    "r4_ragged": lambda c, P: _ragged(c, P) and c.r == 4 and c.s == 1 and c.d == 1,
    "s2_wide": lambda c, P: _multi(c, P) and c.s == 2 and P["cib"] == 1 and c.cg >= 8,
    # grouped wide layers: the OCB = 4 remainder (oc0 + j >= og) together with the group offset
    "g4_og5": lambda c, P: _lds(c, P) and c.g == 4 and c.cg >= 6 and c.og == 5 and P["ocb"] == 4,
    "g4_og6": lambda c, P: _lds(c, P) and c.g == 4 and c.cg >= 6 and c.og == 6 and P["ocb"] == 4,
    "g4_og7": lambda c, P: _lds(c, P) and c.g == 4 and c.cg >= 6 and c.og == 7 and P["ocb"] == 4,
    "depthwise24": lambda c, P: (_lds(c, P) and c.C == c.O == c.g == 24 and P["ocb"] == 1
                                 and P["cib"] == 1),
    "og2_multi": lambda c, P: _multi(c, P) and c.og == 2 and P["ocb"] == 2,
    "og3_multi": lambda c, P: _multi(c, P) and c.og == 3 and P["ocb"] == 3,
    # each padding mode at cg > cib
    "pad_reflect2": lambda c, P: _multi(c, P) and c.mode == "reflect" and c.p == 2,
    "pad_circular2": lambda c, P: _multi(c, P) and c.mode == "circular" and c.p == 2,
    "pad_replicate": lambda c, P: _multi(c, P) and c.mode == "replicate" and c.p >= 1,
    "pad_const_value": lambda c, P: _multi(c, P) and c.mode == "constant" and c.p >= 1 and c.pv != 0.0,
    # dense radius-2 layers the MFMA kernel would take or nearly take
    "dense_natural": lambda c, P: _multi(c, P) and _dense_r2(c) and c.O < 16 and _plain(c) and not c.mfma_off,
    "dense_mfma_off": lambda c, P: _multi(c, P) and _dense_r2(c) and c.O >= 16 and _plain(c) and c.mfma_off,
    # batch loop: several images per workgroup, a short last workgroup
    "batch_2051": lambda c, P: _batch(c, P, 2051),
    "batch_4100": lambda c, P: _batch(c, P, 4100),
    # k_hexconv_direct with real channel structure
    "direct_s3_grouped": lambda c, P: (P["direct"] and c.s == 3 and c.r == 2 and c.g == 2 and c.cg >= 5
                                       and c.og >= 3 and c.w_dt == F32),
    "direct_s2_f64": lambda c, P: P["direct"] and c.s == 2 and c.w_dt == F64 and c.g == 2 and c.cg >= 3,
    "direct_reflect": lambda c, P: P["direct"] and c.mode == "reflect" and c.p >= 1 and c.cg > 1,
    "direct_nobias": lambda c, P: P["direct"] and not c.bias and c.cg > 1,
    # input / output dtypes on a multi-chunk layer
    "in_bf16": lambda c, P: _multi(c, P) and c.x_dt == BF16,
    "in_f16": lambda c, P: _multi(c, P) and c.x_dt == F16,
    "in_u8": lambda c, P: _multi(c, P) and c.x_dt == U8,
    "in_f64": lambda c, P: _multi(c, P) and c.x_dt == F64 and c.w_dt == F32,
    "out_f32": lambda c, P: _multi(c, P) and c.y_dt == F32 and c.w_dt == F32,
    "out_bf16": lambda c, P: _multi(c, P) and c.y_dt == BF16,
    "out_f16": lambda c, P: _multi(c, P) and c.y_dt == F16,
    "out_f64_w64": lambda c, P: _multi(c, P) and c.y_dt == F64 and c.w_dt == F64,
    # the fused epilogue on a multi-chunk layer and on a direct-kernel layer
    "epi_scale": lambda c, P: _multi(c, P) and _epi(c, True, False),
    "epi_shift": lambda c, P: _multi(c, P) and _epi(c, False, True),
    "epi_both": lambda c, P: _multi(c, P) and _epi(c, True, True),
    "epi_leaky": lambda c, P: _multi(c, P) and c.epi is not None and c.epi[2] == LEAKY,
    "epi_sigmoid": lambda c, P: _multi(c, P) and c.epi is not None and c.epi[2] == SIGMOID,
    "epi_f64": lambda c, P: _multi(c, P) and c.epi is not None and c.w_dt == F64,
    "epi_direct": lambda c, P: P["direct"] and c.epi is not None and c.cg > 1,
}

CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- multi-chunk k_hexconv at stride 1 --------------------------------------------------------
add("r2_c10_o5", ["r2_f32_exact", "out_f32"], 2, 10, 5, 33, 131, stream="C>3", mfma="O<16")
add("r2_c13_o7_off1", ["r2_f32_ragged", "dense_natural"], 1, 13, 7, 23, 137, p=0, off=1,
    stream="C>3", mfma="O<16")
add("r2_c4_o3_f64", ["r2_f64_exact", "out_f64_w64", "og3_multi"], 1, 4, 3, 21, 133, w_dt=F64,
    x_dt=F64, off=1, stream="f64", mfma="f64")
add("r2_c5_o6_f64", ["r2_f64_ragged"], 2, 5, 6, 19, 130, w_dt=F64, x_dt=F64, stream="f64",
    mfma="f64")
add("r3_c20_o4", ["r3_exact"], 1, 20, 4, 23, 134, r=3, p=2, stream="radius", mfma="radius")
add("r3_c13_o6_off1", ["r3_ragged"], 1, 13, 6, 25, 137, r=3, p=1, off=1, stream="radius",
    mfma="radius")
add("d2_c10_o3", ["d2_exact"], 1, 10, 3, 23, 134, d=2, p=2, off=1, stream="dilation",
    mfma="dilation")
add("d2_r3_c7_o5", ["d2_ragged"], 1, 7, 5, 27, 140, r=3, d=2, p=1, stream="radius", mfma="radius")
add("r4_c8_o5", ["r4_exact"], 1, 8, 5, 23, 136, r=4, p=2, off=1, stream="radius", mfma="radius")
add("r4_c6_o2", ["r4_ragged", "og2_multi"], 1, 6, 2, 25, 138, r=4, p=1, stream="radius",
    mfma="radius")
# stride 2: one channel per pass
add("s2_c8_o8", ["s2_wide"], 1, 8, 8, 45, 270, s=2, stream="stride", mfma="stride")
add("s2_c9_o5_off1", ["s2_wide"], 1, 9, 5, 41, 266, s=2, p=0, off=1, stream="stride",
    mfma="stride")

# ---- grouped wide layers ----------------------------------------------------------------------
add("g4_24_28", ["g4_og7"], 2, 24, 28, 21, 131, g=4, stream="C>3", mfma="groups")
add("g4_24_20_off1", ["g4_og5"], 1, 24, 20, 19, 132, g=4, p=2, off=1, stream="C>3",
    mfma="groups")
add("g4_24_24_d2", ["g4_og6"], 1, 24, 24, 23, 134, g=4, d=2, p=1, stream="C>3", mfma="groups")
add("depthwise_24", ["depthwise24"], 2, 24, 24, 21, 131, g=24, off=1, stream="C>3",
    mfma="groups")
add("g2_12_4", ["og2_multi"], 1, 12, 4, 21, 131, g=2, stream="C>3", mfma="groups")
add("g2_14_6_off1", ["og3_multi"], 1, 14, 6, 21, 131, g=2, off=1, stream="C>3", mfma="groups")

# ---- each padding mode at cg > cib ------------------------------------------------------------
add("pad_reflect2_c7", ["pad_reflect2"], 1, 7, 5, 19, 130, p=2, mode="reflect", stream="pad_mode",
    mfma="O<16")
add("pad_circular2_c7_off1", ["pad_circular2"], 1, 7, 5, 19, 130, p=2, mode="circular", off=1,
    stream="pad_mode", mfma="O<16")
add("pad_replicate_c7", ["pad_replicate"], 1, 7, 5, 21, 131, p=1, mode="replicate", off=1,
    stream="pad_mode", mfma="O<16")
add("pad_value_c7", ["pad_const_value"], 1, 7, 5, 19, 130, p=2, pv=0.3, stream="C>3", mfma="O<16")

# ---- dense radius-2 layers --------------------------------------------------------------------
add("dense_37_12", ["dense_natural", "r2_f32_ragged"], 1, 37, 12, 21, 131, stream="C>3",
    mfma="O<16")
add("dense_32_48_mfma_off", ["dense_mfma_off"], 1, 32, 48, 21, 131, off=1, mfma_off=True,
    stream="C>3", mfma="env")

# ---- batch loop: one tile, several images per workgroup, a short last workgroup ---------------
add("batch_2051_reflect", ["batch_2051"], 2051, 2, 5, 5, 6, mode="reflect", spatial="one",
    stream="pad_mode", mfma="O<16")
add("batch_4100_g2", ["batch_4100"], 4100, 4, 6, 5, 6, g=2, off=1, spatial="one", stream="C>3",
    mfma="groups")

# ---- k_hexconv_direct -------------------------------------------------------------------------
add("direct_s3_10_6_g2", ["direct_s3_grouped"], 2, 10, 6, 40, 100, s=3, g=2, spatial="blocks",
    stream="stride", mfma="stride")
add("direct_s2_f64_6_8_g2", ["direct_s2_f64"], 1, 6, 8, 33, 77, s=2, g=2, off=1, w_dt=F64,
    x_dt=F64, spatial="blocks", stream="f64", mfma="f64")
add("direct_s3_reflect", ["direct_reflect"], 1, 5, 4, 37, 91, s=3, p=2, mode="reflect", off=1,
    spatial="blocks", stream="stride", mfma="stride")
add("direct_s4_r3_nobias", ["direct_nobias"], 1, 4, 6, 45, 120, r=3, s=4, g=2, bias=False,
    spatial="blocks", stream="radius", mfma="radius")

# ---- input / output dtypes on a multi-chunk layer (f32 weights) -------------------------------
add("in_bf16_out_f32", ["in_bf16", "out_f32"], 1, 7, 5, 21, 131, x_dt=BF16, stream="C>3",
    mfma="O<16")
add("in_bf16_out_bf16", ["in_bf16", "out_bf16"], 1, 7, 5, 21, 131, x_dt=BF16, y_dt=BF16, off=1,
    stream="C>3", mfma="O<16")
add("in_f16_out_f16", ["in_f16", "out_f16"], 1, 7, 5, 21, 131, x_dt=F16, y_dt=F16, stream="C>3",
    mfma="O<16")
add("in_u8_out_f32", ["in_u8", "out_f32"], 1, 7, 5, 21, 131, x_dt=U8, off=1, stream="C>3",
    mfma="O<16")
add("in_f64_out_f32", ["in_f64", "out_f32"], 1, 7, 5, 21, 131, x_dt=F64, stream="C>3",
    mfma="O<16")
add("in_f32_out_bf16_s2", ["out_bf16", "s2_wide"], 1, 8, 6, 41, 266, s=2, y_dt=BF16,
    stream="stride", mfma="stride")

# ---- fused epilogue ---------------------------------------------------------------------------
add("epi_scale_c7", ["epi_scale"], 1, 7, 5, 21, 131, epi=(True, False, NONE, 0.0), stream="C>3",
    mfma="O<16")
add("epi_shift_sigmoid_c7", ["epi_shift", "epi_sigmoid"], 1, 7, 5, 21, 131, off=1,
    epi=(False, True, SIGMOID, 0.0), stream="C>3", mfma="O<16")
add("epi_both_leaky_g2", ["epi_both", "epi_leaky"], 1, 12, 14, 21, 131, g=2,
    epi=(True, True, LEAKY, 0.1), stream="C>3", mfma="groups")
add("epi_both_leaky_f64", ["epi_f64", "epi_both", "epi_leaky"], 1, 5, 6, 19, 130, w_dt=F64,
    x_dt=F64, off=1, epi=(True, True, LEAKY, 0.2), stream="f64", mfma="f64")
add("epi_direct_s3", ["epi_direct"], 1, 6, 4, 40, 100, s=3, g=2, spatial="blocks",
    epi=(True, True, LEAKY, 0.1), stream="stride", mfma="stride")

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"

# ---- backward: ops.hexconv2d_backward on the wide cases ---------------------------------------
# slices = 4096 / O, the (cg K) / 16 pass count and the oo < og loop at width, grouped and dense
BACKWARD = ["g4_24_28", "depthwise_24", "s2_c8_o8", "r3_c13_o6_off1", "dense_37_12",
            "pad_reflect2_c7", "r2_c5_o6_f64"]
# (case, need_x, need_k, need_b): partial requests
BACKWARD_PARTIAL = [("g4_24_28", True, False, False), ("r3_c13_o6_off1", False, True, False)]
