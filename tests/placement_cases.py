"""The case table of the guard-band placement tests (tests/placement.py): one entry per kernel
route, shared by tests/test_gpu_placement.py (which runs it on the device) and
tests/test_placement_cpu.py (which checks without a device that the table covers every C-ABI
export with a destination pointer, that every placed tensor gets its guards, and that each
shape takes the kernel its entry names).

A Case names the exports whose destinations it covers, the sibling parity test whose tolerance
it borrows, seeded CPU inputs, the call, the expected outputs (shape, dtype) and an fp64
reference with one comparison per output.  Shapes are the smallest of the sibling's own list (or
built from hg_fused_layout the way tests/fused_variants.py builds them) with at least two row
bands, two column windows and a ragged last window, batch 2, so the start of the first image
and the end of the last one are real edges of the allocation.

Not a conftest and not a test: imported like tests/fused_variants.py."""
import numpy as np
import torch

from oracle import oracle as O
from pool_cases import pool_args

BF16, F16, F32, F64, U8 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.uint8
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11}

# exports whose only pointers are host out-parameters: nothing on the device to guard
EXEMPT = {
    "hg_fused_layout": "host-only query; band_rows / win_own / win_halo are host ints",
    "hg_hexconv2d_out_shape": "host-only shape rule; ho / wo are host int64s",
    "hg_hexconv2d_generic_plan": "host-only query; direct / cib / ocb / bc / tiles are host ints",
}


# ---- comparisons (the siblings' own forms) ---------------------------------------------------
def close(rtol, atol_rel=None):
    """assert_allclose(rtol, atol = atol_rel * max|ref|); atol_rel defaults to rtol
    (tests/test_gpu_parity.py::close)."""
    atol_rel = rtol if atol_rel is None else atol_rel

    def cmp(got, ref):
        scale = max(float(np.abs(ref).max()), 1e-30) if ref.size else 1.0
        np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale)
    return cmp


def absclose(tol):
    """assert_allclose(rtol = atol = tol) (tests/test_gpu_pool.py)."""
    def cmp(got, ref):
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol)
    return cmp


def one_rounding(ulp):
    """Per element |got - ref| <= ulp |ref| + 1e-5 max|ref| (tests/test_gpu_pipeline.py)."""
    def cmp(got, ref):
        tol = ulp * np.abs(ref) + 1e-5 * np.abs(ref).max()
        bad = np.abs(got - ref) > tol
        assert not bad.any(), (f"{int(bad.sum())} of {bad.size} beyond one rounding of the oracle "
                               f"(worst excess {float((np.abs(got - ref) - tol).max()):.3e})")
    return cmp


def maxnorm(ulp):
    """max|got - ref| <= ulp max|ref| (tests/test_gpu_down.py, _triup.py, _hexdown.py)."""
    def cmp(got, ref):
        assert np.abs(got - ref).max() <= ulp * max(float(np.abs(ref).max()), 1e-30)
    return cmp


def exact(got, ref):
    np.testing.assert_array_equal(got, ref)


def out_cmp(dt, fp32=1e-5):
    """fp32 / fp64 outputs at rtol 1e-5 of max|ref|, 16-bit ones at one rounding of the dtype."""
    return close(ULP[dt]) if dt in ULP else close(fp32)


class Case:
    """name; exports covered; sibling test (tolerance source); inputs() -> dict of CPU tensors;
    placed: the input names that are sources (placed in arenas), the rest are small parameters;
    run(t) -> list of outputs (None for a gradient not requested) or None when the op declines;
    outs: [(shape, dtype) | None]; ref(inp) -> list of fp64 arrays; cmp: one per output;
    atomic: outputs summed with float atomics (hygrid.h documents last-bit run-to-run
    differences: compared through the oracle instead of bit for bit); env: A/B switches set
    around every call; declines(src_bytes, dst_bytes): the placements at which the host code
    documents that the op returns HG_EUNSUP (ops returns None); route() -> (expected, actual)
    kernel codes from the library's own host-side query; workspace: the call takes a workspace
    slab, which the package allocates per (device, stream) and the test places as well."""

    def __init__(self, name, exports, sibling, inputs, placed, run, outs, ref, cmp, atomic=(),
                 env=None, declines=None, route=None, workspace=False):
        self.name, self.exports, self.sibling = name, tuple(exports), sibling
        self.inputs, self.placed, self.run, self.outs = inputs, tuple(placed), run, outs
        self.ref, self.cmp, self.atomic = ref, cmp, frozenset(atomic)
        self.env = env or {}
        self.declines = declines or (lambda src_bytes, dst_bytes: False)
        self.route = route
        self.workspace = workspace

    def __repr__(self):
        return self.name

    def placed_tensors(self):
        """(shape, dtype) of every tensor the GPU test puts in an arena."""
        inp = self.inputs()
        return ([(tuple(inp[k].shape), inp[k].dtype) for k in self.placed]
                + [o for o in self.outs if o is not None])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, dt, seed, lo=0.0):
    if dt == U8:   # no byte equals the integer sentinel 0xA5: a copied 0xA5 is then unwritten
        x = torch.randint(0, 256, shape, generator=_gen(seed), dtype=U8)
        x[x == 0xA5] = 0xA6
        return x
    return (torch.rand(shape, generator=_gen(seed)) + lo).to(dt)


def _np(t):
    return t.double().numpy()


def _layout(md):
    from HyGrid import _abi
    return _abi.fused_layout(md)


CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


# ---- fused chain forward: hg_pipeline_r2h_conv_h2r -------------------------------------------
def _chain_ref(inp, off, groups):
    h = O.rect_to_hex(_np(inp["x"]), None, 1)
    c = O.hexconv2d(h, _np(inp["k"]), _np(inp["b"]), off, 2, padding=1, groups=groups)
    return [O.hex_to_rect(c, None, 1)]


def fused_forward(name, sibling, B, C, H, W, off, groups, x_dt, y_dt, cmp):
    def inputs():
        return dict(x=_rand((B, C, H, W), x_dt, 7 * H + W),
                    k=_rand((C, C // groups, 1, 7), F32, 3 + off, -0.5),
                    b=_rand((C,), F32, 5 + off, -0.5))

    def run(t):
        from HyGrid import ops
        y = ops.pipeline_r2h_conv_h2r(t["x"], t["k"], t["b"], None, None, 1, groups, off, 0.0, y_dt)
        assert y is not None, "the fused kernel should cover this call"
        return [y]

    add(name, ["hg_pipeline_r2h_conv_h2r"], sibling, inputs, ["x"], run, [((B, C, H, W), y_dt)],
        lambda inp: _chain_ref(inp, off, groups), [cmp])


R6, OWN6, _ = _layout(6)
R0_, OWN0, _ = _layout(0)
# k_fused4: bf16, C = O = 3, w % 4 == 0; two bands and a ragged second window; the second shape
# has a whole odd band, which walks upwards (tests/fused_variants.py census)
fused_forward("fused4_off0", "tests/test_gpu_fused4.py::test_fused4_bit_identical_to_two_column_and_vs_oracle",
              2, 3, R6 + 7, OWN6 + 4, 0, 1, BF16, BF16, one_rounding(2.0 ** -8))
fused_forward("fused4_off1_up", "tests/test_gpu_fused4.py::test_fused4_bit_identical_to_two_column_and_vs_oracle",
              2, 3, 2 * R6 + 3, OWN6 + 8, 1, 1, BF16, BF16, one_rounding(2.0 ** -8))
# k_fused MD 0 (the shapes of fused_variants.md0_cases: rows + 7, own + 2)
fused_forward("fused_md0_f32", "tests/test_gpu_pipeline.py::test_fused_vs_oracle_fp32",
              2, 3, R0_ + 7, OWN0 + 2, 1, 3, F32, F32, close(1e-5))
fused_forward("fused_md0_f16", "tests/test_gpu_pipeline.py::test_fused_two_column_kernel_dtypes",
              2, 3, R0_ + 7, OWN0 + 2, 0, 1, F16, F16, one_rounding(2.0 ** -11))
fused_forward("fused_md0_bf16_c1", "tests/test_gpu_pipeline.py::test_fused_two_column_kernel_dtypes",
              2, 1, R0_ + 7, OWN0 + 2, 0, 1, BF16, BF16, one_rounding(2.0 ** -8))
# an odd width leaves the two-column kernel: the one-column kernel of pipeline.hip
fused_forward("fused_oddwidth_bf16", "tests/test_gpu_pipeline.py::test_fused_vs_oracle_fp32",
              2, 3, 70, 131, 1, 1, BF16, F32, close(1e-5))


# ---- fused chain backward: hg_pipeline_r2h_conv_h2r_backward ----------------------------------
TR, TC, BAND = _layout(9)
BWD = "tests/test_gpu_pipeline_backward.py::test_fp32_vs_oracle"
grad_close = close(1e-4, 1e-5)      # tests/test_gpu_pipeline_backward.py::grad_close


def fused_backward(name, sibling, B, C, H, W, off, groups, x_dt, gy_dt, need=(True, True, True)):
    def inputs():
        return dict(x=_rand((B, C, H, W), x_dt, 1000 * H + W), gy=_rand((B, C, H, W), gy_dt, H + W),
                    k=_rand((C, C // groups, 1, 7), F32, 11, -0.5))

    def run(t):
        from HyGrid import ops
        out = ops.pipeline_r2h_conv_h2r_backward(t["gy"], t["x"], t["k"], None, None, 1, groups, off,
                                                 0.0, need_x=need[0], need_k=need[1], need_b=need[2])
        assert out is not None, "the fused backward should cover this call"
        return list(out)

    def ref(inp):
        u = O.rect_to_hex(_np(inp["x"]), (H, W))
        gz = O.hex_to_rect_backward(_np(inp["gy"]), (H, W))
        du, dk, db = O.hexconv2d_backward(u, _np(inp["k"]), gz, off, 2, padding=1, groups=groups)
        return [O.rect_to_hex_backward(du, (H, W)), dk.reshape(C, C // groups, 7), db]

    shapes = [((B, C, H, W), x_dt), ((C, C // groups, 7), F32), ((C,), F32)]
    dx_cmp = grad_close if x_dt == F32 else one_rounding(2.0 ** -8 if x_dt == BF16 else 2.0 ** -10)
    add(name, ["hg_pipeline_r2h_conv_h2r_backward"], sibling, inputs, ["x", "gy"], run,
        [s if n else None for s, n in zip(shapes, need)], ref, [dx_cmp, grad_close, grad_close],
        workspace=need[1] or need[2])


fused_backward("chain_bwd_f32", BWD, 2, 3, TR + 5, TC + 11, 0, 1, F32, F32)
fused_backward("chain_bwd_bf16", "tests/test_gpu_pipeline_backward.py::test_dtypes",
               2, 3, TR + 5, TC + 10, 1, 1, BF16, BF16)
fused_backward("chain_bwd_two_weight_bands", BWD, 1, 3, TR * BAND + 2 * TR + 3, TC + 10, 1, 1, F32, F32)
fused_backward("chain_bwd_no_dx", "tests/test_gpu_pipeline_backward.py::test_requested_gradients_only",
               2, 3, TR + 5, TC + 11, 0, 3, F32, F32, need=(False, True, True))
fused_backward("chain_bwd_dx_only", "tests/test_gpu_pipeline_backward.py::test_requested_gradients_only",
               2, 3, TR + 5, TC + 11, 0, 1, BF16, F32, need=(True, False, False))


# ---- round trip: hg_pipeline_r2h_h2r (k_fused MD 2) --------------------------------------------
def roundtrip(name, sibling, B, C, H, W, dt, cmp):
    def run(t):
        from HyGrid import ops
        y = ops.pipeline_r2h_h2r(t["x"], None, dt)
        assert y is not None
        return [y]

    add(name, ["hg_pipeline_r2h_h2r"], sibling, lambda: dict(x=_rand((B, C, H, W), dt, H + 3 * W)),
        ["x"], run, [((B, C, H, W), dt)],
        lambda inp: [O.hex_to_rect(O.rect_to_hex(_np(inp["x"]), (H, W), 1), (H, W), 1)], [cmp])


R2, OWN2, _ = _layout(2)
roundtrip("roundtrip_f32", "tests/test_gpu_roundtrip.py::test_roundtrip_fp32_vs_oracle",
          2, 3, R2 + 7, OWN2 + 2, F32, close(1e-5))
roundtrip("roundtrip_bf16", "tests/test_gpu_roundtrip.py::test_roundtrip_16bit_vs_fp32_chain",
          2, 3, R2 + 7, OWN2 + 2, BF16, close(2.0 ** -8))


# ---- resamplers: hg_rect_to_hex / hg_hex_to_rect / hg_hexresize -------------------------------
RESAMPLE = {"rect_to_hex": ("hg_rect_to_hex", 0, O.rect_to_hex),
            "hex_to_rect": ("hg_hex_to_rect", 1, O.hex_to_rect),
            "hexresize": ("hg_hexresize", 2, O.hexresize)}
GENERAL, NEAREST, STREAM, DOWN, UP = range(5)      # enum hg_kernel


def resample(name, sibling, op, shape, size, x_dt, y_dt, interp, kernel, cmp, seed=1):
    export, code, ofn = RESAMPLE[op]
    h, w = shape[-2:]
    planes = int(np.prod(shape[:-2]))

    def run(t):
        from HyGrid import ops
        return [getattr(ops, op)(t["x"], size, interp=interp, out_dtype=y_dt)]

    def route():
        from HyGrid import _abi
        return kernel, _abi.resample_kernel(code, _abi.dtype_code(x_dt), _abi.dtype_code(y_dt),
                                            planes, h, w, size[0], size[1], interp)

    add(name, [export], sibling, lambda: dict(x=_rand(shape, x_dt, seed + h * 31 + w)), ["x"], run,
        [(tuple(shape[:-2]) + tuple(size), y_dt)],
        lambda inp: [ofn(_np(inp["x"]), size, interp)], [cmp], route=route)


PAR = "tests/test_gpu_parity.py::test_tensor_ops_vs_oracle"
resample("r2h_general_f32", PAR, "rect_to_hex", (2, 33, 47), (17, 24), F32, F32, 1, GENERAL, close(1e-5))
resample("h2r_general_bf16", PAR, "hex_to_rect", (2, 33, 47), (17, 24), BF16, BF16, 1, GENERAL,
         close(2.0 ** -8))
resample("hexresize_general_f32", PAR, "hexresize", (2, 33, 47), (17, 24), F32, F32, 1, GENERAL,
         close(1e-5))
resample("hexresize_general_f16_odd", PAR, "hexresize", (2, 33, 125), (16, 62), F16, F16, 1, GENERAL,
         close(2.0 ** -11))
resample("r2h_nearest_f16", PAR, "rect_to_hex", (2, 33, 47), (33, 47), F16, F16, 0, NEAREST, exact)
resample("h2r_nearest_u8", PAR, "hex_to_rect", (2, 33, 47), (17, 24), U8, U8, 0, NEAREST, exact)
# the row-streaming kernels: 128-row bands, 256-column windows (tests/test_gpu_stream.py)
resample("r2h_stream_bf16", "tests/test_gpu_stream.py::test_r2h_stream_vs_oracle", "rect_to_hex",
         (2, 129, 516), (129, 516), BF16, BF16, 1, STREAM, close(2.0 ** -8))
resample("r2h_stream_f32", "tests/test_gpu_stream.py::test_r2h_stream_vs_oracle", "rect_to_hex",
         (2, 129, 516), (129, 516), F32, F32, 1, STREAM, close(1e-5))
resample("h2r_stream_f16", "tests/test_gpu_stream.py::test_h2r_stream_vs_oracle", "hex_to_rect",
         (2, 129, 516), (129, 516), F16, F16, 1, STREAM, close(2.0 ** -11))
resample("h2r_stream_bf16_f32", "tests/test_gpu_stream.py::test_h2r_stream_vs_oracle", "hex_to_rect",
         (2, 129, 516), (129, 516), BF16, F32, 1, STREAM, close(1e-5))
# ~2x downsampling rect -> hex (tests/test_gpu_down.py); u8 nearest is ConvertToHexagon's call
resample("r2h_down_bf16", "tests/test_gpu_down.py::test_bilinear_2x", "rect_to_hex",
         (2, 100, 1000), (50, 500), BF16, BF16, 1, DOWN, maxnorm(2.0 ** -8))
resample("r2h_down_f16_f32", "tests/test_gpu_down.py::test_bilinear_2x", "rect_to_hex",
         (2, 65, 130), (32, 65), F16, F32, 1, DOWN, close(1e-5))
resample("r2h_down_nearest_u8", "tests/test_gpu_down.py::test_convert_to_hexagon_nearest_u8",
         "rect_to_hex", (2, 3, 65, 130), (32, 65), U8, U8, 0, DOWN, exact)
resample("r2h_down_nearest_bf16", "tests/test_gpu_down.py::test_nearest_16bit", "rect_to_hex",
         (2, 64, 66), (32, 33), BF16, BF16, 0, DOWN, exact)
# the upsampling triangle kernel; a source that is not 4-B aligned declines to the general
# kernels (tri_up.hip:427), bit-identical: tests/test_gpu_triup.py:160-168
resample("h2r_triup_bf16", "tests/test_gpu_triup.py::test_linear_up_bit_identical_and_vs_oracle",
         "hex_to_rect", (2, 1, 33, 260), (65, 520), BF16, BF16, 1, UP, maxnorm(2.0 ** -8))
resample("hexresize_triup_f32", "tests/test_gpu_triup.py::test_linear_up_bit_identical_and_vs_oracle",
         "hexresize", (2, 1, 33, 260), (65, 520), F32, F32, 1, UP, close(1e-5))
resample("h2r_triup_nearest_u8", "tests/test_gpu_triup.py::test_nearest_up_bit_identical_and_vs_oracle",
         "hex_to_rect", (2, 1, 33, 260), (65, 520), U8, U8, 0, UP, exact)
# the ~2x downsampling hexresize kernel; a source 4-B but not 16-B aligned takes its 4-B-piece
# layout, a 2-B aligned one the general kernel (hexresize_down.hip:358-359), all bit-identical:
# tests/test_gpu_hexdown.py:128-138
resample("hexresize_down_f16", "tests/test_gpu_hexdown.py::test_hexresize_2x_bit_identical_and_vs_oracle",
         "hexresize", (2, 1, 65, 130), (32, 65), F16, F16, 1, DOWN, maxnorm(2.0 ** -11))
resample("hexresize_down_bf16_f32", "tests/test_gpu_hexdown.py::test_hexresize_2x_bit_identical_and_vs_oracle",
         "hexresize", (2, 1, 128, 250), (64, 125), BF16, F32, 1, DOWN, close(1e-5))


# ---- resampler backward through autograd: hg_resample_backward --------------------------------
def resample_backward(name, op, shape, size, dt, interp):
    export, code, ofn = RESAMPLE[op]
    h, w = shape[-2:]
    bwd = getattr(O, op + "_backward")
    tol = 1e-12 if dt == F64 else 1e-5

    def inputs():
        g = _gen(3 + h + w)
        return dict(x=torch.rand(shape, generator=g, dtype=dt),
                    gy=torch.randn(tuple(shape[:-2]) + tuple(size), generator=g, dtype=dt))

    def run(t):
        from HyGrid import ops
        x = t["x"].requires_grad_(True)
        y = getattr(ops, op)(x, size, interp=interp)
        y.backward(t["gy"])
        return [y.detach(), x.grad]

    add(name, ["hg_resample_backward", export],
        "tests/test_gpu_resample_grad.py::test_backward_elementwise_vs_oracle_adjoint", inputs,
        ["x", "gy"], run, [(tuple(shape[:-2]) + tuple(size), dt), (tuple(shape), dt)],
        lambda inp: [ofn(_np(inp["x"]), size, interp), bwd(_np(inp["gy"]), (h, w), interp)],
        [close(tol), close(tol)], atomic=[1])


resample_backward("r2h_backward_f32", "rect_to_hex", (2, 3, 64, 96), (64, 96), F32, 1)
resample_backward("h2r_backward_f64", "hex_to_rect", (2, 3, 16, 20), (8, 10), F64, 1)
resample_backward("hexresize_backward_f32_nearest", "hexresize", (2, 3, 9, 12), (20, 25), F32, 0)
resample_backward("hexresize_backward_f64", "hexresize", (2, 3, 64, 96), (64, 96), F64, 1)


# ---- lattice maps: hg_lattice_maps, hg_hex_homography_maps -----------------------------------
MAP_KEYS = ("i_n", "j_n", "flag", "valid", "argmin", "i_f", "j_f", "alpha", "beta", "gamma")


def lattice_maps(op, h, w, h1, w1):
    ofn = {"rect_to_hex": O.r2h_maps, "hex_to_rect": O.h2r_maps, "hexresize": O.hexresize_maps}[op]
    keys = [k for k in MAP_KEYS if k in ofn(2, 2, 2, 2)]

    def run(t):
        from HyGrid import ops
        m = ops.lattice_maps(op, h, w, h1, w1, "cuda:0")
        return [m[k] for k in keys]

    def ref(inp):
        m = ofn(h, w, h1, w1)
        return [m[k].astype(np.float64) for k in keys]

    add(f"lattice_maps_{op}", ["hg_lattice_maps"],
        "tests/test_gpu_parity.py::test_lattice_maps_full_size_vs_oracle", dict, [], run,
        [((h1, w1), torch.int32 if k in MAP_KEYS[:5] else F64) for k in keys], ref, [exact] * len(keys))


lattice_maps("rect_to_hex", 33, 47, 33, 47)
lattice_maps("hex_to_rect", 33, 47, 65, 93)
lattice_maps("hexresize", 64, 66, 32, 33)


def rand_affine(seed):
    """tests/test_gpu_transform.py::_rand_affine."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi)
    s = rng.uniform(0.4, 2.2, size=2)
    sh = rng.uniform(-0.4, 0.4)
    A = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ \
        np.array([[s[0], sh], [0.0, s[1]]])
    H = np.eye(3)
    H[:2, :2] = A
    H[:2, 2] = rng.uniform(-5, 5, size=2)
    return H


HMAT = rand_affine(7)


def _homography_size(h, w):
    from HyGrid import ops
    xs, ys, _ = ops.homography_plan(h, w, HMAT)
    return len(xs), len(ys)


def homography_maps(h, w):
    keys = ("i_n", "j_n", "flag", "valid", "argmin")
    h1, w1 = _homography_size(h, w)

    def run(t):
        from HyGrid import ops
        m = ops.homography_maps(h, w, HMAT, "cuda:0")
        return [m[k] for k in keys]

    def ref(inp):
        maps = O.image_geometric_transformation(np.zeros((1, h, w)), HMAT, 1)[1]
        return [np.asarray(maps[k], np.float64).reshape(h1, w1) for k in keys]

    add("homography_maps", ["hg_hex_homography_maps"],
        "tests/test_gpu_transform.py::test_igt_random_affine_vs_oracle", dict, [], run,
        [((h1, w1), torch.int32)] * 5, ref, [exact] * 5)


homography_maps(40, 52)


# ---- transform: hg_hex_homography -------------------------------------------------------------
def homography(name, shape, x_dt, y_dt, interp):
    h, w = shape[-2:]
    h1, w1 = _homography_size(h, w)

    def run(t):
        from HyGrid import ops
        return [ops.hex_homography(t["x"], HMAT, interp, y_dt)]

    def ref(inp):
        r = O.image_geometric_transformation(_np(inp["x"]), HMAT, interp)[0]
        r = r.reshape(tuple(shape[:-2]) + (h1, w1))
        return [r.astype(np.float32).astype(np.float64) if y_dt == F32 else r]

    add(name, ["hg_hex_homography"], "tests/test_gpu_transform.py::test_igt_dtypes_and_batch",
        lambda: dict(x=_rand(shape, x_dt, 9) if x_dt == U8 else (_rand(shape, F32, 9) * 200).to(x_dt)),
        ["x"], run, [(tuple(shape[:-2]) + (h1, w1), y_dt)], ref, [exact])


homography("homography_linear_f32", (2, 3, 40, 52), F32, F32, 1)
homography("homography_linear_bf16_f64", (2, 3, 40, 52), BF16, F64, 1)
homography("homography_nearest_u8", (2, 3, 40, 52), U8, U8, 0)
homography("homography_nearest_f16", (2, 3, 40, 52), F16, F16, 0)


# ---- formats: hg_hex_to_type1, hg_strided_copy2d ----------------------------------------------
def type1(name, shape, dt, off, rr):
    h, w = shape[-2:]

    def run(t):
        from HyGrid import ops
        return [ops.hex_to_type1(t["x"], off, rr)]

    add(name, ["hg_hex_to_type1"], "tests/test_gpu_formats.py::test_type1_type2_vs_oracle_and_loops",
        lambda: dict(x=_rand(shape, dt, 2) if dt == U8 else (_rand(shape, F32, 2) * 200).to(dt)),
        ["x"], run, [(tuple(shape[:-2]) + (h * rr, 2 * w + 1), dt)],
        lambda inp: [np.repeat(O.heximage_to_type1(_np(inp["x"]), off), rr, axis=-2)], [exact])


type1("type1_bf16", (2, 3, 16, 20), BF16, 1, 1)
type1("type1_u8", (2, 3, 7, 9), U8, 0, 1)
type1("type1_f64", (2, 3, 7, 9), F64, 1, 1)
type1("type2_f32", (2, 3, 16, 20), F32, 0, 2)
type1("type2_u8", (2, 3, 7, 9), U8, 1, 2)


def strided_copy(name, shape, dt, args):
    r0, rs, c0, cs = args
    H, W = shape[-2:]
    ho, wo = len(range(r0, H, rs)), len(range(c0, W, cs))

    def run(t):
        from HyGrid import ops
        return [ops.strided_copy2d(t["x"], *args)]

    add(name, ["hg_strided_copy2d"], "tests/test_gpu_formats.py::test_strided_copy_equals_slices",
        lambda: dict(x=_rand(shape, dt, 4)), ["x"], run, [(tuple(shape[:-2]) + (ho, wo), dt)],
        lambda inp: [_np(inp["x"])[..., r0::rs, c0::cs]], [exact])


strided_copy("strided_copy_f32", (2, 3, 10, 21), F32, (1, 3, 0, 5))
strided_copy("strided_copy_type1_decode_bf16", (2, 3, 10, 21), BF16, (0, 1, 1, 2))
strided_copy("strided_copy_u8", (2, 3, 10, 21), U8, (0, 2, 1, 2))


# ---- hexconv2d: hg_hexconv2d, hg_hexconv2d_epilogue -------------------------------------------
def conv(name, sibling, B, C, Oc, h, w, x_dt, y_dt, cmp, r=2, stride=1, pad=1, groups=1, off=0,
         mode="constant", pv=0.0, epilogue=False, env=None):
    K = 3 * r * r - 3 * r + 1
    ho, wo = O.hexconv2d_out_shape(h, w, r, stride, pad, 1)

    def inputs():
        bound = 1.0 / np.sqrt(K * C // groups)
        d = dict(x=_rand((B, C, h, w), x_dt, h * 13 + w, -0.5),
                 k=(_rand((Oc, C // groups, 1, K), F32, 21, -0.5) * 2 * bound),
                 b=_rand((Oc,), F32, 22, -0.5))
        if epilogue:
            d["scale"] = _rand((Oc,), F32, 23, 0.5)
            d["shift"] = _rand((Oc,), F32, 24, -0.5)
        return d

    def run(t):
        from HyGrid import ops
        epi = (t["scale"], t["shift"], 2, 0.1) if epilogue else None      # hg_act 2: LeakyReLU
        return [ops.hexconv2d(t["x"], t["k"], t["b"], off, r, stride, pad, 1, groups, mode, pv,
                              out_dtype=y_dt, epilogue=epi)]

    def ref(inp):
        y = O.hexconv2d(_np(inp["x"]), _np(inp["k"]), _np(inp["b"]), off, r, stride, pad, 1, groups,
                        mode, pv)
        if epilogue:
            y = y * _np(inp["scale"])[None, :, None, None] + _np(inp["shift"])[None, :, None, None]
            y = np.where(y >= 0, y, 0.1 * y)
        return [y]

    add(name, ["hg_hexconv2d_epilogue" if epilogue else "hg_hexconv2d"], sibling, inputs, ["x"], run,
        [((B, Oc, ho, wo), y_dt)], ref, [cmp], env=env)


R1, OWN1, _ = _layout(1)
FC = "tests/test_gpu_fused_conv.py::test_fused_conv_fp32_vs_oracle"
MF = "tests/test_gpu_conv_mfma.py::"
# the generic LDS kernel
conv("conv_generic_r3_s2_reflect", "tests/test_gpu_parity.py::test_hexconv_param_space_vs_oracle",
     2, 2, 5, 61, 133, F32, F32, close(1e-5), r=3, stride=2, pad=2, off=1, mode="reflect")
conv("conv_generic_bf16_groups", "tests/test_gpu_parity.py::test_hexconv_large_vs_oracle",
     2, 6, 4, 31, 45, BF16, BF16, close(2.0 ** -8), groups=2, mode="circular")
# conv_stream.hip (a pad value other than 0 leaves the fused kernel): 126-row bands
conv("conv_stream_f32", "tests/test_gpu_parity.py::test_hexconv_stream_path_vs_oracle",
     2, 3, 3, 127, 130, F32, F32, close(1e-5), pv=0.375)
conv("conv_stream_bf16_oddwidth", "tests/test_gpu_parity.py::test_hexconv_large_vs_oracle",
     2, 3, 3, 127, 131, BF16, BF16, close(2.0 ** -8), off=1)
# k_fused MD 1: the HexConv2d 3 -> 3 drop-in on the two-column streaming kernel
conv("conv_fused_md1_f32", FC, 2, 3, 3, R1 + 7, OWN1 + 2, F32, F32, close(1e-5), off=1)
conv("conv_fused_md1_bf16", "tests/test_gpu_fused_conv.py::test_fused_conv_16bit_vs_stream_kernel",
     2, 3, 3, R1 + 7, OWN1 + 2, BF16, BF16, close(2.0 ** -8))
conv("conv_fused_md1_f16_c1", "tests/test_gpu_fused_conv.py::test_fused_conv_16bit_vs_stream_kernel",
     2, 1, 1, R1 + 7, OWN1 + 2, F16, F32, close(1e-5))
# conv_mfma.hip: f32, bf16 register-staged, bf16 LDS-DMA.  A source that is not 4-B aligned
# keeps the register staging (conv_fwd_route's alignment condition), bit-identical to the DMA
# kernel: tests/test_gpu_conv_mfma.py, test_mfma_bf16_dma_bit_identical_to_register_staging and
# test_mfma_bf16_dma_vs_oracle_and_unaligned
conv("conv_mfma_f32", MF + "test_mfma_conv_fp32_vs_oracle", 2, 16, 16, 33, 70, F32, F32, close(1e-5))
conv("conv_mfma_bf16_regs", MF + "test_mfma_bf16_conv_vs_oracle", 2, 13, 20, 30, 260, BF16, F32,
     close(1e-5), env={"HYGRID_CONV_DMA": "0"})
conv("conv_mfma_bf16_dma", MF + "test_mfma_bf16_conv_vs_oracle", 2, 13, 20, 30, 260, BF16, F32,
     close(1e-5))
conv("conv_mfma_bf16_dma_bf16_out", MF + "test_mfma_conv_16bit_vs_generic", 2, 13, 20, 30, 260,
     BF16, BF16, close(2.0 ** -8), off=1)
# 16-bit outputs with wo % 4 != 0: the scalar-store tail of the column-store epilogue, with the
# fused BN-affine + LeakyReLU epilogue (bf16 in: the DMA kernel, f16 in: the f32-MFMA kernel)
conv("conv_mfma_colstore_tail_bf16", MF + "test_mfma_column_store_epilogue_vs_generic",
     2, 3, 32, 17, 38, BF16, BF16, close(2.0 ** -8), epilogue=True)
conv("conv_mfma_colstore_tail_f16", MF + "test_mfma_column_store_epilogue_vs_generic",
     2, 16, 48, 9, 38, F16, F16, close(2.0 ** -11), epilogue=True)
conv("conv_generic_epilogue_f32", MF + "test_mfma_hexconvmodule_epilogue_vs_generic",
     2, 3, 6, 31, 45, F32, F32, close(1e-5), epilogue=True, off=1)


# ---- hexconv2d backward: hg_hexconv2d_backward ------------------------------------------------
def conv_backward(name, B, C, Oc, h, w, x_dt, mode="constant"):
    ho, wo = O.hexconv2d_out_shape(h, w, 2, 1, 1, 1)
    cfg = dict(off=0, r=2, stride=1, pad=1, dilation=1, groups=1, padding_mode=mode,
               padding_value=0.0, out_dtype=None)

    def inputs():
        g = _gen(11 + h)
        return dict(x=torch.rand((B, C, h, w), generator=g).to(x_dt),
                    gy=torch.randn((B, Oc, ho, wo), generator=g),
                    k=torch.rand((Oc, C, 1, 7), generator=g) - 0.5, b=torch.rand((Oc,), generator=g))

    def run(t):
        from HyGrid import ops
        return list(ops.hexconv2d_backward(t["gy"], t["x"], t["k"], t["b"], cfg))

    # the oracle on the (bf16-) rounded x; dk / db at the file's 1e-4 (test_gpu_backward.py::close)
    def ref(inp):
        return list(O.hexconv2d_backward(_np(inp["x"]), _np(inp["k"]), _np(inp["gy"]), 0, 2, 1, 1, 1,
                                         1, mode, 0.0))

    dx_cmp = close(1e-4, 1e-5) if x_dt == F32 else close(2.0 ** -8)
    add(name, ["hg_hexconv2d_backward"],
        "tests/test_gpu_backward.py::test_backward_bf16_input_and_fp64_kernel", inputs, ["x", "gy"],
        run, [((B, C, h, w), x_dt), ((Oc, C, 1, 7), F32), ((Oc,), F32)], ref,
        [dx_cmp, close(1e-4, 1e-5), close(1e-4, 1e-5)], atomic=[1, 2])


conv_backward("conv_backward_f32", 2, 3, 3, 33, 47, F32)
conv_backward("conv_backward_bf16_x", 2, 3, 3, 64, 96, BF16)
conv_backward("conv_backward_f32_reflect", 2, 3, 6, 31, 45, F32, mode="reflect")


# ---- pooling: hg_hex_pool2d, hg_hex_pool2d_backward -------------------------------------------
def pool(name, shape, dt, meta, ytol, gtol):
    h, w = shape[-2:]
    args = pool_args(dict(h=h, w=w, **meta))
    hn, wn = args[5], args[6]
    lead = tuple(shape[:-2])

    def inputs():
        g = _gen(17 + h)
        return dict(x=torch.randn(shape, generator=g).to(dt),
                    gy=torch.randn(lead + (hn, wn), generator=g).to(dt))

    def run(t):
        from HyGrid import ops
        x = t["x"].requires_grad_(True)
        y = ops.hex_pool2d(x, *args)
        y.backward(t["gy"])
        return [y.detach(), x.grad]

    add(name, ["hg_hex_pool2d", "hg_hex_pool2d_backward"],
        "tests/test_gpu_pool.py::test_pool_random_vs_oracle", inputs, ["x", "gy"], run,
        [(lead + (hn, wn), dt), (tuple(shape), dt)],
        lambda inp: [O.hex_pool2d(_np(inp["x"]), *args),
                     O.hex_pool2d_backward(_np(inp["x"]), _np(inp["gy"]), *args)],
        [exact if ytol is None else absclose(ytol), absclose(gtol)], atomic=[1])


# small windows (one thread per output); the reflect frame folds its atomics onto x
pool("pool_small_min_reflect_f32", (2, 2, 67, 96), F32,
     dict(kind="pool", method="min", k=[3, 2], s=[2, 2], pad=1, mode="reflect"), None, 1e-5)
pool("pool_small_average_bf16", (2, 2, 67, 96), BF16,
     dict(kind="pool", method="average", k=3, s=2, pad=1), 1.6e-2, 3e-2)
pool("pool_small_max_ceil_circular_f64", (2, 2, 67, 96), F64,
     dict(kind="pool", method="max", k=3, s=3, pad=1, mode="circular", ceil=True), None, 1e-13)
# windows of 512 elements and more: one workgroup per output (pool.hip PL_LARGE)
pool("pool_large_global_average_f32", (2, 3, 24, 32), F32, dict(kind="global", method="average"),
     2e-6, 1e-5)
pool("pool_large_adaptive_max_f16", (2, 3, 70, 99), F16, dict(kind="adaptive", method="max", outsize=2),
     None, 4e-3)
# the large kernels behind HexPool2d: 23 x 23 windows whose reflect frame folds onto x
pool("pool_large_min_reflect_ceil_f32", (2, 2, 50, 61), F32,
     dict(kind="pool", method="min", k=23, s=23, pad=3, mode="reflect", ceil=True), None, 1e-5)


# ---- pyramid: hg_hex_pyramid_level, hg_hex_pyramid_chain --------------------------------------
PYR_FUSED, PYR_FUSED_SHORT, PYR_STREAM, PYR_LDS = range(4)      # enum hg_pyr_kernel


def _level_ref(x, taps, bias, off, from_rect, size):
    h, w = x.shape[-2:]
    hx = O.rect_to_hex(x, (h, w), 1).reshape(x.shape) if from_rect else x
    c = O.hexconv2d(hx, taps, bias, off, 2, padding=1, groups=x.shape[1])
    return O.hexresize(c, size, 1).reshape(x.shape[:2] + tuple(size))


def pyramid_level(name, B, C, h, w, dt, y_dt, off, from_rect, kernels, which=None, env=None):
    size = (h // 2, w // 2)
    env = dict(env or {}, **({"HYGRID_PYR_KERNEL": which} if which else {}))

    def inputs():
        g = _gen(h * 3 + w + off)
        return dict(taps=torch.rand((C, 1, 1, 7), generator=g) - 0.3,
                    bias=torch.rand((C,), generator=g) - 0.5,
                    x=torch.rand((B, C, h, w), generator=g).to(dt))

    def run(t):
        from HyGrid import ops
        y = ops.hex_pyramid_level(t["x"], t["taps"], t["bias"], size, off, from_rect=from_rect,
                                  out_dtype=y_dt)
        return None if y is None else [y]

    def route():
        from HyGrid import _abi
        return kernels, _abi.pyramid_level_kernel(_abi.dtype_code(dt), _abi.dtype_code(y_dt), B, C,
                                                  h, w, size[0], size[1], off, from_rect)

    # every level kernel loads dwords: a 16-bit source that is not 4-B aligned is HG_EUNSUP on
    # all three (pyramid_fused.hip:105, pyramid_stream.hip:452, pyramid.hip:576)
    add(name, ["hg_hex_pyramid_level"],
        "tests/test_gpu_pyramid.py::test_pyramid_level_kernels_vs_oracle", inputs, ["x"], run,
        [((B, C) + size, y_dt)],
        lambda inp: [_level_ref(_np(inp["x"]), _np(inp["taps"]), _np(inp["bias"]), off, from_rect, size)],
        [out_cmp(y_dt)], env=env,
        declines=lambda src_bytes, dst_bytes: dt in ULP and src_bytes % 4 != 0, route=route)


pyramid_level("pyramid_fused_from_rect_f16", 2, 3, 64, 130, F16, F16, 0, True, (PYR_FUSED,))
pyramid_level("pyramid_fused_short_bf16", 2, 3, 64, 130, BF16, BF16, 1, False, (PYR_FUSED_SHORT,))
pyramid_level("pyramid_fused_bf16_f32", 2, 1, 64, 130, BF16, F32, 0, False, (PYR_FUSED_SHORT,))
pyramid_level("pyramid_fused_long_bands_f16", 2, 3, 64, 130, F16, F16, 0, False, (PYR_FUSED,),
              env={"HYGRID_PYR_SHORT": "0"})
pyramid_level("pyramid_stream_f16", 2, 3, 64, 130, F16, F16, 1, True, (PYR_STREAM,), "stream")
pyramid_level("pyramid_lds_bf16", 2, 3, 64, 130, BF16, BF16, 0, False, (PYR_LDS,), "lds")
pyramid_level("pyramid_lds_f32", 2, 3, 37, 53, F32, F32, 1, True, (PYR_LDS,))


def pyramid_chain(name, B, h, w, dt, levels, off):
    sizes = [(h >> (l + 1), w >> (l + 1)) for l in range(levels)]

    def inputs():
        g = _gen(8 + h)
        taps = torch.tensor([1, 1, 1, 6, 1, 1, 1], dtype=F32).div(12).expand(3, 7).contiguous()
        return dict(taps=taps, x=torch.rand((B, 3, h, w), generator=g).to(dt))

    def run(t):
        from HyGrid import _abi, ops
        outs = ops.hex_pyramid_chain(t["x"], t["taps"], None, levels, off)
        if outs is None:
            return None
        torch.cuda.synchronize()
        ws = ops.chain_workspace(t["x"].device, _abi.stream_of(t["x"]), 0)
        assert int(ws[1]) == 0, "chain fault word set (a workgroup waited > ~1 s for its input)"
        return list(outs)

    # one rounding per stored level, fp64 inside a level (tests/test_gpu_pyramid.py::oracle_levels)
    def ref(inp):
        cur, taps, outs = _np(inp["x"]), _np(inp["taps"]).reshape(3, 1, 1, 7), []
        for l, size in enumerate(sizes):
            cur = _level_ref(cur, taps, None, off, l == 0, size)
            cur = _np(torch.from_numpy(cur).to(dt))
            outs.append(cur)
        return outs

    # level l + 1 loads dwords from level l's output: the chain declines (pf_prepare,
    # pyramid_fused.hip:105 / :288) unless the source and the outputs are 4-B aligned
    add(name, ["hg_hex_pyramid_chain"],
        "tests/test_gpu_pyramid.py::test_hex_pyramid_8k_fused_full_size", inputs, ["x"], run,
        [((B, 3) + s, dt) for s in sizes], ref, [maxnorm(3 * 2.0 ** -11 if dt == F16 else 3 * 2.0 ** -8)] * levels,
        declines=lambda src_bytes, dst_bytes: src_bytes % 4 != 0 or dst_bytes % 4 != 0, workspace=True)


pyramid_chain("pyramid_chain_f16", 2, 136, 248, F16, 3, 0)
pyramid_chain("pyramid_chain_bf16_two_levels", 2, 136, 252, BF16, 2, 1)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
