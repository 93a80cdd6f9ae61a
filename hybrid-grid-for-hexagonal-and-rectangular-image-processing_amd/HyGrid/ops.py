"""Tensor-level entry points: torch device tensors in, torch device tensors out.

Thin layer over the C ABI (`_abi`): shape/dtype policy, output allocation (the
caller — here torch's caching allocator — owns every buffer), and the current
HIP stream.  The reference-compatible surfaces (geometry_np, geometry_torch,
HexFrames, ...) are built on these.

Layout: a raster batch is any tensor (..., H, W); all leading dims are flattened
into `planes`, which the kernels walk with the lattice maps computed once.
"""
import ctypes

import torch

from . import _abi

_FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _planes(x):
    if x.dim() < 2:
        raise ValueError(f"expected a raster (..., H, W), got shape {tuple(x.shape)}")
    x = x.contiguous()
    lead = tuple(x.shape[:-2])
    planes = 1
    for d in lead:
        planes *= d
    return x, lead, planes


_RESAMPLE_OP = {"hg_rect_to_hex": _abi.HG_OP_RECT_TO_HEX, "hg_hex_to_rect": _abi.HG_OP_HEX_TO_RECT,
                "hg_hexresize": _abi.HG_OP_HEXRESIZE}


class _ResampleFn(torch.autograd.Function):
    """Autograd of a resample: backward = hg_resample_backward (the transpose of the
    forward's lattice weights)."""

    @staticmethod
    def forward(ctx, x, fn_name, size, interp, out_dtype):
        ctx.meta = (_RESAMPLE_OP[fn_name], tuple(x.shape), x.dtype, int(interp))
        return _resample_raw(fn_name, x, size, interp, out_dtype)

    @staticmethod
    def backward(ctx, gy):
        op, shape, xdt, interp = ctx.meta
        acc = torch.float64 if torch.float64 in (gy.dtype, xdt) else torch.float32
        g = gy.contiguous().to(acc)
        h, w = shape[-2], shape[-1]
        h1, w1 = int(g.shape[-2]), int(g.shape[-1])
        planes = 1
        for d in shape[:-2]:
            planes *= d
        dx = torch.empty(shape, dtype=acc, device=gy.device)
        st = _abi.lib().hg_resample_backward(op, _abi.ptr(g), _abi.ptr(dx), _abi.dtype_code(acc),
                                             planes, h, w, h1, w1, interp, _abi.stream_of(g))
        _abi.check(st, "hg_resample_backward")
        return dx.to(xdt), None, None, None, None


def _resample(fn_name, x, size, interp, out_dtype):
    if torch.is_grad_enabled() and x.requires_grad and x.is_floating_point():
        return _ResampleFn.apply(x, fn_name, size, interp, out_dtype)
    return _resample_raw(fn_name, x, size, interp, out_dtype)


def _resample_raw(fn_name, x, size, interp, out_dtype):
    _abi.require_device(x)
    x = x.detach()
    x, lead, planes = _planes(x)
    h, w = int(x.shape[-2]), int(x.shape[-1])
    h1, w1 = (h, w) if size is None else (int(size[0]), int(size[1]))
    if interp == _abi.HG_NEAREST:
        out_dtype = x.dtype
    elif out_dtype is None:
        out_dtype = x.dtype if x.dtype in _FLOATS else torch.float32
    y = torch.empty(lead + (h1, w1), dtype=out_dtype, device=x.device)
    st = getattr(_abi.lib(), fn_name)(
        _abi.ptr(x), _abi.ptr(y), _abi.dtype_code(x.dtype), _abi.dtype_code(out_dtype),
        planes, h, w, h1, w1, int(interp), _abi.stream_of(x))
    _abi.check(st, fn_name)
    return y


def rect_to_hex(x, size=None, interp=_abi.HG_LINEAR, out_dtype=None):
    """rect (..., H, W) -> hex (..., H1, W1); geometry_np.py:358-519."""
    return _resample("hg_rect_to_hex", x, size, interp, out_dtype)


def hex_to_rect(x, size=None, interp=_abi.HG_LINEAR, out_dtype=None):
    """hex (..., H, W) -> rect (..., H1, W1); geometry_np.py:191-356."""
    return _resample("hg_hex_to_rect", x, size, interp, out_dtype)


def hexresize(x, size, interp=_abi.HG_LINEAR, out_dtype=None):
    """hex (..., H, W) -> hex (..., H1, W1); geometry_np.py:520-681."""
    return _resample("hg_hexresize", x, size, interp, out_dtype)


_OPS = {"rect_to_hex": _abi.HG_OP_RECT_TO_HEX, "hex_to_rect": _abi.HG_OP_HEX_TO_RECT,
        "hexresize": _abi.HG_OP_HEXRESIZE}


def lattice_maps(op, h, w, h1, w1, device=None):
    """The integer lattice maps + fp64 coefficients a resample uses (parity tests)."""
    device = torch.device("cuda") if device is None else torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("HyGrid needs a HIP device (MI355X); none is available.")
    im = torch.empty((5, h1, w1), dtype=torch.int32, device=device)
    fm = torch.empty((5, h1, w1), dtype=torch.float64, device=device)
    st = _abi.lib().hg_lattice_maps(_OPS[op], h, w, h1, w1, _abi.ptr(im), _abi.ptr(fm),
                                    _abi.stream_of(im))
    _abi.check(st, "hg_lattice_maps")
    keys = ("i_n", "j_n", "flag", "valid", "argmin")
    out = {k: im[i] for i, k in enumerate(keys)}
    out.update({k: fm[i] for i, k in enumerate(("i_f", "j_f", "alpha", "beta", "gamma"))})
    return out


def homography_plan(h, w, H):
    """Host planning of image_geometric_transformation (geometry_np.py:56-102): the
    output axes of the transformed corners and inv(H), in NumPy exactly as the
    reference computes them (O(h1 + w1) work).  Returns (xs, ys, hinv) as float64
    ndarrays; h1 = len(xs), w1 = len(ys)."""
    import numpy as np
    H = np.asarray(H.detach().cpu() if isinstance(H, torch.Tensor) else H, dtype=np.float64)
    if H.shape != (3, 3):
        raise ValueError(f"H must be 3x3, got shape {H.shape}")
    corner = np.array([[-(h / 2 - 0.5), -((w + 0.5) / 2 - 0.5), 1.],
                       [-(h / 2 - 0.5), (w + 0.5) / 2 - 0.5, 1.],
                       [h / 2 - 0.5, -((w + 0.5) / 2 - 0.5), 1.],
                       [h / 2 - 0.5, (w + 0.5) / 2 - 0.5, 1.]]).transpose()
    c = np.matmul(H, corner)
    h1_inf, w1_inf = np.min(c[0], axis=-1), np.min(c[1], axis=-1)
    h1_sup, w1_sup = np.max(c[0], axis=-1), np.max(c[1], axis=-1)
    xs = np.arange(h1_inf, h1_sup + 1, 1).astype(np.float64)
    ys = np.arange(w1_inf, w1_sup + 0.5, 1).astype(np.float64)
    hinv = np.ascontiguousarray(np.linalg.inv(H), dtype=np.float64)
    return xs, ys, hinv


def _homography_args(x, H):
    import numpy as np
    h, w = int(x.shape[-2]), int(x.shape[-1])
    xs, ys, hinv = homography_plan(h, w, H)
    dxs = torch.from_numpy(xs).to(x.device)
    dys = torch.from_numpy(ys).to(x.device)
    return h, w, dxs, dys, hinv.ctypes.data_as(ctypes.c_void_p), hinv


def hex_homography(x, H, interp=_abi.HG_LINEAR, out_dtype=None):
    """hex (..., H, W) -> hex (..., h1, w1) under the affine map H
    (image_geometric_transformation, geometry_np.py:6-189), by hg_hex_homography.
    'linear' blends in fp64 and returns out_dtype (default: x's float dtype, float32 for
    integer input); 'nearest' copies the first-minimum vertex (geometry_torch.py:165-173)."""
    _abi.require_device(x)
    x = x.detach()
    x, lead, planes = _planes(x)
    h, w, dxs, dys, hptr, _keep = _homography_args(x, H)
    h1, w1 = int(dxs.numel()), int(dys.numel())
    if interp == _abi.HG_NEAREST:
        out_dtype = x.dtype
    elif out_dtype is None:
        out_dtype = x.dtype if x.dtype in _FLOATS else torch.float32
    y = torch.empty(lead + (h1, w1), dtype=out_dtype, device=x.device)
    st = _abi.lib().hg_hex_homography(
        _abi.ptr(x), _abi.ptr(y), _abi.dtype_code(x.dtype), _abi.dtype_code(out_dtype),
        planes, h, w, h1, w1, _abi.ptr(dxs), _abi.ptr(dys), hptr, int(interp),
        _abi.stream_of(x))
    _abi.check(st, "hg_hex_homography")
    return y


def homography_maps(h, w, H, device=None):
    """Lattice maps of one image_geometric_transformation (parity tests): the keys of
    lattice_maps plus the inverse-mapped point x_, y_ (geometry_np.py:104-105)."""
    device = torch.device("cuda") if device is None else torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("HyGrid needs a HIP device (MI355X); none is available.")
    probe = torch.empty((h, w), device=device)
    h, w, dxs, dys, hptr, _keep = _homography_args(probe, H)
    h1, w1 = int(dxs.numel()), int(dys.numel())
    im = torch.empty((5, h1, w1), dtype=torch.int32, device=device)
    fm = torch.empty((7, h1, w1), dtype=torch.float64, device=device)
    st = _abi.lib().hg_hex_homography_maps(h, w, h1, w1, _abi.ptr(dxs), _abi.ptr(dys), hptr,
                                           _abi.ptr(im), _abi.ptr(fm), _abi.stream_of(im))
    _abi.check(st, "hg_hex_homography_maps")
    keys = ("i_n", "j_n", "flag", "valid", "argmin")
    out = {k: im[i] for i, k in enumerate(keys)}
    out.update({k: fm[i] for i, k in enumerate(("i_f", "j_f", "alpha", "beta", "gamma",
                                                 "x_", "y_"))})
    return out


POOL_METHODS = {"max": 0, "min": 1, "average": 2}
_POOL_PAD_MODES = _abi.PAD_MODES


def pool_plan(h, w, kh, kw, sh, sw, padding=0, ceil_mode=False, count_include_pad=True):
    """HexPool2d's window geometry (HexFrames.py:286-319): the padded frame, the ceil-mode
    extension (F.pad(input, (0, ph, 0, pw)) — ph columns on the right, pw rows at the
    bottom, as the reference passes them, :295-300) and the output size.  Returns
    dict(hn, wn, ext_h, ext_w, ext_value).  Raises IndexError where the reference's
    gather would index outside the frame."""
    H0, W0 = h + 2 * padding, w + 2 * padding
    ext_h = ext_w = 0
    ext_value = 0.0
    if ceil_mode:
        hn0 = H0 // sh
        wn0 = (W0 - sw // 2 - sw) // sw + 1
        ph = (kh - H0 + hn0 * sh) % kh
        pw = (kw - W0 + (wn0 * sw + sw // 2)) % kw
        ext_w, ext_h = ph, pw
        ext_value = 0.0 if count_include_pad else float("nan")
    H, W = H0 + ext_h, W0 + ext_w
    hn = (H - kh) // sh + 1
    wn = (W - sw // 2) // sw
    if hn < 0 or wn < 0:
        raise RuntimeError(f"hex pooling: window {kh}x{kw} / stride {sh}x{sw} does not fit "
                           f"a {H}x{W} frame")
    if hn > 0 and wn > 0:
        shift = sw // 2 if hn >= 2 else 0
        if (hn - 1) * sh + kh > H or (wn - 1) * sw + shift + kw > W:
            raise IndexError(f"hex pooling: windows ({kh}x{kw}, stride {sh}x{sw}) reach "
                             f"outside the {H}x{W} frame (the reference's gather raises)")
    return dict(hn=hn, wn=wn, ext_h=ext_h, ext_w=ext_w, ext_value=ext_value)


def _pool_args(x, method, kh, kw, sh, sw, hn, wn, pad, pad_mode, pad_value, ext_h, ext_w,
               ext_value):
    h, w = int(x.shape[-2]), int(x.shape[-1])
    return (POOL_METHODS[method], h, w, int(pad), _POOL_PAD_MODES[pad_mode], float(pad_value),
            int(ext_h), int(ext_w), float(ext_value), int(kh), int(kw), int(sh), int(sw),
            int(hn), int(wn))


def _pool_raw(x, args):
    _abi.require_device(x)
    if x.dtype not in _FLOATS:
        raise TypeError(f"hex pooling needs a floating-point raster, got {x.dtype} (the "
                        f"reference's NaN masking, HexFrames.py:461-479)")
    x, lead, planes = _planes(x.detach())
    m, h, w, pad, mode, pv, eh, ew, ev, kh, kw, sh, sw, hn, wn = args
    y = torch.empty(lead + (hn, wn), dtype=x.dtype, device=x.device)
    st = _abi.lib().hg_hex_pool2d(_abi.ptr(x), _abi.ptr(y), _abi.dtype_code(x.dtype), m, planes,
                                  h, w, pad, mode, pv, eh, ew, ev, kh, kw, sh, sw, hn, wn,
                                  _abi.stream_of(x))
    _abi.check(st, "hg_hex_pool2d")
    return y


class _HexPoolFn(torch.autograd.Function):
    """Autograd of hex pooling: hg_hex_pool2d_backward (gy to the selected element of a
    max / min window, gy / count to the non-NaN elements of an average window, folded
    back through the padding) — the reference's autograd of HexFrames.py:286-343."""

    @staticmethod
    def forward(ctx, x, args):
        ctx.save_for_backward(x)
        ctx.args = args
        return _pool_raw(x, args)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        m, h, w, pad, mode, pv, eh, ew, ev, kh, kw, sh, sw, hn, wn = ctx.args
        acc = torch.float64 if x.dtype == torch.float64 else torch.float32
        xc, lead, planes = _planes(x.detach())
        g = gy.contiguous().to(acc)
        dx = torch.empty(tuple(x.shape), dtype=acc, device=x.device)
        st = _abi.lib().hg_hex_pool2d_backward(
            _abi.ptr(xc), _abi.ptr(g), _abi.ptr(dx), _abi.dtype_code(x.dtype),
            _abi.dtype_code(acc), m, planes, h, w, pad, mode, pv, eh, ew, ev, kh, kw, sh, sw,
            hn, wn, _abi.stream_of(xc))
        _abi.check(st, "hg_hex_pool2d_backward")
        return dx.to(x.dtype), None


def hex_pool2d(x, method, kh, kw, sh, sw, hn, wn, pad=0, pad_mode="constant", pad_value=0.0,
               ext_h=0, ext_w=0, ext_value=0.0):
    """Hex pooling of (..., h, w) -> (..., hn, wn) by hg_hex_pool2d (geometry: pool_plan).
    Differentiable in x."""
    if pad_mode not in _POOL_PAD_MODES:
        raise NotImplementedError(f"padding mode {pad_mode!r}")
    if _POOL_PAD_MODES[pad_mode] != 0 and pad_value not in (0, None):
        raise RuntimeError(f'Padding mode "{pad_mode}" doesn\'t take in value argument')
    args = _pool_args(x, method, kh, kw, sh, sw, hn, wn, pad, pad_mode,
                      0.0 if pad_value is None else pad_value, ext_h, ext_w, ext_value)
    if torch.is_grad_enabled() and x.requires_grad:
        return _HexPoolFn.apply(x, args)
    return _pool_raw(x, args)


def reduce_last(x, method):
    """The reference's max_pooling / min_pooling / average_pooling (HexFrames.py:461-479):
    NaN-aware reduction over the last dim, as a 1 x n window of hg_hex_pool2d."""
    n = int(x.shape[-1])
    y = hex_pool2d(x.unsqueeze(-2), method, 1, n, 1, max(n, 1), 1, 1)
    return y[..., 0, 0]


def hexconv2d_out_shape(h, w, radius, stride=1, padding=0, dilation=1):
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    st = _abi.lib().hg_hexconv2d_out_shape(h, w, radius, stride, padding, dilation,
                                          ctypes.byref(ho), ctypes.byref(wo))
    _abi.check(st, "hexconv2d_out_shape")
    return ho.value, wo.value


def hexconv2d(x, kernel, bias, even_odd_offset, radius, stride=1, padding=0, dilation=1,
              groups=1, padding_mode="constant", padding_value=0.0, out_dtype=None,
              epilogue=None):
    """HexConv2d forward (HexFrames.py:96-169) on (B, C, H, W) -> (B, O, Ho, Wo).

    kernel: (O, C/groups, 1, K) or (O, C/groups, K) float32/float64 — the
    accumulation dtype, as the reference's `input.to(self.kernel.dtype)` (:107).
    epilogue: None or (scale, shift, act, slope) — per-channel affine (tensors (O,) or
    None) and hg_act activation fused into the store (hg_hexconv2d_epilogue).
    """
    _abi.require_device(x)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    k = kernel.detach()
    if k.dtype not in (torch.float32, torch.float64):
        k = k.float()
    k = k.reshape(k.shape[0], k.shape[1], -1).contiguous()
    O = int(k.shape[0])
    if int(k.shape[1]) * groups != C:
        raise ValueError(f"kernel expects {int(k.shape[1]) * groups} input channels, got {C}")
    b = None
    if bias is not None:
        b = bias.detach().to(k.dtype).contiguous()
    if out_dtype is None:
        out_dtype = torch.get_default_dtype()
    ho, wo = hexconv2d_out_shape(h, w, radius, stride, padding, dilation)
    y = torch.empty((B, O, ho, wo), dtype=out_dtype, device=x.device)
    pm = _abi.PAD_MODES.get(padding_mode)
    if pm is None:
        raise ValueError(f"unsupported padding_mode {padding_mode!r}")
    if epilogue is None:
        st = _abi.lib().hg_hexconv2d(
            _abi.ptr(x), _abi.ptr(k), _abi.ptr(b), _abi.ptr(y), _abi.dtype_code(x.dtype),
            _abi.dtype_code(k.dtype), _abi.dtype_code(out_dtype), B, C, O, h, w, radius, stride,
            padding, dilation, groups, int(even_odd_offset), pm, float(padding_value),
            _abi.stream_of(x))
        _abi.check(st, "hg_hexconv2d")
        return y
    scale, shift, act, slope = epilogue
    sc = None if scale is None else scale.detach().to(k.dtype).contiguous()
    sf = None if shift is None else shift.detach().to(k.dtype).contiguous()
    for t in (sc, sf):
        if t is not None and t.numel() != O:
            raise ValueError(f"epilogue scale/shift must have {O} elements")
    st = _abi.lib().hg_hexconv2d_epilogue(
        _abi.ptr(x), _abi.ptr(k), _abi.ptr(b), _abi.ptr(y), _abi.dtype_code(x.dtype),
        _abi.dtype_code(k.dtype), _abi.dtype_code(out_dtype), B, C, O, h, w, radius, stride,
        padding, dilation, groups, int(even_odd_offset), pm, float(padding_value),
        _abi.ptr(sc), _abi.ptr(sf), int(act), float(slope), _abi.stream_of(x))
    _abi.check(st, "hg_hexconv2d_epilogue")
    return y


def hexconv2d_backward(gy, x, kernel, bias, cfg, need_x=True, need_k=True, need_b=True):
    """Gradients of hexconv2d (hg_hexconv2d_backward): (d x, d kernel, d bias).

    gy: (B, O, ho, wo); x: the forward input (B, C, H, W); kernel: the parameter
    (O, C/groups, 1, K) (its dtype, float32 or float64, is the accumulation dtype, as
    the forward's `input.to(self.kernel.dtype)`, HexFrames.py:107).  Returns None for
    the gradients not requested; d x has x's dtype, d kernel / d bias the parameters'.
    """
    _abi.require_device(gy)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    k = kernel.detach()
    if k.dtype not in (torch.float32, torch.float64):
        k = k.float()
    kshape = tuple(kernel.shape)
    k = k.reshape(k.shape[0], k.shape[1], -1).contiguous()
    O, K = int(k.shape[0]), int(k.shape[2])
    g = gy.detach().to(k.dtype).contiguous()
    dx = torch.empty_like(x) if need_x else None
    dk = torch.empty((O, int(k.shape[1]), K), dtype=k.dtype, device=x.device) if need_k else None
    db = (torch.empty((O,), dtype=k.dtype, device=x.device)
          if (need_b and bias is not None) else None)
    pm = _abi.PAD_MODES.get(cfg["padding_mode"])
    if pm is None:
        raise ValueError(f"unsupported padding_mode {cfg['padding_mode']!r}")
    st = _abi.lib().hg_hexconv2d_backward(
        _abi.ptr(x), _abi.ptr(k), _abi.ptr(g), _abi.ptr(dx), _abi.ptr(dk), _abi.ptr(db),
        _abi.dtype_code(x.dtype), _abi.dtype_code(k.dtype), B, C, O, h, w, cfg["r"],
        cfg["stride"], cfg["pad"], cfg["dilation"], cfg["groups"], int(cfg["off"]), pm,
        float(cfg["padding_value"]), _abi.stream_of(x))
    _abi.check(st, "hg_hexconv2d_backward")
    gk = dk.reshape(kshape).to(kernel.dtype) if dk is not None else None
    gb = db.to(bias.dtype) if db is not None else None
    return dx, gk, gb


def hexconv2d_backward_plan(x_dtype, w_dtype, batch, in_channels, out_channels, h, w, radius,
                            stride=1, padding=0, dilation=1, groups=1, padding_mode="constant"):
    """(d input kernel, d kernel kernel) of hexconv2d_backward for this layer, each
    _abi.HG_CONV_BWD_GENERIC or _abi.HG_CONV_BWD_MFMA (hg_hexconv2d_backward_plan): which
    kernels the call would run, HYGRID_CONV_BWD_MFMA included.  Nothing is launched and no
    device is needed.  x_dtype / w_dtype: torch dtypes or hg_dtype codes."""
    pm = _abi.PAD_MODES.get(padding_mode)
    if pm is None:
        raise ValueError(f"unsupported padding_mode {padding_mode!r}")
    xd = x_dtype if isinstance(x_dtype, int) else _abi.dtype_code(x_dtype)
    wd = w_dtype if isinstance(w_dtype, int) else _abi.dtype_code(w_dtype)
    dxk, dwk = ctypes.c_int(), ctypes.c_int()
    st = _abi.lib().hg_hexconv2d_backward_plan(
        xd, wd, int(batch), int(in_channels), int(out_channels), int(h), int(w), int(radius),
        int(stride), int(padding), int(dilation), int(groups), pm, ctypes.byref(dxk),
        ctypes.byref(dwk))
    _abi.check(st, "hg_hexconv2d_backward_plan")
    return dxk.value, dwk.value


def _pad_mode(padding_mode):
    pm = _abi.PAD_MODES.get(padding_mode)
    if pm is None:
        raise ValueError(f"unsupported padding_mode {padding_mode!r}")
    return pm


def hexconv2d_weight_grad_plan(x_dtype, w_dtype, batch, in_channels, out_channels, h, w, radius,
                               stride=1, padding=0, dilation=1, groups=1, padding_mode="constant"):
    """Which kernel hexconv2d_weight_grad runs for d kernel (+ d bias) of this layer
    (hg_hexconv2d_weight_grad_plan): _abi.HG_CONV_WGRAD_GENERIC, _MFMA (stride 1) or _MFMA_S2
    (stride 2), the switches HYGRID_CONV_BWD_MFMA / HYGRID_CONV_BWD_MFMA_S2 included.  Nothing is
    launched and no device is needed.  dtypes: torch dtypes or hg_dtype codes."""
    pm = _pad_mode(padding_mode)
    xd = x_dtype if isinstance(x_dtype, int) else _abi.dtype_code(x_dtype)
    wd = w_dtype if isinstance(w_dtype, int) else _abi.dtype_code(w_dtype)
    kern = ctypes.c_int()
    st = _abi.lib().hg_hexconv2d_weight_grad_plan(
        xd, wd, int(batch), int(in_channels), int(out_channels), int(h), int(w), int(radius),
        int(stride), int(padding), int(dilation), int(groups), pm, ctypes.byref(kern))
    _abi.check(st, "hg_hexconv2d_weight_grad_plan")
    return kern.value


def hexconv2d_training_plan(x_dtype, w_dtype, batch, in_channels, out_channels, h, w, radius,
                            stride=1, padding=0, dilation=1, groups=1, even_odd_offset=0,
                            padding_mode="constant"):
    """(d input route, d kernel route) of hexconv2d_grads for this layer.  d input: "convt_s2"
    (stride 2, constant padding: hexconv_transpose2d on gy where hexconv_transpose2d_plan, asked
    with the channel counts swapped, answers _abi.HG_CONVT_MFMA_S2), else what
    hexconv2d_backward_plan says for d input, "mfma" or "generic".  d kernel: the
    hg_conv_wgrad_kernel value of hexconv2d_weight_grad_plan.  Every switch is read as the calls
    read it (HYGRID_CONVT_MFMA=0 also switches "convt_s2" off).  Nothing is launched and no
    device is needed; gy is taken to have the weights' dtype, as hexconv2d_grads makes it."""
    pm = _pad_mode(padding_mode)
    xd = x_dtype if isinstance(x_dtype, int) else _abi.dtype_code(x_dtype)
    wd = w_dtype if isinstance(w_dtype, int) else _abi.dtype_code(w_dtype)
    dk_route = hexconv2d_weight_grad_plan(xd, wd, batch, in_channels, out_channels, h, w, radius,
                                          stride, padding, dilation, groups, padding_mode)
    floats = (_abi.HG_F16, _abi.HG_BF16, _abi.HG_F32, _abi.HG_F64)
    if stride == 2 and pm == 0 and batch > 0 and xd in floats:
        ho, wo = hexconv2d_out_shape(h, w, radius, stride, padding, dilation)
        if ho > 0 and wo > 0 and hexconv_transpose2d_plan(
                wd, wd, xd, batch, out_channels, in_channels, ho, wo, h, w, radius, stride,
                padding, dilation, groups, even_odd_offset) == _abi.HG_CONVT_MFMA_S2:
            return "convt_s2", dk_route
    dxk, _ = hexconv2d_backward_plan(xd, wd, batch, in_channels, out_channels, h, w, radius,
                                     stride, padding, dilation, groups, padding_mode)
    return ("mfma" if dxk == _abi.HG_CONV_BWD_MFMA else "generic"), dk_route


def hexconv2d_weight_grad(gy, x, kernel, bias, cfg, need_k=True, need_b=True):
    """(d kernel, d bias) of hexconv2d (hg_hexconv2d_weight_grad), hexconv2d_backward's
    arguments and contract: None for a gradient not requested (d bias also when bias is None),
    the parameters' shapes and dtypes."""
    _abi.require_device(gy)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    kdt = kernel.dtype if kernel.dtype in (torch.float32, torch.float64) else torch.float32
    kshape = tuple(kernel.shape)
    O, cg = int(kshape[0]), int(kshape[1])
    K = int(kernel.numel()) // max(O * cg, 1)
    g = gy.detach().to(kdt).contiguous()
    dk = torch.empty((O, cg, K), dtype=kdt, device=x.device) if need_k else None
    db = (torch.empty((O,), dtype=kdt, device=x.device)
          if (need_b and bias is not None) else None)
    st = _abi.lib().hg_hexconv2d_weight_grad(
        _abi.ptr(x), _abi.ptr(g), _abi.ptr(dk), _abi.ptr(db), _abi.dtype_code(x.dtype),
        _abi.dtype_code(kdt), B, C, O, h, w, cfg["r"], cfg["stride"], cfg["pad"], cfg["dilation"],
        cfg["groups"], int(cfg["off"]), _pad_mode(cfg["padding_mode"]),
        float(cfg["padding_value"]), _abi.stream_of(x))
    _abi.check(st, "hg_hexconv2d_weight_grad")
    gk = dk.reshape(kshape).to(kernel.dtype) if dk is not None else None
    gb = db.to(bias.dtype) if db is not None else None
    return gk, gb


def hexconv2d_grads(gy, x, kernel, bias, cfg, need_x=True, need_k=True, need_b=True):
    """The gradients a layer's autograd asks for, (d x, d kernel, d bias) with
    hexconv2d_backward's contract, each on the fastest kernel it has
    (hexconv2d_training_plan): d kernel / d bias through hexconv2d_weight_grad; d input of a
    stride-2 layer as hexconv_transpose2d of gy with the layer's own kernel (a HexConv2d
    kernel [O, C, 1, K] is the transposed layer's [in, out, 1, K]: no copy; the pad value never
    reaches d input), otherwise hexconv2d_backward's d input."""
    _abi.require_device(gy)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    dx = gk = gb = None
    if need_k or (need_b and bias is not None):
        gk, gb = hexconv2d_weight_grad(gy, x, kernel, bias, cfg, need_k, need_b)
    if need_x:
        B, C, h, w = (int(s) for s in x.shape)
        kdt = kernel.dtype if kernel.dtype in (torch.float32, torch.float64) else torch.float32
        route = "generic"
        if x.dtype in _abi.TORCH_DTYPE:
            route, _ = hexconv2d_training_plan(
                x.dtype, kdt, B, C, int(kernel.shape[0]), h, w, cfg["r"], cfg["stride"],
                cfg["pad"], cfg["dilation"], cfg["groups"], int(cfg["off"]), cfg["padding_mode"])
        if route == "convt_s2":
            dx = hexconv_transpose2d(gy.detach().to(kdt), kernel, None, cfg["off"], cfg["r"], 2,
                                     cfg["pad"], 1, 1, output_size=(h, w), out_dtype=x.dtype)
        else:
            dx = hexconv2d_backward(gy, x, kernel, bias, cfg, True, False, False)[0]
    return dx, gk, gb


def hexconv2d_forward_plan(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, h, w,
                           radius, stride=1, padding=0, dilation=1, groups=1, even_odd_offset=0,
                           padding_mode="constant", padding_value=0.0):
    """Which wide-channel kernel hexconv2d would run for this layer (hg_hexconv2d_forward_plan):
    _abi.HG_CONV_FWD_MFMA_F32, _MFMA_BF16, _MFMA_BF16_DMA, or _abi.HG_CONV_FWD_OTHER (the
    streaming or generic kernels), the HYGRID_CONV_MFMA* / HYGRID_CONV_DMA switches included.
    Answered for a 16-byte-aligned x (a less than 4-byte-aligned bf16 x runs _MFMA_BF16 where
    this says _DMA).  Nothing is launched and no device is needed.  dtypes: torch dtypes or
    hg_dtype codes."""
    pm = _abi.PAD_MODES.get(padding_mode)
    if pm is None:
        raise ValueError(f"unsupported padding_mode {padding_mode!r}")
    xd, wd, yd = (d if isinstance(d, int) else _abi.dtype_code(d)
                  for d in (x_dtype, w_dtype, y_dtype))
    kern = ctypes.c_int()
    st = _abi.lib().hg_hexconv2d_forward_plan(
        xd, wd, yd, int(batch), int(in_channels), int(out_channels), int(h), int(w), int(radius),
        int(stride), int(padding), int(dilation), int(groups), int(even_odd_offset), pm,
        float(padding_value), ctypes.byref(kern))
    _abi.check(st, "hg_hexconv2d_forward_plan")
    return kern.value


def _convt_valid_sizes(hin, win, radius, stride, padding, dilation):
    """([h...], [w...]) ascending: every output size a HexConv2d of these arguments maps onto
    (hin, win), found by searching hexconv2d_out_shape around its inverse."""
    kh = (2 * radius - 2) * dilation + 1
    kw = 2 * dilation * (2 * radius - 2) + 1
    h0 = (hin - 1) * stride + kh - 2 * padding
    w0 = (2 * stride * (win - 1) + stride + kw + 1) // 2 - 2 * padding
    hs, ws = [], []
    for h in range(max(h0 - 1, 1), h0 + stride + 1):
        for w in range(max(w0 - 1, 1), w0 + stride + 1):
            try:
                ho, wo = hexconv2d_out_shape(h, w, radius, stride, padding, dilation)
            except ValueError:
                continue
            if ho == hin and h not in hs:
                hs.append(h)
            if wo == win and w not in ws:
                ws.append(w)
    return hs, ws


def hexconv_transpose2d_out_shape(hin, win, radius, stride=1, padding=0, dilation=1,
                                  output_size=None):
    """Output size (h, w) of hexconv_transpose2d for a (hin, win) input.  Valid sizes are those
    the adjoint HexConv2d maps back: hexconv2d_out_shape(h, w, radius, stride, padding, dilation)
    == (hin, win); stride s leaves s choices per axis.  output_size=None picks the largest valid
    h and the smallest valid w, (2 hin + 2 - 2p, 2 win + 2 - 2p) at radius 2, stride 2: exactly
    x2 at padding 1.  Any other output_size raises ValueError."""
    hin, win = int(hin), int(win)
    if hin < 1 or win < 1:
        raise ValueError(f"hexconv_transpose2d: empty input {(hin, win)}")
    hs, ws = _convt_valid_sizes(hin, win, radius, stride, padding, dilation)
    if not hs or not ws:
        raise ValueError(f"hexconv_transpose2d: no output size maps onto {(hin, win)}")
    if output_size is None:
        return max(hs), min(ws)
    h, w = (int(v) for v in tuple(output_size)[-2:])
    if h not in hs or w not in ws:
        raise ValueError(f"hexconv_transpose2d: output_size {(h, w)} is not one of "
                         f"{[(a, b) for a in hs for b in ws]} for input {(hin, win)}")
    return h, w


def hexconv_transpose2d_plan(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, hin,
                             win, h, w, radius, stride=1, padding=0, dilation=1, groups=1,
                             even_odd_offset=0):
    """Which route hexconv_transpose2d takes for this layer (hg_hexconv_transpose2d_plan):
    _abi.HG_CONVT_MFMA_S2 (k_hexconvt_s2 on the matrix cores) or _abi.HG_CONVT_ADJOINT (the
    adjoint conv's d input, then a bias add), HYGRID_CONVT_MFMA included.  Nothing is launched
    and no device is needed.  dtypes: torch dtypes or hg_dtype codes."""
    xd, wd, yd = (d if isinstance(d, int) else _abi.dtype_code(d)
                  for d in (x_dtype, w_dtype, y_dtype))
    kern = ctypes.c_int()
    st = _abi.lib().hg_hexconv_transpose2d_plan(
        xd, wd, yd, int(batch), int(in_channels), int(out_channels), int(hin), int(win), int(h),
        int(w), int(radius), int(stride), int(padding), int(dilation), int(groups),
        int(even_odd_offset), ctypes.byref(kern))
    _abi.check(st, "hg_hexconv_transpose2d_plan")
    return kern.value


def hexconv_transpose2d_taps(even_odd_offset, padding, row_class, col_class):
    """[(t, rofs, qofs), ...] of output class (iy mod 4, ix mod 2) at radius 2, stride 2: the
    table k_hexconvt_s2 is launched with (hg_hexconv_transpose2d_taps; host only)."""
    out = (ctypes.c_int * 7)()
    st = _abi.lib().hg_hexconv_transpose2d_taps(int(even_odd_offset), int(padding),
                                                int(row_class), int(col_class), out)
    _abi.check(st, "hg_hexconv_transpose2d_taps")
    return [tuple(out[1 + 3 * j:4 + 3 * j]) for j in range(out[0])]


def hexconv_transpose2d(x, kernel, bias, even_odd_offset, radius, stride=1, padding=0,
                        dilation=1, groups=1, output_size=None, out_dtype=None):
    """HexConvTranspose2d forward (hg_hexconv_transpose2d): the adjoint of
    hexconv2d(., kernel, None, even_odd_offset, radius, stride, padding, dilation, groups) with
    constant zero padding, plus bias.  x: (B, I, hin, win) -> (B, O, h, w), (h, w) by
    hexconv_transpose2d_out_shape.  kernel: (I, O/groups, 1, K) or (I, O/groups, K), float32 /
    float64 (the accumulation dtype); even_odd_offset is the output's row offset.
    On the adjoint route (hexconv_transpose2d_plan) x is converted to the kernel's dtype and the
    result to out_dtype, as hexconv2d_backward does; the matrix-core route reads x and writes
    out_dtype directly."""
    _abi.require_device(x)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, I, hin, win = (int(s) for s in x.shape)
    k = kernel.detach()
    if k.dtype not in (torch.float32, torch.float64):
        k = k.float()
    k = k.reshape(k.shape[0], k.shape[1], -1).contiguous()
    if int(k.shape[0]) != I:
        raise ValueError(f"kernel expects {int(k.shape[0])} input channels, got {I}")
    O = int(k.shape[1]) * groups
    b = None
    if bias is not None:
        b = bias.detach().to(k.dtype).contiguous()
        if b.numel() != O:
            raise ValueError(f"bias must have {O} elements")
    if out_dtype is None:
        out_dtype = torch.get_default_dtype()
    h, w = hexconv_transpose2d_out_shape(hin, win, radius, stride, padding, dilation, output_size)
    if not x.dtype.is_floating_point:
        x = x.to(k.dtype)
    route = hexconv_transpose2d_plan(x.dtype, k.dtype, out_dtype, B, I, O, hin, win, h, w, radius,
                                     stride, padding, dilation, groups, even_odd_offset)
    y_dtype = out_dtype
    if route == _abi.HG_CONVT_ADJOINT:
        x, y_dtype = x.to(k.dtype), k.dtype
    y = torch.empty((B, O, h, w), dtype=y_dtype, device=x.device)
    st = _abi.lib().hg_hexconv_transpose2d(
        _abi.ptr(x), _abi.ptr(k), _abi.ptr(b), _abi.ptr(y), _abi.dtype_code(x.dtype),
        _abi.dtype_code(k.dtype), _abi.dtype_code(y_dtype), B, I, O, hin, win, h, w, radius,
        stride, padding, dilation, groups, int(even_odd_offset), _abi.stream_of(x))
    _abi.check(st, "hg_hexconv_transpose2d")
    return y if y_dtype == out_dtype else y.to(out_dtype)


def hex_to_type1(x, even_odd_offset, row_repeat=1, out_dtype=None):
    """Offset-row hex raster (..., H, W) -> type1 (..., H*row_repeat, 2W+1) on the GPU
    (hg_hex_to_type1): row_repeat 1 = HexFrames.heximage_to_type1 (HexFrames.py:417-445),
    2 = heximage_to_type2 (:446-449).  out_dtype converts first (the reference's torch
    version returns the default float dtype)."""
    _abi.require_device(x)
    if out_dtype is not None and x.dtype != out_dtype:
        x = x.to(out_dtype)
    x, lead, planes = _planes(x)
    h, w = int(x.shape[-2]), int(x.shape[-1])
    y = torch.empty(lead + (h * row_repeat, 2 * w + 1), dtype=x.dtype, device=x.device)
    st = _abi.lib().hg_hex_to_type1(_abi.ptr(x), _abi.ptr(y), x.element_size(), planes, h, w,
                                    int(even_odd_offset) & 1, int(row_repeat), _abi.stream_of(x))
    _abi.check(st, "hg_hex_to_type1")
    return y


def strided_copy2d(x, row_start, row_step, col_start, col_step, h_out=None, w_out=None):
    """Contiguous x[..., row_start::row_step, col_start::col_step] (bounded by h_out /
    w_out) by one gfx950 gather (hg_strided_copy2d): type1 / type2 decoding
    (HexImage.py:108-111, HexFrames.py:450-458) into a kernel-ready raster."""
    _abi.require_device(x)
    x, lead, planes = _planes(x)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    if h_out is None:
        h_out = len(range(row_start, H, row_step))
    if w_out is None:
        w_out = len(range(col_start, W, col_step))
    y = torch.empty(lead + (h_out, w_out), dtype=x.dtype, device=x.device)
    st = _abi.lib().hg_strided_copy2d(_abi.ptr(x), _abi.ptr(y), x.element_size(), planes, H, W,
                                      row_start, row_step, col_start, col_step, h_out, w_out,
                                      _abi.stream_of(x))
    _abi.check(st, "hg_strided_copy2d")
    return y


HG_EUNSUP = _abi.HG_EUNSUP


def pipeline_r2h_h2r(x, hex_size=None, out_dtype=None):
    """Fused rect -> hex (bilinear) -> rect (linear) round trip, no conv: the same result as
    hex_to_rect(rect_to_hex(x, hex_size), hex_size) (geometry_np.py:358-519, :191-356) with
    the hex image kept in fp32 on chip.  x: (..., h, w) device tensor -> (..., h1, w1).

    Returns None when the fused kernel does not cover the geometry / dtypes (the caller then
    runs the two resamplers); raises on argument errors.
    """
    _abi.require_device(x)
    x = x.contiguous()
    h, w = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // max(h * w, 1)
    h1, w1 = (h, w) if hex_size is None else (int(hex_size[0]), int(hex_size[1]))
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float16) else torch.float32
    y = torch.empty(tuple(x.shape[:-2]) + (h1, w1), dtype=out_dtype, device=x.device)
    st = _abi.lib().hg_pipeline_r2h_h2r(_abi.ptr(x), _abi.ptr(y), _abi.dtype_code(x.dtype),
                                        _abi.dtype_code(out_dtype), planes, h, w, h1, w1,
                                        _abi.stream_of(x))
    if st in (HG_EUNSUP, _abi.HG_EDTYPE):
        return None
    _abi.check(st, "hg_pipeline_r2h_h2r")
    return y


def pipeline_r2h_conv_h2r(x, kernel, bias, hex_size=None, rect_size=None, padding=1, groups=1,
                          even_odd_offset=0, padding_value=0.0, out_dtype=None):
    """Fused rect -> hex (bilinear) -> HexConv2d (radius 2) -> hex -> rect (linear).

    Returns None when the fused kernel does not cover the geometry / dtypes (the
    caller then runs the three operators); raises on argument errors.
    """
    _abi.require_device(x)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    h1, w1 = (h, w) if hex_size is None else (int(hex_size[0]), int(hex_size[1]))
    ho, wo = hexconv2d_out_shape(h1, w1, 2, 1, padding, 1)
    h2, w2 = (ho, wo) if rect_size is None else (int(rect_size[0]), int(rect_size[1]))
    k = kernel.detach().float().reshape(kernel.shape[0], -1).contiguous()
    O = int(k.shape[0])
    b = bias.detach().float().contiguous() if bias is not None else None
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float16) else torch.float32
    y = torch.empty((B, O, h2, w2), dtype=out_dtype, device=x.device)
    st = _abi.lib().hg_pipeline_r2h_conv_h2r(
        _abi.ptr(x), _abi.ptr(k), _abi.ptr(b), _abi.ptr(y), _abi.dtype_code(x.dtype),
        _abi.dtype_code(out_dtype), B, C, O, h, w, h1, w1, h2, w2, int(padding), int(groups),
        int(even_odd_offset), float(padding_value), _abi.stream_of(x))
    if st in (HG_EUNSUP, _abi.HG_EDTYPE):
        return None
    _abi.check(st, "hg_pipeline_r2h_conv_h2r")
    return y


def _chain_geometry(x, kernel, hex_size, rect_size, padding):
    B, C, h, w = (int(s) for s in x.shape)
    h1, w1 = (h, w) if hex_size is None else (int(hex_size[0]), int(hex_size[1]))
    ho, wo = hexconv2d_out_shape(h1, w1, 2, 1, padding, 1)
    h2, w2 = (ho, wo) if rect_size is None else (int(rect_size[0]), int(rect_size[1]))
    return B, C, int(kernel.shape[0]), h, w, h1, w1, h2, w2


def pipeline_r2h_conv_h2r_backward_workspace(x, gy_dtype, kernel, hex_size=None, rect_size=None,
                                             padding=1, groups=1, even_odd_offset=0,
                                             padding_value=0.0):
    """Bytes of workspace the fused backward of pipeline_r2h_conv_h2r needs for the 4-D input x
    and an upstream gradient of gy_dtype, or None when the backward does not cover the call
    (hg_pipeline_r2h_conv_h2r_backward_workspace; nothing is launched)."""
    if x.dim() != 4 or x.dtype not in _abi.TORCH_DTYPE or gy_dtype not in _abi.TORCH_DTYPE:
        return None
    try:
        geo = _chain_geometry(x, kernel, hex_size, rect_size, int(padding))
    except ValueError:
        return None
    B, C, O, h, w, h1, w1, h2, w2 = geo
    need = int(_abi.lib().hg_pipeline_r2h_conv_h2r_backward_workspace(
        _abi.dtype_code(x.dtype), _abi.dtype_code(gy_dtype), B, C, O, h, w, h1, w1, h2, w2,
        int(padding), int(groups), int(even_odd_offset), float(padding_value)))
    return need if need > 0 else None


# one byte workspace per (device, stream) for the fused backward's slab of partial sums (every
# call writes the rows it reads; calls on one stream are ordered, so they can share it)
_BWD_WS = {}


def _backward_workspace(device, stream, nbytes):
    key = (device.index, int(stream.value or 0))
    ws = _BWD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        _BWD_WS[key] = ws
    return ws


def pipeline_r2h_conv_h2r_backward(gy, x, kernel, hex_size=None, rect_size=None, padding=1,
                                   groups=1, even_odd_offset=0, padding_value=0.0, need_x=True,
                                   need_k=True, need_b=True):
    """Gradients of pipeline_r2h_conv_h2r (hg_pipeline_r2h_conv_h2r_backward): (d x, d kernel,
    d bias) for the upstream gradient gy (B, O, h2, w2) and the forward's input x (B, C, h, w),
    with no hex-sized tensor in memory (the hex image is recomputed on chip).

    d x has x's dtype; d kernel (O, C/groups, 7) and d bias (O,) are float32 and bit-reproducible
    from call to call.  None for the gradients not requested.  Returns None (not a tuple) when
    the fused backward does not cover the call; raises on argument errors.
    """
    _abi.require_device(gy)
    x = x.detach().contiguous()
    gy = gy.detach()
    if gy.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        gy = gy.float()
    gy = gy.contiguous()
    need = pipeline_r2h_conv_h2r_backward_workspace(x, gy.dtype, kernel, hex_size, rect_size,
                                                    padding, groups, even_odd_offset,
                                                    padding_value)
    if need is None:
        return None
    B, C, O, h, w, h1, w1, h2, w2 = _chain_geometry(x, kernel, hex_size, rect_size, int(padding))
    if tuple(gy.shape) != (B, O, h2, w2):
        raise ValueError(f"gy has shape {tuple(gy.shape)}, expected {(B, O, h2, w2)}")
    k = kernel.detach().float().reshape(O, -1).contiguous()
    dx = torch.empty_like(x) if need_x else None
    dk = torch.empty((O, k.shape[1] // 7, 7), dtype=torch.float32, device=x.device) if need_k else None
    db = torch.empty((O,), dtype=torch.float32, device=x.device) if need_b else None
    st_ = _abi.stream_of(x)
    ws = _backward_workspace(x.device, st_, need) if (need_k or need_b) else None
    st = _abi.lib().hg_pipeline_r2h_conv_h2r_backward(
        _abi.ptr(x), _abi.ptr(k), _abi.ptr(gy), _abi.ptr(dx), _abi.ptr(dk), _abi.ptr(db),
        _abi.dtype_code(x.dtype), _abi.dtype_code(gy.dtype), B, C, O, h, w, h1, w1, h2, w2,
        int(padding), int(groups), int(even_odd_offset), float(padding_value), _abi.ptr(ws),
        ws.numel() if ws is not None else 0, st_)
    if st == HG_EUNSUP:
        return None
    _abi.check(st, "hg_pipeline_r2h_conv_h2r_backward")
    return dx, dk, db


# one int32 workspace per (device, stream) for hg_hex_pyramid_chain (each call zeroes it on the
# stream first; calls on one stream are ordered, so they can share it)
_CHAIN_WS = {}


def chain_workspace(device, stream, nbytes):
    """The (device, stream)'s pyramid-chain workspace, at least nbytes (int [1] after a call:
    the chain's fault word, 0 unless a workgroup waited > ~1 s for its input)."""
    key = (device.index, int(stream.value or 0))
    ws = _CHAIN_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.zeros(max(nbytes // 4 + 4, 1024), dtype=torch.int32, device=device)
        _CHAIN_WS[key] = ws
    return ws


def hex_pyramid_chain(x, taps, bias=None, levels=3, even_odd_offset=0):
    """`levels` pyramid levels from the rect image x in ONE launch (hg_hex_pyramid_chain):
    level 0 = hex_pyramid_level(x, from_rect=True), level l = hex_pyramid_level(level l - 1),
    each (h // 2, w // 2) of the one before, all in x's dtype (16-bit), bit-identical to those
    calls.  Returns the list of levels, or None outside the chain's domain (levels 2-3, C = 3,
    every level on the fused kernel: the caller then runs the levels one launch each)."""
    _abi.require_device(x)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    if x.dtype not in (torch.float16, torch.bfloat16) or not 2 <= levels <= 3:
        return None
    k = taps.detach().float().reshape(C, 7).contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    outs, hl, wl = [], h, w
    for _ in range(levels):
        hl, wl = hl // 2, wl // 2
        outs.append(torch.empty((B, C, hl, wl), dtype=x.dtype, device=x.device))
    L = _abi.lib()
    need = int(L.hg_hex_pyramid_chain_workspace(int(levels), B, h))
    if need < 0:
        _abi.check(need, "hg_hex_pyramid_chain_workspace")
    st_ = _abi.stream_of(x)
    ws = chain_workspace(x.device, st_, need)
    ys = (ctypes.c_void_p * levels)(*[o.data_ptr() for o in outs])
    st = L.hg_hex_pyramid_chain(_abi.ptr(x), ys, int(levels), _abi.dtype_code(x.dtype), B, C, h,
                                w, _abi.ptr(k), _abi.ptr(b), int(even_odd_offset), _abi.ptr(ws),
                                ws.numel() * 4, st_)
    if st in (HG_EUNSUP, _abi.HG_EDTYPE):
        return None
    _abi.check(st, "hg_hex_pyramid_chain")
    return outs


def hex_pyramid_level(x, taps, bias=None, size=None, even_odd_offset=0, from_rect=False,
                      out_dtype=None, out=None):
    """One hex Gaussian pyramid level in one pass: hexresize(HexConv2d_depthwise(x))
    (geometry_np.py:520-681 after HexFrames.py:96-169, radius 2, padding 1, pad value 0),
    with rect_to_hex(x) (geometry_np.py:358-519) first when from_rect.

    x: (B, C, h, w) device tensor; taps: the depthwise kernel (C, 1, 1, 7) or (C, 7);
    size: (h1, w1), default (h // 2, w // 2).  out: an optional contiguous (B, C, h1, w1)
    tensor of out_dtype to write into (e.g. a slice of a larger batch).  Returns None when the
    fused kernel does not cover the geometry / dtypes (the caller then runs the operators).
    """
    _abi.require_device(x)
    while x.dim() < 4:
        x = x.unsqueeze(0)
    x = x.contiguous()
    B, C, h, w = (int(s) for s in x.shape)
    h1, w1 = (h // 2, w // 2) if size is None else (int(size[0]), int(size[1]))
    k = taps.detach().float().reshape(C, 7).contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float16) else torch.float32
    if out is None:
        y = torch.empty((B, C, h1, w1), dtype=out_dtype, device=x.device)
    else:
        if (tuple(out.shape) != (B, C, h1, w1) or out.dtype != out_dtype
                or out.device != x.device or not out.is_contiguous()):
            raise ValueError(f"hex_pyramid_level: out must be a contiguous {(B, C, h1, w1)} "
                             f"{out_dtype} tensor on {x.device}")
        y = out
    st = _abi.lib().hg_hex_pyramid_level(
        _abi.ptr(x), _abi.ptr(y), _abi.dtype_code(x.dtype), _abi.dtype_code(out_dtype), B, C,
        h, w, h1, w1, _abi.ptr(k), _abi.ptr(b), int(even_odd_offset), int(bool(from_rect)),
        _abi.stream_of(x))
    if st in (HG_EUNSUP, _abi.HG_EDTYPE):
        return None
    _abi.check(st, "hg_hex_pyramid_level")
    return y
