"""The case table of the hex pooling kernels (csrc/pool.hip) on tied, quantised and large-window
inputs, shared by tests/test_gpu_pool_windows.py (which runs it on the device against the fp64
oracle) and tests/test_pool_window_cases_cpu.py (which checks without a device, from the
library's route query hg_hex_pool2d_route, that every case lies in the regions it is filed under,
that every region has a case for every method and type it claims, that the tied inputs are tied,
and that the oracle agrees with torch's own autograd on every float64 case).

pool.hip has four kernels: k_pool_small / k_pool_bwd_small (one thread per output, a sequential
walk of the window) and k_pool_large / k_pool_bwd_large (windows of 512 elements and more: one
256-thread workgroup per output, thread t holding window elements t, t + 256, ..., then an LDS
tree).  max / min keep the FIRST extreme in window order, which a forward value cannot show and
continuous random data never exercises: here the data are integers in 0..3 (a ReLU or a quantiser
before the pool), constant planes, all-NaN planes, signed zeros and NaN / infinity windows, the
windows sit on both sides of the 512-element threshold, and the large kernels run through
HexPool2d's padded, ceil-extended and overlapping windows as well.

A case is (geometry, data, method, dtype).  It goes through the public modules (HexPool2d,
HexAdaptivePool2d, HexGlobalPool2d, max_pooling / min_pooling / average_pooling).  The table
holds no route: a region is a predicate on the case, its window geometry and the route the
library reports, so a change of the threshold fails the CPU test instead of un-covering a kernel.

Not a conftest and not a test: imported like tests/resample_plane_cases.py."""
import functools
import zlib

import torch
import torch.nn.functional as F

from pool_cases import pool_args

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTYPES = (F64, F32, BF16, F16)
DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32", F64: "f64"}
METHODS = ("max", "min", "average")
SMALL, LARGE = 0, 1                                       # enum hg_pool_kernel
N_MAX = 2048        # every window: an f16 count stays exact, nothing overflows

# ---- geometries: name -> (kind, lead dims, h, w, meta) ----------------------------------------
# kind "reduce": max_pooling / min_pooling / average_pooling over rows of w values (a 1 x w
# window); "global" / "adaptive" / "pool": the modules (meta as tests/pool_cases.py reads it).
GEOMS = {
    # one thread per output
    "reduce511": ("reduce", (3, 8), 1, 511, {}),
    "adaptive3_60x77": ("adaptive", (2, 4), 60, 77, dict(outsize=3)),                 # 20 x 22
    "pool3s2_const3": ("pool", (2, 4), 13, 16, dict(k=3, s=2, pad=1, value=3.0)),
    "pool3s2_const0": ("pool", (2, 4), 13, 16, dict(k=3, s=2, pad=1, value=0.0)),
    "pool3x2s2_reflect_ceil": ("pool", (2, 4), 13, 16,
                               dict(k=[3, 2], s=[2, 2], pad=1, mode="reflect", ceil=True, cip=False)),
    # one workgroup per output
    "reduce512": ("reduce", (3, 8), 1, 512, {}),
    "reduce513": ("reduce", (3, 8), 1, 513, {}),
    "global16x32": ("global", (2, 4), 16, 32, {}),                                    # 512
    "global17x31": ("global", (2, 4), 17, 31, {}),                                    # 527
    "adaptive2_48x60": ("adaptive", (2, 4), 48, 60, dict(outsize=2)),                 # 24 x 24
    "pool23_reflect_ceil": ("pool", (2, 4), 50, 61,
                            dict(k=23, s=23, pad=3, mode="reflect", ceil=True, cip=True)),
    "pool23_const3_ceil_nocip": ("pool", (2, 4), 50, 61,
                                 dict(k=23, s=23, pad=2, value=3.0, ceil=True, cip=False)),
    "pool23_const0": ("pool", (2, 4), 50, 60, dict(k=23, s=23, pad=2, value=0.0)),
    "pool23_replicate": ("pool", (2, 4), 50, 60, dict(k=23, s=23, pad=2, mode="replicate")),
    "pool23_circular": ("pool", (2, 4), 50, 60, dict(k=23, s=23, pad=2, mode="circular")),
    # (the reference's output width assumes kw <= sw; 5 columns of overlap fit a 68-wide frame)
    "pool20x30_s7x25_reflect": ("pool", (2, 4), 50, 66,
                                dict(k=[20, 30], s=[7, 25], pad=1, mode="reflect")),   # 600
}
# tie-free controls (distinct values) and the constant planes of the 16-bit count check
FREE_GEOMS = ("reduce511", "pool3s2_const3", "global17x31", "pool20x30_s7x25_reflect")
CONST_GEOMS = ("reduce511", "reduce512", "reduce513", "global17x31")

# plane p of a "mixed" input holds class MIXED[p % 8]
MIXED = ("ints_nan", "ints_nan", "ints_nan_inf", "constant", "all_nan", "signed_zeros",
         "nan_first_inf", "ints")
INT_CLASSES = ("ints_nan", "ints_nan_inf", "ints")
# "const" inputs: plane p holds value v on n_valid elements of its one window and NaN on the
# rest, (v, n_valid) = const_planes(n)[p % len].  bf16 rounds the counts 257, 511, 513 and 527
# to 256, 512, 512 and 528.  With the sum s rounded to bf16 first, s / 512 is s's own mantissa
# and s / 511 or s / 513 lies within half a bf16 step of it for every s (s / 511 <= s * 2^-8 *
# 255/256 of a step at the top of a binade), so at 511 and 513 an unrounded count cannot show
# in the forward value; at 527 (145/128: 1.125 against 1.1328125) and 257 (1.0: 1 against
# 0.99609375) it does.
CONST_VALUES = {257: (1.0, 1.5), 511: (1.0, 0.75), 513: (1.0, 1.75), 527: (1.0, 145 / 128)}


def const_planes(n):
    return [(v, nv) for nv in sorted(CONST_VALUES) if nv <= n for v in CONST_VALUES[nv]]


class Case:
    """geom: a GEOMS key; data: "mixed" (the plane classes MIXED), "free" (distinct values, 5 %
    NaN: no window holds its extreme at two elements) or "const" (constant planes with a known
    number of NaN); method; dtype; regions: the REGIONS entries the case is filed under."""

    def __init__(self, geom, data, method, dtype, regions):
        self.geom, self.data, self.method, self.dtype = geom, data, method, dtype
        self.kind, self.lead, self.h, self.w, meta = GEOMS[geom]
        self.meta = dict(meta, kind=self.kind, method=method, h=self.h, w=self.w)
        self.regions = tuple(regions)
        self.name = f"{geom}-{data}-{method}-{DT_NAME[dtype]}"

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        """Shape of the tensor handed to the module (reduce: rows of w values)."""
        return self.lead + ((self.w,) if self.kind == "reduce" else (self.h, self.w))

    @property
    def args(self):
        """(method, kh, kw, sh, sw, hn, wn, pad, mode, value, ext_h, ext_w, ext_value): the
        window arguments of oracle.hex_pool2d on the (lead, h, w) raster."""
        if self.kind == "reduce":
            return (self.method, 1, self.w, 1, self.w, 1, 1, 0, "constant", 0, 0, 0, 0.0)
        return pool_args(self.meta)

    @property
    def n(self):
        return self.args[1] * self.args[2]

    def route(self, backward=False):
        """The kernel pair the library runs the case on (hg_hex_pool2d_route)."""
        from HyGrid import _abi
        return _abi.hex_pool2d_route(self.args[1], self.args[2], backward)

    def apply(self, x):
        """The case through the package's public surface (x on the device)."""
        from HyGrid import HexFrames as HF
        from pool_cases import module_for
        if self.kind == "reduce":
            return {"max": HF.max_pooling, "min": HF.min_pooling,
                    "average": HF.average_pooling}[self.method](x)
        return module_for(self.meta)(x)

    def raster(self, x):
        """x as the (lead, h, w) raster of the oracle; out(y): y as (lead, hn, wn)."""
        return x.unsqueeze(-2) if self.kind == "reduce" else x

    def out(self, y):
        return y.reshape(self.lead + self.args[5:7])


# ---- the operation restated in torch (CPU, differentiable): window gather ----------------------
def window_index(args):
    """(rows, cols), each (hn, wn, kh*kw): frame coordinates of window (i, j)'s elements in
    row-major window order: rows i*sh + [0, kh), columns (i % 2) * sw // 2 + j*sw + [0, kw)."""
    _, kh, kw, sh, sw, hn, wn = args[:7]
    i = torch.arange(hn).view(-1, 1, 1)
    j = torch.arange(wn).view(1, -1, 1)
    k = torch.arange(kh * kw).view(1, 1, -1)
    rows = (i * sh + k // kw).expand(hn, wn, kh * kw)
    cols = ((i % 2) * sw // 2 + j * sw + k % kw).expand(hn, wn, kh * kw)
    return rows, cols


def frame(x4, args, pad_value=None, ext_value=None):
    """The padded, then ceil-extended frame of a (b, c, h, w) tensor."""
    pad, mode, value, ext_h, ext_w, ev = args[7:13]
    value = value if pad_value is None else pad_value
    ev = ev if ext_value is None else ext_value
    if pad:
        if mode in ("constant", "zeros"):
            x4 = F.pad(x4, (pad,) * 4, value=float(value))
        else:
            x4 = F.pad(x4, (pad,) * 4, mode=mode)
    if ext_h or ext_w:
        x4 = F.pad(x4, (0, ext_w, 0, ext_h), value=float(ev))
    return x4


def gather(x, args, pad_value=None, ext_value=None):
    """(lead, hn, wn, kh*kw): every window of the (lead, h, w) raster x, as a differentiable
    torch expression."""
    x4 = x.reshape((-1, 1) + tuple(x.shape[-2:]))
    rows, cols = window_index(args)
    g = frame(x4, args, pad_value, ext_value)[:, 0][:, rows, cols]
    return g.reshape(tuple(x.shape[:-2]) + tuple(g.shape[1:]))


def source_index(case):
    """(hn, wn, kh*kw) int64: the element of the h x w plane each window element reads; -1
    constant padding, -2 the ceil-mode extension."""
    idx = torch.arange(case.h * case.w, dtype=F64).view(1, case.h, case.w)
    return gather(idx, case.args, -1.0, -2.0)[0].long()


def pool_torch(x, args):
    """Hex pooling of the raster x by the operation's definition: NaN counts as -inf / +inf for
    max / min (torch.max / torch.min: the first extreme's index, where autograd sends the
    gradient; masked_fill passes none to a NaN); the average is the sum of the non-NaN values
    over their count, NaN for none."""
    g = gather(x, args)
    nan = g.isnan()
    if args[0] == "max":
        return torch.max(g.masked_fill(nan, float("-inf")), dim=-1).values
    if args[0] == "min":
        return torch.min(g.masked_fill(nan, float("inf")), dim=-1).values
    count = (~nan).to(g.dtype).sum(-1)
    total = torch.where(nan, torch.zeros_like(g), g).sum(-1)
    return torch.where(count == 0, torch.full_like(total, float("nan")), total / count)


# ---- inputs -----------------------------------------------------------------------------------
SALT = 3      # chosen so that the conditions of tests/test_pool_window_cases_cpu.py (b) hold


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr((SALT,) + key).encode()))


def _mixed_plane(case, cls, p, far):
    """One (h, w) plane of class cls; far: -inf for max and average, +inf for min."""
    gen = _gen(case.geom, "mixed", p)
    shape = (case.h, case.w)
    ints = torch.randint(0, 4, shape, generator=gen).to(F64)
    u = torch.rand(shape, generator=gen, dtype=F64)
    if cls == "ints":
        return ints
    if cls == "ints_nan":
        return ints.masked_fill(u < 0.05, float("nan"))
    if cls == "ints_nan_inf":
        return ints.masked_fill(u < 0.05, float("nan")).masked_fill(u > 0.98, far)
    if cls == "constant":
        return torch.full(shape, 2.0, dtype=F64)
    if cls == "all_nan":
        return torch.full(shape, float("nan"), dtype=F64)
    if cls == "signed_zeros":
        return torch.where(u < 0.5, -torch.zeros(shape, dtype=F64), torch.zeros(shape, dtype=F64))
    assert cls == "nan_first_inf"
    first = source_index(case)[..., 0].reshape(-1)
    plane = torch.full((case.h * case.w,), far, dtype=F64)
    plane[first[first >= 0]] = float("nan")
    return plane.view(shape)


@functools.lru_cache(maxsize=None)
def _inputs(geom, data, far):
    case = Case(geom, data, "max", F64, ())
    planes = case.lead[0] * case.lead[1]
    if data == "mixed":
        x = torch.stack([_mixed_plane(case, MIXED[p % 8], p, far) for p in range(planes)])
    elif data == "free":
        # every plane a draw without replacement from 3582 values that bf16 and f16 hold
        # exactly (+-m/128 * 2^e), none equal to a pad value: no two elements of a window tie
        vals = torch.tensor([s * m / 128 * 2.0 ** e for s in (1, -1) for e in range(-10, 4)
                             for m in range(128, 256)], dtype=F64)
        vals = vals[vals.abs() != 3.0]
        gen = _gen(geom, "free")
        x = torch.stack([vals[torch.randperm(len(vals), generator=gen)[: case.h * case.w]]
                         for _ in range(planes)]).view(planes, case.h, case.w)
        x[torch.rand(x.shape, generator=gen) < 0.05] = float("nan")
    else:
        n, cp = case.h * case.w, const_planes(case.h * case.w)
        x = torch.empty((planes, n), dtype=F64)
        for p in range(planes):
            v, nv = cp[p % len(cp)]
            x[p] = v
            x[p, torch.randperm(n, generator=_gen(geom, "const", p))[: n - nv]] = float("nan")
    return x.reshape(case.shape)


def inputs(case):
    """The case's seeded CPU input, float64 holding values that every one of the four types
    holds exactly.  The same tensor for every method and type of a (geometry, data) pair, but
    for the sign of the infinities (+inf for min)."""
    far = float("inf") if case.method == "min" else float("-inf")
    return _inputs(case.geom, case.data, far if case.data == "mixed" else 0.0).clone()


def grad_output(case):
    """Upstream gradient, whole numbers in -8..8: every partial sum of a max / min backward is
    then exact in float32 in any order (atomics, overlapping windows), survives the rounding of
    dx to a 16-bit type, and a gradient sent to the wrong one of two tied elements is an error
    of a whole number."""
    hn, wn = case.args[5:7]
    shape = case.lead if case.kind in ("reduce", "global") else case.lead + (hn, wn)
    return torch.randint(-8, 9, shape, generator=_gen(case.geom, "gy")).to(F64)


def plane_classes(case):
    planes = case.lead[0] * case.lead[1]
    return [MIXED[p % 8] for p in range(planes)] if case.data == "mixed" else [case.data] * planes


# ---- facts about a case's windows, computed from its inputs ------------------------------------
@functools.lru_cache(maxsize=None)
def _windows(geom, data, method):
    """(masked window values (planes, hn*wn, n), source index (hn*wn, n)) of a max / min case."""
    case = Case(geom, data, method, F64, ())
    g = gather(case.raster(inputs(case)), case.args)
    g = g.reshape((-1, g.shape[-3] * g.shape[-2], g.shape[-1]))
    g = g.masked_fill(g.isnan(), float("inf") if method == "min" else float("-inf"))
    return g, source_index(case).reshape(-1, g.shape[-1])


def tie_share(case, classes=INT_CLASSES):
    """Share of the windows (of the planes of the given classes) whose extreme occurs at two
    window positions or more that read different elements (an element and its own reflection
    are one place for the gradient)."""
    g, src = _windows(case.geom, case.data, case.method)
    keep = [p for p, c in enumerate(plane_classes(case)) if c in classes]
    g = g[keep]
    ext = g.min(-1, keepdim=True).values if case.method == "min" else g.max(-1, keepdim=True).values
    at = g == ext
    big = case.h * case.w
    lo = torch.where(at, src[None], torch.full_like(src, big)[None]).min(-1).values
    hi = torch.where(at, src[None], torch.full_like(src, -3)[None]).max(-1).values
    # (padding positions all read "the pad value": one place, which takes no gradient)
    return float((lo != hi).double().mean())


def tree_order_matters(case, threads=256):
    """Some window's first extreme is not the one the lowest thread of k_pool_large's tree
    holds: thread t walks elements t, t + 256, ..., so a tree that kept the lower thread's
    candidate on equal values (instead of the lower window index) would pick another element."""
    g, src = _windows(case.geom, case.data, case.method)
    ext = g.min(-1, keepdim=True).values if case.method == "min" else g.max(-1, keepdim=True).values
    idx = torch.arange(case.n).expand_as(g)
    big = 1 << 40
    first = torch.where(g == ext, idx, big).min(-1).values
    by_thread = torch.where(g == ext, (idx % threads) * 4096 + idx, big).min(-1).values % 4096
    s = src[None].expand(g.shape[0], -1, -1)
    return bool((s.gather(-1, first[..., None]) != s.gather(-1, by_thread[..., None])).any())


def pad_tie_first(case):
    """Some window's first element is constant padding whose value equals the extreme of the
    window's interior elements (it then gets the gradient, and drops it)."""
    if case.method == "average" or case.data != "mixed" or case.args[7] == 0 \
            or case.args[8] != "constant":
        return False
    g, src = _windows(case.geom, case.data, case.method)
    inner = g.masked_fill((src < 0)[None], float("inf") if case.method == "min" else float("-inf"))
    ext = inner.min(-1).values if case.method == "min" else inner.max(-1).values
    hit = (src[:, 0] == -1)[None] & (ext == float(case.args[9])) & (g[..., 0] == ext)
    return bool(hit.any())


def nan_first_far(case):
    """Some window of the input is [NaN, then only the far infinity (or NaN)]."""
    if case.method == "average" or case.data != "mixed":
        return False
    far = float("inf") if case.method == "min" else float("-inf")
    x = case.raster(inputs(case))
    raw = gather(x, case.args).reshape(-1, case.n)
    return bool((raw[:, 0].isnan() & ((raw[:, 1:] == far) | raw[:, 1:].isnan()).all(-1)
                 & (raw[:, 1:] == far).any(-1)).any())


def _reached(case, code):
    return bool((source_index(case) == code).any())


def _overlap(case):
    _, kh, kw, sh, sw, hn, wn = case.args[:7]
    return (sh < kh and hn > 1) or (sw < kw and wn > 1)


def _has(cls):
    return lambda c, r: c.data == "mixed" and cls in plane_classes(c)


def _at(route, pred):
    return lambda c, r: r == route and pred(c, r)


def _frame(mode):
    return lambda c, r: c.kind == "pool" and c.args[7] > 0 and c.args[8] == mode


# ---- regions: predicates on (case, route) ------------------------------------------------------
REGIONS = {"small_n511": lambda c, r: r == SMALL and c.n == 511}
for _n in (512, 513, 527, 576, 600):
    REGIONS[f"large_n{_n}"] = (lambda n: lambda c, r: r == LARGE and c.n == n)(_n)
REGIONS.update({
    # a 1 x n window of max_pooling / min_pooling / average_pooling on the large kernels
    "large_row": lambda c, r: r == LARGE and c.kind == "reduce",
    # the large kernels through HexPool2d: frame_src's -1 / -2 branches and the folds
    "large_const_pad": _at(LARGE, lambda c, r: _frame("constant")(c, r) and c.args[9] != 0
                           and _reached(c, -1)),
    "large_reflect": _at(LARGE, _frame("reflect")),
    "large_replicate": _at(LARGE, _frame("replicate")),
    "large_circular": _at(LARGE, _frame("circular")),
    "large_ext_zero": _at(LARGE, lambda c, r: _reached(c, -2) and c.args[12] == 0.0),
    "large_ext_nan": _at(LARGE, lambda c, r: _reached(c, -2) and c.args[12] != c.args[12]),
    # stride below kernel: several windows add into one dx element
    "small_overlap": _at(SMALL, lambda c, r: _overlap(c)),
    "large_overlap": _at(LARGE, lambda c, r: _overlap(c)),
})
DATA_REGIONS = {
    "tied_ints": lambda c, r: _has("ints")(c, r) and _has("ints_nan")(c, r)
    and _has("ints_nan_inf")(c, r),
    "constant_plane": _has("constant"),
    "all_nan_plane": _has("all_nan"),
    "signed_zeros": _has("signed_zeros"),
    "nan_first_inf": lambda c, r: _has("nan_first_inf")(c, r) and nan_first_far(c),
    "pad_tie_first": lambda c, r: pad_tie_first(c),
    # the controls: distinct values, no window with two equal extremes
    "tie_free": lambda c, r: c.data == "free",
    # constant planes with known counts (the 16-bit count arithmetic of the average)
    "const_counts": lambda c, r: c.data == "const" and c.method == "average",
}
for _name, _pred in DATA_REGIONS.items():
    for _route, _tag in ((SMALL, "small"), (LARGE, "large")):
        REGIONS[f"{_tag}_{_name}"] = _at(_route, _pred)

# what each region claims: (methods, dtypes); every (region, method, dtype) needs a case
EXTREMES = ("max", "min")
CLAIMS = {name: (METHODS, DTYPES) for name in REGIONS}
for _tag in ("small", "large"):
    CLAIMS[f"{_tag}_nan_first_inf"] = (EXTREMES, DTYPES)
    CLAIMS[f"{_tag}_pad_tie_first"] = (EXTREMES, DTYPES)
    CLAIMS[f"{_tag}_const_counts"] = (("average",), DTYPES)
# regions whose integer planes must be tied (share of windows with a repeated extreme >= 1/2)
TIED = ("small_tied_ints", "large_tied_ints")

# ---- the table --------------------------------------------------------------------------------
_GEOM_REGIONS = {
    "reduce511": ["small_n511"],
    "adaptive3_60x77": [],
    "pool3s2_const3": ["small_overlap"],
    "pool3s2_const0": ["small_overlap"],
    "pool3x2s2_reflect_ceil": ["small_overlap"],
    "reduce512": ["large_n512", "large_row"],
    "reduce513": ["large_n513", "large_row"],
    "global16x32": ["large_n512"],
    "global17x31": ["large_n527"],
    "adaptive2_48x60": ["large_n576"],
    "pool23_reflect_ceil": ["large_reflect", "large_ext_zero"],
    "pool23_const3_ceil_nocip": ["large_const_pad", "large_ext_nan"],
    "pool23_const0": [],
    "pool23_replicate": ["large_replicate"],
    "pool23_circular": ["large_circular"],
    "pool20x30_s7x25_reflect": ["large_n600", "large_overlap", "large_reflect"],
}
_SMALL_GEOMS = ("reduce511", "adaptive3_60x77", "pool3s2_const3", "pool3s2_const0",
                "pool3x2s2_reflect_ceil")
_PAD_TIE = {"pool3s2_const3": ("max",), "pool3s2_const0": ("min",),
            "pool23_const3_ceil_nocip": ("max",), "pool23_const0": ("min",)}
_MIXED_REGIONS = ("tied_ints", "constant_plane", "all_nan_plane", "signed_zeros")

CASES = []
for _geom, _regions in _GEOM_REGIONS.items():
    # (the data regions carry the route in their names; the CPU test holds them to the query)
    _tag = "small" if _geom in _SMALL_GEOMS else "large"
    for _method in METHODS:
        for _dt in DTYPES:
            _r = list(_regions) + [f"{_tag}_{d}" for d in _MIXED_REGIONS]
            if _method in EXTREMES:
                _r.append(f"{_tag}_nan_first_inf")
            if _method in _PAD_TIE.get(_geom, ()):
                _r.append(f"{_tag}_pad_tie_first")
            CASES.append(Case(_geom, "mixed", _method, _dt, _r))
            if _geom in FREE_GEOMS:
                CASES.append(Case(_geom, "free", _method, _dt, list(_regions) + [f"{_tag}_tie_free"]))
            if _geom in CONST_GEOMS and _method == "average":
                CASES.append(Case(_geom, "const", _method, _dt, list(_regions) + [f"{_tag}_const_counts"]))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names are unique"
