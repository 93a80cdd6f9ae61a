"""The case table of the resamplers' plane loops, shared by tests/test_gpu_resample_planes.py
(which runs it against the fp64 oracle, the general kernels and single-plane calls) and
tests/test_resample_plane_cases_cpu.py (which checks without a device, from the library's own plan
query hg_resample_plan, that every case lies in the regions it is filed under, that every region
has a case for every kernel instantiation it applies to, and pins every case's plan).

Every resampler walks a chunk of `pc` planes per work unit with the unit's lattice records kept
in registers:
  k_tri_up (tri_up.hip) and k_hexresize_down (hexresize_down.hip): one wave per (window, band,
      chunk), the input rows of PDP planes in flight, counted s_waitcnt values that differ between
      the first PDP planes and the steady state, a prologue and prefetches addressed past the
      chunk's last plane, np = min(pc, planes - p0) planes in the last chunk;
  k_resample_lds / _direct / _nearest (resample.hip) and k_resample_bwd (resample_bwd.hip): one
      workgroup per (tile, chunk);
  k_r2h_stream / k_h2r_stream (resample_stream.hip), k_r2h_down (resample_down.hip): pc = 1, one
      workgroup per (plane, band, 4 windows), XCD-swizzled.
At the shapes the other parity files use, pc is 1 (or 2-3 at 4K in one dtype), so the loops over
planes ran one trip.  Here the spatial sizes are tiny (an 8 x 12 input where the kernel allows)
and the plane counts and the A/B switches HYGRID_TU_CHUNKS / HYGRID_TSK_CHUNKS (plane chunks per
tile), HYGRID_TU_GRID / HYGRID_TSK_GRID (one wave per unit or the resident-wave rule) and
HYGRID_TSK_UPW choose pc.

The table holds no pc / chunk / unit numbers: a region is a predicate on the plan the library
reports (REGIONS), evaluated under the case's environment, so a change of a launch rule fails the
CPU test instead of silently un-covering a loop.  The numbers are pinned once, in PINNED of the
CPU test.

Not a conftest and not a test: imported like tests/conv_generic_cases.py."""
import contextlib
import os

import torch

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U8, I16, I32 = torch.uint8, torch.int16, torch.int32
NEAREST, LINEAR = 0, 1                                      # enum hg_interp
R2H, H2R, RESIZE = 0, 1, 2                                  # enum hg_op
GENERAL, NEAR_K, STREAM, DOWN, UP, BACKWARD = range(6)      # enum hg_kernel
OP_NAME = {R2H: "rect_to_hex", H2R: "hex_to_rect", RESIZE: "hexresize"}
DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32", F64: "f64", U8: "u8", I16: "i16", I32: "i32"}
TU_CPP, HD_CPP = 24, 48             # tri_up.hip / hexresize_down.hip: planes per unit in grid mode


@contextlib.contextmanager
def environ(env):
    """The HYGRID_* switches of a case, set for the duration (the library reads them per call)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Case:
    """One call: `planes` rasters (h, w) of in_dt -> (h1, w1) of out_dt through op (R2H / H2R /
    RESIZE) with interp, under the switches env; align: the source's offset in bytes from a
    16-byte boundary (4: a sliced view, which k_hexresize_down loads in 4-byte pieces);
    backward: the call is hg_resample_backward (in_dt its accumulator).  family: the kernel the
    case is about ("tri_up", "hexdown", "general", "nearest", "backward", "r2h_stream",
    "h2r_stream", "r2h_down"); regions: the REGIONS entries it is filed under."""

    def __init__(self, family, regions, op, planes, shape, in_dt, out_dt=None, interp=LINEAR,
                 env=None, align=0, backward=False, tag=""):
        self.family, self.regions = family, tuple(regions)
        self.op, self.planes = op, planes
        self.h, self.w, self.h1, self.w1 = shape
        self.in_dt, self.out_dt = in_dt, in_dt if out_dt is None else out_dt
        self.interp, self.env, self.align, self.backward = interp, dict(env or {}), align, backward
        sw = "".join(f",{k[7:]}={v}" for k, v in sorted(self.env.items()))
        self.name = (f"{family}{tag}-{OP_NAME[op]}-{self.h}x{self.w}to{self.h1}x{self.w1}-"
                     f"{DT_NAME[self.in_dt]}_{DT_NAME[self.out_dt]}-"
                     f"{'lin' if interp else 'near'}-p{planes}{sw}{',a%d' % align if align else ''}")

    def __repr__(self):
        return self.name

    def plan(self, env=None):
        """The library's plan for the call (hg_resample_plan; nothing is launched), under the
        case's switches (or env)."""
        from HyGrid import _abi
        with environ(self.env if env is None else env):
            return _abi.resample_plan(self.op, _abi.dtype_code(self.in_dt),
                                      _abi.dtype_code(self.out_dt), self.planes, self.h, self.w,
                                      self.h1, self.w1, self.interp, self.align, self.backward)

    def inst(self, P):
        """The kernel instantiation the plan selects, as the dispatchers template it."""
        io = (DT_NAME[self.in_dt], DT_NAME[self.out_dt])
        if self.family == "tri_up":
            esz = torch.empty((), dtype=self.in_dt).element_size()
            io = io if self.interp else (f"{esz}B",)
            return ("k_tri_up", "linear" if self.interp else "nearest") + io + \
                   ("K1" if P["K"] == 1 else "Knat",)
        if self.family == "hexdown":
            return ("k_hexresize_down",) + io + (f"DB{P['DB']}", "K4" if P["K"] == 4 else "KP",
                                                 "SEP" if P["SEP"] else "shared")
        return (self.family,)


# ---- regions: predicates on (case, plan) ------------------------------------------------------
def _chunked(c, P):
    return c.family in ("tri_up", "hexdown") and P["kernel"] == (UP if c.family == "tri_up" else DOWN)


def _last(c, P):
    """planes in the last chunk"""
    return c.planes - (P["chunks"] - 1) * P["pc"]


def _tail(r):
    # the steady-state wait, at least two trips of the loop unrolled by PDP, a tail of r planes
    return lambda c, P: _chunked(c, P) and P["pc"] >= 2 * P["pdp"] and P["pc"] % P["pdp"] == r \
        and r < P["pdp"]


def _cpp(c):
    return TU_CPP if c.family == "tri_up" else HD_CPP


def _sw(c, name):
    return c.env.get(("HYGRID_TU_" if c.family == "tri_up" else "HYGRID_TSK_") + name)


REGIONS = {
    # one plane per unit: the prologue alone, every prefetch past the chunk
    "np=1": lambda c, P: _chunked(c, P) and P["pc"] == 1,
    # the first-planes waits only
    "2<=np<=PDP": lambda c, P: _chunked(c, P) and 2 <= P["pc"] <= P["pdp"],
    "tail=0": _tail(0), "tail=1": _tail(1), "tail=2": _tail(2),
    # np = min(pc, planes - p0) < pc in the last chunk
    "last_chunk=1": lambda c, P: _chunked(c, P) and P["pc"] >= 3 and _last(c, P) == 1,
    "last_chunk=pc-1": lambda c, P: _chunked(c, P) and P["pc"] >= 3 and _last(c, P) == P["pc"] - 1,
    # one wave per unit, pc from the CHUNKS switch
    "grid": lambda c, P: _chunked(c, P) and c.planes >= 2 * _cpp(c) and P["wave_per_unit"] == 1
    and P["pc"] > P["pdp"] and _sw(c, "CHUNKS") and _sw(c, "GRID") is None,
    # the old rule forced on a call grid mode would take
    "grid=0": lambda c, P: _chunked(c, P) and c.planes >= 2 * _cpp(c) and _sw(c, "GRID") == "0"
    and P["wave_per_unit"] == 0 and P["pc"] > P["pdp"],
    # grid mode forced on a call with too few planes for it
    "grid=1": lambda c, P: c.family == "tri_up" and _chunked(c, P) and c.planes < 2 * TU_CPP
    and _sw(c, "GRID") == "1" and P["wave_per_unit"] == 1 and P["pc"] > P["pdp"],
    # a wave strides over at least two units
    "two_units_per_wave": lambda c, P: _chunked(c, P) and P["wave_per_unit"] == 0
    and P["units"] > P["launched"],
    # HYGRID_TSK_UPW read by the launch
    "upw": lambda c, P: c.family == "hexdown" and _chunked(c, P) and _sw(c, "UPW") == "2",
    # the workgroup loops over planes of the general kernels and the backward
    "wg_pc=2": lambda c, P: not _chunked(c, P) and P["pc"] == 2 and c.planes % 2 == 1,
    "wg_pc=3": lambda c, P: not _chunked(c, P) and P["pc"] == 3 and c.planes % 3 != 0,
    "direct": lambda c, P: P["kernel"] == GENERAL and P["lds"] == 0 and P["pc"] >= 2,
    # one workgroup per plane, a grid that is no multiple of the 8 XCDs
    "blocks%8": lambda c, P: P["kernel"] in (STREAM, DOWN) and P["pc"] == 1
    and P["launched"] % 8 != 0 and P["launched"] > 8 and c.planes >= 3,
}
# the regions every instantiation of a chunked kernel must reach, by its prefetch depth
CHUNK_REGIONS = {
    1: ("np=1", "tail=0", "last_chunk=1", "last_chunk=pc-1"),
    2: ("np=1", "2<=np<=PDP", "tail=0", "tail=1", "last_chunk=1", "last_chunk=pc-1"),
    3: ("np=1", "2<=np<=PDP", "tail=0", "tail=1", "tail=2", "last_chunk=1", "last_chunk=pc-1"),
}
GRID_REGIONS = {"tri_up": ("grid", "grid=0", "grid=1"), "hexdown": ("grid", "grid=0")}

# (planes, chunks switch or None, regions) per prefetch depth: pc = ceil(planes / chunks)
PLANE_CONFIGS = {
    1: [(3, None, ["np=1"]), (5, 2, ["tail=0", "last_chunk=pc-1"]), (10, 4, ["tail=0", "last_chunk=1"])],
    2: [(3, None, ["np=1"]), (3, 2, ["2<=np<=PDP"]), (7, 2, ["tail=0", "last_chunk=pc-1"]),
        (9, 2, ["tail=1", "last_chunk=pc-1"]), (13, 4, ["tail=0", "last_chunk=1"])],
    3: [(3, None, ["np=1"]), (5, 2, ["2<=np<=PDP"]), (31, 6, ["tail=0", "last_chunk=1"]),
        (13, 2, ["tail=1", "last_chunk=pc-1"]), (15, 2, ["tail=2", "last_chunk=pc-1"])],
}

CASES = []


def _chunk_cases(family, op, shape, in_dt, out_dt, interp, pdp, env=None, align=0, grid=True):
    sw = "HYGRID_TU_" if family == "tri_up" else "HYGRID_TSK_"
    base = dict(env or {})
    for planes, chunks, regions in PLANE_CONFIGS[pdp]:
        e = dict(base, **({sw + "CHUNKS": str(chunks)} if chunks else {}))
        CASES.append(Case(family, regions, op, planes, shape, in_dt, out_dt, interp, e, align))
    if not grid:
        return
    n = 2 * (TU_CPP if family == "tri_up" else HD_CPP) + 2      # 50 / 98 planes, pc 10 / 14
    e = dict(base, **{sw + "CHUNKS": str(n // 10 if family == "tri_up" else 7)})
    CASES.append(Case(family, ["grid"], op, n, shape, in_dt, out_dt, interp, e, align))
    CASES.append(Case(family, ["grid=0"], op, n, shape, in_dt, out_dt, interp,
                      dict(e, **{sw + "GRID": "0"}), align))
    if family == "tri_up":
        CASES.append(Case(family, ["grid=1"], op, 9, shape, in_dt, out_dt, interp,
                          dict(base, HYGRID_TU_CHUNKS="2", HYGRID_TU_GRID="1"), align))


# ---- k_tri_up: PDP 3; natural K (8 / 4 / 2 columns per lane for 1 / 2 / 4-byte inputs) and K = 1
TU_SHAPES = {"Knat": (8, 12, 16, 24), "K1": (8, 12, 16, 23)}
_n = 0
for _shape in TU_SHAPES.values():
    for _i in (BF16, F16, F32):
        for _o in (BF16, F16, F32):
            _chunk_cases("tri_up", (H2R, RESIZE)[_n % 2], _shape, _i, _o, LINEAR, 3)
            _n += 1
    for _e in (U8, I16, I32):
        _chunk_cases("tri_up", (H2R, RESIZE)[_n % 2], _shape, _e, _e, NEAREST, 3)
        _n += 1

# ---- k_hexresize_down: {bf16, f16} in x {bf16, f16, f32} out x (DB, K, SEP) ---------------------
# DB 16 (PDP 1): ~2x and stronger column ratios from a 16-byte-aligned source; DB 4 (PDP 2): the
# same source 4 bytes off a 16-byte boundary, or an up-lattice with HYGRID_UP=0.  K = 4 while a
# window holds more than 64 P output columns, else K = P (P = 1 / 2 for DB 16 / 4).  SEP: the
# rows of a 2-row band share no input rows (>= ~3x row downsampling).
HD_GEOM = {   # (DB, K4?, SEP) -> (op, shape, align, env)
    (16, True, False): (RESIZE, (17, 32, 9, 16), 0, {}),
    (16, False, False): (RESIZE, (17, 256, 9, 32), 0, {}),
    (16, True, True): (H2R, (64, 32, 8, 16), 0, {}),
    (16, False, True): (RESIZE, (64, 256, 8, 32), 0, {}),
    (4, True, False): (H2R, (8, 12, 16, 24), 0, {"HYGRID_UP": "0"}),
    (4, False, False): (RESIZE, (17, 32, 9, 16), 4, {}),
    (4, True, True): (RESIZE, (64, 16, 8, 24), 4, {}),
    (4, False, True): (H2R, (64, 32, 8, 16), 4, {}),
}
for (_db, _k4, _sep), (_op, _shape, _al, _env) in HD_GEOM.items():
    for _i in (BF16, F16):
        for _o in (BF16, F16, F32):
            _chunk_cases("hexdown", _op, _shape, _i, _o, LINEAR, 1 if _db == 16 else 2, _env, _al)
# the up-lattice on the other op, and a K = 1 up-lattice (odd w1)
_chunk_cases("hexdown", RESIZE, (8, 12, 16, 24), BF16, BF16, LINEAR, 2, {"HYGRID_UP": "0"}, grid=False)
_chunk_cases("hexdown", H2R, (8, 12, 16, 23), F16, F32, LINEAR, 2, {"HYGRID_UP": "0"}, grid=False)
CASES.append(Case("hexdown", ["upw", "np=1"], RESIZE, 3, (16, 32, 8, 16), F16, F16, LINEAR,
                  {"HYGRID_TSK_UPW": "2"}))

# ---- a wave walking two units without grid mode (more units than resident waves) ---------------
CASES.append(Case("tri_up", ["two_units_per_wave"], H2R, 3, (130, 512, 260, 1023), BF16, BF16, LINEAR))
# ('nearest' bands are 4 rows: 1040 tiles, one chunk per plane up to 4)
CASES.append(Case("tri_up", ["two_units_per_wave"], RESIZE, 4, (130, 512, 260, 1023), U8, U8, NEAREST))
# (260 tiles of 256 columns x 3 planes stay below the resident waves; 32-column windows, the
# A/B switch HYGRID_TSK_NOUT, make 2080)
CASES.append(Case("hexdown", ["two_units_per_wave"], RESIZE, 3, (520, 1024, 260, 512), F16, F16, LINEAR,
                  {"HYGRID_TSK_NOUT": "32"}))

# ---- the general kernels and the backward: thousands of tiny planes, one tile ------------------
for _planes, _region in ((4099, "wg_pc=2"), (8200, "wg_pc=3")):
    for _op in (R2H, H2R, RESIZE):
        CASES.append(Case("general", [_region], _op, _planes, (8, 12, 5, 7), F32, F32, LINEAR))
        CASES.append(Case("nearest", [_region], _op, _planes, (8, 12, 5, 7), U8, U8, NEAREST))
        # k_resample_direct: a ~3x downsampling 16 x 128 tile's footprint bound (the bound is of
        # the lattice steps, not of this one small tile) exceeds the LDS budget
        CASES.append(Case("general", [_region, "direct"], _op, _planes, (12, 18, 5, 7), F32, F32,
                          LINEAR, tag="_direct"))
        for _dt in (F32, F64):
            for _interp in (LINEAR, NEAREST):
                CASES.append(Case("backward", [_region], _op, _planes, (8, 12, 5, 7), _dt, _dt,
                                  _interp, backward=True))
CASES.append(Case("general", ["wg_pc=2"], RESIZE, 4099, (8, 12, 5, 7), F32, BF16, LINEAR))
CASES.append(Case("general", ["wg_pc=3"], H2R, 8200, (8, 12, 5, 7), F16, F64, LINEAR))

# ---- one workgroup per (plane, band, 4 windows): grids that are no multiple of 8 ---------------
for _i, _o in ((F32, F32), (BF16, BF16), (F16, F32), (F32, F16)):
    CASES.append(Case("r2h_stream", ["blocks%8"], R2H, 5, (33, 260, 33, 260), _i, _o, LINEAR))
    CASES.append(Case("h2r_stream", ["blocks%8"], H2R, 7, (33, 260, 33, 260), _i, _o, LINEAR))
CASES.append(Case("r2h_stream", ["blocks%8"], R2H, 11, (90, 512, 91, 512), BF16, F32, LINEAR))
for _i, _o, _interp in ((U8, U8, NEAREST), (I16, I16, NEAREST), (BF16, BF16, LINEAR),
                        (F16, F32, LINEAR), (BF16, F16, LINEAR)):
    CASES.append(Case("r2h_down", ["blocks%8"], R2H, 11, (65, 130, 32, 65), _i, _o, _interp))
    CASES.append(Case("r2h_down", ["blocks%8"], R2H, 13, (17, 40, 8, 20), _i, _o, _interp))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names are unique"

# the kernel a family's cases must be routed to (hg_kernel)
FAMILY_KERNEL = {"tri_up": UP, "hexdown": DOWN, "general": GENERAL, "nearest": NEAR_K,
                 "backward": BACKWARD, "r2h_stream": STREAM, "h2r_stream": STREAM, "r2h_down": DOWN}
# the switch that sends a family's call to the general kernels (bit-identity reference)
GENERAL_SWITCH = {"tri_up": {"HYGRID_DOWN": "0"}, "hexdown": {"HYGRID_DOWN": "0"},
                  "r2h_down": {"HYGRID_DOWN": "0"},
                  # (HYGRID_STREAM=0 alone: a same-size hex -> rect then runs k_tri_up)
                  "r2h_stream": {"HYGRID_STREAM": "0", "HYGRID_DOWN": "0"},
                  "h2r_stream": {"HYGRID_STREAM": "0", "HYGRID_DOWN": "0"}}
# one ragged-chunk case per chunked kernel whose output is placed between guard bands
PLACED = [c.name for c in CASES
          if (c.family, c.planes, c.in_dt, c.out_dt) in (("tri_up", 13, BF16, F32), ("tri_up", 13, U8, U8),
                                                        ("hexdown", 9, F16, BF16), ("hexdown", 5, BF16, F32))]


def sample_planes(c, P):
    """Planes compared with single-plane calls: the first and last, both sides of the first and
    the last chunk boundary, the ragged chunk's first plane, and a stride through the rest."""
    pc, n = P["pc"], c.planes
    last0 = (P["chunks"] - 1) * pc
    s = {0, n - 1, pc - 1, min(pc, n - 1), max(last0 - 1, 0), last0}
    s.update(range(0, n, max(1, n // 5)))
    return sorted(p for p in s if 0 <= p < n)


def inputs(c):
    """Seeded CPU source (planes, h, w) of in_dt (the backward: the upstream gradient (planes, h1,
    w1)), different in every plane; a view c.align bytes past a 16-byte boundary."""
    import zlib
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    shape = (c.planes, c.h1, c.w1) if c.backward else (c.planes, c.h, c.w)
    if c.in_dt == U8:
        return torch.randint(0, 256, shape, generator=gen, dtype=U8)
    if c.in_dt in (I16, I32):
        top = 2 ** 15 if c.in_dt == I16 else 2 ** 31
        return torch.randint(-top, top - 1, shape, generator=gen, dtype=torch.int64).to(c.in_dt)
    return (torch.rand(shape, generator=gen, dtype=F64) - 0.25).to(c.in_dt)
