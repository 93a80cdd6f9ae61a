"""Which compile-time loop variant of the fused streaming kernels each wave runs, mirrored on
the CPU, and the shape lists the GPU parity tests of those kernels share.

k_fused4 (csrc/fused4.hip, layout mode 6) and k_fused (csrc/fused_kernel.h: MD 0 the fused
pipeline, MD 1 the HexConv2d stream, MD 2 the round trip) are families of loops; a wave (one
band x one window) picks its loop at run time from the lattice: a column class cd, a row class
rc, the walking direction and, on a partial last band, a hand-unrolled tail of n % 6 steps.
census(md, H, W) restates those selection rules in NumPy from the library's own layout numbers
(_abi.fused_layout) and the fp64 lattice formulas of csrc/lattice.h, so that
tests/test_fused_variants_cpu.py can pin that the shapes below reach every variant, and a failing
GPU comparison can name the loop that produced the first bad element.

This module is a MIRROR of the kernels, not a part of them.  If it drifts from the kernels (a
rule restated wrongly, a kernel changed without it), the coverage it promises silently drops,
but no parity test fails falsely through its class or tail records: those only choose shapes and
label failure messages.  (The one rule a GPU assertion depends on is the band direction, which
test_gpu_fused4.py uses to tell bit-identical rows from reordered sums.)

Not a conftest and not a test: imported like tests/pool_cases.py."""
from collections import namedtuple

import numpy as np

MODES = (6, 0, 1, 2)
# the (cd, rc) loops compiled besides the generic one (fused4.hip:434-438,
# fused_kernel.h:898-903); MD 1 has the inner and the generic loop (fused_kernel.h:890-896)
CLASS_LOOPS = ("cd1rc1", "cd1rc2", "cd2rc1", "cd2rc2", "generic")
CONV_LOOPS = ("inner", "generic")
BUCKETS = ("n<6", "6<=n<12", "n>=12")
FILLS = ("full", "ragged", "empty")
# C, O, groups the dispatchers instantiate (fused.hip fused_channels, fused_conv.hip
# fconv_channels)
CHANNELS = ((3, 3, 1), (3, 3, 3), (1, 1, 1))
GROUP_WAVES = 4        # windows (waves) per workgroup: F4_GW, FU_GW
STEP_BLOCK = 6         # steps per unrolled block: ring slots x row parities

Wave = namedtuple("Wave", "md band win n direction cd rc loop tail bucket fill")


def layout(md):
    """(band rows, owned columns, halo columns, window width) of mode md, from the library."""
    from HyGrid import _abi
    rows, own, halo = _abi.fused_layout(md)
    return rows, own, halo, own + 2 * halo


def width_multiple(md):
    """Widths the kernel takes: fused4_try wants w % 4 == 0, the two-column kernel even widths."""
    return 4 if md == 6 else 2


def loops(md):
    return CONV_LOOPS if md == 1 else CLASS_LOOPS


def directions(md):
    """MD 0 always walks down (REVOK, fused_kernel.h:320); the others walk odd full bands up."""
    return ("down",) if md == 0 else ("down", "up")


def op_of(off, padding=1):
    """The OP template parameter: the tap column class (even_odd_offset + padding) & 1."""
    return (off + padding) & 1


# ---- the r2h lattice, csrc/lattice.h in fp64 -------------------------------------------------
def _axis(start, stop, n):
    """make_axis + axis_at (lattice.h:23-43): numpy.linspace(start, stop, n) bit for bit."""
    k = np.arange(n, dtype=np.float64)
    if n > 1:
        delta = stop - start
        div = float(n - 1)
        step = delta / div
        y = (k / div) * delta if step == 0.0 else k * step
        y = y + start
        y[-1] = stop
        return y
    return k * (stop - start) + start


def r2h_rows(h, h1):
    """i_n, i_f of every hex row (lattice.h:57, :83-87; the fused kernels' row table)."""
    i_ = _axis(-(float(h) / 2.0), float(h) / 2.0, h1) + float(h - 1) * 0.5
    i_n = np.trunc(i_).astype(np.int64)
    return i_n, i_ - i_n.astype(np.float32).astype(np.float64)


def r2h_cols(w, w1):
    """j_n, j_f of every hex column (lattice.h:58, :84-88)."""
    j_ = _axis(-(float(w) / 2.0 + 0.5), float(w) / 2.0 + 0.5, w1) + float(w - 1) * 0.5
    j_n = np.trunc(j_).astype(np.int64)
    return j_n, j_ - j_n.astype(np.float32).astype(np.float64)


def _row_terms(H):
    """Per u row r of a same-size lattice: does its table entry have a non-zero a (rect row
    r - 1) / c (rect row r + 1) term?  fused4.hip:103-116, fused_kernel.h:354-369."""
    i_n, i_f = r2h_rows(H, H)
    r = np.arange(H)
    w0 = np.where((i_n >= 0) & (i_n < H), (1.0 - i_f).astype(np.float32), np.float32(0))
    w1 = np.where((i_n + 1 >= 0) & (i_n + 1 < H), i_f.astype(np.float32), np.float32(0))
    has_a = (i_n == r - 1) & (w0 != 0)
    has_c = (i_n == r) & (w1 != 0)
    return has_a, has_c


def _col_terms(W):
    """Per hex column q: a non-zero left (rect column q - 1) / right (q + 1) r2h weight?
    fused4.hip:134-155, fused_kernel.h:390-406 (the 0.75 fold keeps zeros zero)."""
    j_n, j_f = r2h_cols(W, W)
    q = np.arange(W)
    left = np.zeros(W, np.float32)
    right = np.zeros(W, np.float32)
    for kk, acc in ((-1, left), (1, right)):
        in_w = (q + kk >= 0) & (q + kk < W)
        acc += np.where((kk == j_n - q) & in_w, (1.0 - j_f).astype(np.float32), np.float32(0))
        acc += np.where((kk == j_n + 1 - q) & in_w, j_f.astype(np.float32), np.float32(0))
    return left != 0, right != 0


def _klass(any_first, any_second):
    """rc = !any_c ? 1 : (!any_a ? 2 : 0) (fused4.hip:129, fused_kernel.h:385) and
    cd = !any_r ? 1 : (!any_l ? 2 : 0) (fused4.hip:160, fused_kernel.h:516)."""
    return 1 if not any_second else (2 if not any_first else 0)


def bucket_of(n):
    """k_fused walks pairs of 6-step blocks, then a single block, then the tail
    (fused_kernel.h:875-884)."""
    return BUCKETS[0] if n < STEP_BLOCK else (BUCKETS[1] if n < 2 * STEP_BLOCK else BUCKETS[2])


def census(md, H, W):
    """One Wave record per (band, window) wave of mode md (6: k_fused4; 0, 1, 2: k_fused) on a
    same-size H x W call: band and window index, n rows in the band, direction, cd, rc, the
    effective loop, the tail n % 6 (None on an upward band, which is always whole), the block
    bucket and the window fill."""
    assert md in MODES
    rows, own, halo, width = layout(md)
    nband = -(-H // rows)
    nwin = -(-W // own)
    ngrp = -(-nwin // GROUP_WAVES)
    uin = md == 1                                   # u rows are input rows: no r2h classes
    if not uin:
        has_a, has_c = _row_terms(H)
        has_l, has_r = _col_terms(W)
    out = []
    for band in range(nband):
        s0 = band * rows
        s1 = min(s0 + rows, H)
        n = s1 - s0
        # fused4.hip:99 (F4_REV), fused_kernel.h:320, :351 (REVOK: MD 1 and MD 2 only)
        up = md != 0 and band % 2 == 1 and n == rows
        rc = 0
        if not uin:
            # table rows s0 - 1 .. s0 + rows inside the raster (fused4.hip:103-130,
            # fused_kernel.h:354-386)
            lo, hi = max(s0 - 1, 0), min(s0 + rows + 1, H)
            rc = _klass(bool(has_a[lo:hi].any()), bool(has_c[lo:hi].any()))
        for win in range(ngrp * GROUP_WAVES):       # win >= nwin: runs, owns nothing
            w0 = win * own - halo
            lo, hi = max(w0, 0), min(w0 + width, W)
            if uin:
                # fused_kernel.h:412, :894: every table row and every lane's columns inside
                cd = 0
                inner = s0 >= 1 and s1 + 1 <= H and w0 >= 0 and w0 + width - 2 < W
                loop = "inner" if inner else "generic"
            else:
                # fused4.hip:156-160, fused_kernel.h:514-516 (a wave past the raster has no
                # weights at all: cd 1)
                cd = _klass(bool(has_l[lo:hi].any()), bool(has_r[lo:hi].any())) if lo < hi else 1
                loop = f"cd{cd}rc{rc}" if cd and rc else "generic"
            fill = "empty" if win >= nwin else ("full" if (win + 1) * own <= W else "ragged")
            out.append(Wave(md, band, win, n, "up" if up else "down", cd, rc, loop,
                            None if up else n % STEP_BLOCK, bucket_of(n), fill))
    return out


def up_rows(md, H):
    """Boolean per output row: inside a band that walks upwards."""
    rows = layout(md)[0]
    up = np.zeros(H, bool)
    for wv in census(md, H, width_multiple(md)):
        if wv.win == 0 and wv.direction == "up":
            up[wv.band * rows:wv.band * rows + wv.n] = True
    return up


def wave_at(md, H, W, r, q):
    """The census record of the wave that owns output (r, q)."""
    rows, own, _, _ = layout(md)
    for wv in census(md, H, W):
        if wv.band == r // rows and wv.win == q // own:
            return wv
    raise LookupError((md, H, W, r, q))


def describe_first_bad(md, bad):
    """For a failure message: the first True of bad (..., H, W) and the loop that made it."""
    bad = np.asarray(bad)
    if not bad.any():
        return ""
    H, W = bad.shape[-2:]
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    wv = wave_at(md, H, W, idx[-2], idx[-1])
    return (f"{int(bad.sum())} of {bad.size} bad; first at {idx}: md {md} band {wv.band} "
            f"(n {wv.n}, {wv.direction}, tail {wv.tail}, {wv.bucket}) window {wv.win} "
            f"({wv.fill}) loop {wv.loop} (cd {wv.cd}, rc {wv.rc})")


# ---- the shapes the GPU parity tests run -----------------------------------------------------
# New shapes are built from the layout numbers, so a retune of a band length or a window keeps
# the coverage (or fails tests/test_fused_variants_cpu.py): six bands and a 5- or 3-row tail put
# whole bands above, across and below the middle row in both directions; two windows, a ragged
# third and a fourth wave that owns nothing put windows left of, across and right of the middle
# column.
def _round_up(v, m):
    return -(-v // m) * m


def _wide(md):
    _, own, halo, _ = layout(md)
    return _round_up(2 * own + 2 * halo + 4, width_multiple(md))


def fused4_shapes():
    """(B, H, W) of test_gpu_fused4.py, each run at both offsets (bf16, C = O = 3)."""
    rows = layout(6)[0]
    old = [(1, 8, 12), (2, 48, 96), (1, 91, 248), (2, 100, 500), (1, 130, 964), (1, 44, 3840)]
    return old + [(1, 6 * rows + 5, _wide(6)), (1, 6 * rows + 3, _wide(6))]


def fused4_new_shapes():
    return fused4_shapes()[6:]


def md0_cases():
    """(B, C, H, W, off, groups) added to test_gpu_pipeline.py::test_fused_vs_oracle_fp32 (fp32
    in and out runs k_fused MD 0, not k_fused4): every class for each channel configuration and
    offset, every tail and block bucket for each offset."""
    rows, own, _, _ = layout(0)
    cases = []
    for off in (0, 1):
        for c, _, g in CHANNELS:
            cases.append((1, c, 6 * rows + 5, _wide(0), off, g))          # tail 5, n < 6
        # tails 1 .. 4; n = 7 and 10 run the single block before the tail
        for i, extra in enumerate((7, 2, 3, 10)):
            c, _, g = CHANNELS[(i + off) % 3]
            cases.append((2 if i == 0 else 1, c, rows + extra, own + 2 * (i + 1), off, g))
    return cases


def fconv_cases():
    """(B, C, O, groups, h, w) of test_gpu_fused_conv.py::test_fused_conv_fp32_vs_oracle, each
    run at both offsets with and without a bias."""
    rows = layout(1)[0]
    old = [(2, 3, 3, 1, 7, 8), (1, 3, 3, 1, 9, 10), (2, 3, 3, 1, 127, 242), (1, 3, 3, 3, 130, 250),
           (3, 1, 1, 1, 33, 122), (1, 3, 3, 1, 253, 360), (1, 1, 1, 1, 1, 2), (1, 3, 3, 3, 2, 4)]
    # the 5-step tail (3/3/1); the inner loop in both directions for 1/1/1 (the other two
    # configurations reach it at 253 x 360 and 130 x 250)
    return old + [(1, 3, 3, 1, 6 * rows + 5, _wide(1)), (2, 1, 1, 1, 6 * rows + 4, _wide(1))]


def fconv_new_cases():
    return fconv_cases()[8:]


def roundtrip_shapes():
    """(B, C, H, W) of test_gpu_roundtrip.py::test_roundtrip_fp32_vs_oracle (MD 2 has no conv:
    one instantiation, OP 0)."""
    return [(2, 3, 64, 130), (1, 1, 37, 250), (3, 2, 200, 96), (1, 3, 131, 246), (1, 1, 2, 4),
            (2, 3, 135, 968)]
