"""Case tables shared by tests/test_conv_transpose_cpu.py and tests/test_gpu_conv_transpose.py:
the shapes of the HexConvTranspose2d tests, the NumPy restatement of the layer from the kernel's
tap table, and the fp64 oracle reference (computed once per case, never modified)."""
import functools

import numpy as np

from oracle import oracle as O

R, S = 2, 2

# (hin, win, padding): the smallest layer; a small one; output widths 70 / 71, 130 / 131 and
# 258 / 259 (crossing one, two and four 64-column class tiles = 128-column workgroup tiles, and
# rows 33 / 34, 17 / 18: no multiple of 4); padding 2 with widths 64 / 65.
SHAPES = [(1, 2, 0), (5, 5, 1), (17, 35, 1), (17, 65, 1), (9, 129, 1), (3, 33, 2)]
# (in, out): partial K chunks (3, 100, 33, 1), partial M tiles (24, 70), the 16-channel threshold
CHANNELS = [(8, 16), (16, 16), (64, 32), (3, 64), (100, 24), (33, 70), (1, 16)]
BATCH2 = {(5, 5, 1), (17, 35, 1), (3, 33, 2)}           # shapes run with B = 2

# the guard-band case of every device-writing export of include/hygrid_layers.h
GUARD_CASES = {
    "hg_hexconv_transpose2d": "tests/test_gpu_conv_transpose.py::test_placement_inside_guard_arenas",
}


def valid_sizes(hin, win, p):
    """The four output sizes of a radius-2 stride-2 layer (the issue's closed form; the CPU
    test checks it against the out-shape rule)."""
    return [(h, w) for h in (2 * hin + 1 - 2 * p, 2 * hin + 2 - 2 * p)
            for w in (2 * win + 2 - 2 * p, 2 * win + 3 - 2 * p)]


def gpu_cases():
    """(B, cin, cout, hin, win, p, h, w, off): every shape x valid size x offset with the channel
    pairs dealt round-robin, then every channel pair x offset on (17, 35, 1) at its default size."""
    out, n = [], 0
    for shp in SHAPES:
        hin, win, p = shp
        for (h, w) in valid_sizes(hin, win, p):
            for off in (0, 1):
                ci, co = CHANNELS[n % len(CHANNELS)]
                n += 1
                out.append((2 if shp in BATCH2 else 1, ci, co, hin, win, p, h, w, off))
    for (ci, co) in CHANNELS:
        for off in (0, 1):
            c = (2, ci, co, 17, 35, 1, 34, 70, off)
            if c not in out:
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def data(case, x_dtype="float32"):
    """(x, kernel, bias) as float32 NumPy arrays (x rounded to x_dtype's values first) and the
    fp64 oracle's y - bias: hexconv2d_backward's d input of the adjoint conv."""
    import torch
    B, ci, co, hin, win, p, h, w, off = case
    g = torch.Generator().manual_seed(hin * 131 + win * 7 + ci + 3 * p + off + 1000 * h + w)
    x = (torch.rand((B, ci, hin, win), generator=g) - 0.5).to(getattr(torch, x_dtype)).float()
    k = ((torch.rand((ci, co, 1, 7), generator=g) - 0.5) / np.sqrt(2 * ci)).float()
    b = (torch.rand((co,), generator=g) - 0.5).float()
    ref = oracle_adjoint(x.double().numpy(), k.double().numpy(), h, w, off, p)
    for a in (ref,):
        a.setflags(write=False)
    return (x.numpy(), k.numpy(), b.numpy()), ref


def oracle_adjoint(x, k, h, w, off, p, r=R, s=S, d=1, groups=1):
    """y - bias in oracle terms: d input of HexConv2d(out -> in) for gy = x."""
    B = x.shape[0]
    co = k.shape[1] * groups
    return O.hexconv2d_backward(np.zeros((B, co, h, w)), k, x, off, r, s, p, d, groups)[0]


def from_taps(taps, x, k, h, w):
    """y - bias rebuilt in NumPy (fp64) from the kernel's class table: taps[rc][cc] is the list
    of (t, rofs, qofs) of output class (iy mod 4, ix mod 2); sample (4a + rc, 2b + cc) takes tap
    t from x[2a + rofs, b + qofs] where that is inside x."""
    x = np.asarray(x, np.float64)
    k = np.asarray(k, np.float64).reshape(k.shape[0], k.shape[1], -1)
    B, ci, hin, win = x.shape
    y = np.zeros((B, k.shape[1], h, w))
    for iy in range(h):
        a, rc = divmod(iy, 4)
        for cc in (0, 1):
            nb = len(range(cc, w, 2))
            for (t, rofs, qofs) in taps[rc][cc]:
                ro = 2 * a + rofs
                if ro < 0 or ro >= hin:
                    continue
                b0, b1 = max(0, -qofs), min(nb, win - qofs)
                if b1 <= b0:
                    continue
                y[:, :, iy, cc + 2 * b0:cc + 2 * b1:2] += np.einsum(
                    "oc,boq->bcq", k[:, :, t], x[:, :, ro, b0 + qofs:b1 + qofs])
    return y
