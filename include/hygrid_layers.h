/*
 * hygrid_layers.h — C ABI of libhygrid_hip.so, part two: layers built on the operators of
 * hygrid.h.  Same library, same ABI version, same contract.
 *
 * Contract (all entry points):
 *   - Plain pointers to DEVICE memory, caller-allocated and contiguous
 *     (planar, row-major: (planes, h, w) for the resamplers, (B, C, H, W) for
 *     the convolution).  The library never allocates, frees or retains caller
 *     memory and holds no global mutable state: every call is reentrant.
 *   - Work is enqueued on `stream` (a hipStream_t; NULL = the null stream) with
 *     no host synchronisation inside, so calls may be captured in a hipGraph.
 *   - Return value: HG_OK (0) on success, a negative HG_E* for argument / shape
 *     / dtype errors (nothing is launched), or a positive hipError_t.
 *     hg_strerror() renders either kind.
 *
 * The reference (Tesla-Albert/Hybrid-Grid-for-Hexagonal-and-Rectangular-Image-Processing) has
 * no transposed hex convolution; the layer here is defined as the adjoint of its HexConv2d
 * (HexFrames.py:96-169), the way torch defines ConvTranspose2d next to Conv2d.
 */
#ifndef HYGRID_LAYERS_H
#define HYGRID_LAYERS_H

#include "hygrid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HexConvTranspose2d forward: the exact adjoint of the HexConv2d layer
 *     A = HexConv2d(out_channels -> in_channels, even_odd_offset, radius, stride, padding,
 *                   dilation, groups, constant padding with 0)
 * plus a bias.  x: (B, in_channels, hin, win) of x_dtype, a hex image of row offset 0 (as A's
 * output); kernel: (in_channels, out_channels / groups, K), K = 3r^2-3r+1, of w_dtype (F32 or
 * F64): A's own kernel tensor, torch's transposed-conv layout; bias: (out_channels,) of w_dtype
 * or NULL; y: (B, out_channels, h, w) of y_dtype, a hex image of row offset even_odd_offset.
 * With (dy_t, dk_t(par)) A's taps and p its padding,
 *     y[b,c,iy,ix] = bias[c] + sum_{o,t} kernel[o,c,t] * x[b,o,ro,q]
 * over the taps for which ro = (iy + p - dy_t) / s and q = (ix + p - dk_t(ro & 1)) / s are
 * integers inside x's raster: y - bias is hg_hexconv2d_backward's dx for gy = x.
 * (h, w) must be a size A maps onto (hin, win): hg_hexconv2d_out_shape(h, w, ...) == (hin, win),
 * else HG_ESHAPE.  Every element of y is written; those no tap reaches hold the bias.
 * Radius 2, stride 2, dilation 1, groups 1, float32 weights, padding 0..2, out_channels >= 16
 * and x, y each of F16 / BF16 / F32 run as implicit GEMMs on the f32 matrix cores
 * (k_hexconvt_s2, conv_transpose_mfma.hip; no atomics, bit-reproducible).  Everything else,
 * and every call with the environment variable HYGRID_CONVT_MFMA=0, runs
 * hg_hexconv2d_backward's d input followed by a per-channel bias add; that route needs
 * x_dtype == y_dtype == w_dtype (HG_EDTYPE otherwise). */
int hg_hexconv_transpose2d(const void* x, const void* kernel, const void* bias, void* y,
                           int x_dtype, int w_dtype, int y_dtype, int64_t batch,
                           int64_t in_channels, int64_t out_channels, int64_t hin, int64_t win,
                           int64_t h, int64_t w, int radius, int stride, int padding,
                           int dilation, int groups, int even_odd_offset, void* stream);

/* Which route hg_hexconv_transpose2d would take for this layer (nothing is launched, no device
 * is touched); the same host function routes the real call, HYGRID_CONVT_MFMA included.
 * Returns the negative status the call would return for bad sizes, groups or dtypes (*kernel
 * is then left alone); the adjoint route's equal-dtype rule is the call's alone, so that a
 * caller can ask first and convert afterwards. */
enum hg_convt_kernel { HG_CONVT_ADJOINT = 0, HG_CONVT_MFMA_S2 = 1 };
int hg_hexconv_transpose2d_plan(int x_dtype, int w_dtype, int y_dtype, int64_t batch,
                                int64_t in_channels, int64_t out_channels, int64_t hin,
                                int64_t win, int64_t h, int64_t w, int radius, int stride,
                                int padding, int dilation, int groups, int even_odd_offset,
                                hg_host_int_out kernel);

/* The tap table k_hexconvt_s2 is launched with (radius 2, stride 2, padding 0..2), for the
 * output samples of class (row_class, col_class) = (iy mod 4, ix mod 2): out[0] = n (1 or 2),
 * then n triples (t, rofs, qofs): sample (4a + row_class, 2b + col_class) takes tap t from x row
 * 2a + rofs, column b + qofs where that lies inside x.  out: 7 ints in HOST memory.  Host only;
 * for the index test that precedes any run of the kernel. */
int hg_hexconv_transpose2d_taps(int even_odd_offset, int padding, int row_class, int col_class,
                                hg_host_int_out out);

#ifdef __cplusplus
}
#endif

#endif /* HYGRID_LAYERS_H */
