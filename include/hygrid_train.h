/*
 * hygrid_train.h — C ABI of libhygrid_hip.so, part three: the gradients a training step takes
 * one at a time.  Same library, same ABI version, same contract.
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
 * hg_hexconv2d_backward (hygrid.h) computes all three gradients of a HexConv2d in one call and
 * keeps strided layers on its generic kernels.  The entry points here are what a layer's
 * autograd uses instead: d kernel / d bias on their own, at stride 2 on the matrix cores too.
 * (d input of a stride-2 layer is hg_hexconv_transpose2d of hygrid_layers.h, applied to gy.)
 */
#ifndef HYGRID_TRAIN_H
#define HYGRID_TRAIN_H

#include "hygrid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d kernel and d bias of hg_hexconv2d, hg_hexconv2d_backward's definition and arguments:
 * x: (B, C, h, w) of x_dtype; gy: (B, O, ho, wo) of w_dtype (F32 or F64); dkernel:
 * (O, C/groups, K) of w_dtype, or NULL; dbias: (O,) of w_dtype, or NULL.  Outputs are
 * overwritten; x is read only for dkernel.  Both are sums over B*ho*wo samples accumulated with
 * float atomics (run-to-run last-bit differences).  Bad arguments get the negative status
 * hg_hexconv2d_backward gives them, in the same order; an empty batch zeroes the outputs.
 * Routing (hg_hexconv2d_weight_grad_plan tells):
 *   - stride 2, radius 2, dilation 1, groups 1, padding 0..2, float32 weights, x of F16 / BF16 /
 *     F32 and out_channels >= 16: k_hexconv_bwd_weight_mfma_s2 on the f32 matrix cores
 *     (conv_mfma_bwd.hip), every padding mode; the environment variable
 *     HYGRID_CONV_BWD_MFMA_S2=0 sends these layers to the generic kernels;
 *   - stride 1: the kernel hg_hexconv2d_backward runs for d kernel (HYGRID_CONV_BWD_MFMA);
 *   - everything else, and d bias asked for alone: the generic passes of hexconv_bwd.hip. */
int hg_hexconv2d_weight_grad(const void* x, const void* gy, void* dkernel, void* dbias,
                             int x_dtype, int w_dtype, int64_t batch, int64_t in_channels,
                             int64_t out_channels, int64_t h, int64_t w, int radius, int stride,
                             int padding, int dilation, int groups, int even_odd_offset,
                             int pad_mode, double pad_value, void* stream);

/* Which kernel hg_hexconv2d_weight_grad would run for d kernel (+ d bias) of this layer
 * (nothing is launched, no device is touched); the same host function routes the real call,
 * both switches included.  Returns the negative status the call would return for bad arguments
 * (*kernel is then left alone); an empty batch plans HG_CONV_WGRAD_GENERIC. */
enum hg_conv_wgrad_kernel { HG_CONV_WGRAD_GENERIC = 0, HG_CONV_WGRAD_MFMA = 1,
                            HG_CONV_WGRAD_MFMA_S2 = 2 };
int hg_hexconv2d_weight_grad_plan(int x_dtype, int w_dtype, int64_t batch, int64_t in_channels,
                                  int64_t out_channels, int64_t h, int64_t w, int radius,
                                  int stride, int padding, int dilation, int groups, int pad_mode,
                                  hg_host_int_out kernel);

#ifdef __cplusplus
}
#endif

#endif /* HYGRID_TRAIN_H */
