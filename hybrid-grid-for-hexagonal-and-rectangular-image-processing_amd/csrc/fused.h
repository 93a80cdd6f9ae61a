// fused.h — the two-column streaming fused kernel (fused.hip), tried first by
// hg_pipeline_r2h_conv_h2r (pipeline.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice.h"

namespace hg {

// Runs the fused pass if the call is in the kernel's domain (same-size round trip,
// padding 1 with pad value 0, radius 2, C/O/groups in {3/3/1, 3/3/3, 1/1/1}, 16/32-bit
// floats, even widths); returns HG_EUNSUP (nothing launched) otherwise.
int fused_try(const void* x, const float* kernel, const float* bias, void* y, int x_dtype,
              int y_dtype, int64_t batch, int C, int O, int G, int64_t h, int64_t w,
              int64_t h1, int64_t w1, int64_t h2, int64_t w2, int padding, int op,
              double pad_value, hipStream_t st);

// rect -> hex -> rect round trip (no conv) on the same kernel, same-size lattices, even
// widths, planes of (h, w) -> (h1, w1); HG_EUNSUP otherwise.
int fused_rt_try(const void* x, void* y, int x_dtype, int y_dtype, int64_t planes, int64_t h,
                 int64_t w, int64_t h1, int64_t w1, hipStream_t st);

// HexConv2d alone on the same kernel (fused_conv.hip): radius 2, stride 1, padding 1,
// pad value 0, no epilogue, C/O/groups as above, even widths; HG_EUNSUP otherwise.
int fused_conv_try(const void* x, const float* kernel, const float* bias, void* y, int x_dtype,
                   int y_dtype, int64_t batch, int C, int O, int G, int64_t h, int64_t w,
                   int padding, int off, double pad_value, bool epilogue, hipStream_t st);

// Does the same-size streaming kernel cover this r2h lattice (in(r) - r and jn(q) - q in
// {-1, 0} wherever a tap is inside the raster)?  Exact, O(h1 + w1) fp64 on the host.
bool fused_geometry_ok(const Geom& g);

// pipeline_bwd.hip: tile rows / columns of the chain's backward passes and the tiles a
// weight-pass workgroup walks top to bottom (hg_fused_layout md 9).
void chain_bwd_layout(int* tile_rows, int* tile_cols, int* band_tiles);

}  // namespace hg
