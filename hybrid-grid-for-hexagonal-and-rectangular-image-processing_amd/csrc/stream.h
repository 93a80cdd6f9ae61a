// stream.h — row-streaming resample kernels for near-identity lattices
// (resample_stream.hip), tried first by hg_rect_to_hex / hg_hex_to_rect (resample.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hg {

// What a resample call would be launched with (hg_resample_plan, include/hygrid.h: the fields
// of enum hg_resample_plan_field).  Every *_try below takes a `plan`: null launches the kernel;
// otherwise the same host code that sizes the launch fills *plan and nothing is launched (only
// the low bits of src are looked at then: the plan query passes its src_align as the pointer).
struct ResamplePlan {
    int kernel = 0, k = 0, window_cols = 0, band_rows = 0, pdp = 0, pc = 0;
    int64_t chunks = 0, units = 0, launched = 0;
    int wave_per_unit = 0, db = 0, p = 0, sep = 0, nout = 0, lds = -1;
};

// Runs the streaming kernel if the call is in its domain (r2h with a near-identity
// lattice, h2r at the same size; 16/32-bit float in and out; widths a multiple of 4);
// returns HG_EUNSUP (nothing launched) otherwise.  Bit-identical to the general kernels.
// plan: only the domain check and the launch plan (HG_OK = the kernel would run).
int stream_try(int op, const void* src, void* dst, int sdt, int ddt, int64_t planes, int64_t h,
               int64_t w, int64_t h1, int64_t w1, hipStream_t st, ResamplePlan* plan = nullptr);

// ~2x downsampling rect->hex (ConvertToHexagon's (h//2, w//2) 'nearest' on 8/16-bit data, the
// demo's bilinear on bf16/f16; resample_down.hip); HG_EUNSUP (nothing launched) otherwise.
// hexresize_down.hip: triangle-blend resamples (op HG_OP_HEXRESIZE / HG_OP_HEX_TO_RECT,
// linear, 16-bit in) whose vertices for a run of output columns fit a 128-column input
// window (~2x hexresize: the pyramid levels; hex (h/2, w/2) -> rect (h, w)); HG_EUNSUP otherwise
int tristream_try(int op, const void* src, void* dst, int sdt, int ddt, int64_t planes, int64_t h,
                  int64_t w, int64_t h1, int64_t w1, hipStream_t st, ResamplePlan* plan);
// tri_up.hip: upsampling triangle resamples (op HG_OP_HEX_TO_RECT / HG_OP_HEXRESIZE whose output
// steps are <= one input sample: the inverse of ConvertToHexagon's lattice), 'linear' on 16/32-bit
// floats with fp32 accumulation and 'nearest' on 8/16/32-bit elements; HG_EUNSUP otherwise
int triup_try(int op, const void* src, void* dst, int sdt, int ddt, int64_t planes, int64_t h,
              int64_t w, int64_t h1, int64_t w1, int interp, hipStream_t st, ResamplePlan* plan);
int down_try(const void* src, void* dst, int sdt, int ddt, int64_t planes, int64_t h, int64_t w,
             int64_t h1, int64_t w1, int interp, hipStream_t st, ResamplePlan* plan = nullptr);
// resample_bwd.hip: the launch plan of hg_resample_backward's kernel for (planes, h1 x w1)
void resample_bwd_plan(int64_t planes, int64_t h1, int64_t w1, ResamplePlan* plan);

}  // namespace hg
