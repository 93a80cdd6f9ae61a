// conv_mfma.h — what the wide-channel HexConv2d kernels share: the forward implicit GEMM
// (conv_mfma.hip) and the backward kernels built on its tile (conv_mfma_bwd.hip): tile
// constants, the geometry struct and the fp32 staging of the padded input P in LDS.
#pragma once
#include <algorithm>
#include <climits>

#include "common.h"
#include "hexconv_geom.h"

namespace hg {

constexpr int CM_THREADS = 256;
constexpr int CM_ROWS = 4;                  // output rows per workgroup (one per wave)
constexpr int CM_Q = 64;                    // output columns per workgroup
constexpr int CM_OMAX = 64;                 // output channels per workgroup (NOT = 4 tiles;
                                            // 2 tiles = 32 channels when O <= 32)
constexpr int CM_CC = 8;                    // input channels per LDS chunk (28.6 KB LDS: 4 WGs per CU)
constexpr int CM_PR = CM_ROWS + 2;          // staged P rows (taps reach rows r .. r+2)
constexpr int CM_PP = 72;                   // staged P pitch: 64 + tap column span (<= 4),
                                            // 6*72 = 432 = 16 mod 32 banks: conflict-free B reads
constexpr int CM_CST = CM_PR * CM_PP;       // P channel stride
constexpr int CM_WST = 7 * CM_OMAX + 16;    // weight channel stride (= 16 mod 32 banks)


// Stride 2 (forward, and the d kernel GEMM of conv_mfma_bwd.hip): a workgroup's 4 x 64 outputs read staged rows 2 r0 .. 2 r0 + 8 and
// staged columns 2 q0 + mink + (0..129).  Each staged row is kept as two column-parity planes:
// sample column j sits in plane j & 1 at slot j >> 1, so the 16 columns 2 q + dk of a B fragment
// (dk fixed within a tap and row parity) are 16 consecutive slots, as at stride 1.
constexpr int CS_PR = 2 * (CM_ROWS - 1) + 3;    // staged P rows (wave wv reads rows 2 wv + dy, dy <= 2)
constexpr int CS_SL = CM_Q + 1;                 // slots per plane in use (dk <= 3: slot q + 1)
constexpr int CS_PL = 72;                       // plane pitch
constexpr int CS_PP = 2 * CS_PL;                // row pitch; 9 * 144 = 1296 = 16 mod 32 banks
constexpr int CS_CST = CS_PR * CS_PP;           // P channel stride

typedef float cm_f4 __attribute__((ext_vector_type(4)));

struct MfmaGeom {
    int64_t B;
    int C, O, h, w, ho, wo, p, pad_mode;
    int mink;                   // smallest tap column offset over both parities
    int dy[7], dk[2][7];        // tap rows / columns (staged frame, relative to mink)
    int ntq, ntr, nto;          // tiles along columns / rows / output channels
    // the staged frame against the source raster (h x w): staged sample (py, px) is source
    // sample (py - oy, px - ox) under the padding rule, and 0 at py >= Hp or px >= Wp.
    // Forward: oy = ox = p, Hp = h + 2p, Wp = w + 2p (past it: the type1 structural zero).
    // Adjoint (d input, conv_mfma_bwd.hip): the source is gy, the origin the tap span's far
    // corner, no upper bound (constant padding with 0 outside gy).
    int oy, ox, Hp, Wp;
    float pad_value;
    Epilogue epi;
};

// The forward's 32-bit-offset size limits (one plane set of a batch element below 2 GiB of
// fp32, tile counts in int).
inline bool conv_mfma_size_ok(int64_t C, int64_t O, int64_t h, int64_t w) {
    if (C > INT_MAX / 16 || O > INT_MAX / 16 || h > INT_MAX / 4 || w > INT_MAX / 4) return false;
    return C * h * w * 4 < ((int64_t)1 << 31);
}

// The forward geometry of a dense radius-2, dilation-1 layer of stride 1 or 2: shapes, tap
// tables, staged frame, row / column tile counts (nto is the caller's: it picks the tile count
// per workgroup).  false when the layer has no output or its taps do not fit the staged tile
// (stride 1: 6 rows x CM_PP columns; stride 2: CS_PR rows x 2 planes of CS_SL slots).
inline bool conv_mfma_forward_geom(MfmaGeom& G, int64_t B, int64_t C, int64_t O, int64_t h,
                                   int64_t w, int padding, int off, int pad_mode,
                                   double pad_value, int stride = 1) {
    G.B = B; G.C = (int)C; G.O = (int)O; G.h = (int)h; G.w = (int)w; G.p = padding;
    G.pad_mode = pad_mode; G.pad_value = (float)pad_value;
    G.oy = G.ox = padding; G.Hp = G.h + 2 * padding; G.Wp = G.w + 2 * padding;
    int64_t ho, wo;
    if (stride != 1 && stride != 2) return false;
    if (conv_out_shape(h, w, 2, stride, padding, 1, &ho, &wo)) return false;
    G.ho = (int)ho; G.wo = (int)wo;
    const int op = (off + padding) & 1;
    int mink = INT_MAX, maxk = INT_MIN, maxdy = 0;
    int dyv[7], dk0[7], dk1[7];
    for (int t = 0; t < 7; ++t) {
        tap_geom(2, stride, 1, op, t, &dyv[t], &dk0[t], &dk1[t]);
        mink = std::min(mink, std::min(dk0[t], dk1[t]));
        maxk = std::max(maxk, std::max(dk0[t], dk1[t]));
        maxdy = std::max(maxdy, dyv[t]);
    }
    if (stride == 1 && maxk - mink + CM_Q > CM_PP) return false;
    if (stride == 2 && (mink < 0 || 2 * (CM_Q - 1) + (maxk - mink) >= 2 * CS_SL ||
                        2 * (CM_ROWS - 1) + maxdy >= CS_PR))
        return false;
    G.mink = mink;
    for (int t = 0; t < 7; ++t) {
        G.dy[t] = dyv[t];
        G.dk[0][t] = dk0[t] - mink;
        G.dk[1][t] = dk1[t] - mink;
    }
    G.ntq = (G.wo + CM_Q - 1) / CM_Q;
    G.ntr = (G.ho + CM_ROWS - 1) / CM_ROWS;
    return true;
}

// Stage P rows r0 .. r0+5 (staged frame), columns q0 + mink + (0..71), of channels
// c0 .. c0+CM_CC-1 as fp32 [c][row][col] in ps.  216 threads = 72 columns x 3 row phases;
// each thread keeps its column's source index (padding rules applied once) and walks rows
// pr = phase, phase + 3, ... of every channel of the chunk.  (Loading the next chunk into
// registers during the MFMAs instead needs ~60 more VGPRs and spilled at 2 waves per SIMD.)
template <typename Tin>
__device__ __forceinline__ void cm_stage_p(float* __restrict__ ps, const Tin* __restrict__ xb,
                                           const MfmaGeom& G, int c0, int q0, int r0, int tid) {
    if (tid < 3 * CM_PP) {
        const int pc = tid % CM_PP, ph = tid / CM_PP;
        const int px = q0 + G.mink + pc;
        const bool zc = px >= G.Wp;                      // type1 structural zero column
        const int64_t xi = zc ? -1 : pad_map(px - G.ox, G.w, G.pad_mode);
#pragma unroll 4
        for (int rr = ph; rr < CM_CC * CM_PR; rr += 3) {
            const int cc = rr / CM_PR, pr = rr - cc * CM_PR;
            const int c = c0 + cc, py = r0 + pr;
            float v = 0.f;
            if (!zc && c < G.C && py < G.Hp) {
                const int64_t yi = pad_map(py - G.oy, G.h, G.pad_mode);
                v = (yi < 0 || xi < 0) ? G.pad_value
                                       : (float)xb[((int64_t)c * G.h + yi) * G.w + xi];
            }
            ps[cc * CM_CST + pr * CM_PP + pc] = v;
        }
    }
}

// Where a wave's tap (dy, dk) starts in a staged P channel, in slots: stride 1 row wv + dy,
// column dk; stride 2 row 2 wv + dy of the two column-parity planes (above): plane dk & 1,
// slot dk >> 1.  The 16 columns of a fragment are the 16 slots from there.
__device__ __forceinline__ int cs_slot(int row, int dk) {     // staged (row, column 2 q' + dk) at q' = 0
    return row * CS_PP + (dk & 1) * CS_PL + (dk >> 1);
}
template <int S>
__device__ __forceinline__ int cm_pslot(int wv, int dy, int dk) {
    static_assert(S == 1 || S == 2, "stride");
    return S == 1 ? (wv + dy) * CM_PP + dk : cs_slot(2 * wv + dy, dk);
}

// Stride 2: stage P rows 2 r0 .. 2 r0 + 8 (staged frame), columns 2 q0 + mink + (0..129), of
// channels c0 .. c0+CC-1 as fp32 [c][row][plane][slot].  195 threads = 65 slots x 3 row phases;
// a thread owns the two columns of its slot (their source indices computed once, cm_stage_p's
// padding rules) and walks rows pr = phase, phase + 3, ... of every channel of the chunk.
template <int CC, typename Tin>
__device__ __forceinline__ void cs_stage_p(float* __restrict__ ps, const Tin* __restrict__ xb,
                                           const MfmaGeom& G, int c0, int q0, int r0, int tid) {
    if (tid < 3 * CS_SL) {
        const int sl = tid % CS_SL, ph = tid / CS_SL;
        const int px = 2 * q0 + G.mink + 2 * sl;          // plane 0's column; plane 1's is px + 1
        const bool z0 = px >= G.Wp, z1 = px + 1 >= G.Wp;  // type1 structural zero columns
        const int64_t x0 = z0 ? -1 : pad_map(px - G.ox, G.w, G.pad_mode);
        const int64_t x1 = z1 ? -1 : pad_map(px + 1 - G.ox, G.w, G.pad_mode);
#pragma unroll 4
        for (int rr = ph; rr < CC * CS_PR; rr += 3) {
            const int cc = rr / CS_PR, pr = rr - cc * CS_PR;
            const int c = c0 + cc, py = 2 * r0 + pr;
            float v0 = 0.f, v1 = 0.f;
            if (c < G.C && py < G.Hp) {
                const int64_t yi = pad_map(py - G.oy, G.h, G.pad_mode);
                const int64_t row = ((int64_t)c * G.h + yi) * G.w;
                if (!z0) v0 = (yi < 0 || x0 < 0) ? G.pad_value : (float)xb[row + x0];
                if (!z1) v1 = (yi < 0 || x1 < 0) ? G.pad_value : (float)xb[row + x1];
            }
            float* const d = ps + cc * CS_CST + pr * CS_PP + sl;
            d[0] = v0;
            d[CS_PL] = v1;
        }
    }
}

// Which wide-channel forward kernel hg_hexconv2d runs for a layer whose arguments passed its
// checks (enum hg_conv_fwd_kernel; HG_CONV_FWD_OTHER: none of them, the call goes on to the
// generic kernels).  Host only; the one statement of the conditions, the env switches
// HYGRID_CONV_MFMA / _MFMA_BF16 / _DMA included: conv_mfma_try launches from it and
// hg_hexconv2d_forward_plan reports it.  x_align: the low bits of x's address (0 for the query).
int conv_fwd_route(int x_dtype, int w_dtype, int y_dtype, int64_t B, int64_t C, int64_t O,
                   int64_t h, int64_t w, int radius, int stride, int padding, int dilation,
                   int groups, int off, int pad_mode, double pad_value, unsigned x_align);

// Launches k_hexconv_mfma<x_dtype, y_dtype, nt> (the f32-MFMA forward kernel, nt = 2 or 4
// output-channel tiles per workgroup; stride 2: k_hexconv_mfma_s2) on a complete geometry of
// that stride; HG_EUNSUP for a dtype pair it does not have.  conv_mfma.hip.
int conv_mfma_launch_f32(const void* x, const float* k, const float* b, void* y, int x_dtype,
                         int y_dtype, const MfmaGeom& G, int nt, hipStream_t st, int stride = 1);

}  // namespace hg
