// conv_transpose_mfma.hip — HexConvTranspose2d (hygrid_layers.h): the exact adjoint of a
// HexConv2d with constant zero padding, plus a bias; at stride 2 the learnable x2 upsampler of
// an encoder-decoder, and element for element the d input of a stride-2 HexConv2d.
//
// With (dy_t, dk_t(par)) the adjoint conv's taps (tap_geom(r, s, d, (off + p) & 1, t)) and p its
// padding,
//     y[b,c,iy,ix] = bias[c] + sum_{o,t} W[o,c,t] * x[b,o,ro,q],
//     ro = (iy + p - dy_t) / s,  q = (ix + p - dk_t(ro & 1)) / s,  both exact and inside x.
//
// Radius 2, stride 2 (k_hexconvt_s2).  dk_t(1) = dk_t(0) + 1 and dy_t in {0, 1, 2}, so which
// taps reach an output sample, and from where, depends on (iy mod 4, ix mod 2) only: with
// iy = 4a + rc, ix = 2b + cc a tap of the class reads x row 2a + rofs, column b + qofs,
//     rofs = (rc + p - dy_t) / 2,  qofs = (cc + p - dk_t(0) - (rofs & 1)) / 2   (convt_class_taps).
// A class has one or two taps, 7/4 on average: rows of even iy + p take one tap from each of two
// x rows, rows of odd iy + p two or one taps of one x row, alternating by column.  Per class the
// sum is an implicit GEMM, M = out channels, K = in channels x (1 or 2) taps, N = the pixels of
// the class; consecutive output columns of one parity read consecutive x columns, so a B
// fragment is 16 consecutive LDS slots of the x tile as staged: no zero-stuffed copy of x, and
// absent taps are not multiplied at all.
//
// Workgroup = 4 waves = output rows 4a .. 4a + 3 (one per wave: its row class is the wave
// index) x 128 output columns (64 of each column class = 64 x columns) x 16 or 32 output
// channels.  Per chunk of CT_CC = 8 in channels it stages x rows 2a + rmin .. + 2, columns
// q0 - 1 .. q0 + 64 (out of raster: 0) and the chunk's weights straight from [in][out][7] (the
// K index is outermost already) in LDS, 14.7 KB.  v_mfma_f32_16x16x4_f32, products fp32-exact as
// in conv_mfma_bwd.hip.  D register v of lane (li, lk) is channel 4 lk + v at x column li of the
// fragment in both column classes, i.e. two adjacent output columns: stored together (8 B f32,
// 4 B for the 16-bit types) with the bias added.  Every output element is written exactly once,
// untapped ones (at p = 0 the last row and columns of the larger sizes) with the bias alone; no
// atomics, bit-reproducible.
// An x sample outside the raster is staged as 0 and multiplied (0 * w = 0 for finite weights),
// as the forward kernels do with their padding.
//
// Everything outside that domain runs hg_hexconv2d_backward's d input (the generic gather, or at
// stride 1 the adjoint-geometry MFMA launch) and then k_convt_bias_add.
#include <algorithm>
#include <climits>

#include "common.h"
#include "conv_mfma.h"
#include "hexconv_geom.h"
#include "../../include/hygrid_layers.h"

namespace hg {

constexpr int CT_MIN_O = 16;                // out channels from which the layer runs here
constexpr int CT_QI = 64;                   // x columns per workgroup (128 output columns)
constexpr int CT_CC = 8;                    // in channels per LDS chunk
constexpr int CT_PR = 3;                    // staged x rows
constexpr int CT_SC = CT_QI + 2;            // staged x columns: q0 - 1 .. q0 + 64
constexpr int CT_PP = 68;                   // staged row pitch
constexpr int CT_CST = 4 * CT_PP;           // x channel stride: 272 = 16 mod 32 banks
static_assert(CT_PR * CT_PP <= CT_CST && CT_SC <= CT_PP, "x tile");

// weight channel stride of a [k][t][o] chunk of 16 NOT channels: = 16 mod 32 banks
template <int NOT> constexpr int ct_wst = 7 * 16 * NOT + (NOT == 1 ? 0 : 16);

// The taps of class (rc, cc) = (iy mod 4, ix mod 2): n of them, each (t, rofs, qofs)
struct ConvtClass { int n, t[2], rofs[2], qofs[2]; };

static bool convt_class_taps(int off, int p, int rc, int cc, ConvtClass& K) {
    K.n = 0;
    for (int t = 0; t < 7; ++t) {
        int dy, dk0, dk1;
        tap_geom(2, 2, 1, (off + p) & 1, t, &dy, &dk0, &dk1);
        if (dk1 != dk0 + 1) return false;                // what the class structure rests on
        const int vy = rc + p - dy;
        if (vy & 1) continue;
        const int rofs = vy / 2;                         // exact, may be -1
        const int vx = cc + p - dk0 - (rofs & 1);
        if (vx & 1) continue;
        if (K.n == 2) return false;
        K.t[K.n] = t; K.rofs[K.n] = rofs; K.qofs[K.n] = vx / 2;
        ++K.n;
    }
    return K.n >= 1;
}

struct ConvtGeom {
    int64_t B;
    int C, O;                   // in / out channels (K / M of the GEMM)
    int hin, win, h, w;         // x and y rasters
    int ntq, ntr, nto;          // tiles along output columns / rows / out channels
    int rmin;                   // first staged x row is 2a + rmin
    int vec;                    // column pairs stored as one: w even, y aligned to a pair
    // row class rc, slot 2 cc + j: tap index (-1: the class has one tap only) and where its B
    // fragments start in a staged x channel
    int tap[4][4], slot[4][4];
};

template <typename Tin, typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconvt_s2(const Tin* __restrict__ x,
                                                            const float* __restrict__ kern,
                                                            const float* __restrict__ bias,
                                                            Tout* __restrict__ y, ConvtGeom G) {
    constexpr int CT_O = 16 * NOT, WST = ct_wst<NOT>;
    __shared__ float ps[CT_CC * CT_CST];                 // x chunk [k][row][col]
    __shared__ float ws[CT_CC * WST];                    // weight chunk [k][t][o]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tq = (int)(bid % G.ntq); bid /= G.ntq;
    const int tr = (int)(bid % G.ntr); bid /= G.ntr;
    const int to = (int)(bid % G.nto);
    const int64_t b = bid / G.nto;
    const int q0 = tq * CT_QI, a = tr, o0 = to * CT_O;
    const int r = 4 * a + wv;                            // this wave's output row, class wv
    const int li = lane & 15, lk = lane >> 4;            // fragment row / column, k of this lane

    // this wave's four tap slots (uniform): column class 0 slots 0, 1; class 1 slots 2, 3
    int tp[4], sl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        tp[s] = wv == 0 ? G.tap[0][s] : wv == 1 ? G.tap[1][s] : wv == 2 ? G.tap[2][s] : G.tap[3][s];
        sl[s] = wv == 0 ? G.slot[0][s] : wv == 1 ? G.slot[1][s] : wv == 2 ? G.slot[2][s] : G.slot[3][s];
    }

    cm_f4 acc[NOT][2][4];                                // [channel tile][column class][x column tile]
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) acc[ot][cc][qt] = cm_f4{0.f, 0.f, 0.f, 0.f};

    const Tin* xb = x + b * (int64_t)G.C * G.hin * G.win;
    const int row0 = 2 * a + G.rmin, col0 = q0 - 1;
    for (int c0 = 0; c0 < G.C; c0 += CT_CC) {
        // ---- x rows row0 .. row0 + 2, columns col0 .. col0 + 65 of the chunk; 0 outside ----
        for (int e = tid; e < CT_CC * CT_PR * CT_SC; e += CM_THREADS) {
            const int pc = e % CT_SC, rr = e / CT_SC;
            const int pr = rr % CT_PR, kk = rr / CT_PR;
            const int k = c0 + kk, yi = row0 + pr, xi = col0 + pc;
            float v = 0.f;
            if (k < G.C && yi >= 0 && yi < G.hin && xi >= 0 && xi < G.win)
                v = (float)xb[((int64_t)k * G.hin + yi) * G.win + xi];
            ps[kk * CT_CST + pr * CT_PP + pc] = v;
        }
        // ---- weights W[c0 .. c0+7][o0 .. o0+CT_O-1][t] as [k][t][o]; 0 past C or O ----------
        for (int e = tid; e < CT_CC * CT_O * 7; e += CM_THREADS) {
            const int kk = e / (CT_O * 7), ot7 = e - kk * (CT_O * 7);
            const int o = ot7 / 7, t = ot7 - 7 * o;
            const int k = c0 + kk;
            float v = 0.f;
            if (k < G.C && o0 + o < G.O) v = kern[((int64_t)k * G.O + o0 + o) * 7 + t];
            ws[kk * WST + t * CT_O + o] = v;
        }
        __syncthreads();
        if (r < G.h) {                                   // wave-uniform
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (tp[s] < 0) continue;                 // uniform: an absent tap costs nothing
                const float* pb = ps + lk * CT_CST + sl[s] + li;
                const float* wb = ws + lk * WST + tp[s] * CT_O + li;
#pragma unroll
                for (int cq = 0; cq < CT_CC / 4; ++cq) {
                    float af[NOT], bf[4];
#pragma unroll
                    for (int ot = 0; ot < NOT; ++ot) af[ot] = wb[cq * 4 * WST + ot * 16];
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt) bf[qt] = pb[cq * 4 * CT_CST + qt * 16];
#pragma unroll
                    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                        for (int qt = 0; qt < 4; ++qt)
                            acc[ot][s >> 1][qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                af[ot], bf[qt], acc[ot][s >> 1][qt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- store: register v is channel 4 lk + v; the two classes are columns 2 q, 2 q + 1 ----
    if (r >= G.h) return;
    Tout* yb = y + b * (int64_t)G.O * G.h * G.w;
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + lk * 4 + v;
            if (o >= G.O) continue;
            const float bv = bias ? bias[o] : 0.f;
            Tout* const yr = yb + ((int64_t)o * G.h + r) * G.w;
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                const int ix = 2 * (q0 + qt * 16 + li);
                if (ix >= G.w) continue;
                const Tout v0 = (Tout)(acc[ot][0][qt][v] + bv), v1 = (Tout)(acc[ot][1][qt][v] + bv);
                if (G.vec) {                             // w even: ix + 1 < w as well
                    typedef Tout t2v __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<t2v*>(yr + ix) = t2v{v0, v1};
                } else {
                    yr[ix] = v0;
                    if (ix + 1 < G.w) yr[ix + 1] = v1;
                }
            }
        }
}

// y[b][c][..] += bias[c] after the adjoint route's gather (A: the weights' type)
template <typename Ty, typename A>
__global__ __launch_bounds__(256) void k_convt_bias_add(Ty* __restrict__ y, const A* __restrict__ bias,
                                                        int64_t total, int64_t plane, int64_t O) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        y[i] = from_acc<Ty>(to_acc<A>(y[i]) + bias[(i / plane) % O]);
}

// Argument checks of the layer (and of its plan query), in the order the call reports them.
// The adjoint conv maps out_channels -> in_channels channels and (h, w) -> (hin, win).
static int convt_check(int x_dtype, int w_dtype, int y_dtype, int64_t batch, int64_t in_channels,
                       int64_t out_channels, int64_t hin, int64_t win, int64_t h, int64_t w,
                       int radius, int stride, int padding, int dilation, int groups) {
    int64_t ho, wo;
    int st = conv_out_shape(h, w, radius, stride, padding, dilation, &ho, &wo);
    if (st) return st;
    if (ho != hin || wo != win) return HG_ESHAPE;
    st = conv_check_args(batch, out_channels, in_channels, h, w, groups, padding, HG_PAD_CONSTANT);
    if (st) return st;
    if (3 * radius * radius - 3 * radius + 1 > 128) return HG_EUNSUP;    // hexconv_bwd.hip's tap table
    if (w_dtype != HG_F32 && w_dtype != HG_F64) return HG_EDTYPE;
    if (!dtype_is_float(x_dtype) || !dtype_is_float(y_dtype)) return HG_EDTYPE;
    return HG_OK;
}

// Which route a layer whose arguments passed convt_check takes (enum hg_convt_kernel): the one
// statement of the kernel's domain, for the call and for hg_hexconv_transpose2d_plan.
// A/B switch HYGRID_CONVT_MFMA=0: the adjoint route.
static int convt_route(int x_dtype, int w_dtype, int y_dtype, int64_t B, int64_t C, int64_t O,
                       int64_t hin, int64_t win, int64_t h, int64_t w, int radius, int stride,
                       int padding, int dilation, int groups) {
    if (env_is("HYGRID_CONVT_MFMA", "0")) return HG_CONVT_ADJOINT;
    if (radius != 2 || stride != 2 || dilation != 1 || groups != 1) return HG_CONVT_ADJOINT;
    if (padding < 0 || padding > 2 || w_dtype != HG_F32 || O < CT_MIN_O) return HG_CONVT_ADJOINT;
    for (int dt : {x_dtype, y_dtype})
        if (dt != HG_BF16 && dt != HG_F16 && dt != HG_F32) return HG_CONVT_ADJOINT;
    if (B < 1 || C < 1 || hin < 1 || win < 1 || h < 1 || w < 1) return HG_CONVT_ADJOINT;
    if (!conv_mfma_size_ok(C, O, hin, win) || !conv_mfma_size_ok(O, C, h, w)) return HG_CONVT_ADJOINT;
    if (C * O * 7 > INT_MAX) return HG_CONVT_ADJOINT;
    const int64_t nto = (O + (O <= 16 ? 16 : 32) - 1) / (O <= 16 ? 16 : 32);
    const int64_t blocks = B * nto * ((h + 3) / 4) * ((w + 2 * CT_QI - 1) / (2 * CT_QI));
    if (blocks > INT_MAX) return HG_CONVT_ADJOINT;
    return HG_CONVT_MFMA_S2;
}

static int convt_mfma_launch(const void* x, const float* kern, const float* bias, void* y,
                             int x_dtype, int y_dtype, int64_t B, int64_t C, int64_t O, int64_t hin,
                             int64_t win, int64_t h, int64_t w, int padding, int off,
                             hipStream_t st) {
    ConvtGeom G = {};
    G.B = B; G.C = (int)C; G.O = (int)O;
    G.hin = (int)hin; G.win = (int)win; G.h = (int)h; G.w = (int)w;
    ConvtClass K[4][2];
    int rmin = INT_MAX, rmax = INT_MIN;
    for (int rc = 0; rc < 4; ++rc)
        for (int cc = 0; cc < 2; ++cc) {
            if (!convt_class_taps(off, padding, rc, cc, K[rc][cc])) return HG_EUNSUP;
            for (int j = 0; j < K[rc][cc].n; ++j) {
                rmin = std::min(rmin, K[rc][cc].rofs[j]);
                rmax = std::max(rmax, K[rc][cc].rofs[j]);
                if (K[rc][cc].qofs[j] < -1 || K[rc][cc].qofs[j] > 1) return HG_EUNSUP;
            }
        }
    if (rmax - rmin >= CT_PR) return HG_EUNSUP;          // the staged tile holds every tap
    G.rmin = rmin;
    for (int rc = 0; rc < 4; ++rc)
        for (int s = 0; s < 4; ++s) {
            const ConvtClass& k = K[rc][s >> 1];
            const int j = s & 1;
            G.tap[rc][s] = j < k.n ? k.t[j] : -1;
            G.slot[rc][s] = j < k.n ? (k.rofs[j] - rmin) * CT_PP + k.qofs[j] + 1 : 0;
        }
    const int nt = O <= 16 ? 1 : 2;
    G.nto = (int)((O + 16 * nt - 1) / (16 * nt));
    G.ntr = (G.h + 3) / 4;
    G.ntq = (G.w + 2 * CT_QI - 1) / (2 * CT_QI);
    const size_t pair = 2 * (size_t)dtype_size(y_dtype);
    G.vec = (G.w % 2) == 0 && (reinterpret_cast<uintptr_t>(y) % pair) == 0;
    const dim3 grid((unsigned)(B * G.nto * G.ntr * G.ntq)), blk(CM_THREADS);
#define HG_CT_LAUNCH(TI, TO)                                                                  \
    {                                                                                         \
        if (nt == 1)                                                                          \
            hipLaunchKernelGGL((k_hexconvt_s2<TI, TO, 1>), grid, blk, 0, st, (const TI*)x, kern, bias, (TO*)y, G); \
        else                                                                                  \
            hipLaunchKernelGGL((k_hexconvt_s2<TI, TO, 2>), grid, blk, 0, st, (const TI*)x, kern, bias, (TO*)y, G); \
        return launch_status();                                                               \
    }
#define HG_CT_OUT(TI)                                                                         \
    switch (y_dtype) {                                                                        \
    case HG_BF16: HG_CT_LAUNCH(TI, __bf16)                                                    \
    case HG_F16: HG_CT_LAUNCH(TI, _Float16)                                                   \
    case HG_F32: HG_CT_LAUNCH(TI, float)                                                      \
    default: return HG_EUNSUP;                                                                \
    }
    switch (x_dtype) {
    case HG_BF16: HG_CT_OUT(__bf16)
    case HG_F16: HG_CT_OUT(_Float16)
    case HG_F32: HG_CT_OUT(float)
    default: return HG_EUNSUP;
    }
#undef HG_CT_OUT
#undef HG_CT_LAUNCH
}

template <typename A>
static int convt_bias_launch(void* y, const void* bias, int y_dtype, int64_t total, int64_t plane,
                             int64_t O, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 1 << 20);
    HG_DISPATCH_FLOAT_OUT(y_dtype, TY, {
        hipLaunchKernelGGL((k_convt_bias_add<TY, A>), dim3((unsigned)blocks), dim3(256), 0, st,
                           (TY*)y, (const A*)bias, total, plane, O);
        return launch_status();
    });
    return HG_EDTYPE;
}

}  // namespace hg

extern "C" int hg_hexconv_transpose2d(const void* x, const void* kernel, const void* bias, void* y,
                                      int x_dtype, int w_dtype, int y_dtype, int64_t batch,
                                      int64_t in_channels, int64_t out_channels, int64_t hin,
                                      int64_t win, int64_t h, int64_t w, int radius, int stride,
                                      int padding, int dilation, int groups, int even_odd_offset,
                                      void* stream) {
    using namespace hg;
    const int st = convt_check(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, hin,
                               win, h, w, radius, stride, padding, dilation, groups);
    if (st) return st;
    const int route = convt_route(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, hin,
                                  win, h, w, radius, stride, padding, dilation, groups);
    if (route == HG_CONVT_ADJOINT && (x_dtype != w_dtype || y_dtype != w_dtype)) return HG_EDTYPE;
    if (batch == 0 || h == 0 || w == 0) return HG_OK;
    if (!x || !kernel || !y) return HG_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (route == HG_CONVT_MFMA_S2)
        return convt_mfma_launch(x, (const float*)kernel, (const float*)bias, y, x_dtype, y_dtype,
                                 batch, in_channels, out_channels, hin, win, h, w, padding,
                                 even_odd_offset & 1, s);
    // the adjoint conv's d input: its x is y here, its gy is x
    const int rc = hg_hexconv2d_backward(nullptr, kernel, x, y, nullptr, nullptr, y_dtype, w_dtype,
                                         batch, out_channels, in_channels, h, w, radius, stride,
                                         padding, dilation, groups, even_odd_offset,
                                         HG_PAD_CONSTANT, 0.0, stream);
    if (rc || !bias) return rc;
    const int64_t plane = h * w, total = batch * out_channels * plane;
    if (w_dtype == HG_F64) return convt_bias_launch<double>(y, bias, y_dtype, total, plane, out_channels, s);
    return convt_bias_launch<float>(y, bias, y_dtype, total, plane, out_channels, s);
}

extern "C" int hg_hexconv_transpose2d_plan(int x_dtype, int w_dtype, int y_dtype, int64_t batch,
                                           int64_t in_channels, int64_t out_channels, int64_t hin,
                                           int64_t win, int64_t h, int64_t w, int radius,
                                           int stride, int padding, int dilation, int groups,
                                           int even_odd_offset, hg_host_int_out kernel) {
    using namespace hg;
    (void)even_odd_offset;                               // the offset moves taps, never the route
    if (!kernel) return HG_EINVAL;
    const int st = convt_check(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, hin,
                               win, h, w, radius, stride, padding, dilation, groups);
    if (st) return st;
    *kernel = convt_route(x_dtype, w_dtype, y_dtype, batch, in_channels, out_channels, hin, win, h,
                          w, radius, stride, padding, dilation, groups);
    return HG_OK;
}

extern "C" int hg_hexconv_transpose2d_taps(int even_odd_offset, int padding, int row_class,
                                           int col_class, hg_host_int_out out) {
    using namespace hg;
    if (!out || row_class < 0 || row_class > 3 || col_class < 0 || col_class > 1) return HG_EINVAL;
    if (padding < 0 || padding > 2) return HG_EUNSUP;
    ConvtClass K;
    if (!convt_class_taps(even_odd_offset & 1, padding, row_class, col_class, K)) return HG_EUNSUP;
    out[0] = K.n;
    for (int j = 0; j < K.n; ++j) {
        out[1 + 3 * j] = K.t[j];
        out[2 + 3 * j] = K.rofs[j];
        out[3 + 3 * j] = K.qofs[j];
    }
    return HG_OK;
}
