// conv_mfma_bwd.hip — HexConv2d backward for wide channel counts on the f32 matrix cores:
// the gradients of the layers conv_mfma.hip runs forward (dense radius 2, stride 1,
// dilation 1, f32 weights; HexConvModule stacks, HexModules.py:97-288).  Both paths use
// v_mfma_f32_16x16x4_f32, whose products are fp32-exact, so the gradients keep the generic
// kernels' fp32 semantics (hexconv_bwd.hip) up to summation order.
//
// d kernel / d bias (k_hexconv_bwd_weight_mfma):
//     dW[o][c][t] = sum_{b,ro,q} gy[b,o,ro,q] * P[b,c][ro + dy_t][q + dk_t(ro & 1)]
// is a GEMM with M = O, N = (c, t) pairs, K = pixels.  A workgroup takes the forward's tile
// (4 output rows, one per wave, x 64 columns), one chunk of CM_CC = 8 input channels (P staged
// by the forward's cm_stage_p) and 32 or 64 output channels, and walks a slice of consecutive
// tiles with the accumulators in registers.  N is the chunk's 8 * 7 = 56 (c, t) pairs in 4
// tiles of 16: lane j of an N tile keeps the LDS offset of its own pair; slot 56 supplies the
// constant 1 (its column of D is d bias), slots 57..63 supply 0.  For one MFMA the k index
// may name any pixel as long as A and B agree, so lane (i, k) loads the 16-B vector
// gy[o_i][r][q + 4k .. 4k+3] straight from global memory and feeds its 4 elements to 4 MFMAs,
// whose B operands are read from LDS at pixel 4k + m: no LDS for gy, 4 global loads and 16 LDS
// reads per 64 MFMAs.  Pixels outside the output (edge tiles) contribute nothing, whatever x
// holds there: both operands are zeroed (a masked gy alone would give 0 * Inf = NaN).
//
// d input: with (dy_t, dk_t) the forward's taps and p the padding,
//     dx[b,c,iy,ix] = sum_{o,t} W[o,c,t] * gy[b,o, iy + p - dy_t, ix + p - dk_t(par_ro)],
//     par_ro = (iy + p + dy_t) & 1,  gy = 0 outside its raster,
// has the forward's structure (7 taps, row offsets 2 - dy_t in {0, 1, 2}, column offsets that
// depend on the output row's parity only), so k_hexconv_mfma<float, Tx> computes it from an
// adjoint MfmaGeom built here and the transposed weights W'[c][o][t].  Constant padding only
// (the pad value never reaches d input); the other modes fold their pad bands back onto input
// pixels and keep the generic gather.  No atomics: bit-reproducible.
//
// Stride 2: d kernel / d bias on the sibling k_hexconv_bwd_weight_mfma_s2 (below), reached
// through hg_hexconv2d_weight_grad (hygrid_train.h) only: hg_hexconv2d_backward keeps strided
// layers on the generic kernels.  d input of a stride-2 layer is k_hexconvt_s2
// (conv_transpose_mfma.hip) applied to gy.
#include <algorithm>
#include <climits>

#include "common.h"
#include "conv_mfma.h"
#include "hexconv_geom.h"
#include "../../include/hygrid_train.h"

namespace hg {

// channel counts from which each gradient runs here (the forward's thresholds, confirmed
// faster than the generic kernels at 16 channels: DESIGN.md 8)
constexpr int CMB_MIN_O = 16;               // d kernel: output channels
constexpr int CMB_MIN_C = 16;               // d input: input channels
constexpr int CMB_NS = 64;                  // N slots per chunk: 56 (c, t) pairs, 1, 7 zeros
// workgroups aimed at: the ones resident at once on 256 CUs, so the grid is one round (by
// registers 3 waves per SIMD with 4 output-channel tiles, 5 with 2)
constexpr int CMB_CUS = 256;
constexpr int CMB_MIN_TILES = 8;            // ... of at least this many tiles each: a workgroup ends with
                                            // a 4-wave LDS reduction and up to 64 * 57 atomics
constexpr int cmb_wgs(int nt) { return CMB_CUS * (nt == 2 ? 5 : 3); }

template <typename Tin, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_bwd_weight_mfma(
        const Tin* __restrict__ x, const float* __restrict__ gy, float* __restrict__ dk,
        float* __restrict__ db, MfmaGeom G, int nch, int64_t ntile, int64_t per, int gvec) {
    __shared__ float ps[CM_CC * CM_CST];                 // P chunk [c][row][col]
    __shared__ float red[16 * NOT * CMB_NS];             // the workgroup's sums [o][slot]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // consecutive logical blocks share an XCD: the chunks of one slice read the same gy
    // while it is in that XCD's L2
    unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int ci = (int)(bid % nch); bid /= nch;
    const int to = (int)(bid % G.nto);
    const int64_t sl = bid / G.nto;
    const int c0 = ci * CM_CC, o0 = to * (16 * NOT);
    const int li = lane & 15, lk = lane >> 4;            // fragment row / column, k of this lane
    const int par = wv & 1;                              // tiles start at rows r0 % 4 == 0

    // this lane's B operand per N tile: the LDS offset of pair (c, t) = slot / 7, slot % 7 at
    // this wave's row and pixel 4 lk; slots >= 56 read a valid address and are replaced
    int off[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int slot = 16 * nt + li;
        const int c = slot < 56 ? slot / 7 : 0, t = slot < 56 ? slot - 7 * c : 0;
        int dy = 0, dkk = 0;
#pragma unroll
        for (int tt = 0; tt < 7; ++tt)
            if (t == tt) { dy = G.dy[tt]; dkk = par ? G.dk[1][tt] : G.dk[0][tt]; }
        off[nt] = c * CM_CST + (wv + dy) * CM_PP + dkk + 4 * lk;
    }
    const float cst = li == 8 ? 1.f : 0.f;               // N tile 3, slots 56 (1) and 57..63 (0)

    cm_f4 acc[NOT][4];
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[ot][nt] = cm_f4{0.f, 0.f, 0.f, 0.f};

    const int64_t plane = (int64_t)G.ho * G.wo;
    const int64_t t1 = (sl + 1) * per < ntile ? (sl + 1) * per : ntile;
    for (int64_t tile = sl * per; tile < t1; ++tile) {
        const int tq = (int)(tile % G.ntq);
        const int64_t tb = tile / G.ntq;
        const int tr = (int)(tb % G.ntr);
        const int64_t b = tb / G.ntr;
        const int q0 = tq * CM_Q, r0 = tr * CM_ROWS;
        const int r = r0 + wv;                           // this wave's output row
        // lane (i, k)'s gy of column group g: 4 adjacent columns of NOT output channels,
        // zero outside the output (and for channels past O)
        const float* gr = gy + ((b * G.O + o0 + li) * G.ho + r) * (int64_t)G.wo;
        auto load_gy = [&](int g, cm_f4 (&a)[NOT]) {
            const int q = q0 + 16 * g + 4 * lk;
#pragma unroll
            for (int ot = 0; ot < NOT; ++ot) {
                a[ot] = cm_f4{0.f, 0.f, 0.f, 0.f};
                if (g < 4 && r < G.ho && o0 + 16 * ot + li < G.O && q < G.wo) {
                    const float* gp = gr + 16 * ot * plane + q;
                    if (gvec) {                          // wo % 4 == 0: all four inside
                        a[ot] = *reinterpret_cast<const cm_f4*>(gp);
                    } else {
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            if (q + m < G.wo) a[ot][m] = gp[m];
                    }
                }
            }
        };
        cm_f4 a[NOT], an[NOT];
        load_gy(0, a);                                   // in flight during the staging
        cm_stage_p(ps, x + b * (int64_t)G.C * G.h * G.w, G, c0, q0, r0, tid);
        __syncthreads();
        if (r < G.ho) {                                  // wave-uniform
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {
                const int qg = q0 + 16 * g;
                if (qg >= G.wo) break;
                const bool edge = qg + 16 > G.wo;        // wave-uniform: some pixel is outside
                const int q = qg + 4 * lk;
                load_gy(g + 1, an);                      // the next group's, during these MFMAs
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float bf[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bf[nt] = ps[off[nt] + 16 * g + m];
                    if (li >= 8) bf[3] = cst;
                    if (edge) {
                        const bool in = q + m < G.wo;
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) bf[nt] = in ? bf[nt] : 0.f;
                    }
#pragma unroll
                    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[ot][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ot][m], bf[nt], acc[ot][nt], 0, 0, 0);
                }
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) a[ot] = an[ot];
            }
        }
        __syncthreads();
    }

    // ---- the four waves' sums, added in LDS in wave order; one atomic per (o, c, t) and o ----
    // D[4 lk + v][li] is register v: row = output channel, column = slot of the N tile
#pragma unroll 1
    for (int w4 = 0; w4 < CM_THREADS / 64; ++w4) {
        if (wv == w4) {
#pragma unroll
            for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        float* const rp = red + (16 * ot + 4 * lk + v) * CMB_NS + 16 * nt + li;
                        *rp = w4 ? *rp + acc[ot][nt][v] : acc[ot][nt][v];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < 16 * NOT * 57; e += CM_THREADS) {
        const int ol = e / 57, slot = e - ol * 57;
        const int o = o0 + ol;
        if (o >= G.O) continue;
        const float s = red[ol * CMB_NS + slot];
        if (slot == 56) {
            if (db && ci == 0) atomicAdd(db + o, s);
            continue;
        }
        const int cc = slot / 7, c = c0 + cc;
        if (dk && c < G.C) atomicAdd(dk + ((int64_t)o * G.C + c) * 7 + (slot - 7 * cc), s);
    }
}

// ---- stride 2 ------------------------------------------------------------------------------
// d kernel / d bias of a stride-2 layer:
//     dW[o][c][t] = sum_{b,ro,q} gy[b,o,ro,q] * P[b,c][2 ro + dy_t][2 q + dk_t(ro & 1)]
// The GEMM, the tile walk, the gy loads, the constant-1 slot, the edge masking of both operands
// and the reduction are k_hexconv_bwd_weight_mfma's.  P is what differs: staged by the stride-2
// forward's cs_stage_p (rows 2 r0 .. 2 r0 + 8 as two column-parity planes, conv_mfma.h), so
// within a tap and row parity the 16 columns 2 q + dk of a B fragment are 16 consecutive slots,
// as at stride 1.  A chunk is CC input channels: N = 7 CC (c, t) pairs, the constant 1 and
// zeros up to CC / 2 tiles of 16.  The sums are reduced in the LDS that held P (the tile loop
// ends with a barrier), so a workgroup needs max(P, sums) only.  A sibling kernel, not a stride
// template argument: the stride-1 kernel keeps its symbol and bits.
//
// Channels per chunk, measured on 64 -> 128 1080p b4, 128 -> 256 540p b2, 16 -> 16 540p b8 and
// the 3 -> 64 1080p b4 stem (bf16 x, f32 gy, padding 1; DESIGN.md 8,
// profiles/conv_bwd_mfma_stride2_ab.txt).
constexpr int CMB_S2_CC = 4;
static_assert(CMB_S2_CC == 4 || CMB_S2_CC == 8, "chunk: 2 or 4 whole N tiles");
constexpr int CMB_S2_MIN_O = 16;            // d kernel at stride 2: output channels from which it pays
// resident workgroups per CU the grid is sized for (LDS: 20.7 KB at 4 channels, 41.5 KB at 8;
// registers: tests/test_kernel_resources_bwd_s2.py prints them)
constexpr int cmb_s2_wgs(int nt) {
    return CMB_CUS * (CMB_S2_CC == 8 ? (nt == 2 ? 3 : 2) : (nt == 2 ? 5 : 4));
}

template <typename Tin, int NOT, int CC>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_bwd_weight_mfma_s2(
        const Tin* __restrict__ x, const float* __restrict__ gy, float* __restrict__ dk,
        float* __restrict__ db, MfmaGeom G, int nch, int64_t ntile, int64_t per, int gvec) {
    constexpr int NNT = CC / 2;                          // N tiles: 7 CC pairs, the 1, zeros
    constexpr int NS = 16 * NNT;                         // N slots
    constexpr int NP = 7 * CC;                           // (c, t) pairs = the constant-1 slot
    constexpr int BL = NP - 16 * (NNT - 1);              // ... which is lane column BL of the last N tile
    constexpr int PSZ = CC * CS_CST, RSZ = 16 * NOT * NS;
    __shared__ float ps[PSZ > RSZ ? PSZ : RSZ];          // P chunk [c][row][plane][slot]; then
    float* const red = ps;                               // the workgroup's sums [o][slot]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // consecutive logical blocks share an XCD: the chunks of one slice read the same gy
    // while it is in that XCD's L2
    unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int ci = (int)(bid % nch); bid /= nch;
    const int to = (int)(bid % G.nto);
    const int64_t sl = bid / G.nto;
    const int c0 = ci * CC, o0 = to * (16 * NOT);
    const int li = lane & 15, lk = lane >> 4;            // fragment row / column, k of this lane
    const int par = wv & 1;                              // tiles start at rows r0 % 4 == 0

    // this lane's B operand per N tile: the LDS offset of pair (c, t) = slot / 7, slot % 7 at
    // this wave's staged row 2 wv + dy_t, column 2 (4 lk) + dk_t(par); slots >= NP read a valid
    // address and are replaced
    int off[NNT];
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt) {
        const int slot = 16 * nt + li;
        const int c = slot < NP ? slot / 7 : 0, t = slot < NP ? slot - 7 * c : 0;
        int dy = 0, dkk = 0;
#pragma unroll
        for (int tt = 0; tt < 7; ++tt)
            if (t == tt) { dy = G.dy[tt]; dkk = par ? G.dk[1][tt] : G.dk[0][tt]; }
        off[nt] = c * CS_CST + cm_pslot<2>(wv, dy, dkk) + 4 * lk;
    }
    const float cst = li == BL ? 1.f : 0.f;              // last N tile, slots NP (1) and above (0)

    cm_f4 acc[NOT][NNT];
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int nt = 0; nt < NNT; ++nt) acc[ot][nt] = cm_f4{0.f, 0.f, 0.f, 0.f};

    const int64_t plane = (int64_t)G.ho * G.wo;
    const int64_t t1 = (sl + 1) * per < ntile ? (sl + 1) * per : ntile;
    for (int64_t tile = sl * per; tile < t1; ++tile) {
        const int tq = (int)(tile % G.ntq);
        const int64_t tb = tile / G.ntq;
        const int tr = (int)(tb % G.ntr);
        const int64_t b = tb / G.ntr;
        const int q0 = tq * CM_Q, r0 = tr * CM_ROWS;
        const int r = r0 + wv;                           // this wave's output row
        // lane (i, k)'s gy of column group g: 4 adjacent columns of NOT output channels,
        // zero outside the output (and for channels past O)
        const float* gr = gy + ((b * G.O + o0 + li) * G.ho + r) * (int64_t)G.wo;
        auto load_gy = [&](int g, cm_f4 (&a)[NOT]) {
            const int q = q0 + 16 * g + 4 * lk;
#pragma unroll
            for (int ot = 0; ot < NOT; ++ot) {
                a[ot] = cm_f4{0.f, 0.f, 0.f, 0.f};
                if (g < 4 && r < G.ho && o0 + 16 * ot + li < G.O && q < G.wo) {
                    const float* gp = gr + 16 * ot * plane + q;
                    if (gvec) {                          // wo % 4 == 0: all four inside
                        a[ot] = *reinterpret_cast<const cm_f4*>(gp);
                    } else {
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            if (q + m < G.wo) a[ot][m] = gp[m];
                    }
                }
            }
        };
        cm_f4 a[NOT], an[NOT];
        load_gy(0, a);                                   // in flight during the staging
        cs_stage_p<CC>(ps, x + b * (int64_t)G.C * G.h * G.w, G, c0, q0, r0, tid);
        __syncthreads();
        if (r < G.ho) {                                  // wave-uniform
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {
                const int qg = q0 + 16 * g;
                if (qg >= G.wo) break;
                const bool edge = qg + 16 > G.wo;        // wave-uniform: some pixel is outside
                const int q = qg + 4 * lk;
                load_gy(g + 1, an);                      // the next group's, during these MFMAs
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float bf[NNT];
#pragma unroll
                    for (int nt = 0; nt < NNT; ++nt) bf[nt] = ps[off[nt] + 16 * g + m];
                    if (li >= BL) bf[NNT - 1] = cst;
                    if (edge) {
                        const bool in = q + m < G.wo;
#pragma unroll
                        for (int nt = 0; nt < NNT; ++nt) bf[nt] = in ? bf[nt] : 0.f;
                    }
#pragma unroll
                    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                        for (int nt = 0; nt < NNT; ++nt)
                            acc[ot][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ot][m], bf[nt], acc[ot][nt], 0, 0, 0);
                }
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) a[ot] = an[ot];
            }
        }
        __syncthreads();                                 // P is free: the next tile's, or the sums
    }

    // ---- the four waves' sums, added in LDS in wave order; one atomic per (o, c, t) and o ----
    // D[4 lk + v][li] is register v: row = output channel, column = slot of the N tile
#pragma unroll 1
    for (int w4 = 0; w4 < CM_THREADS / 64; ++w4) {
        if (wv == w4) {
#pragma unroll
            for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                for (int nt = 0; nt < NNT; ++nt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        float* const rp = red + (16 * ot + 4 * lk + v) * NS + 16 * nt + li;
                        *rp = w4 ? *rp + acc[ot][nt][v] : acc[ot][nt][v];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < 16 * NOT * (NP + 1); e += CM_THREADS) {
        const int ol = e / (NP + 1), slot = e - ol * (NP + 1);
        const int o = o0 + ol;
        if (o >= G.O) continue;
        const float s = red[ol * NS + slot];
        if (slot == NP) {
            if (db && ci == 0) atomicAdd(db + o, s);
            continue;
        }
        const int cc = slot / 7, c = c0 + cc;
        if (dk && c < G.C) atomicAdd(dk + ((int64_t)o * G.C + c) * 7 + (slot - 7 * cc), s);
    }
}

// W'[c][o][t] = W[o][c][t]: the adjoint GEMM's weights (M = C)
__global__ __launch_bounds__(256) void k_wtranspose(const float* __restrict__ kern,
                                                    float* __restrict__ wt, int C, int O) {
    const int n = C * O * 7;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int t = e % 7, co = e / 7;
        const int o = co % O, c = co / O;
        wt[e] = kern[((int64_t)o * C + c) * 7 + t];
    }
}

// Which kernel each gradient of this layer runs on (hg_conv_bwd_kernel); ho, wo from
// conv_out_shape.  A/B switch HYGRID_CONV_BWD_MFMA=0: the generic kernels.
void conv_bwd_route(int x_dtype, int w_dtype, int64_t B, int64_t C, int64_t O, int64_t h,
                    int64_t w, int64_t ho, int64_t wo, int radius, int stride, int padding,
                    int dilation, int groups, int pad_mode, int* dx_kernel, int* dw_kernel) {
    *dx_kernel = *dw_kernel = HG_CONV_BWD_GENERIC;
    if (env_is("HYGRID_CONV_BWD_MFMA", "0")) return;
    if (radius != 2 || stride != 1 || dilation != 1 || groups != 1) return;
    if (padding < 0 || padding > 2 || w_dtype != HG_F32) return;
    if (x_dtype != HG_BF16 && x_dtype != HG_F16 && x_dtype != HG_F32) return;
    if (B < 1 || C < 1 || O < 1 || h < 1 || w < 1 || ho < 1 || wo < 1) return;
    // the forward's limits, for x and (the adjoint's source) gy
    if (!conv_mfma_size_ok(C, O, h, w) || !conv_mfma_size_ok(O, C, ho, wo)) return;
    if (C * O * 7 > INT_MAX) return;
    if (O >= CMB_MIN_O) *dw_kernel = HG_CONV_BWD_MFMA;
    if (C >= CMB_MIN_C && pad_mode == HG_PAD_CONSTANT) *dx_kernel = HG_CONV_BWD_MFMA;
}

// Which kernel d kernel / d bias of this layer run on (enum hg_conv_wgrad_kernel,
// hygrid_train.h); ho, wo from conv_out_shape.  Stride 1 is conv_bwd_route's d kernel answer
// (switch HYGRID_CONV_BWD_MFMA); stride 2 has its own switch, HYGRID_CONV_BWD_MFMA_S2=0.
int conv_wgrad_route(int x_dtype, int w_dtype, int64_t B, int64_t C, int64_t O, int64_t h,
                     int64_t w, int64_t ho, int64_t wo, int radius, int stride, int padding,
                     int dilation, int groups, int pad_mode) {
    if (stride == 1) {
        int dxk, dwk;
        conv_bwd_route(x_dtype, w_dtype, B, C, O, h, w, ho, wo, radius, stride, padding, dilation,
                       groups, pad_mode, &dxk, &dwk);
        return dwk == HG_CONV_BWD_MFMA ? HG_CONV_WGRAD_MFMA : HG_CONV_WGRAD_GENERIC;
    }
    if (env_is("HYGRID_CONV_BWD_MFMA_S2", "0")) return HG_CONV_WGRAD_GENERIC;
    if (radius != 2 || stride != 2 || dilation != 1 || groups != 1) return HG_CONV_WGRAD_GENERIC;
    if (padding < 0 || padding > 2 || w_dtype != HG_F32) return HG_CONV_WGRAD_GENERIC;
    if (x_dtype != HG_BF16 && x_dtype != HG_F16 && x_dtype != HG_F32) return HG_CONV_WGRAD_GENERIC;
    if (B < 1 || C < 1 || O < CMB_S2_MIN_O || h < 1 || w < 1 || ho < 1 || wo < 1)
        return HG_CONV_WGRAD_GENERIC;
    if (!conv_mfma_size_ok(C, O, h, w) || !conv_mfma_size_ok(O, C, ho, wo)) return HG_CONV_WGRAD_GENERIC;
    if (C * O * 7 > INT_MAX) return HG_CONV_WGRAD_GENERIC;
    return HG_CONV_WGRAD_MFMA_S2;
}

// d kernel (and d bias when db) of a layer conv_bwd_route (stride 1) or conv_wgrad_route
// (stride 2) sends here; both overwritten
int conv_mfma_bwd_weight(const void* x, const float* gy, float* dk, float* db, int x_dtype,
                         int64_t B, int64_t C, int64_t O, int64_t h, int64_t w, int padding,
                         int off, int pad_mode, double pad_value, hipStream_t st, int stride) {
    MfmaGeom G = {};
    if (!conv_mfma_forward_geom(G, B, C, O, h, w, padding, off, pad_mode, pad_value, stride))
        return HG_EUNSUP;
    const int nt = G.O <= 32 ? 2 : 4;
    G.nto = (G.O + 16 * nt - 1) / (16 * nt);
    const int cc = stride == 2 ? CMB_S2_CC : CM_CC;
    const int nch = (G.C + cc - 1) / cc;
    const int64_t ntile = B * (int64_t)G.ntr * G.ntq;
    const int wgs = stride == 2 ? cmb_s2_wgs(nt) : cmb_wgs(nt);
    int64_t slices = std::max<int64_t>(1, wgs / ((int64_t)nch * G.nto));
    slices = std::min(slices, std::max<int64_t>(1, ntile / CMB_MIN_TILES));
    const int64_t per = (ntile + slices - 1) / slices;
    slices = (ntile + per - 1) / per;
    const int64_t blocks = slices * nch * G.nto;
    if (blocks > INT_MAX) return HG_EUNSUP;
    hipError_t e = hipMemsetAsync(dk, 0, sizeof(float) * (size_t)(O * C * 7), st);
    if (e != hipSuccess) return hip_status(e);
    if (db) {
        e = hipMemsetAsync(db, 0, sizeof(float) * (size_t)O, st);
        if (e != hipSuccess) return hip_status(e);
    }
    // 16-B gy loads: every row start and column group 16-B aligned
    const int gvec = (G.wo % 4) == 0 && (reinterpret_cast<uintptr_t>(gy) & 15) == 0;
    const dim3 grid((unsigned)blocks), blk(CM_THREADS);
#define HG_CW_ARGS grid, blk, 0, st, (const TI*)x, gy, dk, db, G, nch, ntile, per, gvec
#define HG_CW_LAUNCH(TI_)                                                                     \
    {                                                                                         \
        using TI = TI_;                                                                       \
        if (stride == 2 && nt == 2)                                                           \
            hipLaunchKernelGGL((k_hexconv_bwd_weight_mfma_s2<TI, 2, CMB_S2_CC>), HG_CW_ARGS); \
        else if (stride == 2)                                                                 \
            hipLaunchKernelGGL((k_hexconv_bwd_weight_mfma_s2<TI, 4, CMB_S2_CC>), HG_CW_ARGS); \
        else if (nt == 2)                                                                     \
            hipLaunchKernelGGL((k_hexconv_bwd_weight_mfma<TI, 2>), HG_CW_ARGS);               \
        else                                                                                  \
            hipLaunchKernelGGL((k_hexconv_bwd_weight_mfma<TI, 4>), HG_CW_ARGS);               \
        return launch_status();                                                               \
    }
    switch (x_dtype) {
    case HG_BF16: HG_CW_LAUNCH(__bf16)
    case HG_F16: HG_CW_LAUNCH(_Float16)
    case HG_F32: HG_CW_LAUNCH(float)
    default: return HG_EUNSUP;
    }
#undef HG_CW_LAUNCH
#undef HG_CW_ARGS
}

// d input of a layer conv_bwd_route sends here: the forward f32 kernel on the adjoint geometry
int conv_mfma_bwd_input(const float* kern, const float* gy, void* dx, int x_dtype, int64_t B,
                        int64_t C, int64_t O, int64_t h, int64_t w, int64_t ho, int64_t wo,
                        int padding, int off, hipStream_t st) {
    MfmaGeom G = {};
    G.B = B; G.C = (int)O; G.O = (int)C;                 // M = C, K = 7 O
    G.h = (int)ho; G.w = (int)wo;                        // the source raster: gy
    G.ho = (int)h; G.wo = (int)w;                        // the output raster: dx
    G.p = padding; G.pad_mode = HG_PAD_CONSTANT; G.pad_value = 0.f;
    int dy[7], dk[2][7], mink = INT_MAX, maxk = INT_MIN;
    for (int t = 0; t < 7; ++t) {
        tap_geom(2, 1, 1, (off + padding) & 1, t, &dy[t], &dk[0][t], &dk[1][t]);
        mink = std::min(mink, std::min(dk[0][t], dk[1][t]));
        maxk = std::max(maxk, std::max(dk[0][t], dk[1][t]));
    }
    if (maxk - mink + CM_Q > CM_PP) return HG_EUNSUP;
    // output row iy of parity par reads gy row iy + p - dy_t = (iy + 2 - dy_t) - (2 - p) and
    // column ix + p - dk = (ix + maxk - dk) - (maxk - p), dk of the forward row's parity
    // (iy + p + dy_t) & 1
    G.mink = 0;
    for (int t = 0; t < 7; ++t) {
        G.dy[t] = 2 - dy[t];
        for (int par = 0; par < 2; ++par) G.dk[par][t] = maxk - dk[(par + padding + dy[t]) & 1][t];
    }
    G.oy = 2 - padding; G.ox = maxk - padding;
    G.Hp = G.Wp = INT_MAX;                               // no structural zero: 0 outside gy
    G.ntq = (G.wo + CM_Q - 1) / CM_Q;
    G.ntr = (G.ho + CM_ROWS - 1) / CM_ROWS;
    const int nt = G.O <= 32 ? 2 : 4;
    G.nto = (G.O + 16 * nt - 1) / (16 * nt);
    const int n = (int)(C * O * 7);
    float* wt = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&wt), sizeof(float) * (size_t)n, st);
    if (e != hipSuccess) return hip_status(e);
    hipLaunchKernelGGL(k_wtranspose, dim3((unsigned)std::min((n + 255) / 256, 1024)), dim3(256), 0, st,
                       kern, wt, (int)C, (int)O);
    int rc = launch_status();
    if (rc == HG_OK) rc = conv_mfma_launch_f32(gy, wt, nullptr, dx, HG_F32, x_dtype, G, nt, st);
    const hipError_t fe = hipFreeAsync(wt, st);
    return rc != HG_OK ? rc : hip_status(fe);
}

}  // namespace hg
