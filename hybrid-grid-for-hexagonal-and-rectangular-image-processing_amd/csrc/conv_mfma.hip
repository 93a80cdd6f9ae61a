// conv_mfma.hip — HexConv2d for wide channel counts (HexConvModule in segmentation
// models, HexModules.py:97-288) as an implicit GEMM on the f32 matrix cores.
//
// For one output row r of image b (HexFrames.py:96-169 restated as in hexconv.hip):
//     Y[o][q] = bias[o] + sum_{c,t} W[o][c][t] * P[c][r + dy_t][q + dk_t(r & 1)]
// i.e. a GEMM with M = O (output channels), N = q (columns), K = 7 C (taps x input
// channels), where P is the padded input and a column past the padded width is the
// type1 raster's structural zero (heximage_to_type1, HexFrames.py:417-445).
//
// v_mfma_f32_16x16x4_f32 computes it exactly as an f32 fmaf chain (MI355X matrix cores
// take f32 operands at the vector rate, cdna_hip_programming.md §3), so the result has
// the reference's fp32 semantics (F.conv2d in fp32, :107, :157-160) up to summation
// order, for every input dtype (16-bit inputs are staged as their exact f32 values).
//
// Workgroup = 4 waves = 4 consecutive output rows (one per wave: its parity fixes its tap
// columns) x 32 or 64 output channels.  Per chunk of CM_CC = 8 input channels the
// workgroup stages P (6 rows x 72 columns x 8 channels, padding applied) and the
// weights (8 x 7 x 64) in LDS; each wave then runs 7 taps x 2 channel quads x
// (2-4 x 4 tiles of 16x16) MFMAs into up to 64 accumulator registers.  Fragment maps
// (MI355X_MICROARCH.md / cdna_hip_programming.md §3): A[i=o][k] from lane (k*16 + i),
// B[k][j=q] from lane (k*16 + j), D[4*(l/16)+v][l%16] in register v of lane l.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "conv_mfma.h"
#include "hexconv_geom.h"

namespace hg {

// ---- what the kernels share ----------------------------------------------------------------
// Each step below exists once; a kernel picks its variant by template integers and types only
// (NOT / NQT tiles, channels per chunk CC, the transposed-D flag TD, the P slot's stride S).
// k_hexconv_mfma_bf16, k_hexconv_mfma_s2 and k_hexconv_mfma_bf16_s2 are built from them, and
// k_wsplit_bf16 from cb_split_w.  Not shared:
//  * one-offs: the DMA issue lambdas, the two fp32 P stagers (cm_stage_p and cs_stage_p, both
//    in conv_mfma.h for the backward kernels) and the stride-2 bf16 P stager;
//  * the two MFMA loops (f32 and bf16): as force-inlined helpers they took a wave per SIMD from
//    the NOT = 2 kernels (profiles/conv_mfma_refactor_resources.txt);
//  * k_hexconv_mfma and k_hexconv_mfma_bf16d, which keep their own text throughout: built from
//    the shared steps they kept their registers and waves but ran 0.5-1.3 % slower on four
//    stride-1 shapes (profiles/conv_mfma_refactor_ab.txt).  A fix to a shared step has to be
//    made in these two as well.

// CM_TD: the MFMAs take the P fragment as A and the weights as B, so D is [column][channel]:
// a lane's 4 registers are 4 adjacent output columns of one channel (one 8-B store for
// 16-bit outputs instead of four 2-B stores); the same products summed in the same order.
// 16-bit outputs only (fp32 outputs as two 8-B stores: 3.9 % slower than 2-B stores,
// profiles/r06/conv_mfma_transposed_d_ab.txt).  k_hexconv_mfma_bf16 (the A/B fallback of the
// DMA kernel) never had the path and passes TD = false.
constexpr bool CM_TD = true;
template <typename Tout>
constexpr bool cm_td = CM_TD && sizeof(Tout) == 2;

constexpr int CM_NQT = CM_Q / 16;           // 16-column tiles per workgroup

typedef __bf16 cm_b8 __attribute__((ext_vector_type(8)));
typedef unsigned cm_u4 __attribute__((ext_vector_type(4)));
// The bf16 kernels' weight-fragment LDS layout: channel o's four k-group fragments (16 B each)
// in a rotated order, so each of ds_read_b128's four 16-lane groups ({0-3,12-15,20-27},
// {4-11,16-19,28-31}, and the same + 32: MI355X_MICROARCH.md section LDS) reads 16 distinct
// 16-B bank slots; the plain order o * 4 + g put lanes li and li + 12 (and li + 4, li + 8) of a
// group on one slot (2-way conflicts; r04 session O counters: 39 % of the LDS cycles).
__host__ __device__ constexpr int cd_wslot(int o, int g) { return (g + 2 * ((o & 15) >> 2)) & 3; }

constexpr int CB_PP = CM_PP;                // staged columns: cm_pslot<1> serves both P layouts
constexpr int CB_PSZ = CM_PR * CB_PP + 1;   // P fragments per chunk (+1: the zero fragment)
constexpr int CSB_PSZ = CS_PR * CS_PP + 1;  // ... at stride 2

// Input channels per LDS chunk of k_hexconv_mfma_s2: 4 (20.7 KB of P + 7.4 KB of weights = 28.2 KB,
// 3-4 waves per SIMD) against 8 (56.3 KB, 2 workgroups per CU): 4.55 against 5.90 ms on
// 64 -> 128 1080p b4 f32, 0.264 / 0.397 ms on the 3 -> 64 stem, 0.230 / 0.346 ms on 16 -> 16
// 540p b8, 2.40 / 3.07 ms on 128 -> 256 540p b2 (profiles/conv_mfma_stride2_ab.txt): as at
// stride 1, occupancy, not barrier count, is what the staging latency needs.
constexpr int CS_CC = 4;
static_assert(CS_CC % 4 == 0 && CS_CC <= CM_CC, "chunk: whole MFMA k quads, the weight stride's rows");

// Which tile of which image a workgroup computes, and this lane's place in the fragments.
template <int NOT>
struct CmBlock {
    int tid, wv;                // thread; wave = row of the tile (uniform)
    int64_t b;                  // image
    int q0, r0, o0;             // first output column / row / channel of the tile
    int r, par;                 // this wave's output row and its parity
    int li, lk;                 // fragment row (or column), k group of this lane
    __device__ __forceinline__ explicit CmBlock(const MfmaGeom& G) {
        tid = threadIdx.x;
        wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
        const int tq = (int)(bid % G.ntq); bid /= G.ntq;
        const int tr = (int)(bid % G.ntr); bid /= G.ntr;
        const int to = (int)(bid % G.nto);
        b = bid / G.nto;
        q0 = tq * CM_Q; r0 = tr * CM_ROWS; o0 = to * (16 * NOT);
        r = r0 + wv;
        par = r & 1;
        const int lane = tid & 63;
        li = lane & 15; lk = lane >> 4;
    }
};

// The accumulators start at the bias.  Plain D: register v of lane (li, lk) is channel
// 4 lk + v of the tile; TD: D is [column][channel], every register is channel li.
template <bool TD, int NOT, int NQT>
__device__ __forceinline__ void cm_bias_init(cm_f4 (&acc)[NOT][NQT], const float* __restrict__ bias,
                                             const MfmaGeom& G, int o0, int li, int lk) {
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + (TD ? li : lk * 4 + v);
            const float bv = (bias && o < G.O) ? bias[o] : 0.f;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) acc[ot][qt][v] = bv;
        }
    }
}

// 8 x u16 -> one 16-B fragment, element 0 lowest
__device__ __forceinline__ cm_u4 cb_pack(const unsigned short (&u)[8]) {
    return cm_u4{u[0] | ((unsigned)u[1] << 16), u[2] | ((unsigned)u[3] << 16),
                 u[4] | ((unsigned)u[5] << 16), u[6] | ((unsigned)u[7] << 16)};
}

// f32 weights W[o0 .. o0+16 NOT-1][c0 .. c0+CC-1][t] -> ws as [c][t][o].  Per output channel
// the chunk's CC x 7 weights are contiguous: CC * 7 / 4 float4 loads when the chunk is whole and
// 16-B aligned, scalar loads (0 past C) otherwise.
template <int CC, int NOT>
__device__ __forceinline__ void cm_stage_w(float* __restrict__ ws, const float* __restrict__ kern,
                                           const MfmaGeom& G, int c0, int o0, int tid) {
    constexpr int CM_O = 16 * NOT, F4 = CC * 7 / 4;
    for (int e = tid; e < CM_O * F4; e += CM_THREADS) {
        const int o = e / F4, f = e - o * F4;
        const int og = o0 + o;
        float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const int64_t base = ((int64_t)og * G.C + c0) * 7 + 4 * f;   // first of 4 (c, t)
        if (og < G.O) {
            if (c0 + CC <= G.C && (base & 3) == 0) {
                v4 = *reinterpret_cast<const float4*>(kern + base);
            } else {
                float tmp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ct = 4 * f + j, c = c0 + ct / 7;
                    tmp[j] = c < G.C ? kern[((int64_t)og * G.C + c) * 7 + ct % 7] : 0.f;
                }
                v4 = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
            }
        }
        const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ct = 4 * f + j, cc = ct / 7, t = ct - cc * 7;
            ws[cc * CM_WST + t * CM_O + o] = vv[j];
        }
    }
}

// bf16 weight split: the weights of (output channel og, tap t; t = 7: zeros) for the 8 input
// channels from c0 as w = h + m + l in bf16, stored as the three fragments of slot (o, t) of a
// [part][kb][o][g] block with `ostride` channels per (part, kb).  Returns nonzero when some m / l
// part is (+-0 is zero): when none of a chunk is, the MFMA loop skips parts 2 and 3: half the MFMA
// work for bf16-exact weights, and an infinite input times a weight then stays +-Inf as in one
// fp32 product instead of meeting a zero part as Inf * 0 = NaN.
__device__ __forceinline__ int cb_split_w(const float* __restrict__ kern, int C, int O, int og, int c0,
                                          int t, cm_u4* __restrict__ dst, int ostride, int o) {
    unsigned short h[8], m[8], l[8];
    int ml = 0;
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
        const int c = c0 + cc;
        const float wf = (t < 7 && og < O && c < C) ? kern[((int64_t)og * C + c) * 7 + t] : 0.f;
        const __bf16 bh = (__bf16)wf;
        const float r1 = wf - (float)bh;
        const __bf16 bm = (__bf16)r1;
        const __bf16 bl = (__bf16)(r1 - (float)bm);
        h[cc] = __builtin_bit_cast(unsigned short, bh);
        m[cc] = __builtin_bit_cast(unsigned short, bm);
        l[cc] = __builtin_bit_cast(unsigned short, bl);
        ml |= (m[cc] | l[cc]) & 0x7fff;
    }
    const int kb = t >> 2, g = t & 3;
    dst[((0 * 2 + kb) * ostride + o) * 4 + cd_wslot(o, g)] = cb_pack(h);
    dst[((1 * 2 + kb) * ostride + o) * 4 + cd_wslot(o, g)] = cb_pack(m);
    dst[((2 * 2 + kb) * ostride + o) * 4 + cd_wslot(o, g)] = cb_pack(l);
    return ml;
}

// A workgroup's weight chunk split in the kernel (the register-staged bf16 kernels): thread
// (o, t) as above into wsb; 3 when the chunk needs all three parts, else 1 (uniform; barrier).
template <int NOT>
__device__ __forceinline__ int cb_stage_w(cm_u4* __restrict__ wsb, const float* __restrict__ kern,
                                          const MfmaGeom& G, int c0, int o0, int tid) {
    constexpr int CM_O = 16 * NOT;
    int ml = 0;
    for (int e = tid; e < CM_O * 8; e += CM_THREADS) {
        const int o = e >> 3, t = e & 7;
        ml |= cb_split_w(kern, G.C, G.O, o0 + o, c0, t, wsb, CM_O, o);
    }
    return __syncthreads_or(ml != 0) ? 3 : 1;
}

// bf16 P at stride 1, through registers: rows r0 .. r0+5, columns q0 + mink + (0..71) of the 8
// channels from c0 as [row][col] fragments (channel innermost), cm_stage_p's padding rules and
// structural zero column.  216 threads = 72 columns x 3 row phases, two rows each.
__device__ __forceinline__ void cb_stage_p(cm_u4* __restrict__ psb, const unsigned short* __restrict__ xb,
                                           const MfmaGeom& G, int c0, int q0, int r0, int tid) {
    if (tid < 3 * CB_PP) {
        const unsigned short padv = __builtin_bit_cast(unsigned short, (__bf16)G.pad_value);
        const int pc = tid % CB_PP, ph = tid / CB_PP;
        const int px = q0 + G.mink + pc;
        const bool zc = px >= G.Wp;                      // type1 structural zero column
        const int64_t xi = zc ? -1 : pad_map(px - G.p, G.w, G.pad_mode);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int pr = ph + 3 * k, py = r0 + pr;
            const int64_t yi = (!zc && py < G.Hp) ? pad_map(py - G.p, G.h, G.pad_mode) : -1;
            unsigned short v[8];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const int c = c0 + cc;
                unsigned short e = 0;
                if (!zc && c < G.C && py < G.Hp)
                    e = (yi < 0 || xi < 0) ? padv : xb[((int64_t)c * G.h + yi) * G.w + xi];
                v[cc] = e;
            }
            psb[pr * CB_PP + pc] = cb_pack(v);
        }
    }
}

// This lane's P fragment per k block: tap t = 4 kb + lk at its cm_pslot, fragment column li;
// the 8th tap slot (-1) reads the zero fragment.
template <int S>
__device__ __forceinline__ void cb_pidx(int (&pidx)[2], const MfmaGeom& G, int wv, int par, int li, int lk) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int t = 4 * kb + lk;
        pidx[kb] = t < 7 ? cm_pslot<S>(wv, G.dy[t], par ? G.dk[1][t] : G.dk[0][t]) + li : -1;
    }
}

// CM_TD epilogue (16-bit outputs): lane (li, lk) holds output channel oc + 16 ot, columns
// q + 16 qt .. + 3 in its 4 registers: one 8-B store per (ot, qt) when every row's start keeps
// q % 4 == 0 aligned (wo % 4 == 0); scalar stores otherwise
template <typename Tout, int NOT, int NQT>
__device__ __forceinline__ void cm_store_cols(const cm_f4 (&acc)[NOT][NQT], Tout* yb, const MfmaGeom& G,
                                              int oc, int q, int r) {
    const bool vec = (G.wo & 3) == 0;
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot) {
        const int o = oc + ot * 16;
        if (o >= G.O) continue;
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            const int qq = q + qt * 16;
            if (qq >= G.wo) continue;
            float val[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                val[v] = acc[ot][qt][v];
                if (G.epi.on) val[v] = epi_apply(val[v], o, G.epi);
            }
            Tout* const dst = yb + ((int64_t)o * G.ho + r) * G.wo + qq;
            if (vec && sizeof(Tout) == 2) {
                typedef Tout t4v __attribute__((ext_vector_type(4)));
                *reinterpret_cast<t4v*>(dst) = t4v{(Tout)val[0], (Tout)val[1], (Tout)val[2], (Tout)val[3]};
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (qq + v < G.wo) dst[v] = (Tout)val[v];
            }
        }
    }
}

// Epilogue: bias was the accumulator's start; BN / activation (epi_apply); bounds; cast; store.
// Plain D: one store per register; TD: cm_store_cols.
template <bool TD, typename Tout, int NOT, int NQT>
__device__ __forceinline__ void cm_store(const cm_f4 (&acc)[NOT][NQT], Tout* __restrict__ y,
                                         const MfmaGeom& G, const CmBlock<NOT>& K) {
    if (K.r >= G.ho) return;
    Tout* yb = y + K.b * (int64_t)G.O * G.ho * G.wo;
    if constexpr (TD) {
        cm_store_cols<Tout, NOT, NQT>(acc, yb, G, K.o0 + K.li, K.q0 + K.lk * 4, K.r);
        return;
    }
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = K.o0 + ot * 16 + K.lk * 4 + v;
            if (o >= G.O) continue;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                const int q = K.q0 + qt * 16 + K.li;
                if (q >= G.wo) continue;
                float val = acc[ot][qt][v];
                if (G.epi.on) val = epi_apply(val, o, G.epi);
                yb[((int64_t)o * G.ho + K.r) * G.wo + q] = (Tout)val;
            }
        }
}

// ---- the kernels ------------------------------------------------------------------------------

// The parent text, not the shared steps: with them the NOT = 2 instantiations ran 0.5-0.6 % slower
// (profiles/conv_mfma_refactor_ab.txt)
template <typename Tin, typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_mfma(const Tin* __restrict__ x,
                                                                const float* __restrict__ kern,
                                                                const float* __restrict__ bias,
                                                                Tout* __restrict__ y, MfmaGeom G) {
    __shared__ float ps[CM_CC * CM_CST];                 // P chunk [c][row][col]
    __shared__ float ws[CM_CC * CM_WST];                 // weight chunk [c][t][o]
    constexpr int CM_O = 16 * NOT;                       // output channels of this workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tq = (int)(bid % G.ntq); bid /= G.ntq;
    const int tr = (int)(bid % G.ntr); bid /= G.ntr;
    const int to = (int)(bid % G.nto);
    const int64_t b = bid / G.nto;
    const int q0 = tq * CM_Q, r0 = tr * CM_ROWS, o0 = to * (16 * NOT);
    const int r = r0 + wv;                               // this wave's output row
    const int par = r & 1;
    const int li = lane & 15, lk = lane >> 4;            // fragment row / k of this lane

    // 16-bit outputs only (fp32 outputs as two 8-B stores: 3.9 % slower than 2-B stores,
    // profiles/r06/conv_mfma_transposed_d_ab.txt)
    constexpr bool TD = CM_TD && sizeof(Tout) == 2;
    cm_f4 acc[NOT][4];
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + (TD ? li : lk * 4 + v);   // TD: D is [column][channel]
            const float bv = (bias && o < G.O) ? bias[o] : 0.f;
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) acc[ot][qt][v] = bv;
        }
    }

    const Tin* xb = x + b * (int64_t)G.C * G.h * G.w;
    for (int c0 = 0; c0 < G.C; c0 += CM_CC) {
        // ---- stage P rows r0 .. r0+5 (padded frame), columns q0 + mink + (0..71) ---------
        cm_stage_p(ps, xb, G, c0, q0, r0, tid);
        // ---- stage weights W[o0 .. o0+63][c0 .. c0+CM_CC-1][t] as [c][t][o] --------------
        // per output channel the chunk's CM_CC x 7 = 56 weights are contiguous: 14 float4 loads
        for (int e = tid; e < CM_O * (CM_CC * 7 / 4); e += CM_THREADS) {
            const int o = e / (CM_CC * 7 / 4), f = e - o * (CM_CC * 7 / 4);
            const int og = o0 + o;
            float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const int64_t base = ((int64_t)og * G.C + c0) * 7 + 4 * f;   // first of 4 (c, t)
            if (og < G.O) {
                if (c0 + CM_CC <= G.C && (base & 3) == 0) {
                    v4 = *reinterpret_cast<const float4*>(kern + base);
                } else {
                    float tmp[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int ct = 4 * f + j, c = c0 + ct / 7;
                        tmp[j] = c < G.C ? kern[((int64_t)og * G.C + c) * 7 + ct % 7] : 0.f;
                    }
                    v4 = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
                }
            }
            const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ct = 4 * f + j, cc = ct / 7, t = ct - cc * 7;
                ws[cc * CM_WST + t * CM_O + o] = vv[j];
            }
        }
        __syncthreads();
        // ---- 7 taps x 4 channel quads x 16 MFMAs --------------------------------------
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int dy = G.dy[t], dk = par ? G.dk[1][t] : G.dk[0][t];
            const float* pb = ps + lk * CM_CST + (wv + dy) * CM_PP + dk + li;
            const float* wb = ws + lk * CM_WST + t * CM_O + li;
#pragma unroll
            for (int cq = 0; cq < CM_CC / 4; ++cq) {
                float af[NOT], bf[4];
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) af[ot] = wb[cq * 4 * CM_WST + ot * 16];
#pragma unroll
                for (int qt = 0; qt < 4; ++qt) bf[qt] = pb[cq * 4 * CM_CST + qt * 16];
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt)
                        acc[ot][qt] = TD ? __builtin_amdgcn_mfma_f32_16x16x4f32(bf[qt], af[ot], acc[ot][qt], 0, 0, 0)
                                            : __builtin_amdgcn_mfma_f32_16x16x4f32(af[ot], bf[qt], acc[ot][qt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: bias was the accumulator's start; BN / activation; store -------------
    if (r >= G.ho) return;
    Tout* yb = y + b * (int64_t)G.O * G.ho * G.wo;
    if constexpr (TD) {
        cm_store_cols<Tout, NOT, 4>(acc, yb, G, o0 + li, q0 + lk * 4, r);
        return;
    }
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + lk * 4 + v;
            if (o >= G.O) continue;
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                const int q = q0 + qt * 16 + li;
                if (q >= G.wo) continue;
                float val = acc[ot][qt][v];
                if (G.epi.on) val = epi_apply(val, o, G.epi);
                yb[((int64_t)o * G.ho + r) * G.wo + q] = (Tout)val;
            }
        }
}

// bf16 inputs, register staging (the DMA kernel's fallback: odd widths, unaligned sources,
// HYGRID_CONV_DMA=0, and its reference in the tests).  P chunk: [row][col] fragments of the 8
// channels (16 B each, channel innermost); weights: [part][kb][o][g] fragments of the 8 channels
// of tap 4 kb + g.  Plain D only (TD = false).
template <typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_mfma_bf16(const __bf16* __restrict__ x,
                                                                  const float* __restrict__ kern,
                                                                  const float* __restrict__ bias,
                                                                  Tout* __restrict__ y, MfmaGeom G) {
    __shared__ cm_u4 psb[CB_PSZ];
    __shared__ cm_u4 wsb[3 * 2 * 16 * NOT * 4];
    const CmBlock<NOT> K(G);
    cm_f4 acc[NOT][CM_NQT];
    cm_bias_init<false>(acc, bias, G, K.o0, K.li, K.lk);
    if (K.tid == 0) psb[CB_PSZ - 1] = cm_u4{0u, 0u, 0u, 0u};
    int pidx[2];
    cb_pidx<1>(pidx, G, K.wv, K.par, K.li, K.lk);

    const unsigned short* xb = reinterpret_cast<const unsigned short*>(x) + K.b * (int64_t)G.C * G.h * G.w;
    for (int c0 = 0; c0 < G.C; c0 += CM_CC) {
        cb_stage_p(psb, xb, G, c0, K.q0, K.r0, K.tid);
        const int nparts = cb_stage_w<NOT>(wsb, kern, G, c0, K.o0, K.tid);   // barrier inside
        // ---- 2 k blocks x 4 column tiles x nparts weight parts x NOT channel tiles ---------
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            cm_b8 bf[CM_NQT];
#pragma unroll
            for (int qt = 0; qt < CM_NQT; ++qt)
                bf[qt] = __builtin_bit_cast(cm_b8, psb[pidx[kb] < 0 ? CB_PSZ - 1 : pidx[kb] + qt * 16]);
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                if (pt >= nparts) break;
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) {
                    const cm_b8 af = __builtin_bit_cast(cm_b8, wsb[((pt * 2 + kb) * (16 * NOT) + ot * 16 + K.li) * 4 + cd_wslot(K.li, K.lk)]);
#pragma unroll
                    for (int qt = 0; qt < CM_NQT; ++qt)
                        acc[ot][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[qt], acc[ot][qt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    cm_store<false>(acc, y, G, K);
}


// ---- bf16 inputs, staging by LDS-DMA (round 4) -------------------------------------------
// The same GEMM and fragment maps as k_hexconv_mfma_bf16, with the staging taken off the
// critical path: (1) the three bf16 weight parts are split once per call by k_wsplit_bf16
// into a stream-ordered scratch buffer already in the LDS fragment layout, so a workgroup's
// weight chunk is a plain 1-KiB-piece LDS-DMA copy (double-buffered: chunk i + 1 lands while
// chunk i's MFMAs run); (2) P's rows arrive by LDS-DMA in their natural [channel][row][col]
// order (one dword per lane, 40 lanes = 80 columns per piece), also one chunk ahead, and a
// short LDS -> LDS pass packs them channel-innermost for the ds_read_b128 B fragments.  No
// staging value passes through VGPRs, so the prefetch costs no occupancy (the register
// prefetch of round 3 did: 2 waves per SIMD, 27 % slower).  Workgroups whose P tile needs
// padding or the type1 structural zero column keep the register staging for P.
constexpr int CD_PRW = 40;                    // raw P row: 40 dwords = 80 columns (>= 72 + 1)
constexpr int CD_PRAW = CM_CC * CM_PR * CD_PRW;   // dwords of one raw P chunk

// one block per (chunk of 8 input channels, 16 output channels); thread (o, t) splits the
// 8 channels' weights of tap t (t = 7: zeros) into h + m + l and stores the three fragments;
// flag[chunk][o / 16] = some m / l part is nonzero (else the MFMA kernel skips parts 2, 3)
__global__ __launch_bounds__(128) void k_wsplit_bf16(const float* __restrict__ kern, cm_u4* __restrict__ wf,
                                                     int* __restrict__ flag, int C, int O, int Opad) {
    const int ci = blockIdx.x, ob = blockIdx.y;
    const int o = ob * 16 + (threadIdx.x >> 3), t = threadIdx.x & 7;
    const int ml = cb_split_w(kern, C, O, o, ci * 8, t, wf + (int64_t)ci * 6 * Opad * 4, Opad, o);
    const int any = __syncthreads_or(ml != 0);
    if (threadIdx.x == 0) flag[ci * (Opad / 16) + ob] = any;
}

template <int N>
__device__ __forceinline__ void cd_wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((0x0f70 & ~0xf) | (N & 0xf) | ((N >> 4) << 14));
}

// Weight chunks are single-buffered: the DMA of chunk i + 1 is issued once chunk i's MFMAs are
// done and waited for at the top of the next chunk (47 KB of LDS -> 3 workgroups per CU, whose
// MFMAs cover each other's waits; double-buffered, 71 KB and 2 workgroups per CU, was 18 %
// slower, and 3 column tiles with one raw-P buffer for a 4th wave per SIMD 4 % slower: both
// removed in round 6).  The raw P rows are double-buffered.
// (its own text, not the shared steps: with them it ran 0.7-1.3 % slower on 32 -> 32 and 64 -> 64,
// profiles/conv_mfma_refactor_ab.txt)
template <typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) __attribute__((amdgpu_waves_per_eu(1)))
void k_hexconv_mfma_bf16d(const __bf16* __restrict__ x,
                                                                   const cm_u4* __restrict__ wf,
                                                                   const int* __restrict__ flag,
                                                                   const float* __restrict__ bias,
                                                                   Tout* __restrict__ y, MfmaGeom G,
                                                                   int Opad) {
    constexpr int CM_O = 16 * NOT;
    constexpr int WSZ = 3 * 2 * CM_O * 4;                // weight fragments of one chunk
    constexpr int WPC = WSZ / 64;                         // their 1-KiB pieces
    constexpr int WPW = WPC / 4;                          // ... per wave
    constexpr int PPW = CM_CC * CM_PR / 4;                // raw P row pieces per wave (12)
    static_assert(WPC % 4 == 0, "pieces");
    // one LDS array (so the DMA's M0 bases come from it): [psb | wsb x 2 | praw x 2]
    constexpr int NQT = 4;                                // 16-column tiles per workgroup
    constexpr int LPSB = CB_PSZ * 16, LWSB = WSZ * 16, LPRAW = CD_PRAW * 4, NWB = 1;
    constexpr int NPB = 2;                                // raw P buffers
    constexpr int TQ = 16 * NQT;                          // output columns of this workgroup
    __shared__ __attribute__((aligned(16))) unsigned char lds[LPSB + NWB * LWSB + NPB * LPRAW];
    cm_u4* const psb = reinterpret_cast<cm_u4*>(lds);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tq = (int)(bid % G.ntq); bid /= G.ntq;
    const int tr = (int)(bid % G.ntr); bid /= G.ntr;
    const int to = (int)(bid % G.nto);
    const int64_t b = bid / G.nto;
    const int q0 = tq * TQ, r0 = tr * CM_ROWS, o0 = to * CM_O;
    const int r = r0 + wv;
    const int par = r & 1;
    const int Wp = G.w + 2 * G.p, Hp = G.h + 2 * G.p;
    const int li = lane & 15, lg = lane >> 4;
    const unsigned short padv = __builtin_bit_cast(unsigned short, (__bf16)G.pad_value);
    const int nch = (G.C + CM_CC - 1) / CM_CC;
    // this tile's P is all inside the image (no padding, no structural zero): DMA staging
    const int px0 = q0 + G.mink - G.p;                    // first staged source column
    const bool interior = r0 - G.p >= 0 && r0 + CM_PR - 1 - G.p < G.h && px0 >= 0 &&
                          px0 + CB_PP - 1 < G.w && q0 + G.mink + CB_PP - 1 < Wp;
    const int xs = px0 & ~1, sh = px0 - xs;               // dword-aligned raw start, shift

    // CM_TD: the MFMAs take the P fragment as A and the weights as B, so D is [column][channel]:
    // a lane's 4 registers are 4 adjacent output columns of one channel (one 8-B store for
    // 16-bit outputs instead of four 2-B stores); the same products summed in the same order
    // 16-bit outputs only (fp32 outputs as two 8-B stores: 3.9 % slower than 2-B stores,
    // profiles/r06/conv_mfma_transposed_d_ab.txt)
    constexpr bool TD = CM_TD && sizeof(Tout) == 2;
    cm_f4 acc[NOT][NQT];
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + (TD ? li : lg * 4 + v);
            const float bv = (bias && o < G.O) ? bias[o] : 0.f;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) acc[ot][qt][v] = bv;
        }
    }
    if (tid == 0) psb[CB_PSZ - 1] = cm_u4{0u, 0u, 0u, 0u};
    int pidx[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int t = 4 * kb + lg;
        pidx[kb] = t < 7 ? (wv + G.dy[t]) * CB_PP + li + (par ? G.dk[1][t] : G.dk[0][t]) : -1;
    }
    const unsigned short* xb = reinterpret_cast<const unsigned short*>(x) + b * (int64_t)G.C * G.h * G.w;
    // buffer views: the image's planes (rows of channels >= C read past the range: zeros),
    // the weight fragments
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)xb, (short)0, (int)((int64_t)G.C * G.h * G.w * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)wf, (short)0, 0x7fffffff, 0x00020000);

    // the DMA address terms are recomputed at every chunk from values the compiler cannot see
    // through (no hoisting: the hoisted per-piece offsets spilled 57-73 SGPRs, round 5)
    auto opq = [](int v) {
        asm volatile("" : "+s"(v));
        return v;
    };
    auto dma_w = [&](int ci) {                            // chunk ci's weights -> the buffer
        const int wvo = opq(wv);
        // weights: pieces j = wv * WPW + i of the chunk's (pt, kb) blocks of CM_O * 4 fragments
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int j = wvo * WPW + i;
            const int blk = j / (CM_O / 16), part = j % (CM_O / 16);   // (pt * 2 + kb), 1-KiB part
            const unsigned so = (unsigned)((((int64_t)ci * 6 + blk) * Opad + o0) * 64 + part * 1024);
            const unsigned lda = lds0 + LPSB + (blk * CM_O * 4) * 16 + part * 1024;
            const unsigned vo = lane * 16u;
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                         "buffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(vo), "s"(wr), "s"(lda), "s"(so) : "memory");
        }
    };
    auto dma_p = [&](int ci) {                            // chunk ci's raw P rows -> buffer (ci & 1)
        const int buf = ci & 1;
        if (interior) {
            const int wvo = opq(wv), ho = opq(G.h), wo = opq(G.w);
            // P rows: pieces j = wv * PPW + i = (cc, pr); lanes 0-39 one dword each
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                const int j = wvo * PPW + i;
                const int cc = j / CM_PR, pr = j % CM_PR;
                const int c = ci * CM_CC + cc;
                const unsigned so = c < G.C ? (unsigned)((((int64_t)c * ho + (r0 + pr - G.p)) * wo + xs) * 2)
                                            : 0x80000000u;
                const unsigned lda = lds0 + LPSB + NWB * LWSB + buf * LPRAW + j * CD_PRW * 4;
                const unsigned vo = lane * 4u;
                unsigned keep;
                if (lane < CD_PRW)
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                                 "buffer_load_dword %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(vo), "s"(xr), "s"(lda), "s"(so) : "memory");
                else
                    asm volatile("" ::: "memory");
            }
        }
    };
    // every wave issues the same number of DMA instructions per chunk (counted waits)
    constexpr int NP_ = PPW;

    dma_w(0);
    dma_p(0);
    for (int ci = 0; ci < nch; ++ci) {
        const int buf = ci & 1;
        const int c0 = ci * CM_CC;
        // chunk ci's pieces are done once at most the ones issued after them are outstanding
        // (vmcnt counts them in issue order): only P(ci+1) (W(ci) was issued at the end of
        // chunk ci-1, before P(ci+1))
        if (ci + 1 < nch) {
            dma_p(ci + 1);
            if (interior) cd_wait_vm<NP_>(); else cd_wait_vm<0>();
        } else {
            cd_wait_vm<0>();
        }
        // ---- P chunk -> psb (channel-innermost fragments) -------------------------------
        if (interior) {
            __builtin_amdgcn_s_barrier();                 // every wave's raw rows have landed
            const unsigned short* raw = reinterpret_cast<const unsigned short*>(lds + LPSB + NWB * LWSB + buf * LPRAW);
            for (int f = tid; f < CM_PR * CB_PP; f += CM_THREADS) {
                const int pr = f / CB_PP, pc = f - pr * CB_PP;
                unsigned short v[8];
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) v[cc] = raw[(cc * CM_PR + pr) * (2 * CD_PRW) + pc + sh];
                psb[f] = cm_u4{v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16),
                               v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16)};
            }
        }
        if (!interior && tid < 3 * CB_PP) {               // the register staging (padding rules)
            const int pc = tid % CB_PP, ph = tid / CB_PP;
            const int px = q0 + G.mink + pc;
            const bool zc = px >= Wp;
            const int64_t xi = zc ? -1 : pad_map(px - G.p, G.w, G.pad_mode);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int pr = ph + 3 * k, py = r0 + pr;
                const int64_t yi = (!zc && py < Hp) ? pad_map(py - G.p, G.h, G.pad_mode) : -1;
                unsigned short v[8];
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) {
                    const int c = c0 + cc;
                    unsigned short e = 0;
                    if (!zc && c < G.C && py < Hp)
                        e = (yi < 0 || xi < 0) ? padv : xb[((int64_t)c * G.h + yi) * G.w + xi];
                    v[cc] = e;
                }
                psb[pr * CB_PP + pc] = cm_u4{v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16),
                                             v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16)};
            }
        }
        int nparts = 1;
#pragma unroll
        for (int ot = 0; ot < NOT; ++ot) nparts |= flag[ci * (Opad / 16) + o0 / 16 + ot] ? 3 : 1;
        __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): this wave's LDS writes
        __builtin_amdgcn_s_barrier();                     // psb and the weights complete
        // ---- 2 k blocks x NQT column tiles x 3 weight parts x NOT channel tiles -----------
        const cm_u4* const wsb = reinterpret_cast<const cm_u4*>(lds + LPSB);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            cm_b8 bf[NQT];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
                bf[qt] = __builtin_bit_cast(cm_b8, psb[pidx[kb] < 0 ? CB_PSZ - 1 : pidx[kb] + qt * 16]);
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                if (pt >= nparts) break;
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) {
                    const cm_b8 af = __builtin_bit_cast(cm_b8, wsb[((pt * 2 + kb) * CM_O + ot * 16 + li) * 4 + cd_wslot(li, lg)]);
#pragma unroll
                    for (int qt = 0; qt < NQT; ++qt)
                        acc[ot][qt] = TD ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[qt], af, acc[ot][qt], 0, 0, 0)
                                            : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[qt], acc[ot][qt], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();                     // psb / this buffer free again
        if (ci + 1 < nch) dma_w(ci + 1);                  // the single weight buffer is free
    }

    if (r >= G.ho) return;
    Tout* yb = y + b * (int64_t)G.O * G.ho * G.wo;
    if constexpr (TD) {
        cm_store_cols<Tout, NOT, NQT>(acc, yb, G, o0 + li, q0 + lg * 4, r);
        return;
    }
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = o0 + ot * 16 + lg * 4 + v;
            if (o >= G.O) continue;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                const int q = q0 + qt * 16 + li;
                if (q >= G.wo) continue;
                float val = acc[ot][qt][v];
                if (G.epi.on) val = epi_apply(val, o, G.epi);
                yb[((int64_t)o * G.ho + r) * G.wo + q] = (Tout)val;
            }
        }
}

// ---- stride 2 ------------------------------------------------------------------------------
// The same GEMMs on a tile that walks the input at twice the output pitch: wave wv's output
// row r0 + wv reads staged rows 2 wv + dy_t, output column q reads staged column 2 (q - q0) +
// dk_t.  Rows are staged as two column-parity planes (conv_mfma.h), so a tap's B fragment is
// 16 consecutive LDS slots of plane dk & 1 starting at slot (dk >> 1) + li, and the fragment
// maps, the weight layouts, the accumulators and the epilogues are the stride-1 kernels'.
// Sibling kernels, not a stride template argument: the stride-1 kernels keep their symbols.

// P is staged by cs_stage_p (conv_mfma.h) in chunks of CS_CC channels.
template <typename Tin, typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_mfma_s2(const Tin* __restrict__ x,
                                                                   const float* __restrict__ kern,
                                                                   const float* __restrict__ bias,
                                                                   Tout* __restrict__ y, MfmaGeom G) {
    __shared__ float ps[CS_CC * CS_CST];                 // P chunk [c][row][plane][slot]
    __shared__ float ws[CS_CC * CM_WST];                 // weight chunk [c][t][o]
    constexpr bool TD = cm_td<Tout>;
    const CmBlock<NOT> K(G);
    cm_f4 acc[NOT][CM_NQT];
    cm_bias_init<TD>(acc, bias, G, K.o0, K.li, K.lk);

    const Tin* xb = x + K.b * (int64_t)G.C * G.h * G.w;
    for (int c0 = 0; c0 < G.C; c0 += CS_CC) {
        cs_stage_p<CS_CC>(ps, xb, G, c0, K.q0, K.r0, K.tid);
        cm_stage_w<CS_CC, NOT>(ws, kern, G, c0, K.o0, K.tid);
        __syncthreads();
        // ---- 7 taps x CS_CC / 4 channel quads x (NOT x 4) MFMAs ---------------------------
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int dk = K.par ? G.dk[1][t] : G.dk[0][t];
            const float* pb = ps + K.lk * CS_CST + cm_pslot<2>(K.wv, G.dy[t], dk) + K.li;
            const float* wb = ws + K.lk * CM_WST + t * (16 * NOT) + K.li;
#pragma unroll
            for (int cq = 0; cq < CS_CC / 4; ++cq) {
                float af[NOT], bf[CM_NQT];
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) af[ot] = wb[cq * 4 * CM_WST + ot * 16];
#pragma unroll
                for (int qt = 0; qt < CM_NQT; ++qt) bf[qt] = pb[cq * 4 * CS_CST + qt * 16];
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
                    for (int qt = 0; qt < CM_NQT; ++qt)
                        acc[ot][qt] = TD ? __builtin_amdgcn_mfma_f32_16x16x4f32(bf[qt], af[ot], acc[ot][qt], 0, 0, 0)
                                            : __builtin_amdgcn_mfma_f32_16x16x4f32(af[ot], bf[qt], acc[ot][qt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    cm_store<TD>(acc, y, G, K);
}

// k_hexconv_mfma_bf16 at stride 2: register-staged P fragments [row][plane][slot] of the 8
// channels, the same weight split and fragment layout.
template <typename Tout, int NOT>
__global__ __launch_bounds__(CM_THREADS) void k_hexconv_mfma_bf16_s2(const __bf16* __restrict__ x,
                                                                     const float* __restrict__ kern,
                                                                     const float* __restrict__ bias,
                                                                     Tout* __restrict__ y, MfmaGeom G) {
    __shared__ cm_u4 psb[CSB_PSZ];
    __shared__ cm_u4 wsb[3 * 2 * 16 * NOT * 4];
    const CmBlock<NOT> K(G);
    const int tid = K.tid, q0 = K.q0, r0 = K.r0, o0 = K.o0;
    const int Wp = G.w + 2 * G.p, Hp = G.h + 2 * G.p;
    const unsigned short padv = __builtin_bit_cast(unsigned short, (__bf16)G.pad_value);

    constexpr bool TD = cm_td<Tout>;
    cm_f4 acc[NOT][CM_NQT];
    cm_bias_init<TD>(acc, bias, G, o0, K.li, K.lk);
    if (tid == 0) psb[CSB_PSZ - 1] = cm_u4{0u, 0u, 0u, 0u};
    int pidx[2];
    cb_pidx<2>(pidx, G, K.wv, K.par, K.li, K.lk);

    const unsigned short* xb = reinterpret_cast<const unsigned short*>(x) + K.b * (int64_t)G.C * G.h * G.w;
    for (int c0 = 0; c0 < G.C; c0 += CM_CC) {
        // ---- stage P rows 2 r0 .. 2 r0+8, columns 2 q0 + mink + (0..129), 8 channels -----
        // 195 threads = 65 slots x 3 row phases; a thread's two columns are its slot's planes
        if (tid < 3 * CS_SL) {
            const int sl = tid % CS_SL, ph = tid / CS_SL;
            const int px = 2 * q0 + G.mink + 2 * sl;
            const bool zc[2] = {px >= Wp, px + 1 >= Wp};     // type1 structural zero columns
            const int64_t xi[2] = {zc[0] ? -1 : pad_map(px - G.p, G.w, G.pad_mode),
                                   zc[1] ? -1 : pad_map(px + 1 - G.p, G.w, G.pad_mode)};
            // one row (16 loads) in flight: unrolled, the 48 loads took 125 VGPRs and 2 waves per SIMD
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                const int pr = ph + 3 * k, py = 2 * r0 + pr;
                const int64_t yi = py < Hp ? pad_map(py - G.p, G.h, G.pad_mode) : -1;
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    unsigned short v[8];
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) {
                        const int c = c0 + cc;
                        unsigned short e = 0;
                        if (!zc[pl] && c < G.C && py < Hp)
                            e = (yi < 0 || xi[pl] < 0) ? padv : xb[((int64_t)c * G.h + yi) * G.w + xi[pl]];
                        v[cc] = e;
                    }
                    psb[pr * CS_PP + pl * CS_PL + sl] = cb_pack(v);
                }
            }
        }
        const int nparts = cb_stage_w<NOT>(wsb, kern, G, c0, o0, tid);   // barrier inside
        // ---- 2 k blocks x 4 column tiles x nparts weight parts x NOT channel tiles ---------
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            cm_b8 bf[CM_NQT];
#pragma unroll
            for (int qt = 0; qt < CM_NQT; ++qt)
                bf[qt] = __builtin_bit_cast(cm_b8, psb[pidx[kb] < 0 ? CSB_PSZ - 1 : pidx[kb] + qt * 16]);
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                if (pt >= nparts) break;
#pragma unroll
                for (int ot = 0; ot < NOT; ++ot) {
                    const cm_b8 af = __builtin_bit_cast(cm_b8, wsb[((pt * 2 + kb) * (16 * NOT) + ot * 16 + K.li) * 4 + cd_wslot(K.li, K.lk)]);
#pragma unroll
                    for (int qt = 0; qt < CM_NQT; ++qt)
                        acc[ot][qt] = TD ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[qt], af, acc[ot][qt], 0, 0, 0)
                                            : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[qt], acc[ot][qt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    cm_store<TD>(acc, y, G, K);
}

// Output-channel tiles per workgroup (A/B switch HYGRID_CONV_NT=2: two for any O)
static int conv_mfma_nt(int64_t O) { return (O <= 32 || env_is("HYGRID_CONV_NT", "2")) ? 2 : 4; }

constexpr int CS_MIN_O = 16;                 // stride 2: out_channels from which the MFMA kernels pay

// Which wide-channel kernel takes the call (conv_mfma.h): dense radius-2, dilation-1 conv of
// stride 1 or 2 with O >= 16, f32 weights, padding 0..2.  Narrow inputs (C < 8: the
// 3-channel stem of a segmentation model, HexModules.py:97-288) run here too, their channel
// chunk padded with zeros (staging and weights read 0 past C): HexConv2d(3 -> 64) 1080p b4
// 2.76 -> 0.50 ms (bf16) and 2.84 -> 1.02 ms (f32) against the generic kernel at stride 1,
// round 6, profiles/r06/stem_conv_ab.txt; stride 2: profiles/conv_mfma_stride2_ab.txt.
// G, nt: the complete geometry (nto included, epilogue off) and the output-channel tiles per
// workgroup of the kernel named, for the launch.
static int fwd_route(int x_dtype, int w_dtype, int y_dtype, int64_t B, int64_t C, int64_t O,
                     int64_t h, int64_t w, int radius, int stride, int padding, int dilation,
                     int groups, int off, int pad_mode, double pad_value, unsigned x_align,
                     MfmaGeom& G, int& nt) {
    if (env_is("HYGRID_CONV_MFMA", "0")) return HG_CONV_FWD_OTHER;   // A/B switch: generic kernels
    if (w_dtype != HG_F32) return HG_CONV_FWD_OTHER;
    if (radius != 2 || (stride != 1 && stride != 2) || dilation != 1 || groups != 1)
        return HG_CONV_FWD_OTHER;
    if (C < 1 || O < (stride == 2 ? CS_MIN_O : 16) || padding < 0 || padding > 2)
        return HG_CONV_FWD_OTHER;
    if (!conv_mfma_size_ok(C, O, h, w)) return HG_CONV_FWD_OTHER;   // 32-bit buffer offsets
    G = {};
    if (!conv_mfma_forward_geom(G, B, C, O, h, w, padding, off, pad_mode, pad_value, stride))
        return HG_CONV_FWD_OTHER;
    nt = conv_mfma_nt(O);
    G.nto = (G.O + 16 * nt - 1) / (16 * nt);
    const int64_t blocks = B * (int64_t)G.ntq * G.ntr * G.nto;
    if (blocks > INT_MAX || blocks <= 0) return HG_CONV_FWD_OTHER;
    // bf16 inputs: the split-weight bf16 kernel, when the pad value is a bf16 (the padded
    // input keeps the input's dtype, as F.pad does; anything else keeps the f32 kernel)
    const bool bf_pad = (double)(float)(__bf16)(float)pad_value == pad_value;
    // A/B switch HYGRID_CONV_MFMA_BF16=0: the f32 kernel
    if (x_dtype == HG_BF16 && bf_pad && !env_is("HYGRID_CONV_MFMA_BF16", "0") &&
        (y_dtype == HG_BF16 || y_dtype == HG_F32)) {
        // LDS-DMA staging, stride 1 only (A/B switch HYGRID_CONV_DMA=0: the register-staged
        // kernel): rows must be dword-aligned (even width, 4-B aligned base)
        if (stride == 1 && !env_is("HYGRID_CONV_DMA", "0") && (w % 2) == 0 && (x_align & 3) == 0)
            return HG_CONV_FWD_MFMA_BF16_DMA;
        return HG_CONV_FWD_MFMA_BF16;
    }
    // the dtype pairs of conv_mfma_launch_f32
    const bool pair = (x_dtype == HG_BF16 && (y_dtype == HG_BF16 || y_dtype == HG_F32)) ||
                      (x_dtype == HG_F16 && (y_dtype == HG_F16 || y_dtype == HG_F32)) ||
                      (x_dtype == HG_F32 && (y_dtype == HG_F32 || y_dtype == HG_BF16 || y_dtype == HG_F16));
    return pair ? HG_CONV_FWD_MFMA_F32 : HG_CONV_FWD_OTHER;
}

int conv_fwd_route(int x_dtype, int w_dtype, int y_dtype, int64_t B, int64_t C, int64_t O,
                   int64_t h, int64_t w, int radius, int stride, int padding, int dilation,
                   int groups, int off, int pad_mode, double pad_value, unsigned x_align) {
    MfmaGeom G;
    int nt;
    return fwd_route(x_dtype, w_dtype, y_dtype, B, C, O, h, w, radius, stride, padding, dilation,
                     groups, off, pad_mode, pad_value, x_align, G, nt);
}

// One launch of a kernel instantiated for NOT = 2 and 4: launch(integral_constant<int, NOT>)
template <typename F>
static int launch_nt(int nt, F&& launch) {
    if (nt == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 4>{});
    return launch_status();
}

template <typename Tout>
static int launch_bf16(int route, const void* x, const float* k, const float* b, void* y,
                       const MfmaGeom& G, int nt, int stride, hipStream_t st) {
    const dim3 grid((unsigned)(G.B * G.ntq * G.ntr * G.nto)), blk(CM_THREADS);
    const __bf16* xx = static_cast<const __bf16*>(x);
    Tout* yy = static_cast<Tout*>(y);
    if (route == HG_CONV_FWD_MFMA_BF16)
        return launch_nt(nt, [&](auto n) {
            auto kn = stride == 2 ? k_hexconv_mfma_bf16_s2<Tout, n()> : k_hexconv_mfma_bf16<Tout, n()>;
            hipLaunchKernelGGL(kn, grid, blk, 0, st, xx, k, b, yy, G);
        });
    // LDS-DMA: the weight parts and their flags, split once into stream-ordered scratch
    const int nch = (G.C + CM_CC - 1) / CM_CC, Opad = G.nto * 16 * nt;
    const size_t wbytes = (size_t)nch * 6 * Opad * 64, fbytes = (size_t)nch * (Opad / 16) * 4;
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, wbytes + fbytes, st);
    if (e != hipSuccess) return (int)e;
    cm_u4* wfr = static_cast<cm_u4*>(ws);
    int* flg = reinterpret_cast<int*>(static_cast<char*>(ws) + wbytes);
    hipLaunchKernelGGL(k_wsplit_bf16, dim3(nch, Opad / 16), dim3(128), 0, st, k, wfr, flg, G.C, G.O, Opad);
    const int ls = launch_nt(nt, [&](auto n) {
        hipLaunchKernelGGL((k_hexconv_mfma_bf16d<Tout, n()>), grid, blk, 0, st, xx, wfr, flg, b, yy, G, Opad);
    });
    const hipError_t fe = hipFreeAsync(ws, st);
    return ls != HG_OK ? ls : (int)fe;
}

// Runs the kernel conv_fwd_route names; HG_EUNSUP when that is none of this file's.
int conv_mfma_try(const void* x, const float* k, const float* b, void* y, int x_dtype,
                  int y_dtype, int64_t B, int64_t C, int64_t O, int64_t h, int64_t w, int radius,
                  int stride, int padding, int dilation, int groups, int off, int pad_mode,
                  double pad_value, const Epilogue& epi, hipStream_t st) {
    MfmaGeom G;
    int nt;
    const int route = fwd_route(x_dtype, HG_F32, y_dtype, B, C, O, h, w, radius, stride, padding,
                                dilation, groups, off, pad_mode, pad_value,
                                (unsigned)(reinterpret_cast<uintptr_t>(x) & 15), G, nt);
    if (route == HG_CONV_FWD_OTHER) return HG_EUNSUP;
    G.epi = epi;
    if (route == HG_CONV_FWD_MFMA_F32) return conv_mfma_launch_f32(x, k, b, y, x_dtype, y_dtype, G, nt, st, stride);
    return y_dtype == HG_BF16 ? launch_bf16<__bf16>(route, x, k, b, y, G, nt, stride, st)
                              : launch_bf16<float>(route, x, k, b, y, G, nt, stride, st);
}

template <typename TI, typename TO>
static int launch_f32(const void* x, const float* k, const float* b, void* y, const MfmaGeom& G,
                      int nt, int stride, hipStream_t st) {
    const dim3 grid((unsigned)(G.B * G.ntq * G.ntr * G.nto)), blk(CM_THREADS);
    return launch_nt(nt, [&](auto n) {
        auto kn = stride == 2 ? k_hexconv_mfma_s2<TI, TO, n()> : k_hexconv_mfma<TI, TO, n()>;
        hipLaunchKernelGGL(kn, grid, blk, 0, st, static_cast<const TI*>(x), k, b, static_cast<TO*>(y), G);
    });
}

int conv_mfma_launch_f32(const void* x, const float* k, const float* b, void* y, int x_dtype,
                         int y_dtype, const MfmaGeom& G, int nt, hipStream_t st, int stride) {
    const int64_t blocks = G.B * (int64_t)G.ntq * G.ntr * G.nto;
    if (blocks > INT_MAX || blocks <= 0) return blocks == 0 ? HG_OK : HG_EUNSUP;
    switch (x_dtype) {
    case HG_BF16:
        if (y_dtype == HG_BF16) return launch_f32<__bf16, __bf16>(x, k, b, y, G, nt, stride, st);
        if (y_dtype == HG_F32) return launch_f32<__bf16, float>(x, k, b, y, G, nt, stride, st);
        return HG_EUNSUP;
    case HG_F16:
        if (y_dtype == HG_F16) return launch_f32<_Float16, _Float16>(x, k, b, y, G, nt, stride, st);
        if (y_dtype == HG_F32) return launch_f32<_Float16, float>(x, k, b, y, G, nt, stride, st);
        return HG_EUNSUP;
    case HG_F32:
        if (y_dtype == HG_F32) return launch_f32<float, float>(x, k, b, y, G, nt, stride, st);
        if (y_dtype == HG_BF16) return launch_f32<float, __bf16>(x, k, b, y, G, nt, stride, st);
        if (y_dtype == HG_F16) return launch_f32<float, _Float16>(x, k, b, y, G, nt, stride, st);
        return HG_EUNSUP;
    default:
        return HG_EUNSUP;
    }
}

}  // namespace hg
