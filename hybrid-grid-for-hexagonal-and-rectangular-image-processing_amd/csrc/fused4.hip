// fused4.hip — the headline pass (rect -> hex -> HexConv2d(r=2) -> hex -> rect, bf16 in and out,
// C = O = 3) with FOUR columns per lane (round 4): lane l owns columns ce .. ce + 3,
// ce = W0 + 4 l, of a 256-column window (240 owned, 8 + 8 halo), as two stride-2 pairs
// P = (ce, ce + 2) and Q = (ce + 1, ce + 3) (round 8; rounds 4-7 held (even, odd) pairs
// A = (ce, ce + 1), B = (ce + 2, ce + 3)).  Everything else is k_fused MD 0 (fused_kernel.h):
// the per-wave row table and row classes, the per-lane column weights and column classes, the
// packed 7-tap stencil with 21 weight pairs in SGPRs, the folded same-size h2r, the 6-step blocks.
//
// Why: per owned column the 2-column kernel spends a neighbour exchange (DPP + pair copies) on
// every pair, 1/16 of its work on the 8-column window halo and reads 1.107x its input bytes;
// here three of a lane's four columns have both neighbours in the lane, the halo is 1/32 and the reads
// ~1.04x; 8-B loads and stores per lane (walk6: the access pattern alone 0.615 -> 0.657 of
// 8 TB/s at 42-row bands, 0.73 at 18-24; profiles/r04/walk6_b.txt).  Registers: 29 of the 32
// weight pairs in SGPRs (106 SGPRs) and two rect rows of prefetch: 136 VGPRs, 3 waves per SIMD
// (round 6; one row of prefetch at 124 VGPRs and 4 waves was rounds 4-5's choice).
//
// Why stride-2 pairs: the kernel is bound by VALU issue, and with (even, odd)
// pairs every odd tap shift needs a pair that straddles A and B, copied together by plain and
// DPP moves (13 + 12 per step).  With P and Q, shift 0 reads (P, Q), +1 reads (Q, (P.y, next
// lane's P.x)), -1 reads ((previous lane's Q.y, Q.x), P): two assembled pairs per channel, and
// half of the horizontal blend and of the h2r become packed ops on aligned pairs.  Every
// product and sum keeps its operands and order.  128-130 VGPRs; 196 VALU issue slots per step
// in the two-term loops instead of 216-220 (profiles/r08/fused4_loop_mix.txt).
//
// Domain: fused_try's (same-size lattice, padding 1, value 0) with bf16 in and out, C = O = 3,
// groups 1, w and w2 multiples of 4.  (Round 5 also built this layout for HexConv2d alone and
// for the round trip, and a per-wave LDS-DMA row ring and cache-policy variants of this kernel:
// all measured slower; removed in round 6.)  Results within the fp32 rounding of k_fused MD 0 (the same
// products and sums per output; a tap order may differ), checked against the oracle chain.
#include <climits>
#include <cmath>
#include <cstdlib>

#include "fused_kernel.h"

namespace hg {

#ifndef F4_RB_
#define F4_RB_ 30                      // output rows per band (multiple of 6; 30 the most even across boxes: profiles/r04/f4)
#endif
#ifndef F4_PD
#define F4_PD 2                        // rect rows loaded ahead of use (1..4): 2 at 136 VGPRs, 3
                                       // waves per SIMD, is 0.9-2.1 % faster than 1 at 124 VGPRs
                                       // and 4 waves once the odd bands walk upwards (round 6,
                                       // profiles/r06/fused4_pd*_ab*.txt)
#endif
#ifndef F4_WPS
#define F4_WPS 29                      // weight pairs in SGPRs (the rest in VGPRs): 102 SGPRs
#endif
#ifndef F4_ORDER
#define F4_ORDER 0                     // workgroup order (A/B): 0 group fastest, 1 band fastest
#endif
#ifndef F4_WPE
#define F4_WPE 3                       // waves per SIMD, both the least and the most: at 128
                                       // VGPRs the bench's instantiation would run 4, which
                                       // is no faster (profiles/r08/fused4_pairs_ab.txt)
#endif
#ifndef F4_REV
#define F4_REV 1                       // odd full bands walk upwards (shared halo rows in L2, below)
#endif
constexpr int F4_GW = 4, F4_THREADS = 256;
constexpr int F4_HL = 8, F4_OWN = 240;  // window halo (left) and owned columns
constexpr int F4_RB = F4_RB_;
static_assert(F4_RB % 6 == 0 && F4_RB > 0, "bands are whole 6-step blocks");

typedef unsigned f4_u2 __attribute__((ext_vector_type(2)));

// the lane's four bf16 columns as the stride-2 f32 pairs p = (c0, c2) and q = (c1, c3)
__device__ __forceinline__ void f4_unpack(f4_u2 r, fu_f2& p, fu_f2& q, unsigned hi16) {
    p = fu_f2{__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.y << 16)};
    q = fu_f2{__builtin_bit_cast(float, r.x & hi16), __builtin_bit_cast(float, r.y & hi16)};
}
// Packed ops on aligned pairs with a per-lane weight pair (no broadcast): d = w * a and
// c += w * a, each half an IEEE multiply / fmaf.  Inline asm like fu_pfma: a half of `a` may
// come from a DPP move (Makefile: compiler-made packed ops on such pairs were wrong).
__device__ __forceinline__ fu_f2 f4_pmul2(fu_f2 w, fu_f2 a) {
    fu_f2 d;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(d) : "v"(w), "v"(a));
    return d;
}
__device__ __forceinline__ fu_f2 f4_pfma2(fu_f2 w, fu_f2 a, fu_f2 c) {
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(a));
    return c;
}
// Multi-instruction statements.  Two things about the compiler's hazard recognizer shape them:
// (1) A DPP operand must be 2 VALU instructions old, and the recognizer does not see an
//     inline-asm packed op as its writer.  Every statement below reads its DPP operand in its
//     third instruction or later: safe whatever precedes it (tools/dpp_hazard.py scans the
//     assembly for it).
// (2) An asm statement that reads a register an earlier asm statement wrote gets an s_nop
//     unless a compiler-made instruction lies between the two (asm statements count as no
//     distance at all), however far apart they are.  Dependent ops that share a statement
//     cost none, and k_fused4's step is ordered in groups of independent statements with
//     the step's ordinary instructions (unpacks, loads, stores) between the groups.
#define F4_SHR_ " wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"   /* f_prev */
#define F4_SHL_ " wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"   /* f_next */
// The vertical blend of one pair as one statement: a x[r-1] + b x[r] + c x[r+1] with the row
// weights (a, b) = lxy and (c, .) = lzw broadcast by op_sel; RC 1 has no c term, RC 2 no a term
// (the ops and their order are k_fused's fu_pmul / fu_pfma chain).
template <int RC>
__device__ __forceinline__ fu_f2 f4_vblend(fu_f2 lxy, fu_f2 lzw, fu_f2 xm, fu_f2 x1, fu_f2 xq) {
    fu_f2 d;
    if constexpr (RC == 1)
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
            "v_pk_fma_f32 %0, %1, %3, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]"
            : "=&v"(d) : "v"(lxy), "v"(xm), "v"(x1));
    else if constexpr (RC == 2)
        asm("v_pk_mul_f32 %0, %1, %3 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
            "v_pk_fma_f32 %0, %2, %4, %0 op_sel_hi:[0,1,1]"
            : "=&v"(d) : "v"(lxy), "v"(lzw), "v"(x1), "v"(xq));
    else
        asm("v_pk_mul_f32 %0, %1, %3 op_sel_hi:[0,1]\n\t"
            "v_pk_fma_f32 %0, %1, %4, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %0, %2, %5, %0 op_sel_hi:[0,1,1]"
            : "=&v"(d) : "v"(lxy), "v"(lzw), "v"(xm), "v"(x1), "v"(xq));
    return d;
}
// CD 1's horizontal blend (taps q-1, q) of vp = (v0, v2), vq = (v1, v3) as one statement:
//   uq = w1q * vq + w0q * vp                       (u1, u3: aligned pairs, pk_mul then pk_fma)
//   up.x = fmaf(w01, v0, w00 * f_prev(v3)),  up.y = fmaf(w11, v2, w10 * v1)
__device__ __forceinline__ void f4_hblend_prev(fu_f2 w0q, fu_f2 w1q, float w00, float w01,
                                               float w10, float w11, fu_f2 vp, fu_f2 vq,
                                               fu_f2& up, fu_f2& uq) {
    float ux, uy;
    asm("v_pk_mul_f32 %0, %3, %5\n\t"
        "v_mul_f32 %2, %9, %13\n\t"
        "v_fmac_f32 %2, %10, %12\n\t"
        "v_mul_f32_dpp %1, %14, %7" F4_SHR_ "\n\t"
        "v_pk_fma_f32 %0, %4, %6, %0\n\t"
        "v_fmac_f32 %1, %8, %11"
        : "=&v"(uq), "=&v"(ux), "=&v"(uy)
        : "v"(w0q), "v"(w1q), "v"(vp), "v"(vq), "v"(w00), "v"(w01), "v"(w10), "v"(w11),
          "v"(vp.x), "v"(vp.y), "v"(vq.x), "v"(vq.y));
    up = fu_f2{ux, uy};
}
// CD 2's (taps q, q+1):
//   up = w2p * vq + w1p * vp                       (u0, u2)
//   uq.x = fmaf(w02, v2, w01 * v1),  uq.y = fmaf(w12, f_next(v0), w11 * v3)
__device__ __forceinline__ void f4_hblend_next(fu_f2 w1p, fu_f2 w2p, float w01, float w02,
                                               float w11, float w12, fu_f2 vp, fu_f2 vq,
                                               fu_f2& up, fu_f2& uq) {
    float ux, uy;
    asm("v_pk_mul_f32 %0, %3, %5\n\t"
        "v_mul_f32 %1, %7, %13\n\t"
        "v_fmac_f32 %1, %8, %12\n\t"
        "v_mul_f32 %2, %9, %14\n\t"
        "v_pk_fma_f32 %0, %4, %6, %0\n\t"
        "v_fmac_f32_dpp %2, %11, %10" F4_SHL_
        : "=&v"(up), "=&v"(ux), "=&v"(uy)
        : "v"(w1p), "v"(w2p), "v"(vp), "v"(vq), "v"(w01), "v"(w02), "v"(w11), "v"(w12),
          "v"(vp.x), "v"(vp.y), "v"(vq.x), "v"(vq.y));
    uq = fu_f2{ux, uy};
}
// The stencil's pairs that straddle a lane, from up = (u0, u2) and uq = (u1, u3):
//   ul = (u-1, u1) = (f_prev(uq.y), uq.x)      shift -1
//   ur = (u2, u4) = (up.y, f_next(up.x))       shifts +1, +2
//   ur2 = (u3, u5) = (uq.y, f_next(uq.x))      shift +2 (tap column class 0, odd centre rows)
// NL / NR2: whether this u row's taps read ul / ur2 (an asm statement is not dead code to the
// compiler).  A row that reads ur2 and not ul makes (ur, ur2); any other (ul, ur) and ur2 if read.
template <bool NL, bool NR2>
__device__ __forceinline__ void f4_straddle(fu_f2 up, fu_f2 uq, fu_f2& ul, fu_f2& ur, fu_f2& ur2) {
    float rx, ry, lx = 0.f, ly = 0.f, sx = 0.f, sy = 0.f;
    if constexpr (NR2 && NL)
        asm("v_mov_b32 %0, %7\n\t"
            "v_mov_b32 %3, %8\n\t"
            "v_mov_b32_dpp %1, %6" F4_SHL_ "\n\t"
            "v_mov_b32_dpp %2, %9" F4_SHR_ "\n\t"
            "v_mov_b32 %4, %9\n\t"
            "v_mov_b32_dpp %5, %8" F4_SHL_
            : "=&v"(rx), "=&v"(ry), "=&v"(lx), "=&v"(ly), "=&v"(sx), "=&v"(sy)
            : "v"(up.x), "v"(up.y), "v"(uq.x), "v"(uq.y));
    else if constexpr (NR2)
        asm("v_mov_b32 %0, %5\n\t"
            "v_mov_b32 %2, %7\n\t"
            "v_mov_b32_dpp %1, %4" F4_SHL_ "\n\t"
            "v_mov_b32_dpp %3, %6" F4_SHL_
            : "=&v"(rx), "=&v"(ry), "=&v"(sx), "=&v"(sy)
            : "v"(up.x), "v"(up.y), "v"(uq.x), "v"(uq.y));
    else
        asm("v_mov_b32 %0, %5\n\t"
            "v_mov_b32 %3, %6\n\t"
            "v_mov_b32_dpp %1, %4" F4_SHL_ "\n\t"
            "v_mov_b32_dpp %2, %7" F4_SHR_
            : "=&v"(rx), "=&v"(ry), "=&v"(lx), "=&v"(ly)
            : "v"(up.x), "v"(up.y), "v"(uq.x), "v"(uq.y));
    ur = fu_f2{rx, ry};
    ul = fu_f2{lx, ly};
    ur2 = fu_f2{sx, sy};
}
// The folded same-size h2r of one conv row held as za = (z0, z2), zb = (z1, z3), cw = (1/3,
// neighbour weight).  Even rows: o[b] = z[b+1] / 3 + z[b], the last one's z[b+1] the next lane's
// z0; odd rows: o[b] = z[b-1] / 3 + z[b], the first one's z[b-1] the previous lane's z3.  The two
// outputs whose terms are aligned pairs are one packed FMA; the neighbour term is a
// v_fmac_f32_dpp (as fu_h2r3_even).  Bit-identical to the four fmaf.
__device__ __forceinline__ void f4_h2r_even(fu_f2 za, fu_f2 zb, fu_f2 cw, float& o0, float& o1,
                                            float& o2, float& o3) {
    fu_f2 d;
    float a, zby = zb.y;
    asm("v_pk_fma_f32 %0, %3, %5, %4 op_sel_hi:[0,1,1]\n\t"
        "v_fma_f32 %1, %9, %7, %8\n\t"
        "v_fmac_f32_dpp %2, %6, %10" F4_SHL_
        : "=&v"(d), "=&v"(a), "+v"(zby)
        : "v"(cw), "v"(za), "v"(zb), "v"(za.x), "v"(za.y), "v"(zb.x), "v"(cw.x), "v"(cw.y));
    o0 = d.x; o1 = a; o2 = d.y; o3 = zby;
}
__device__ __forceinline__ void f4_h2r_odd(fu_f2 za, fu_f2 zb, fu_f2 cw, float& o0, float& o1,
                                           float& o2, float& o3) {
    fu_f2 d;
    float a, zax = za.x;
    asm("v_pk_fma_f32 %0, %3, %4, %5 op_sel_hi:[0,1,1]\n\t"
        "v_fma_f32 %1, %9, %7, %8\n\t"
        "v_fmac_f32_dpp %2, %6, %10" F4_SHR_
        : "=&v"(d), "=&v"(a), "+v"(zax)
        : "v"(cw), "v"(za), "v"(zb), "v"(zb.y), "v"(zb.x), "v"(za.y), "v"(cw.x), "v"(cw.y));
    o0 = zax; o1 = d.x; o2 = a; o3 = d.y;
}
#undef F4_SHR_
#undef F4_SHL_

// rect -> hex -> HexConv2d -> hex -> rect (the headline); OP = the stencil's tap column class
// at padding 1 ((even_odd_offset + 1) & 1).
//
// Band direction (F4_REV, round 6): a band reads its 30 output rows' rect rows plus 2 halo rows
// on each side, and the halo rows of two neighbouring bands are the same 4 rows.  Walking every
// band downwards, band k + 1 reads them first (at its start) and band k last (at its end), a
// whole band walk later, when they have long left the L2: the vertical halo comes from HBM
// twice (34 / 30 = 1.133x the input bytes).  With F4_REV the odd full bands walk upwards, so the
// two bands of a shared boundary reach it at the same time (both at their start, or both at
// their end) while they run side by side on one XCD.  A reversed band produces the same u rows
// (the vertical blend keeps its operand order), but each conv row then accumulates its below
// taps first and its above taps last: the same products, summed in another order (fp32
// rounding level; the bias still comes first).
template <int OP>
__global__ __launch_bounds__(F4_THREADS) __attribute__((amdgpu_waves_per_eu(F4_WPE, F4_WPE)))
void k_fused4(const __bf16* __restrict__ x, const float* __restrict__ kern,
              const float* __restrict__ bias, __bf16* __restrict__ y, FusedGeom F) {
    constexpr int C = 3, O = 3;
    constexpr int PD = F4_PD;
    static_assert(PD >= 1 && PD <= 4, "raw ring: rows k+2 .. k+1+PD in flight in 6 slots");
    constexpr int RB = F4_RB, NLUT = RB + 2;
    __shared__ float4 lut_all[F4_GW][NLUT];
    const int lane = threadIdx.x & 63;
    const int wslot = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4* const lut = lut_all[wslot];
    const int64_t blk = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x);
    const int ngrp = (F.nwin + F4_GW - 1) / F4_GW;
    // block -> (window group, band, image): group fastest (F4_ORDER 0) or band fastest (1)
    const int grp = (int)(F4_ORDER == 1 ? (blk / F.nband) % ngrp : blk % ngrp);
    const int band = (int)(F4_ORDER == 1 ? blk % F.nband : (blk / ngrp) % F.nband);
    const int64_t b = blk / ((int64_t)ngrp * F.nband);
    if (b >= F.B) return;                            // uniform per workgroup
    const int win = grp * F4_GW + wslot;             // may be >= nwin: runs, owns nothing
    const int W0 = win * F4_OWN - F4_HL;
    const int ce = W0 + 4 * lane;                    // columns ce .. ce + 3 (pairs P, Q)
    const int s0 = band * RB;
    const int s1 = min(s0 + RB, F.h2);
    const bool up = F4_REV && (band & 1) && s1 - s0 == RB;   // uniform

    // ---- row table (fp64 lattice math, geometry_np.py:440-486), as k_fused -------------
    // entry e: u row s0 - 1 + e = {a, b, c}: u[r] = a x[r-1] + b x[r] + c x[r+1]
    for (int e = lane; e < NLUT; e += 64) {
        const int r = s0 - 1 + e;
        float4 t = {0.f, 0.f, 0.f, 0.f};
        if (r >= 0 && r < F.h1) {
            const double i_ = axis_at(F.rxs, r) + (double)(F.h - 1) * 0.5;   // :440
            const int in = (int)i_;                                          // :444
            const double f = i_ - (double)(float)in;                         // :448
            const float w0 = (in >= 0 && in < F.h) ? (float)(1.0 - f) : 0.f;
            const float w1 = (in + 1 >= 0 && in + 1 < F.h) ? (float)f : 0.f;
            if (in == r - 1) { t.x = w0; t.y = w1; }
            else if (in == r) { t.y = w0; t.z = w1; }
        }
        lut[e] = t;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    int rc;
    {
        bool has_a = false, has_c = false;
        for (int e = lane; e < NLUT; e += 64) {
            const float4 t = lut[e];
            has_a |= t.x != 0.f;
            has_c |= t.z != 0.f;
        }
        const bool any_a = __builtin_amdgcn_ballot_w64(has_a) != 0;
        const bool any_c = __builtin_amdgcn_ballot_w64(has_c) != 0;
        rc = !any_c ? 1 : (!any_a ? 2 : 0);
    }

    // ---- per-lane column weights of the two pairs (geometry_np.py:441-449, 514-517) -------
    // with the h2r 0.75 folded in (u' = 0.75 u, as k_fused MD 0)
    float we[2][3], wo[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float* wr = s ? wo[k] : we[k];
            wr[0] = wr[1] = wr[2] = 0.f;
            const int q = ce + 2 * k + s;
            if (q >= 0 && q < F.w1) {
                const double j_ = axis_at(F.rys, q) + (double)(F.w - 1) * 0.5;   // :441
                const int jn = (int)j_;
                const double jf = j_ - (double)(float)jn;
#pragma unroll
                for (int kk = -1; kk <= 1; ++kk) {
                    const bool in_w = q + kk >= 0 && q + kk < F.w;
                    if (kk == jn - q && in_w) wr[kk + 1] += (float)(1.0 - jf);
                    if (kk == jn + 1 - q && in_w) wr[kk + 1] += (float)jf;
                }
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) wr[t] *= 0.75f;
        }
    const bool any_l = __builtin_amdgcn_ballot_w64(we[0][0] != 0.f || wo[0][0] != 0.f ||
                                                   we[1][0] != 0.f || wo[1][0] != 0.f) != 0;
    const bool any_r = __builtin_amdgcn_ballot_w64(we[0][2] != 0.f || wo[0][2] != 0.f ||
                                                   we[1][2] != 0.f || wo[1][2] != 0.f) != 0;
    const int cd = !any_r ? 1 : (!any_l ? 2 : 0);
    // the same weights as stride-2 pairs: tap t of columns (ce, ce + 2) and (ce + 1, ce + 3)
    fu_f2 WE[3], WO[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        WE[t] = fu_f2{we[0][t], we[1][t]};
        WO[t] = fu_f2{wo[0][t], wo[1][t]};
    }

    // owned lanes 2 .. 61 (w2 % 4 == 0: a lane is wholly inside or outside the raster)
    const bool own = lane >= F4_HL / 4 && lane < (F4_HL + F4_OWN) / 4 && ce >= 0 && ce < F.w2 &&
                     win < F.nwin;

    // ---- buffers ----------------------------------------------------------------------
    const int64_t cstride = (int64_t)F.h * F.w, ostride = (int64_t)F.h2 * F.w2;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(x + b * C * cstride), (short)0, (int)(C * cstride * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(y + b * O * ostride), (short)0, (int)(O * ostride * 2), 0x00020000);
    const int lc = min(max(ce, 0), F.w - 4);         // clamped load column (x 0 weights outside)
    const unsigned xoff = (unsigned)lc * 2u;
    const unsigned yoff = own ? (unsigned)ce * 2u : 0x80000000u;
    const unsigned xplane = (unsigned)(cstride * 2), yplane = (unsigned)(ostride * 2);
    const unsigned xrow = (unsigned)F.w * 2u, yrow = (unsigned)F.w2 * 2u;
    auto row_off = [&](int r) -> unsigned {
        return (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)min(max(r, 0), F.h - 1) * xrow));
    };

    // ---- weights (29 pairs in SGPRs, the rest opaque VGPR pairs) and bias ---------------
    int vz = 0;
    asm volatile("" : "+v"(vz));
    constexpr int NW = O * C * 7, NWP = (NW + 1) / 2;
    constexpr int NWS = F4_WPS < NWP ? F4_WPS : NWP;
    float wk[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) wk[i] = kern[i + (i / 2 < NWS ? 0 : vz)];
    fu_f2 wkp[NWP];
#pragma unroll
    for (int i = 0; i < NWP; ++i) {
        wkp[i] = fu_f2{wk[2 * i], 2 * i + 1 < NW ? wk[2 * i + 1] : 0.f};
        if (i >= NWS) asm volatile("" : "+v"(wkp[i]));
    }
    float bv[O];
#pragma unroll
    for (int o = 0; o < O; ++o) bv[o] = bias ? bias[o + vz] * 0.75f : 0.f;
    fu_f2 bvp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        bvp[i] = fu_f2{bv[2 * i], 2 * i + 1 < O ? bv[2 * i + 1] : 0.f};
        asm volatile("" : "+v"(bvp[i]));
    }
    float c13 = 1.f / 3.f;
    asm volatile("" : "+v"(c13));
    // h2r neighbours outside the raster (:303-323): column ce + 3's right neighbour (even rows) and
    // column ce's left neighbour (odd rows); the inner ones are always inside
    const float wn_f = (ce + 4 < F.w2) ? c13 : 0.f;
    const float wp_f = (ce - 1 >= 0) ? c13 : 0.f;
    const fu_f2 c13n = {c13, wn_f}, c13p = {c13, wp_f};   // (1/3, neighbour weight) pairs
    unsigned hi16 = 0xffff0000u;
    asm volatile("" : "+v"(hi16));

    // A band is walked in steps k = 0 .. s1 - s0 - 1 over output rows row(k): downwards
    // (row(k) = s0 + k) or, UP, upwards (row(k) = s1 - 1 - k).  Rect row / u row / conv row
    // row(k) lives in ring slot k mod 6 / k mod 3, so the slots and the row parities are
    // compile-time per step of a 6-step block in both directions.
    auto run = [&](auto CDc, auto RCc, auto UPc) {
        constexpr int CD = decltype(CDc)::value;
        constexpr int RC = decltype(RCc)::value;
        constexpr bool UP = decltype(UPc)::value;
        auto row = [&](int k) { return UP ? s1 - 1 - k : s0 + k; };
        // row-table entry of u row row(j)
        auto lut_e = [&](int j) { return UP ? RB - j : j + 1; };
        f4_u2 raw[6][C];                    // rect rows in flight, slot k % 6
        fu_f2 XA[3][C], XB[3][C];           // rect rows as f32 pairs P / Q, slot k % 3
        fu_f2 ZA[3][O], ZB[3][O];           // conv rows being accumulated, columns (0, 2) / (1, 3)

        // live false: the loads return zeros without a memory access (an offset past the buffer)
        auto issue = [&](auto SLc, int r, bool live = true) {
            constexpr int SL = decltype(SLc)::value;
            const unsigned so = row_off(r);
            const unsigned vo = live ? xoff : 0x80000000u;
#pragma unroll
            for (int c = 0; c < C; ++c) raw[SL][c] = __builtin_amdgcn_raw_buffer_load_b64(xrs, vo, so + c * xplane, 0);
        };
        auto convert = [&](auto RSc, auto XSc) {
            constexpr int RS = decltype(RSc)::value, XS = decltype(XSc)::value;
#pragma unroll
            for (int c = 0; c < C; ++c) f4_unpack(raw[RS][c], XA[XS][c], XB[XS][c], hi16);
        };

        // u row row(j), j = PH + 1, from rect rows row(PH), row(PH+1), row(PH+2) (slots S0, S1,
        // S2), scattered into conv rows row(PH+2) (started here with the bias: slot S2), row(PH+1)
        // (centre: S1) and row(PH) (completed here: S0).  Downwards the started row is the one
        // below (u row = its 'above' row: taps 0, 1), upwards the one above (taps 5, 6).
        //
        // Order (see "Multi-instruction statements" above): groups of independent asm statements,
        // fenced by scheduling barriers, with the step's compiler-made instructions between them,
        // which the caller supplies: pre(c) before channel c's vertical blend (its unpack),
        // mid(i), i = 0 .. 5, between the tap groups (its loads), fin() once the completed
        // row's taps are done (its h2r), put(o) after each of the last three groups (its stores).  The channels are skewed by one stage (blend, horizontal blend, straddling
        // pairs); the taps go level by level: group l holds every accumulator's l-th tap of this
        // u row, so each accumulator still takes its taps in channel and tap order.
        auto urow = [&](auto PHc, float4 L, auto CENc, auto BELc, auto&& pre, auto&& mid, auto&& fin,
                        auto&& put) {
            constexpr int PH = decltype(PHc)::value;
            constexpr bool CEN = decltype(CENc)::value, BEL = decltype(BELc)::value;
            constexpr int S0 = fu_mod(PH, 3), S1 = fu_mod(PH + 1, 3), S2 = fu_mod(PH + 2, 3);
            // slots of rect rows r - 1 and r + 1 (r = row(PH + 1))
            constexpr int XM = UP ? S2 : S0, XQ = UP ? S0 : S2;
            // parity of the started / completed rows (row(PH) and row(PH + 2)); s0 and, for an
            // UP band, s1 are even
            constexpr int PB = UP ? fu_mod(PH + 1, 2) : fu_mod(PH, 2), PC = 1 - PB;
            constexpr int TN = UP ? 5 : 0, TD = UP ? 0 : 5;   // first tap of started / completed row
            // which straddling pairs this u row's taps read: shift -1 reads UL, shift +2 reads UR2
            constexpr auto reads = [](int s) {
                bool r = fu_tap_shift(TN, PB, OP) == s || fu_tap_shift(TN + 1, PB, OP) == s;
                if (BEL) r = r || fu_tap_shift(TD, PB, OP) == s || fu_tap_shift(TD + 1, PB, OP) == s;
                if (CEN) r = r || fu_tap_shift(2, PC, OP) == s || fu_tap_shift(3, PC, OP) == s ||
                             fu_tap_shift(4, PC, OP) == s;
                return r;
            };
            constexpr bool NEED_L = reads(-1), NEED_R2 = reads(2);
            const fu_f2 Lxy = {L.x, L.y}, Lzw = {L.z, L.w};
            fu_f2 VP[C], VQ[C];                 // vertical blends of the P / Q pairs
            // the u row: columns ce .. ce+3 as UP = (u0, u2), UQ = (u1, u3), and the stencil's
            // operands that straddle a lane, UR = (u2, u4), UL = (u-1, u1), UR2 = (u3, u5):
            // accumulator ZA = (z0, z2) reads (u[s], u[s+2]), ZB = (z1, z3) reads (u[s+1], u[s+3])
            fu_f2 UP_[C], UQ_[C], UR[C], UL[C], UR2[C];
            auto fence = [] { __builtin_amdgcn_sched_barrier(0); };
            auto vblend = [&](auto Cc) {
                constexpr int c = decltype(Cc)::value;
                VP[c] = f4_vblend<RC>(Lxy, Lzw, XA[XM][c], XA[S1][c], XA[XQ][c]);
                VQ[c] = f4_vblend<RC>(Lxy, Lzw, XB[XM][c], XB[S1][c], XB[XQ][c]);
            };
            // horizontal blend: the lane's left neighbour column is the previous lane's VQ.y,
            // its right one the next lane's VP.x; where both columns of a pair take their terms
            // from aligned pairs the blend is packed (pk_mul then pk_fma: the rounding of
            // fmaf(w1, v, w0 * v'))
            auto hblend = [&](auto Cc) {
                constexpr int c = decltype(Cc)::value;
                const fu_f2 vp = VP[c], vq = VQ[c];
                if constexpr (CD == 1) {            // taps q-1, q
                    f4_hblend_prev(WO[0], WO[1], we[0][0], we[0][1], we[1][0], we[1][1], vp, vq,
                                   UP_[c], UQ_[c]);
                } else if constexpr (CD == 2) {     // taps q, q+1
                    f4_hblend_next(WE[1], WE[2], wo[0][1], wo[0][2], wo[1][1], wo[1][2], vp, vq,
                                   UP_[c], UQ_[c]);
                } else {
                    const fu_f2 tl = {we[0][0] * f_prev(vq.y), we[1][0] * vq.x};
                    UP_[c] = f4_pfma2(WE[2], vq, f4_pfma2(WE[1], vp, tl));
                    const fu_f2 tq = f4_pfma2(WO[1], vq, f4_pmul2(WO[0], vp));
                    UQ_[c] = fu_f2{fmaf(wo[0][2], vp.y, tq.x), fmaf(wo[1][2], f_next(vp.x), tq.y)};
                }
            };
            auto straddle = [&](auto Cc) {
                constexpr int c = decltype(Cc)::value;
                f4_straddle<NEED_L, NEED_R2>(UP_[c], UQ_[c], UL[c], UR[c], UR2[c]);
            };
            // tap T of channel c into the conv row in slot SL (parity PAR), every output channel
            auto tap = [&](auto SLc, auto PARc, auto Cc, auto Tc, auto BIASc) {
                constexpr int SL = decltype(SLc)::value, PAR = decltype(PARc)::value;
                constexpr int c = decltype(Cc)::value, T = decltype(Tc)::value;
                constexpr int s = fu_tap_shift(T, PAR, OP);
                const fu_f2 aA = s == -1 ? UL[c] : (s == 0 ? UP_[c] : (s == 1 ? UQ_[c] : UR[c]));
                const fu_f2 aB = s == -1 ? UP_[c] : (s == 0 ? UQ_[c] : (s == 1 ? UR[c] : UR2[c]));
                fu_sfor<0, O>([&](auto OOc) {
                    constexpr int o = decltype(OOc)::value;
                    constexpr int j = (o * C + c) * 7 + T;
                    constexpr bool WS = (j >> 1) < NWS;
                    if constexpr (decltype(BIASc)::value) {   // a started row's first tap adds the bias
                        ZA[SL][o] = fu_pfma_b<j & 1, o & 1, WS>(wkp[j >> 1], aA, bvp[o >> 1]);
                        ZB[SL][o] = fu_pfma_b<j & 1, o & 1, WS>(wkp[j >> 1], aB, bvp[o >> 1]);
                    } else {
                        ZA[SL][o] = fu_pfma<j & 1, WS>(wkp[j >> 1], aA, ZA[SL][o]);
                        ZB[SL][o] = fu_pfma<j & 1, WS>(wkp[j >> 1], aB, ZB[SL][o]);
                    }
                });
            };
            // level l: the started and completed rows take 2 taps per channel, the centre row 3
            auto level = [&](auto Lc) {
                constexpr int l = decltype(Lc)::value;
                if constexpr (l < 2 * C) {
                    tap(IC<S2>{}, IC<PB>{}, IC<l / 2>{}, IC<TN + l % 2>{}, std::bool_constant<l == 0>{});
                    if constexpr (BEL)
                        tap(IC<S0>{}, IC<PB>{}, IC<l / 2>{}, IC<TD + l % 2>{}, std::false_type{});
                }
                if constexpr (CEN)
                    tap(IC<S1>{}, IC<PC>{}, IC<l / 3>{}, IC<2 + l % 3>{}, std::false_type{});
            };
            static_assert(C == 3, "the stage skew below is written out for three channels");
            fence(); pre(IC<0>{});
            fence(); vblend(IC<0>{});
            fence(); pre(IC<1>{});
            fence(); hblend(IC<0>{}); vblend(IC<1>{});
            fence(); pre(IC<2>{});
            fence(); straddle(IC<0>{}); hblend(IC<1>{}); vblend(IC<2>{});
            fence(); mid(IC<0>{});
            fence(); level(IC<0>{}); straddle(IC<1>{}); hblend(IC<2>{});
            fence(); mid(IC<1>{});
            fence(); level(IC<1>{}); straddle(IC<2>{});
            fence(); mid(IC<2>{});
            fence(); level(IC<2>{});
            fence(); mid(IC<3>{});
            fence(); level(IC<3>{});
            fence(); mid(IC<4>{});
            fence(); level(IC<4>{});
            fence(); mid(IC<5>{});
            fence(); level(IC<5>{});             // the completed row's last taps
            fence(); fin();
            fence(); level(IC<6>{});
            fence(); put(IC<0>{});
            fence(); level(IC<7>{});
            fence(); put(IC<1>{});
            fence(); level(IC<8>{});
            fence(); put(IC<2>{});
            fence();
        };
        auto no1 = [](auto) {};             // the prologue's u rows: nothing to interleave
        auto no0 = [] {};

        // ---- prologue: u rows row(-1) and row(0) ----------------------------------------
        {
            f4_u2 t0[C], t1[C], t2[C];
            const unsigned o0 = row_off(row(-2)), o1 = row_off(row(-1)), o2 = row_off(row(0));
#pragma unroll
            for (int c = 0; c < C; ++c) {
                t0[c] = __builtin_amdgcn_raw_buffer_load_b64(xrs, xoff, o0 + c * xplane, 0);
                t1[c] = __builtin_amdgcn_raw_buffer_load_b64(xrs, xoff, o1 + c * xplane, 0);
                t2[c] = __builtin_amdgcn_raw_buffer_load_b64(xrs, xoff, o2 + c * xplane, 0);
            }
            issue(IC<1>{}, row(1));
#pragma unroll
            for (int i = 0; i < PD; ++i) {          // ring: rect rows row(2) .. row(1 + PD)
                if (i == 0) issue(IC<2>{}, row(2));
                if (i == 1) issue(IC<3>{}, row(3));
                if (i == 2) issue(IC<4>{}, row(4));
                if (i == 3) issue(IC<5>{}, row(5));
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                f4_unpack(t0[c], XA[1][c], XB[1][c], hi16);   // row(-2) -> slot 1
                f4_unpack(t1[c], XA[2][c], XB[2][c], hi16);   // row(-1) -> slot 2
                f4_unpack(t2[c], XA[0][c], XB[0][c], hi16);   // row(0)  -> slot 0
            }
        }
        urow(IC<-2>{}, lut[lut_e(-1)], std::false_type{}, std::false_type{}, no1, no1, no0, no1);   // u row(-1): start only
        convert(IC<1>{}, IC<1>{});                                              // row(1) -> slot 1
        urow(IC<-1>{}, lut[lut_e(0)], std::true_type{}, std::false_type{}, no1, no1, no0, no1);     // u row(0): start, centre
        __builtin_amdgcn_s_waitcnt(0x0f70);                                     // vmcnt(0)

        // ---- main loop -----------------------------------------------------------------
        const int n = s1 - s0;
        float4 lnext = lut[lut_e(1)];
        unsigned lso = row_off(row(min(2 + PD, n + 1)));        // load offset of the next step's row
        // One step: rect row row(k+2) unpacked, row(k+2+PD) requested, u row row(k+1) made and
        // scattered, conv row row(k) through the folded same-size h2r (even rows z'[b] +
        // z'[b+1] / 3, odd rows z'[b-1] / 3 + z'[b], geometry_np.py:347-354) and stored.
        auto step = [&](auto PHc, int k) {
            constexpr int PH = decltype(PHc)::value;
            constexpr int RS = (PH + 2) % 6, XS = (PH + 2) % 3, LS = (PH + 2 + PD) % 6;
            constexpr int S0 = PH % 3;
            constexpr int PAR = UP ? (PH + 1) & 1 : PH & 1;
            const float4 L = lnext;
            float ov[O][4];
            unsigned lvo = 0, sso = 0;
            int nrow = 0;
            auto pre = [&](auto Cc) {                   // rect row row(k+2), channel c
                constexpr int c = decltype(Cc)::value;
                f4_unpack(raw[RS][c], XA[XS][c], XB[XS][c], hi16);
            };
            auto mid = [&](auto Ic) {
                constexpr int i = decltype(Ic)::value;
                if constexpr (i == 0) {
                    // (a row past the band's last halo row is never read: its load goes out of
                    // range, no memory access, instead of a 31st row from HBM)
                    lvo = k + 2 + PD <= n + 1 ? xoff : 0x80000000u;
                }
                if constexpr (i < C)
                    raw[LS][i] = __builtin_amdgcn_raw_buffer_load_b64(xrs, lvo, lso + i * xplane, 0);
                if constexpr (i == 3) lnext = lut[min(max(lut_e(k + 2), 0), NLUT - 1)];
                // the next step's load offset, a piece at a time (scalar instructions for the
                // places that have nothing else to put between two groups)
                if constexpr (i == 4) nrow = row(min(k + 3 + PD, n + 1));
                if constexpr (i == 5) nrow = min(max(nrow, 0), F.h - 1);
            };
            auto fin = [&] {
                lso = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)nrow * xrow));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    if constexpr (PAR == 0) f4_h2r_even(ZA[S0][o], ZB[S0][o], c13n, ov[o][0], ov[o][1], ov[o][2], ov[o][3]);
                    else f4_h2r_odd(ZA[S0][o], ZB[S0][o], c13p, ov[o][0], ov[o][1], ov[o][2], ov[o][3]);
                }
                __builtin_amdgcn_sched_barrier(0);
                sso = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)row(k) * yrow));
            };
            auto put = [&](auto Oc) {
                constexpr int o = decltype(Oc)::value;
                typedef __bf16 t2v __attribute__((ext_vector_type(2)));
                const f4_u2 v = {__builtin_bit_cast(unsigned, t2v{(__bf16)ov[o][0], (__bf16)ov[o][1]}),
                                 __builtin_bit_cast(unsigned, t2v{(__bf16)ov[o][2], (__bf16)ov[o][3]})};
                __builtin_amdgcn_raw_buffer_store_b64(v, yrs, yoff, sso + o * yplane, 0);
            };
            urow(PHc, L, std::true_type{}, std::true_type{}, pre, mid, fin, put);
        };
        auto block6 = [&](int base) {
            step(IC<0>{}, base);
            step(IC<1>{}, base + 1);
            step(IC<2>{}, base + 2);
            step(IC<3>{}, base + 3);
            step(IC<4>{}, base + 4);
            step(IC<5>{}, base + 5);
        };
        int base = 0;
        for (; base + 6 <= n; base += 6) block6(base);
        if constexpr (!UP) {                            // (UP bands are whole 6-step blocks)
            if (base < n) {
                step(IC<0>{}, base);
                if (base + 1 < n) {
                    step(IC<1>{}, base + 1);
                    if (base + 2 < n) {
                        step(IC<2>{}, base + 2);
                        if (base + 3 < n) {
                            step(IC<3>{}, base + 3);
                            if (base + 4 < n) step(IC<4>{}, base + 4);
                        }
                    }
                }
            }
        }
    };
    auto dir = [&](auto CDc, auto RCc) {
        if (F4_REV && up) run(CDc, RCc, std::true_type{});
        else run(CDc, RCc, std::false_type{});
    };
    if (cd == 1 && rc == 1) dir(IC<1>{}, IC<1>{});
    else if (cd == 1 && rc == 2) dir(IC<1>{}, IC<2>{});
    else if (cd == 2 && rc == 1) dir(IC<2>{}, IC<1>{});
    else if (cd == 2 && rc == 2) dir(IC<2>{}, IC<2>{});
    else dir(IC<0>{}, IC<0>{});
}

// The 4-column kernel for a call fused_try has validated (same-size lattice, padding 1,
// value 0); HG_EUNSUP outside its narrower domain (the caller runs k_fused).
int fused4_try(const void* x, const float* k, const float* bias, void* y, int x_dtype, int y_dtype,
               int C, int O, int G, const FusedGeom& F0, int op, hipStream_t st) {
    if (env_is("HYGRID_FUSED4", "0")) return HG_EUNSUP;   // A/B switch: the 2-column kernel
    if (x_dtype != HG_BF16 || y_dtype != HG_BF16 || C != 3 || O != 3 || G != 1) return HG_EUNSUP;
    if ((F0.w % 4) || (F0.w2 % 4) || F0.w < 4) return HG_EUNSUP;
    FusedGeom F = F0;
    F.nwin = (int)((F.w2 + F4_OWN - 1) / F4_OWN);
    F.nband = (int)((F.h2 + F4_RB - 1) / F4_RB);
    const int64_t blocks = F.B * (int64_t)F.nband * ((F.nwin + F4_GW - 1) / F4_GW);
    if (blocks > INT_MAX) return HG_EUNSUP;
    const dim3 grid((unsigned)blocks), blk(F4_THREADS);
    if (op)
        hipLaunchKernelGGL((k_fused4<1>), grid, blk, 0, st, (const __bf16*)x, k, bias, (__bf16*)y, F);
    else
        hipLaunchKernelGGL((k_fused4<0>), grid, blk, 0, st, (const __bf16*)x, k, bias, (__bf16*)y, F);
    return launch_status();
}

}  // namespace hg

namespace hg {
// band rows / owned columns / left halo of the 4-column kernel (hg_fused_layout(6, ...): tests
// place edge inputs from it)
void fused4_layout(int* band_rows, int* win_own, int* win_halo) {
    *band_rows = F4_RB;
    *win_own = F4_OWN;
    *win_halo = F4_HL;
}
}  // namespace hg
