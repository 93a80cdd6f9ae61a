// pipeline_bwd.hip — gradients of the fused rect -> hex -> HexConv2d(r=2) -> hex -> rect pass
// (hg_pipeline_r2h_conv_h2r_backward), with every hex-sized intermediate on chip.
//
// The reference differentiates the chain through torch autograd over rect_to_hex_resample
// (geometry_np.py:358-519, bilinear), HexConv2d (HexFrames.py:96-169, radius 2, stride 1,
// padding 1, constant 0) and hex_to_rect_resample (geometry_np.py:191-356, linear).  The
// domain is the forward streaming kernel's (fused.hip): same-size lattices, so
//   * h2r^T is a two-tap row-parity filter (the transpose of geometry_np.py:347-354 on the
//     exact lattice):  gz[a][q] = 0.75 gy[a][q] + 0.25 gy[a][q-1]  on even rows a,
//                      gz[a][q] = 0.75 gy[a][q] + 0.25 gy[a][q+1]  on odd rows,
//     a term dropped where the forward's vertex was outside the raster;
//   * u = r2h(x) is recomputed from x with the forward's weights (lattice.h, fp64 then fp32);
//   * dK[o][c][t] = sum gz[o][a][q] * P[c][a + ii_t][q + dk_t(a & 1)], P = u padded by one
//     sample of 0, db[o] = sum gz[o];
//   * du = conv^T gz (the 7 taps transposed), dx = r2h^T du.  in(r) - r and jn(q) - q lie in
//     {-1, 0} (fused_geometry_ok), so r2h^T gathers the 3 x 3 hex neighbourhood of a rect pixel.
// Widths may be odd (the forward then runs pipeline.hip's kernels; this file has no
// column-pair loads).
//
// Two passes, plain tiled HIP with LDS staging, no atomics and no memset:
//   k_chain_bwd_w       a workgroup walks CB_BAND tiles (CB_TR hex rows x CB_TC columns each)
//                       of one image, accumulates its pixels' dK / db products in fp32
//                       registers, reduces them in a fixed order and writes one slab row;
//   k_chain_bwd_reduce  sums the slab rows in a fixed order (bit-reproducible call to call);
//   k_chain_bwd_x       one tile of dx per workgroup: gy -> gz -> du -> dx, a pure gather.
#include <climits>

#include "common.h"
#include "fused.h"
#include "lattice.h"

namespace hg {

constexpr int CB_THREADS = 256;
constexpr int CB_TR = 16;     // tile rows (4 per wave)
constexpr int CB_TC = 64;     // tile columns (one per lane)
constexpr int CB_BAND = 8;    // tiles (top to bottom) per workgroup of the weight pass
constexpr int CB_RED = 256;   // threads of the slab reducer
constexpr int CB_U = 6;       // staging loads in flight per thread

struct ChainBwdGeom {
    int64_t B;
    int h, w, h1, w1;
    int op;                // (even_odd_offset + padding) & 1
    int nct, nband, nrt;   // column tiles, weight-pass bands, input-pass row tiles
    Geom r2h;
};

// Tap t of the r = 2 stencil on an output row of parity par: row offset ii and column offset
// dk into the padded image P (hexconv.hip / pipeline.hip's tap_dk, here with run-time par, op).
__host__ __device__ constexpr int cb_ii(int t) { return t < 2 ? 0 : (t < 5 ? 1 : 2); }
__host__ __device__ constexpr int cb_col(int t) {
    return t < 2 ? 1 + 2 * t : (t < 5 ? 2 * (t - 2) : 1 + 2 * (t - 5));
}
__host__ __device__ __forceinline__ int cb_dk(int t, int par, int op) {
    return (1 + par + cb_col(t) - ((par + cb_ii(t) + op) & 1)) >> 1;
}

template <typename T>
__device__ __forceinline__ float cb_load(const T* p, int64_t i) { return to_acc<float>(p[i]); }

// ---------------------------------------------------------------------------
// weight / bias pass
// ---------------------------------------------------------------------------
template <typename Tx, typename Tg, int C, int G>
__global__ __launch_bounds__(CB_THREADS) void k_chain_bwd_w(const Tx* __restrict__ x,
                                                            const Tg* __restrict__ gy,
                                                            float* __restrict__ slab,
                                                            ChainBwdGeom F) {
    constexpr int O = C, CG = C / G, NK = O * CG * 7, NP = NK + O;
    constexpr int XH = CB_TR + 4, XW = CB_TC + 5;   // x rows r0-2 .. r0+TR+1, cols c0-2 .. c0+TC+2
    constexpr int UH = CB_TR + 2, UW = CB_TC + 3;   // u rows r0-1 .. r0+TR,   cols c0-1 .. c0+TC+1
    __shared__ float xs[C][XH][XW];
    __shared__ float us[C][UH][UW];
    constexpr int GSW = CB_TC + 2;                  // gy rows r0 .. r0+TR-1, cols c0-1 .. c0+TC
    __shared__ float gs[O][CB_TR][GSW];
    __shared__ int rin[UH], cjn[UW];
    __shared__ float rfi[UH], rgi[UH], cfj[UW], cgj[UW];
    __shared__ float red[CB_THREADS / 64][NP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = (int)(blockIdx.x % (unsigned)F.nct);
    const int64_t rest = blockIdx.x / (unsigned)F.nct;
    const int band = (int)(rest % F.nband);
    const int64_t b = rest / F.nband;
    const int c0 = ct * CB_TC;
    const int q = c0 + lane;
    const int64_t xplane = (int64_t)F.h * F.w, gplane = (int64_t)F.h1 * F.w1;
    const Tx* xb = x + b * C * xplane;
    const Tg* gb = gy + b * O * gplane;

    // r2h column table of the tile: rect column jn and the weights of jn, jn + 1, a tap
    // outside the raster folded to weight 0 (geometry_np.py:441-486)
    for (int e = tid; e < UW; e += CB_THREADS) {
        const int qq = c0 - 1 + e;
        int jn = 0;
        float fj = 0.f, gj = 0.f;
        if (qq >= 0 && qq < F.w1) {
            const R2HSample s = r2h_sample(F.r2h, 0, qq);
            jn = (int)s.j_n;
            if (jn >= 0 && jn < F.w) gj = (float)(1.0 - s.j_f);
            if (jn + 1 >= 0 && jn + 1 < F.w) fj = (float)s.j_f;
        }
        cjn[e] = jn; cfj[e] = fj; cgj[e] = gj;
    }

    float acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.f;

    for (int ch = 0; ch < CB_BAND; ++ch) {
        const int r0 = (band * CB_BAND + ch) * CB_TR;
        if (r0 >= F.h1) break;
        __syncthreads();   // the previous tile's readers of xs / us / gs / the row table are done
        for (int e = tid; e < UH; e += CB_THREADS) {
            const int r = r0 - 1 + e;
            int in = 0;
            float fi = 0.f, gi = 0.f;
            if (r >= 0 && r < F.h1) {
                const R2HSample s = r2h_sample(F.r2h, r, 0);
                in = (int)s.i_n;
                if (in >= 0 && in < F.h) gi = (float)(1.0 - s.i_f);
                if (in + 1 >= 0 && in + 1 < F.h) fi = (float)s.i_f;
            }
            rin[e] = in; rfi[e] = fi; rgi[e] = gi;
        }
        // Staging loads are branch-free (clamped address, value selected afterwards) and issued
        // CB_U at a time, so a tile costs a few memory latencies, not one per element.
        float* xsf = &xs[0][0][0];
        for (int base = tid; base < C * XH * XW; base += CB_THREADS * CB_U) {
            float v[CB_U];
#pragma unroll
            for (int u = 0; u < CB_U; ++u) {
                const int idx = min(base + u * CB_THREADS, C * XH * XW - 1);
                const int c = idx / (XH * XW), rem = idx - c * (XH * XW);
                const int rr = rem / XW, cc = rem - rr * XW;
                const int i = r0 - 2 + rr, j = c0 - 2 + cc;
                const bool ok = i >= 0 && i < F.h && j >= 0 && j < F.w;
                const float t = cb_load(xb, c * xplane + (int64_t)min(max(i, 0), F.h - 1) * F.w +
                                                min(max(j, 0), F.w - 1));
                v[u] = ok ? t : 0.f;
            }
#pragma unroll
            for (int u = 0; u < CB_U; ++u)
                if (base + u * CB_THREADS < C * XH * XW) xsf[base + u * CB_THREADS] = v[u];
        }
        float* gsf = &gs[0][0][0];
        for (int base = tid; base < O * CB_TR * GSW; base += CB_THREADS * CB_U) {
            float v[CB_U];
#pragma unroll
            for (int u = 0; u < CB_U; ++u) {
                const int idx = min(base + u * CB_THREADS, O * CB_TR * GSW - 1);
                const int o = idx / (CB_TR * GSW), rem = idx - o * (CB_TR * GSW);
                const int rr = rem / GSW, cc = rem - rr * GSW;
                const int a = r0 + rr, qq = c0 - 1 + cc;
                const bool ok = a < F.h1 && qq >= 0 && qq < F.w1;
                const float t = cb_load(gb, o * gplane + (int64_t)min(a, F.h1 - 1) * F.w1 +
                                                min(max(qq, 0), F.w1 - 1));
                v[u] = ok ? t : 0.f;
            }
#pragma unroll
            for (int u = 0; u < CB_U; ++u)
                if (base + u * CB_THREADS < O * CB_TR * GSW) gsf[base + u * CB_THREADS] = v[u];
        }
        __syncthreads();
        // u = r2h(x) on the tile + one sample of halo, 0 outside the hex raster (the padding)
        for (int idx = tid; idx < UH * UW; idx += CB_THREADS) {
            const int rr = idx / UW, cc = idx - rr * UW;
            const int r = r0 - 1 + rr, qq = c0 - 1 + cc;
            const bool ok = r >= 0 && r < F.h1 && qq >= 0 && qq < F.w1;
            // a live tap has in - r, jn - q in {-1, 0}; the clamps only keep a dead one in the tile
            const int ti = min(max(rin[rr] - (r0 - 2), 0), XH - 2);
            const int tj = min(max(cjn[cc] - (c0 - 2), 0), XW - 2);
            const float fi = rfi[rr], gi = rgi[rr], fj = cfj[cc], gj = cgj[cc];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float vl = fi * xs[c][ti + 1][tj] + gi * xs[c][ti][tj];
                const float vr = fi * xs[c][ti + 1][tj + 1] + gi * xs[c][ti][tj + 1];
                us[c][rr][cc] = ok ? fj * vr + gj * vl : 0.f;
            }
        }
        __syncthreads();
        // this wave's 4 rows of the tile, one column per lane
#pragma unroll 1
        for (int k = 0; k < CB_TR / 4; ++k) {
            const int tr = wv * (CB_TR / 4) + k;
            const int a = r0 + tr;
            if (a >= F.h1) break;                       // wave-uniform
            const int par = a & 1;
            const int nc = par ? lane + 2 : lane;       // gy column q + 1 (odd rows) or q - 1
            float gz[O];
#pragma unroll
            for (int o = 0; o < O; ++o) {
                // no conv output past w1: those lanes add nothing
                gz[o] = q < F.w1 ? 0.75f * gs[o][tr][lane + 1] + 0.25f * gs[o][tr][nc] : 0.f;
                acc[NK + o] += gz[o];
            }
            int dk[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) dk[t] = cb_dk(t, par, F.op);
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int t = 0; t < 7; ++t) {
                    // P[a + ii][q + dk] = u[a - 1 + ii][q - 1 + dk]
                    const float p = us[c][tr + cb_ii(t)][lane + dk[t]];
                    if constexpr (G == 1) {
#pragma unroll
                        for (int o = 0; o < O; ++o) acc[(o * C + c) * 7 + t] += gz[o] * p;
                    } else {
                        acc[c * 7 + t] += gz[c] * p;
                    }
                }
            }
        }
    }

    // fixed-order reduction: butterfly inside the wave, then the 4 waves in order
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        float v = acc[i];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) red[wv][i] = v;
    }
    __syncthreads();
    if (tid < NP) {
        float s = red[0][tid];
#pragma unroll
        for (int k = 1; k < CB_THREADS / 64; ++k) s += red[k][tid];
        slab[(int64_t)blockIdx.x * NP + tid] = s;
    }
}

// Column j of the (nrows, np) slab summed in a fixed order: thread t adds rows t, t + 256, ...
// top to bottom, then a fixed tree over the 256 partial sums.  One workgroup per column.
__global__ __launch_bounds__(CB_RED) void k_chain_bwd_reduce(const float* __restrict__ slab,
                                                             int64_t nrows, int np, int nk,
                                                             float* __restrict__ dk,
                                                             float* __restrict__ db) {
    __shared__ float part[CB_RED];
    const int j = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int64_t i = tid; i < nrows; i += CB_RED) s += slab[i * np + j];
    part[tid] = s;
    __syncthreads();
    for (int st = CB_RED / 2; st >= 1; st >>= 1) {
        if (tid < st) part[tid] += part[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        if (j < nk) { if (dk) dk[j] = part[0]; }
        else if (db) db[j - nk] = part[0];
    }
}

// ---------------------------------------------------------------------------
// input pass
// ---------------------------------------------------------------------------
template <typename Tx, typename Tg, int C, int G>
__global__ __launch_bounds__(CB_THREADS) void k_chain_bwd_x(const float* __restrict__ kern,
                                                            const Tg* __restrict__ gy,
                                                            Tx* __restrict__ dx, ChainBwdGeom F) {
    constexpr int O = C, CG = C / G;
    constexpr int GH = CB_TR + 4, GW = CB_TC + 5;   // gz rows i0-2 .. i0+TR+1, cols j0-3 .. j0+TC+1
    constexpr int DH = CB_TR + 2, DW = CB_TC + 2;   // du rows i0-1 .. i0+TR,   cols j0-1 .. j0+TC
    __shared__ float gzs[O][GH][GW];
    __shared__ float dus[C][DH][DW];
    __shared__ float roww[CB_TR][3], colw[CB_TC][3];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = (int)(blockIdx.x % (unsigned)F.nct);
    const int64_t rest = blockIdx.x / (unsigned)F.nct;
    const int rt = (int)(rest % F.nrt);
    const int64_t b = rest / F.nrt;
    const int i0 = rt * CB_TR, j0 = ct * CB_TC;
    const int64_t xplane = (int64_t)F.h * F.w, gplane = (int64_t)F.h1 * F.w1;
    const Tg* gb = gy + b * O * gplane;
    Tx* dxb = dx + b * C * xplane;

    // r2h^T weights: rect row i0 + e gathers hex rows i0 + e - 1 + k, k = 0..2, with the
    // weight the forward gave rect row i in hex row r (geometry_np.py:440-486); columns alike
    for (int e = tid; e < CB_TR * 3; e += CB_THREADS) {
        const int ti = e / 3, k = e - ti * 3;
        const int i = i0 + ti, r = i - 1 + k;
        float wgt = 0.f;
        if (i < F.h && r >= 0 && r < F.h1) {
            const R2HSample s = r2h_sample(F.r2h, r, 0);
            if (s.i_n == i) wgt += (float)(1.0 - s.i_f);
            if (s.i_n + 1 == i) wgt += (float)s.i_f;
        }
        roww[ti][k] = wgt;
    }
    for (int e = tid; e < CB_TC * 3; e += CB_THREADS) {
        const int tj = e / 3, k = e - tj * 3;
        const int j = j0 + tj, qq = j - 1 + k;
        float wgt = 0.f;
        if (j < F.w && qq >= 0 && qq < F.w1) {
            const R2HSample s = r2h_sample(F.r2h, 0, qq);
            if (s.j_n == j) wgt += (float)(1.0 - s.j_f);
            if (s.j_n + 1 == j) wgt += (float)s.j_f;
        }
        colw[tj][k] = wgt;
    }
    // gz = h2r^T gy on the tile + halo, 0 outside the hex raster
    // (loads branch-free and CB_U at a time, as in the weight pass)
    float* gzf = &gzs[0][0][0];
    for (int base = tid; base < O * GH * GW; base += CB_THREADS * CB_U) {
        float v[CB_U];
#pragma unroll
        for (int u = 0; u < CB_U; ++u) {
            const int idx = min(base + u * CB_THREADS, O * GH * GW - 1);
            const int o = idx / (GH * GW), rem = idx - o * (GH * GW);
            const int rr = rem / GW, cc = rem - rr * GW;
            const int a = i0 - 2 + rr, qq = j0 - 3 + cc;
            const int qn = (a & 1) ? qq + 1 : qq - 1;
            const bool ok = a >= 0 && a < F.h1 && qq >= 0 && qq < F.w1;
            const bool nok = ok && qn >= 0 && qn < F.w1;
            const int64_t row = o * gplane + (int64_t)min(max(a, 0), F.h1 - 1) * F.w1;
            const float g = cb_load(gb, row + min(max(qq, 0), F.w1 - 1));
            const float nb = cb_load(gb, row + min(max(qn, 0), F.w1 - 1));
            v[u] = ok ? 0.75f * g + 0.25f * (nok ? nb : 0.f) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CB_U; ++u)
            if (base + u * CB_THREADS < O * GH * GW) gzf[base + u * CB_THREADS] = v[u];
    }
    __syncthreads();
    // du = conv^T gz: u[r][q] = P[r + 1][q + 1] was read by output (a, q') with
    // a = r + 1 - ii_t, q' = q + 1 - dk_t(a & 1)
    for (int idx = tid; idx < DH * DW; idx += CB_THREADS) {
        const int rr = idx / DW, cc = idx - rr * DW;
        const int r = i0 - 1 + rr, qq = j0 - 1 + cc;
        float du[C];
#pragma unroll
        for (int c = 0; c < C; ++c) du[c] = 0.f;
        if (r >= 0 && r < F.h1 && qq >= 0 && qq < F.w1) {
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const int ii = cb_ii(t);
                const int par = (r + 1 - ii) & 1;
                const int gr = rr + 2 - ii;                     // a - (i0 - 2), in [0, GH)
                const int gc = cc + 3 - cb_dk(t, par, F.op);    // q' - (j0 - 3), in [0, GW)
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    const float g = gzs[o][gr][gc];
                    if constexpr (G == 1) {
#pragma unroll
                        for (int c = 0; c < C; ++c) du[c] += kern[(o * CG + c) * 7 + t] * g;
                    } else {
                        du[o] += kern[o * 7 + t] * g;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dus[c][rr][cc] = du[c];
    }
    __syncthreads();
    // dx = r2h^T du: every element written exactly once
    const int j = j0 + lane;
    if (j >= F.w) return;
    const float cw0 = colw[lane][0], cw1 = colw[lane][1], cw2 = colw[lane][2];
#pragma unroll 1
    for (int k = 0; k < CB_TR / 4; ++k) {
        const int ti = wv * (CB_TR / 4) + k;
        const int i = i0 + ti;
        if (i >= F.h) break;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const float* d = &dus[c][ti + m][lane];
                s += roww[ti][m] * ((cw0 * d[0] + cw1 * d[1]) + cw2 * d[2]);
            }
            dxb[c * xplane + (int64_t)i * F.w + j] = from_acc<Tx>(s);
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static bool cb_float(int dt) { return dt == HG_BF16 || dt == HG_F16 || dt == HG_F32; }

// Argument check and work decomposition, shared by the workspace query and the call.
static int chain_bwd_plan(int x_dtype, int gy_dtype, int64_t batch, int64_t channels,
                          int64_t out_channels, int64_t h, int64_t w, int64_t h1, int64_t w1,
                          int64_t h2, int64_t w2, int padding, int groups, int even_odd_offset,
                          double pad_value, ChainBwdGeom* F, int* np, int64_t* slab_rows) {
    if (batch < 0 || h < 1 || w < 1 || h1 < 1 || w1 < 1 || h2 < 0 || w2 < 0 || padding < 0)
        return HG_EINVAL;
    if (groups < 1 || channels < 1 || out_channels < 1 || channels % groups || out_channels % groups)
        return HG_EINVAL;
    if (h > INT_MAX / 4 || w > INT_MAX / 4 || h1 > INT_MAX / 4 || w1 > INT_MAX / 4 ||
        h2 > INT_MAX / 4 || w2 > INT_MAX / 4)
        return HG_ESHAPE;
    // the domain of fused_try (fused.hip), widths of either parity
    if (padding != 1 || pad_value != 0.0) return HG_EUNSUP;
    if (h2 != h1 || w2 != w1) return HG_EUNSUP;
    if (!cb_float(x_dtype) || !cb_float(gy_dtype)) return HG_EUNSUP;
    const int C = (int)channels, O = (int)out_channels, G = groups;
    if (!((C == 3 && O == 3 && (G == 1 || G == 3)) || (C == 1 && O == 1 && G == 1)))
        return HG_EUNSUP;
    if (C * h * w * 8 >= ((int64_t)1 << 31) || O * h2 * w2 * 4 >= ((int64_t)1 << 31))
        return HG_EUNSUP;
    const Geom g = make_r2h(h, w, h1, w1);
    if (!fused_geometry_ok(g)) return HG_EUNSUP;
    F->B = batch;
    F->h = (int)h; F->w = (int)w; F->h1 = (int)h1; F->w1 = (int)w1;
    F->op = (even_odd_offset + padding) & 1;
    F->r2h = g;
    const int64_t wmax = w > w1 ? w : w1;   // both passes tile the same column grid
    F->nct = (int)((wmax + CB_TC - 1) / CB_TC);
    F->nband = (int)((h1 + CB_TR * CB_BAND - 1) / (CB_TR * CB_BAND));
    F->nrt = (int)((h + CB_TR - 1) / CB_TR);
    if (batch * F->nband * F->nct > INT_MAX || batch * F->nrt * F->nct > INT_MAX) return HG_ESHAPE;
    *np = O * (C / G) * 7 + O;
    *slab_rows = batch * F->nband * F->nct;
    return HG_OK;
}

// Workspace bytes of a slab of `rows` rows of np floats: a positive multiple of 16.
static int64_t chain_bwd_bytes(int64_t rows, int np) {
    const int64_t bytes = rows * np * (int64_t)sizeof(float);
    return bytes < 16 ? 16 : (bytes + 15) & ~(int64_t)15;
}

template <typename Tx, typename Tg, int C, int G>
static int chain_bwd_launch(const void* x, const float* kernel, const void* gy, void* dx,
                            float* slab, const ChainBwdGeom& F, bool weights, hipStream_t st) {
    if (weights) {
        const dim3 grid((unsigned)(F.B * F.nband * F.nct)), blk(CB_THREADS);
        hipLaunchKernelGGL((k_chain_bwd_w<Tx, Tg, C, G>), grid, blk, 0, st, (const Tx*)x,
                           (const Tg*)gy, slab, F);
    }
    if (dx) {
        const dim3 grid((unsigned)(F.B * F.nrt * F.nct)), blk(CB_THREADS);
        hipLaunchKernelGGL((k_chain_bwd_x<Tx, Tg, C, G>), grid, blk, 0, st, kernel, (const Tg*)gy,
                           (Tx*)dx, F);
    }
    return launch_status();
}

template <typename Tx, typename Tg>
static int chain_bwd_channels(const void* x, const float* kernel, const void* gy, void* dx,
                              float* slab, const ChainBwdGeom& F, int C, int G, bool weights,
                              hipStream_t st) {
    if (C == 3 && G == 1) return chain_bwd_launch<Tx, Tg, 3, 1>(x, kernel, gy, dx, slab, F, weights, st);
    if (C == 3 && G == 3) return chain_bwd_launch<Tx, Tg, 3, 3>(x, kernel, gy, dx, slab, F, weights, st);
    return chain_bwd_launch<Tx, Tg, 1, 1>(x, kernel, gy, dx, slab, F, weights, st);
}

template <typename Tx>
static int chain_bwd_gy(const void* x, const float* kernel, const void* gy, void* dx, float* slab,
                        const ChainBwdGeom& F, int gy_dtype, int C, int G, bool weights,
                        hipStream_t st) {
    switch (gy_dtype) {
    case HG_BF16: return chain_bwd_channels<Tx, __bf16>(x, kernel, gy, dx, slab, F, C, G, weights, st);
    case HG_F16: return chain_bwd_channels<Tx, _Float16>(x, kernel, gy, dx, slab, F, C, G, weights, st);
    default: return chain_bwd_channels<Tx, float>(x, kernel, gy, dx, slab, F, C, G, weights, st);
    }
}

void chain_bwd_layout(int* tile_rows, int* tile_cols, int* band_tiles) {
    *tile_rows = CB_TR;
    *tile_cols = CB_TC;
    *band_tiles = CB_BAND;
}

}  // namespace hg

extern "C" int64_t hg_pipeline_r2h_conv_h2r_backward_workspace(
        int x_dtype, int gy_dtype, int64_t batch, int64_t channels, int64_t out_channels, int64_t h,
        int64_t w, int64_t h1, int64_t w1, int64_t h2, int64_t w2, int padding, int groups,
        int even_odd_offset, double pad_value) {
    hg::ChainBwdGeom F;
    int np = 0;
    int64_t rows = 0;
    const int rc = hg::chain_bwd_plan(x_dtype, gy_dtype, batch, channels, out_channels, h, w, h1,
                                      w1, h2, w2, padding, groups, even_odd_offset, pad_value, &F,
                                      &np, &rows);
    if (rc != HG_OK) return rc;
    return hg::chain_bwd_bytes(rows, np);
}

extern "C" int hg_pipeline_r2h_conv_h2r_backward(
        const void* x, const float* kernel, const void* gy, void* dx, float* dkernel, float* dbias,
        int x_dtype, int gy_dtype, int64_t batch, int64_t channels, int64_t out_channels, int64_t h,
        int64_t w, int64_t h1, int64_t w1, int64_t h2, int64_t w2, int padding, int groups,
        int even_odd_offset, double pad_value, void* workspace, int64_t workspace_bytes,
        void* stream) {
    using namespace hg;
    ChainBwdGeom F;
    int np = 0;
    int64_t rows = 0;
    const int rc = chain_bwd_plan(x_dtype, gy_dtype, batch, channels, out_channels, h, w, h1, w1,
                                  h2, w2, padding, groups, even_odd_offset, pad_value, &F, &np,
                                  &rows);
    if (rc != HG_OK) return rc;
    if (!x || !gy || !kernel) return HG_EINVAL;
    const bool weights = dkernel || dbias;
    if (weights && (!workspace || workspace_bytes < chain_bwd_bytes(rows, np)))
        return HG_EINVAL;
    if (!weights && !dx) return HG_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int C = (int)channels, G = groups;
    float* slab = static_cast<float*>(workspace);
    if (rows > 0) {
        int lrc;
        switch (x_dtype) {
        case HG_BF16: lrc = chain_bwd_gy<__bf16>(x, kernel, gy, dx, slab, F, gy_dtype, C, G, weights, st); break;
        case HG_F16: lrc = chain_bwd_gy<_Float16>(x, kernel, gy, dx, slab, F, gy_dtype, C, G, weights, st); break;
        default: lrc = chain_bwd_gy<float>(x, kernel, gy, dx, slab, F, gy_dtype, C, G, weights, st); break;
        }
        if (lrc != HG_OK) return lrc;
    }
    if (weights) {   // rows == 0 (an empty batch): the sums are 0
        hipLaunchKernelGGL(k_chain_bwd_reduce, dim3((unsigned)np), dim3(CB_RED), 0, st, slab, rows,
                           np, np - (int)out_channels, dkernel, dbias);
        return launch_status();
    }
    return HG_OK;
}
