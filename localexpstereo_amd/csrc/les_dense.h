// les_dense.h -- the unary cost of a whole label map in one dense pass (gfx950 / CDNA4, wave64).
//
// What is computed (reference: the warm-start branch of FastGCStereo::initCurrentFast, LES/FastGCStereo.h:116-130): for every pixel
// p = (x, y) of a region, with its OWN plane labels[y][x],
//   F       = [x - windR, x + windR] x [y - windR, y + windR] clipped to the image
//   cost(p) = ComputeUnaryPotential(filterRect = F, targetRect = (x, y, 1, 1), labels(p))
// i.e. what the strip kernel (les_kernels.h) returns for one (F, 1 x 1) job per pixel.  Because windR >= 2 (windR / 2), every box of the
// guided filter that reaches p lies inside F, so the sub-region filter's window counts at p are the whole image's:
//   q_p = 1/N_p sum_{k in w_p} (a_k . I_p + b_k),   a_k = Sigma_k^-1 (box_k(c I)/N_k - mu_k box_k(c)/N_k),   b_k = box_k(c)/N_k - a_k . mu_k
// with c_s the raw cost of labels(p) at s, w_k the (2R + 1)^2 box around k clipped to the image and R = windR / 2.
//
// Kernel structure: a workgroup owns a tile of TX x TY output pixels.  The guide statistics of the tile's centres (tile +- R, nine floats each:
// three means, six entries of the symmetric inverse covariance) and the packed guide of the tile's cost window (tile +- 2R) go to LDS once and
// serve every pixel of the tile.  A wave owns one pixel at a time: lane l owns column x - windR + l of F (2 windR + 1 <= 63 columns) and the
// wave marches down the rows of F:
//   G   one raw cost per lane (the device functions of les_kernels.h / les_vdisp.h: the very arithmetic of every other kernel)
//   V   vertical 2R+1 running sums of (I'_0 c, I'_1 c, I'_2 c, c) in fp64 registers; the cost that leaves the window comes back from a ring
//       of 2R+1 rows in LDS, its guide pixel from the tile's guide halo
//   H   once 2R+1 rows are in: the four sums cross the lanes through LDS, the 2R+1 centre lanes add their 2R+1 neighbours (fp64), do the 3x3
//       algebra of VLane::step (les_kernels.h) against the statistics in LDS and add (a_0, a_1, a_2, b) to four fp64 accumulators
// and ends with one butterfly sum over the wave, the weighting by I'(p) and 1/N_p.  Nothing is rounded below fp64 except the products I' c, the
// covariance and (a, b), which are f32 exactly as in the strip kernel.
// The reference sums its boxes with running sums, so a NaN raw cost (the end slices of interpolation 2) at (xn, yn) of F reaches every
// q(x, y) with x >= xn - 2R and y >= yn - 2R (les_nan_spread_kernel): here, any NaN of F at or left of x + 2R and at or above y + 2R.
//
// FILT 1 is the direct form of the same skeleton for the bilateral ("BF" / "BL": q_p = sum_{s in F} exp(-|I_p - I_s|_1 / sig2) c_s, radius
// windR, not normalised) and the unfiltered ("": q_p = c_p bit for bit, radius 0) aggregation; only the guide halo and the weight table are in LDS.
//
// Also compiled by the CPU fiber simulator (test infrastructure only) with LES_SIM defined.  No inline assembly.
#pragma once

#include "les_kernels.h"
#include "les_vdisp.h"
#include "les_bilateral.h"

namespace les {

// Tile and workgroup shape per guided-filter radius: what fits 64 KiB of LDS (statistics halo 36 B x (T + 2R)^2, guide halo 4 B x (T + 4R)^2,
// per wave a cost ring of 2R+1 rows and the exchange buffer of the four sums)
template <int R>
struct DenseCfg {
    static constexpr int TX = R <= 12 ? 8 : 2, TY = R <= 12 ? 8 : 2;
    static constexpr int NW = R <= 10 ? 4 : (R <= 12 ? 2 : 1);      // waves per workgroup
    static constexpr int NT = 64 * NW;
    static constexpr int KS = 2 * R + 1;
    static constexpr int SW = TX + 2 * R, SH = TY + 2 * R;          // centres: statistics halo
    static constexpr int GW = TX + 4 * R, GH = TY + 4 * R;          // cost window: guide halo
    static constexpr int NL = 4 * R + 1;                            // columns of the cost window of one pixel
    static constexpr int LDS_BYTES = SW * SH * 36 + GW * GH * 4 + NW * (KS * NL * 4 + 4 * NL * 8) + (KS + 1) * 8;
    static_assert(LDS_BYTES <= 65536, "tile does not fit the static LDS limit");
    static_assert(4 * R + 3 <= 64, "a wave holds the columns of F");
};

constexpr int DENSE_BF_T = 8, DENSE_BF_NW = 4;                      // FILT 1: 8 x 8 tile, four waves
constexpr int DENSE_BF_GW = DENSE_BF_T + 2 * kBfMaxR;

// SRC as for the strip kernel: 0 cost volume (linear), 1 image-based cost (Plane::v honoured), 2 / 3 cost volume at interpolation 0 / 2
template <int SRC>
__device__ __forceinline__ float dense_raw(const Geom& g, const View& view, float4 pl, int gx, int gy)
{
    if constexpr (SRC == 0) return gather_cost(g, view.vol, pl.x, pl.y, pl.z, gx, gy);
    else if constexpr (SRC == 1) {
        if (pl.w != 0.0f) return vdisp_raw(g, view, pl, gx, gy);
        const NaivePrep np = naive_prepare(g, view.sign, pl.x, pl.y, pl.z, gx, gy);
        const uint32_t px = (uint32_t)gy * (uint32_t)g.W + (uint32_t)gx;
        return naive_finish(view, np, view.feat_self[px], view.feat_other[np.ia], view.feat_other[np.ib]);
    } else return gather_cost_interp<SRC == 2 ? 0 : 2>(g, view.vol, pl.x, pl.y, pl.z, gx, gy);
}

struct DenseArgs {
    int rx, ry, rw, rh;        // region (inside the image)
    int windR;                 // Parameters::windR: F = pixel +- windR
    int check;
};

// FILT 0: guided filter of radius R.  FILT 1 (R = 0): bilateral of radius a.windR (wtab: its 766 weights) or, at radius 0, no aggregation.
template <int R, int SRC, int FILT>
__global__ void __launch_bounds__(FILT == 0 ? DenseCfg<R>::NT : 64 * DENSE_BF_NW)
les_dense_kernel(Geom g, View view, DenseArgs a, const float* __restrict__ wtab, const float4* __restrict__ labels, float* __restrict__ out)
{
    using Cfg = DenseCfg<R>;
    constexpr int TX = FILT == 0 ? Cfg::TX : DENSE_BF_T, TY = FILT == 0 ? Cfg::TY : DENSE_BF_T;
    constexpr int NW = FILT == 0 ? Cfg::NW : DENSE_BF_NW, NT = 64 * NW;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;

    // XCD-aware tile order (as the strip kernel's job order): consecutive tiles run on the same XCD and share volume halos in its L2
    int tile;
    {
        const int nwg = (int)gridDim.x, orig = (int)blockIdx.x;
        const int q = nwg / 8, r = nwg % 8, xcd = orig % 8;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
    }
    const int tiles_x = (a.rw + TX - 1) / TX;
    const int tx0 = a.rx + (tile % tiles_x) * TX, ty0 = a.ry + (tile / tiles_x) * TY;
    const int tw = min(TX, a.rx + a.rw - tx0), th = min(TY, a.ry + a.rh - ty0);
    if (tw <= 0 || th <= 0) return;
    const int windR = a.windR;

    if constexpr (FILT == 0) {
        constexpr int KS = Cfg::KS, SW = Cfg::SW, SH = Cfg::SH, GW = Cfg::GW, GH = Cfg::GH, NL = Cfg::NL;
        __shared__ float s_stats[SH * SW * 9];          // per centre: mean_I'_0..2, inv00, inv01, inv02, inv11, inv12, inv22
        __shared__ uint32_t s_ipk[GH * GW];             // packed guide of the cost window (0 outside the image)
        __shared__ float s_ring[NW][KS][NL];            // the last 2R+1 cost rows of each wave's pixel
        __shared__ double s_hv[NW][4][NL];              // the four vertical sums of the current row, by column
        __shared__ double s_rtab[KS + 1];               // 1/n, n = 0 .. 2R+1

        for (int i = tid; i < SH * SW * 9; i += NT) {
            const int rec = i / 9, j = i - rec * 9;
            const int cy = ty0 - R + rec / SW, cx = tx0 - R + rec % SW;
            // word of the view's {mean_k, inv[k][0..2]} records (k = 0..2, 12 floats per pixel) that holds entry j
            const int off = j < 3 ? 4 * j : (j < 6 ? j - 2 : (j < 8 ? j : 11));
            float v = 0.0f;
            if (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) v = reinterpret_cast<const float*>(view.stats)[((size_t)cy * g.W + cx) * 12 + off];
            s_stats[i] = v;
        }
        for (int i = tid; i < GH * GW; i += NT) {
            const int cy = ty0 - 2 * R + i / GW, cx = tx0 - 2 * R + i % GW;
            s_ipk[i] = (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) ? view.ipk[(size_t)cy * g.W + cx] : 0u;
        }
        if (tid <= KS) s_rtab[tid] = tid > 0 ? 1.0 / (double)tid : 0.0;
        __syncthreads();

        const int dx = lane - windR;                                    // this lane's column of F, relative to the pixel
        const bool col_box = dx >= -2 * R && dx <= 2 * R;               // ... carries box-sum inputs
        const int j = col_box ? dx + 2 * R : 0;                         // its column of the ring / the exchange buffer
        const bool centre_lane = dx >= -R && dx <= R;
        for (int idx = wave; idx < TX * TY; idx += NW) {
            const int py = idx / TX, pxi = idx - py * TX;
            if (pxi >= tw || py >= th) continue;                         // (wave-uniform)
            const int x = tx0 + pxi, y = ty0 + py;
            const float4 pl = labels[(size_t)y * g.W + x];
            const int cx = x + dx;
            const bool col_in = dx <= windR && cx >= 0 && cx < g.W;
            const uint32_t* gcol = &s_ipk[(py) * GW + (pxi + j)];         // guide halo entry of (cx, y - 2R); row stride GW
            double V0 = 0.0, V1 = 0.0, V2 = 0.0, V3 = 0.0;
            double A0 = 0.0, A1 = 0.0, A2 = 0.0, A3 = 0.0;
            int nan_seen = 0;
            const int nxc = window_count(cx, R, 0, g.W);
            for (int dy = -windR; dy <= windR; dy++) {
                const int cy = y + dy;
                const bool row_in = cy >= 0 && cy < g.H;
                float c = 0.0f;
                if (row_in && col_in) c = dense_raw<SRC>(g, view, pl, cx, cy);
                if constexpr (SRC >= 2) nan_seen |= (c != c && dx <= 2 * R && dy <= 2 * R) ? 1 : 0;
                if (dy < -2 * R || dy > 2 * R) continue;                 // (rows of F beyond the cost window: windR odd)
                const int t = dy + 2 * R, slot = t % KS;
                if (col_box) {
                    if (!(row_in && col_in)) c = 0.0f;
                    const uint32_t ip = gcol[t * GW];
                    float co = 0.0f;
                    uint32_t ipo = 0u;
                    if (t >= KS) { co = s_ring[wave][slot][j]; ipo = gcol[(t - KS) * GW]; }
                    s_ring[wave][slot][j] = c;
                    V0 += (double)(guide_centred_f32(ip, 0) * c) - (double)(guide_centred_f32(ipo, 0) * co);
                    V1 += (double)(guide_centred_f32(ip, 1) * c) - (double)(guide_centred_f32(ipo, 1) * co);
                    V2 += (double)(guide_centred_f32(ip, 2) * c) - (double)(guide_centred_f32(ipo, 2) * co);
                    V3 += (double)c - (double)co;
                }
                if (t < 2 * R) continue;
                const int cyc = cy - R;                                   // centre row of the window that just filled
                if (cyc < 0 || cyc >= g.H) continue;                      // (wave-uniform)
                if (col_box) { s_hv[wave][0][j] = V0; s_hv[wave][1][j] = V1; s_hv[wave][2][j] = V2; s_hv[wave][3][j] = V3; }
                wave_sync();
                if (centre_lane && cx >= 0 && cx < g.W) {
                    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0;
                    for (int i = j - R; i <= j + R; i++) { S0 += s_hv[wave][0][i]; S1 += s_hv[wave][1][i]; S2 += s_hv[wave][2][i]; S3 += s_hv[wave][3][i]; }
                    // LES/GuidedFilter.h:204-221 on the centred guide, the arithmetic of VLane::step (les_kernels.h)
                    const double rn1 = s_rtab[nxc] * s_rtab[window_count(cyc, R, 0, g.H)];
                    const float* st = &s_stats[((cyc - (ty0 - R)) * SW + (cx - (tx0 - R))) * 9];
                    const double m0 = S0 * rn1, m1 = S1 * rn1, m2 = S2 * rn1, mp = S3 * rn1;
                    const float cov0 = (float)fma(-(double)st[0], mp, m0), cov1 = (float)fma(-(double)st[1], mp, m1), cov2 = (float)fma(-(double)st[2], mp, m2);
                    const float a0 = fmaf(st[5], cov2, fmaf(st[4], cov1, st[3] * cov0));
                    const float a1 = fmaf(st[7], cov2, fmaf(st[6], cov1, st[4] * cov0));
                    const float a2 = fmaf(st[8], cov2, fmaf(st[7], cov1, st[5] * cov0));
                    const float bb = (float)mp - ((a0 * st[0] + a1 * st[1]) + (a2 * st[2] + 0.0f));
                    A0 += (double)a0; A1 += (double)a1; A2 += (double)a2; A3 += (double)bb;
                }
                wave_sync();
            }
            A0 = wave_sum_tree(A0); A1 = wave_sum_tree(A1); A2 = wave_sum_tree(A2); A3 = wave_sum_tree(A3);
            if constexpr (SRC >= 2) nan_seen = wave_sum_tree(nan_seen);
            if (lane == 0) {
                const uint32_t ip = s_ipk[(py + 2 * R) * GW + (pxi + 2 * R)];
                // LES/GuidedFilter.h:243: (b + a_r I_r + a_g I_g + a_b I_b) / N, summed as the strip kernel's quad does
                const double qn = (A0 * guide_centred_f64(ip, 0) + A1 * guide_centred_f64(ip, 1)) + (A2 * guide_centred_f64(ip, 2) + A3);
                const double rn2 = s_rtab[window_count(y, R, 0, g.H)] * s_rtab[window_count(x, R, 0, g.W)];
                float q = (float)(qn * rn2);
                if (nan_seen) q = __int_as_float(0x7fc00000);
                if (a.check && !label_valid(g, pl.x, pl.y, pl.z, pl.w, x, y)) q = LES_COST_INVALID;
                out[(size_t)y * g.W + x] = q;
            }
        }
    } else {
        __shared__ float s_tab[kBfTabSize];
        __shared__ uint32_t s_g[DENSE_BF_GW * DENSE_BF_GW];             // packed guide of tile +- windR (0 outside the image)
        const int GW = TX + 2 * windR;
        for (int i = tid; i < kBfTabSize; i += NT) s_tab[i] = wtab[i];
        for (int i = tid; i < GW * GW; i += NT) {
            const int cy = ty0 - windR + i / GW, cx = tx0 - windR + i % GW;
            s_g[i] = (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) ? view.ipk[(size_t)cy * g.W + cx] : 0u;
        }
        __syncthreads();
        const int dx = lane - windR;
        for (int idx = wave; idx < TX * TY; idx += NW) {
            const int py = idx / TX, pxi = idx - py * TX;
            if (pxi >= tw || py >= th) continue;                         // (wave-uniform)
            const int x = tx0 + pxi, y = ty0 + py;
            const float4 pl = labels[(size_t)y * g.W + x];
            const int cx = x + dx;
            const bool col_in = dx <= windR && cx >= 0 && cx < g.W;
            const uint32_t gp = s_g[(py + windR) * GW + pxi + windR];
            double acc = 0.0;
            float centre = 0.0f;
            for (int dy = -windR; dy <= windR; dy++) {
                const int cy = y + dy;
                if (cy < 0 || cy >= g.H || !col_in) continue;
                const float c = dense_raw<SRC>(g, view, pl, cx, cy);
                const float w = s_tab[bf_sad(s_g[(py + windR + dy) * GW + pxi + lane], gp)];
                acc += (double)w * (double)c;
                if (dy == 0 && dx == 0) centre = c;
            }
            acc = wave_sum_tree(acc);
            if (lane == windR) {                                         // the lane of the pixel's own column
                // radius 0 (the unfiltered energy): q = raw bit for bit (the sum 0 + 1 * raw would turn -0 into +0)
                float q = windR == 0 ? centre : (float)acc;
                if (a.check && !label_valid(g, pl.x, pl.y, pl.z, pl.w, x, y)) q = LES_COST_INVALID;
                out[(size_t)y * g.W + x] = q;
            }
        }
    }
}

}  // namespace les
