// les_planefit.h -- slanted planes from a disparity map: per pixel an edge-aware weighted least-squares plane fit over its window.  The
// reference has no counterpart: its only start is one random plane per finest-layer cell (LES/FastGCStereo.h:94-115), and every map this
// project builds without a graph cut (les_wtavol.h) is fronto-parallel.  The fitted map is a start for run() or a second labelling for
// the fusion move of les_pairwise.h.
//
// DEFINITION (stated here once; tests/planefit_cases.py restates it in numpy).
//   inputs    the packed guide ipk of the view (B | G << 8 | R << 16); EITHER labels: H x W planes (a, b, c, v) OR disp: H x W floats;
//             fallback (optional): H x W planes; radius r in 1 .. kFitMaxR; the weight table wtab[k] = (float)exp(-k / sig) for
//             k = 0 .. 765 (built on the host in double; sig == 0: all ones); gate0 > 0, gate_slope >= 0, max_slope > 0, min_support >= 3;
//             the disparity range [mind, maxd] of the energy
//   outputs   out: H x W planes; kind (optional): H x W bytes -- 2 slanted fit, 1 fronto-parallel at the pixel's own disparity, 0 fallback
//   d(s)      from labels: (a xs + b ys) + c in f32, not contracted (les_disparity_kernel's order), and v(s) the label's v;
//             from a disparity map: the map's value, and v = 0
//   For the target p = (x, y), d0 = d(p), v = v(p):
//     FALLBACK  the fallback's label at p bit for bit, (0, 0, mind, 0) without a fallback map; kind 0
//     d0 not finite: FALLBACK.
//     The taps s = (x + dx, y + dy), |dx|, |dy| <= r, inside the image, are visited with dy outer and dx inner, both ascending.  A tap is
//     taken iff d(s) is finite and, in f32 in this order, fabsf(d(s) - d0) <= gate0 + gate_slope * (float)max(|dx|, |dy|)  (a NaN falls
//     out here).  Its weight is w = wtab[|I(p) - I(s)|_1].  With delta = d(s) - d0 (f32) the taken taps add to nine fp64 sums, in tap
//     order, every product and every sum rounded on its own (all products are exact: 24 x 24 x 4 bits), and to the count n:
//         S   += w            Sx  += w dx           Sy  += w dy
//         Sxx += (w dx) dx    Sxy += (w dx) dy      Syy += (w dy) dy
//         Sd  += w delta      Sxd += (w delta) dx   Syd += (w delta) dy
//     The normal equations [Sxx Sxy Sx; Sxy Syy Sy; Sx Sy S] (a, b, c')^T = (Sxd, Syd, Sd)^T by cofactors, in fp64, in this order:
//         C00 = Syy S - Sy Sy      C01 = Sx Sy - Sxy S      C02 = Sxy Sy - Syy Sx
//         C11 = Sxx S - Sx Sx      C12 = Sxy Sx - Sxx Sy    C22 = Sxx Syy - Sxy Sxy
//         det = (Sxx C00 + Sxy C01) + Sx C02
//         a  = ((C00 Sxd + C01 Syd) + C02 Sd) / det
//         b  = ((C01 Sxd + C11 Syd) + C12 Sd) / det
//         c' = ((C02 Sxd + C12 Syd) + C22 Sd) / det                                    (three correctly rounded fp64 divisions)
//     The fit is accepted iff  n >= min_support;  det > kFitMinDet ((S S) S)  (collinear or nearly single-tap support is refused);
//     |c'| <= gate0;  af = (float)a and bf = (float)b are finite with |af|, |bf| <= max_slope;
//     cf = (float)(((double)d0 + c') - ((double)af x + (double)bf y)) is finite;  and label_valid(af, bf, cf, 0) holds at (x, y).
//     accepted: (af, bf, cf, v), kind 2.   Otherwise, if mind <= d0 <= maxd: (0, 0, d0, v), kind 1.   Otherwise FALLBACK.
//   The result is a function of the inputs only.
//
// KERNEL  A workgroup of kFitThreads threads owns a tile of kFitTY x kFitTX outputs, one output per thread.  The disparities (computed
// from the labels while staging, when labels are given) and the packed guide of tile +- r and the weight table are staged in LDS once
// (pixels outside the image: NaN, which no gate takes); the tap loop reads LDS only.  A wave is two tile rows of 32 lanes: each half-wave
// reads 32 consecutive words, which no row stride can make collide.  Static LDS at the largest radius:
// 2 x 4 x (8 + 30) x (32 + 30) + 4 x 8 x 32 + 4 x 766 = 22936 bytes (22944 as laid out).
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_bilateral.h"

namespace les {

constexpr int kFitMaxR = 15;                // largest radius: the static LDS tile is sized for it
constexpr double kFitMinDet = 1.0e-3;       // det > kFitMinDet S^3
constexpr int kFitTX = 32, kFitTY = 8;
constexpr int kFitThreads = kFitTX * kFitTY;
constexpr int kFitHX = kFitTX + 2 * kFitMaxR, kFitHY = kFitTY + 2 * kFitMaxR;

struct FitParams {
    int radius, min_support;
    float gate0, gate_slope, max_slope;
};

__device__ __forceinline__ bool fit_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// the decision and the label of one target from its sums: true = accepted (kind 2), o = (af, bf, cf, .)
__device__ __forceinline__ bool fit_solve(const Geom& g, const FitParams& fp, int n, double S, double Sx, double Sy, double Sxx, double Sxy, double Syy,
                                          double Sd, double Sxd, double Syd, float d0, int x, int y, float4& o)
{
    if (n < fp.min_support) return false;
    const double C00 = Syy * S - Sy * Sy, C01 = Sx * Sy - Sxy * S, C02 = Sxy * Sy - Syy * Sx;
    const double C11 = Sxx * S - Sx * Sx, C12 = Sxy * Sx - Sxx * Sy, C22 = Sxx * Syy - Sxy * Sxy;
    const double det = (Sxx * C00 + Sxy * C01) + Sx * C02;
    if (!(det > kFitMinDet * ((S * S) * S))) return false;
    const double a = ((C00 * Sxd + C01 * Syd) + C02 * Sd) / det;
    const double b = ((C01 * Sxd + C11 * Syd) + C12 * Sd) / det;
    const double c = ((C02 * Sxd + C12 * Syd) + C22 * Sd) / det;
    if (!(fabs(c) <= (double)fp.gate0)) return false;
    const float af = (float)a, bf = (float)b;
    if (!fit_finite(af) || !fit_finite(bf) || !(fabsf(af) <= fp.max_slope) || !(fabsf(bf) <= fp.max_slope)) return false;
    const float cf = (float)(((double)d0 + c) - ((double)af * (double)x + (double)bf * (double)y));
    if (!fit_finite(cf) || !label_valid(g, af, bf, cf, 0.0f, x, y)) return false;
    o.x = af; o.y = bf; o.z = cf;
    return true;
}

// grid = (ceil(W / kFitTX), ceil(H / kFitTY)), block = kFitThreads.  Exactly one of labels / disp is non-null.  out may be fallback (each
// target is read and written by one thread), not the input map.
__global__ void __launch_bounds__(kFitThreads)
les_plane_fit_kernel(Geom g, const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, const float4* __restrict__ labels,
                     const float* __restrict__ disp, const float4* fallback, float4* out, uint8_t* kind, FitParams fp)
{
    __shared__ float s_tab[kBfTabSize];
    __shared__ float s_d[kFitHY][kFitHX];               // disparities of tile +- r (NaN outside the image)
    __shared__ uint32_t s_g[kFitHY][kFitHX];            // packed guide of tile +- r
    __shared__ float s_v[kFitTY][kFitTX];               // v of the tile's own labels

    const int tid = (int)threadIdx.x, r = fp.radius;
    const int x0 = (int)blockIdx.x * kFitTX, y0 = (int)blockIdx.y * kFitTY;
    const int hw = kFitTX + 2 * r, hh = kFitTY + 2 * r;
    for (int i = tid; i < kBfTabSize; i += kFitThreads) s_tab[i] = wtab[i];
    for (int i = tid; i < hw * hh; i += kFitThreads) {
        const int hy = i / hw, hx = i - hy * hw;
        const int xs = x0 - r + hx, ys = y0 - r + hy;
        float d = NAN, v = 0.0f;
        uint32_t gs = 0u;
        if (xs >= 0 && xs < g.W && ys >= 0 && ys < g.H) {
            const size_t px = (size_t)ys * g.W + xs;
            if (labels) {
                const float4 l = labels[px];
                d = (l.x * (float)xs + l.y * (float)ys) + l.z;
                v = l.w;
            } else {
                d = disp[px];
            }
            gs = ipk[px];
        }
        s_d[hy][hx] = d;
        s_g[hy][hx] = gs;
        const int ty = hy - r, tx = hx - r;
        if (ty >= 0 && ty < kFitTY && tx >= 0 && tx < kFitTX) s_v[ty][tx] = v;
    }
    __syncthreads();

    const int ty = tid / kFitTX, tx = tid - ty * kFitTX;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= g.W || y >= g.H) return;
    const float d0 = s_d[ty + r][tx + r], v = s_v[ty][tx];
    const uint32_t gc = s_g[ty + r][tx + r];
    const size_t px = (size_t)y * g.W + x;

    float4 o;
    uint8_t k = 0;
    if (fit_finite(d0)) {
        int n = 0;
        double S = 0.0, Sx = 0.0, Sy = 0.0, Sxx = 0.0, Sxy = 0.0, Syy = 0.0, Sd = 0.0, Sxd = 0.0, Syd = 0.0;
        for (int dy = -r; dy <= r; dy++) {
            const float* drow = &s_d[ty + r + dy][tx];
            const uint32_t* grow = &s_g[ty + r + dy][tx];
            const int ady = dy < 0 ? -dy : dy;
            const double fy = (double)dy;
            for (int j = 0; j <= 2 * r; j++) {
                const int dx = j - r, adx = dx < 0 ? -dx : dx;
                const float ds = drow[j];
                const float delta = ds - d0;
                const float lim = fp.gate0 + fp.gate_slope * (float)(adx > ady ? adx : ady);
                if (fit_finite(ds) && fabsf(delta) <= lim) {
                    const double w = (double)s_tab[bf_sad(gc, grow[j])], fx = (double)dx;
                    const double wx = w * fx, wy = w * fy, wd = w * (double)delta;
                    n++;
                    S += w; Sx += wx; Sy += wy;
                    Sxx += wx * fx; Sxy += wx * fy; Syy += wy * fy;
                    Sd += wd; Sxd += wd * fx; Syd += wd * fy;
                }
            }
        }
        o.w = v;
        if (fit_solve(g, fp, n, S, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd, d0, x, y, o)) k = 2;
        else if (d0 >= g.mind && d0 <= g.maxd) { o.x = 0.0f; o.y = 0.0f; o.z = d0; k = 1; }
    }
    if (k == 0) o = fallback ? fallback[px] : make_float4(0.0f, 0.0f, g.mind, 0.0f);
    out[px] = o;
    if (kind) kind[px] = k;
}

}  // namespace les
