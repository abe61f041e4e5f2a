// les_unrectify.h -- the way back from the rectified pair to the raw camera (no reference counterpart: the reference reads rectified pairs only,
// loadData, LES/main.cpp:201-268).  Two kernels: the INVERSE map that says where in the rectified frame every raw pixel lies, and the one that
// turns a rectified-grid label map into points, normals and disparities registered to the raw pixels.  The camera model, RectCamera and the
// layout of a map entry (RectUV) are those of les_rectify.h; the calibration is fixed while frames stream, so the inverse map is built once per
// camera.  Because its layout is the forward map's, les_remap_kernel resamples any rectified-grid byte image onto the raw grid through it.
//
// Both: every operation fp64, rounded, in the order written, not contracted; each output rounded to f32 once at the end; every NaN stored is
// 0x7fc00000.  grid = (ceil(Ws / kRectNT), Hs), kRectNT work-items, one RAW pixel (u, v) each, no LDS, plain loads and stores.  Also compiled
// by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
//
// distort(x, y) below is the camera model in rect_map_pixel's order:
//      xx = x x,  yy = y y,  xy = x y,  r2 = xx + yy
//      num = 1 + r2 (k1 + r2 (k2 + r2 k3))    den = 1 + r2 (k4 + r2 (k5 + r2 k6))
//      den finite and != 0 or the pixel is (NaN, NaN)
//      rad = num / den
//      ex = (x rad + (2 p1) xy) + p2 (r2 + 2 xx)
//      ey = (y rad + p1 (r2 + 2 yy)) + (2 p2) xy
//
// 1. les_unrectify_map_kernel: inv[v][u] = (xs, ys), the rectified position of raw pixel (u, v) of one view.  R (row-major 3 x 3) is the view's
//    rectifying rotation: a ray of the raw camera's frame into the rectified frame (io.stereo_rectify's R0 / R1, the transpose of the forward
//    map's M).  fx, fy, cxr, cyr: the raw camera's; f, cx, cy: the rectified intrinsics.
//      xd = (u - cxr) / fx                    yd = (v - cyr) / fy
//      x = xd,  y = yd
//      `steps` times:  (ex, ey) = distort(x, y);   x = x - (ex - xd);   y = y - (ey - yd)
//      (ex, ey) = distort(x, y)               once more, for the residual
//      converged iff |fx (ex - xd)| <= tol and |fy (ey - yd)| <= tol              (a NaN fails), or the pixel is (NaN, NaN)
//      X = (R0 x + R1 y) + R2                 Y = (R3 x + R4 y) + R5                 Z = (R6 x + R7 y) + R8
//      Z > 0 or the pixel is (NaN, NaN)
//      xs = f (X / Z) + cx,  ys = f (Y / Z) + cy
//    A NaN in either rounded coordinate makes the pixel (NaN, NaN).  The update is the additive fixed point x <- x - (distort(x) - xd): it has
//    no division beyond distort's own, and it converges where the distortion is a contraction about the identity (|d(distort - id)| < 1, the
//    mild distortion of a calibrated lens); it is not Newton's method and does not reach a strongly distorted border in a few steps.  The
//    residual is the forward model's error in RAW pixels, so a position that fails the test is never stored as if it were right.  steps is
//    1 .. 64, tol > 0 (the launcher refuses anything else).
//
// 2. les_unrectify_labels_kernel: the [H][W] label map of one view (planes (a, b, c, .) of the rectified grid, as les_reproject_kernel takes them)
//    as geometry on that view's raw grid [Hs][Ws].  Per raw pixel, (xs, ys) its inverse-map entry as doubles (exact); f, cx, cy, doffs,
//    baseline: the rectified calibration with cx THE VIEW'S OWN principal point; M (row-major 3 x 3) = R^T takes the rectified frame into the
//    raw camera's frame (X right, Y down, Z forward):
//      inside iff 0 <= xs <= W - 1 and 0 <= ys <= H - 1         (compared before any conversion to an integer, as in les_remap_kernel: a NaN,
//                                                                +-inf and coordinates beyond the int range never form an index; -0 is 0)
//      xi = min(floor(xs + 0.5), W - 1),  yi = min(floor(ys + 0.5), H - 1);  l = labels[yi][xi];  dropped = drop && drop[yi][xi] != 0
//      d = (a xs + b ys) + c                                     the nearest pixel's plane at the raw pixel's own sub-pixel position
//      D = d + doffs
//      Zr = (f baseline) / D
//      valid iff inside, d finite, D > 0, not dropped, and Zr <= z_max when z_max > 0
//      Xr = ((xs - cx) Zr) / f                Yr = ((ys - cy) Zr) / f
//      P  = M (Xr, Yr, Zr)                    each row as (M0 Xr + M1 Yr) + M2 Zr
//      nr = (a f, b f, ((a cx + b cy) + c) + doffs)              the label's plane is exactly nr . (Xr, Yr, Zr) = f baseline
//      n  = M nr                              each row as (M0 nrx + M1 nry) + M2 nrz
//      normal = -n / sqrt((nx nx + ny ny) + nz nz)               it faces the camera
//    points, normals: [Hs][Ws][3] f32, points[..][2] is the raw depth; disparity: [Hs][Ws] f32, the rounded d; valid: bytes, 255 or 0.  An
//    invalid pixel holds NaN in every float output; a pixel that is not inside reads neither a label nor the drop mask.  points, normals and
//    disparity may each be null.  Label offsets fit an int: H W < 2^31 (the launcher refuses more).
#pragma once

#include "les_rectify.h"

namespace les {

struct UnrectView { double R[9], f, cx, cy; };                         // a rectified view: the raw frame's rays into it, its intrinsics
struct UnrectGeom { double M[9], f, cx, cy, doffs, baseline; };        // the same view for geometry: its frame into the raw frame, its calibration

// distort(x, y).  false: den is 0 or not finite.
__device__ __forceinline__ bool unrect_distort(const RectCamera& c, double x, double y, double& ex, double& ey)
{
    const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5], k5 = c.dist[6], k6 = c.dist[7];
    const double num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6));
    if (!rect_finite(den) || den == 0.0) return false;
    const double rad = num / den;
    ex = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx);
    ey = (y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy;
    return true;
}

// Definition 1 for one pixel.  false: (NaN, NaN).
__device__ __forceinline__ bool unrect_map_pixel(const RectCamera& c, const UnrectView& r, int steps, double tol, int u, int v, float& xs, float& ys)
{
    const double xd = ((double)u - c.cx) / c.fx, yd = ((double)v - c.cy) / c.fy;
    double x = xd, y = yd, ex, ey;
    for (int i = 0; i < steps; i++) {
        if (!unrect_distort(c, x, y, ex, ey)) return false;
        x = x - (ex - xd);
        y = y - (ey - yd);
    }
    if (!unrect_distort(c, x, y, ex, ey)) return false;
    if (!(fabs(c.fx * (ex - xd)) <= tol && fabs(c.fy * (ey - yd)) <= tol)) return false;
    const double X = (r.R[0] * x + r.R[1] * y) + r.R[2];
    const double Y = (r.R[3] * x + r.R[4] * y) + r.R[5];
    const double Z = (r.R[6] * x + r.R[7] * y) + r.R[8];
    if (!(Z > 0.0)) return false;
    xs = (float)(r.f * (X / Z) + r.cx);
    ys = (float)(r.f * (Y / Z) + r.cy);
    return xs == xs && ys == ys;
}

__global__ void __launch_bounds__(kRectNT)
les_unrectify_map_kernel(RectCamera cam, UnrectView view, int steps, double tol, RectUV* __restrict__ inv, int Hs, int Ws)
{
    const int u = (int)(blockIdx.x * kRectNT + threadIdx.x), v = (int)blockIdx.y;
    if (u >= Ws || v >= Hs) return;
    float xs, ys;
    if (!unrect_map_pixel(cam, view, steps, tol, u, v, xs, ys)) xs = ys = rect_nan();
    inv[(size_t)v * Ws + u] = RectUV{xs, ys};
}

// Definition 2.
__global__ void __launch_bounds__(kRectNT)
les_unrectify_labels_kernel(const float4* __restrict__ labels, int H, int W, const uint8_t* __restrict__ drop, const RectUV* __restrict__ inv, UnrectGeom g,
                            float z_max, float* __restrict__ points, float* __restrict__ normals, float* __restrict__ disparity, uint8_t* __restrict__ valid,
                            int Hs, int Ws)
{
    const int u = (int)(blockIdx.x * kRectNT + threadIdx.x), v = (int)blockIdx.y;
    if (u >= Ws || v >= Hs) return;
    const size_t i = (size_t)v * Ws + u;
    const RectUV m = inv[i];
    const double xs = (double)m.u, ys = (double)m.v;
    const float qnan = rect_nan();
    float p[3] = {qnan, qnan, qnan}, n[3] = {qnan, qnan, qnan}, disp = qnan;
    bool ok = false;
    // (a NaN fails every comparison, +-inf and anything beyond the frame fail one: nothing below converts such a value)
    if (xs >= 0.0 && xs <= (double)(W - 1) && ys >= 0.0 && ys <= (double)(H - 1)) {
        const int xi = min((int)floor(xs + 0.5), W - 1), yi = min((int)floor(ys + 0.5), H - 1);
        const int t = yi * W + xi;
        const float4 l = labels[t];
        const bool dropped = drop != nullptr && drop[t] != 0;
        const double a = (double)l.x, b = (double)l.y, c = (double)l.z;
        const double d = (a * xs + b * ys) + c;
        const double D = d + g.doffs;
        const double Zr = (g.f * g.baseline) / D;
        ok = rect_finite(d) && D > 0.0 && !dropped && !(z_max > 0.0f && !(Zr <= (double)z_max));
        if (ok) {
            const double Xr = ((xs - g.cx) * Zr) / g.f;
            const double Yr = ((ys - g.cy) * Zr) / g.f;
            const double nrx = a * g.f, nry = b * g.f, nrz = ((a * g.cx + b * g.cy) + c) + g.doffs;
            double P[3], N[3];
            for (int j = 0; j < 3; j++) {
                P[j] = (g.M[3 * j] * Xr + g.M[3 * j + 1] * Yr) + g.M[3 * j + 2] * Zr;
                N[j] = (g.M[3 * j] * nrx + g.M[3 * j + 1] * nry) + g.M[3 * j + 2] * nrz;
            }
            const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
            for (int j = 0; j < 3; j++) {
                p[j] = (float)P[j];
                n[j] = (float)(-N[j] / len);
            }
            disp = (float)d;
        }
    }
    for (int j = 0; j < 3; j++) {
        if (points) points[3 * i + j] = p[j];
        if (normals) normals[3 * i + j] = n[j];
    }
    if (disparity) disparity[i] = disp;
    valid[i] = ok ? 255 : 0;
}

}  // namespace les
