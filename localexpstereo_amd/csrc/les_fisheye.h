// les_fisheye.h -- the equidistant (Kannala-Brandt) fisheye camera in the place of les_rectify.h's pinhole with rational distortion (no reference
// counterpart: the reference reads rectified pairs only, loadData, LES/main.cpp:201-268).  Two kernels, the fisheye forms of
// les_rectify_map_kernel and les_unrectify_map_kernel: the map that says where in the raw fisheye image every rectified pixel comes from, and the
// INVERSE map that says where in the rectified frame every raw pixel lies.  Their outputs have the layout of the pinhole maps (RectUV), so the
// sampler, the labels kernel and everything above them work on a fisheye rig unchanged.
//
// CAMERA MODEL (stated here once; io.py, the header comment of include/localexp_hip.h and tests/fisheye_cases.py use this one).  A point
// (X, Y, Z) of the raw camera's frame (X right, Y down, Z forward), pixel centres at integer coordinates, k = (k1, k2, k3, k4), zero skew:
//   a = X / Z,  b = Y / Z,  r = sqrt(a^2 + b^2),  theta = atan(r)
//   theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)
//   u = fx (theta_d / r) a + cx,  v = fy (theta_d / r) b + cy                (r = 0: u = cx, v = cy)
// theta_max in (0, pi] is the largest theta the lens is calibrated for: a ray beyond it has no pixel.  It is the guard against the polynomial
// folding back (io.fisheye_theta_max finds where d theta_d / d theta reaches 0).  Rays with Z <= 0 (a lens beyond 180 degrees) have no pixel.
//
// THE THREE FUNCTIONS.  No library rounds atan, sin and cos correctly, so they are stated here in plain fp64 operations, and the kernels stay a
// function of their arguments alone, bit for bit, on every build.  Every operation fp64, rounded, in the order written, not contracted; the
// coefficients are the correctly rounded quotients 1 / 39, 1 / 6, ... of exactly representable integers (20! = 2^18 x an odd number below 2^44);
// kPi2, kPi4 are the doubles nearest pi / 2 and pi / 4.
//   fe_atan(r), r >= 0 (a NaN passes through; +inf gives kPi2):
//      big = r > 1;  t = big ? 1 / r : r
//      mid = t > T8                              T8 = the double sqrt(2.0) - 1.0 = tan(pi / 8) = 0x1.a827999fcef34p-2
//      s = mid ? (t - 1) / (t + 1) : t           |s| <= tan(pi / 8)
//      z = s s
//      p = 1 / 39;  for n = 18 .. 0:  p = 1 / (2 n + 1) - z p           (the series of atan(s) / s to s^40; the first term left out is below 1e-17)
//      a = s p;  mid: a = kPi4 + a;  big: a = kPi2 - a
//   fe_sincos(theta), 0 <= theta <= pi:
//      q = floor(theta / kPi2 + 0.5)             0, 1 or 2
//      y = theta - q kPi2                        |y| <= pi / 4 (q kPi2 is exact)
//      z = y y
//      S = -1 / 19!;  for k = 17, 15, .., 3:  S = +-1 / k! + z S      (+ where (k - 1) / 2 is even)         sin_y = y + (y z) S
//      C = +1 / 20!;  for k = 18, 16, .., 2:  C = +-1 / k! + z C      (+ where k / 2 is even)               cos_y = 1 + z C
//      q = 0: (sin_y, cos_y);  q = 1: (cos_y, -sin_y);  q = 2: (-sin_y, -cos_y)
//   Against the C library's atan / sin / cos both differ by at most 2.3e-16 (tests/fisheye_cases.py measures it), twelve orders of magnitude
//   below an f32 ulp of a pixel coordinate.
//
// 1. les_fisheye_map_kernel: map[y][x] = (u, v), the raw position of rectified pixel (x, y).  M, f, cx, cy: as in les_rectify_map_kernel.
//      xr = (x - cx) / f                      yr = (y - cy) / f
//      X = (M0 xr + M1 yr) + M2               Y = (M3 xr + M4 yr) + M5               Z = (M6 xr + M7 yr) + M8
//      Z > 0 or the pixel is (NaN, NaN)
//      a = X / Z,  b = Y / Z,  r = sqrt(a a + b b)
//      theta = fe_atan(r)
//      theta <= theta_max or the pixel is (NaN, NaN)                             (a NaN fails)
//      t2 = theta theta
//      P = 1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))
//      theta_d = theta P
//      s = r > 0 ? theta_d / r : 1
//      u = fx (a s) + cxr,  v = fy (b s) + cyr                                   each rounded to f32 once
//    A NaN in either rounded coordinate makes the pixel (NaN, NaN); every NaN stored is 0x7fc00000.
//
// 2. les_fisheye_unmap_kernel: inv[v][u] = (xs, ys), the rectified position of raw pixel (u, v).  R, f, cx, cy: as in les_unrectify_map_kernel.
//      xd = (u - cxr) / fx                    yd = (v - cyr) / fy
//      theta_d = sqrt(xd xd + yd yd)
//      theta = theta_d
//      `steps` times:
//          t2 = theta theta;  P as above
//          Q = 1 + t2 (3 k1 + t2 (5 k2 + t2 (7 k3 + t2 (9 k4))))                 (d theta_d / d theta; the products 3 k1 .. 9 k4 rounded first)
//          Q finite and > 0 or the pixel is (NaN, NaN)                           (beyond the fold there is no unique theta)
//          theta = theta - (theta P - theta_d) / Q
//      once more:  t2, P of the last theta;  e = theta P - theta_d
//      converged iff |fx e| <= tol and |fy e| <= tol                             (a NaN fails), or the pixel is (NaN, NaN)
//      0 <= theta <= theta_max or the pixel is (NaN, NaN)
//      (sn, cs) = fe_sincos(theta)
//      g = theta_d > 0 ? sn / theta_d : 1
//      ray = (xd g, yd g, cs)
//      X = (R0 rx + R1 ry) + R2 rz            Y = (R3 rx + R4 ry) + R5 rz            Z = (R6 rx + R7 ry) + R8 rz
//      Z > 0 or the pixel is (NaN, NaN)
//      xs = f (X / Z) + cx,  ys = f (Y / Z) + cy                                 each rounded to f32 once
//    This is Newton's method on theta P(theta) = theta_d, not the pinhole kernel's additive step: one correctly rounded division per step, and
//    quadratic convergence wherever Q > 0, out to theta_max of a lens of 180 degrees and more.  The residual e is the forward model's error
//    along the radius, in RAW pixels after fx and fy: a position that fails the test is never stored as if it were right.  steps is 1 .. 64,
//    tol > 0 (the launcher refuses anything else).
//
// Both: grid = (ceil(W / kRectNT), H), kRectNT work-items, one pixel each, no LDS, one 8-byte store per pixel, 64-bit offsets.  The fp64
// divisions and the sqrt are the cost: each is a dependent sequence of a dozen fp64 instructions.  Also compiled by the plain check build and
// by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_unrectify.h"

namespace les {

struct FishCamera { double fx, fy, cx, cy, k[4], theta_max; };          // les_hip_fisheye

constexpr double kFePi2 = 0x1.921fb54442d18p+0;          // the double nearest pi / 2
constexpr double kFePi4 = 0x1.921fb54442d18p-1;          // the double nearest pi / 4
constexpr double kFeT8 = 0x1.a827999fcef34p-2;           // the double sqrt(2.0) - 1.0

__device__ __forceinline__ double fe_atan(double r)
{
    const bool big = r > 1.0;
    const double t = big ? 1.0 / r : r;
    const bool mid = t > kFeT8;
    const double s = mid ? (t - 1.0) / (t + 1.0) : t;
    const double z = s * s;
    double p = 1.0 / 39.0;
    p = 1.0 / 37.0 - z * p;
    p = 1.0 / 35.0 - z * p;
    p = 1.0 / 33.0 - z * p;
    p = 1.0 / 31.0 - z * p;
    p = 1.0 / 29.0 - z * p;
    p = 1.0 / 27.0 - z * p;
    p = 1.0 / 25.0 - z * p;
    p = 1.0 / 23.0 - z * p;
    p = 1.0 / 21.0 - z * p;
    p = 1.0 / 19.0 - z * p;
    p = 1.0 / 17.0 - z * p;
    p = 1.0 / 15.0 - z * p;
    p = 1.0 / 13.0 - z * p;
    p = 1.0 / 11.0 - z * p;
    p = 1.0 / 9.0 - z * p;
    p = 1.0 / 7.0 - z * p;
    p = 1.0 / 5.0 - z * p;
    p = 1.0 / 3.0 - z * p;
    p = 1.0 / 1.0 - z * p;
    double a = s * p;
    if (mid) a = kFePi4 + a;
    if (big) a = kFePi2 - a;
    return a;
}

__device__ __forceinline__ void fe_sincos(double theta, double& sn, double& cs)
{
    const double q = floor(theta / kFePi2 + 0.5);
    const double y = theta - q * kFePi2;
    const double z = y * y;
    double S = -1.0 / 121645100408832000.0;              // 19!
    S = 1.0 / 355687428096000.0 + z * S;                 // 17!
    S = -1.0 / 1307674368000.0 + z * S;                  // 15!
    S = 1.0 / 6227020800.0 + z * S;                      // 13!
    S = -1.0 / 39916800.0 + z * S;                       // 11!
    S = 1.0 / 362880.0 + z * S;                          // 9!
    S = -1.0 / 5040.0 + z * S;                           // 7!
    S = 1.0 / 120.0 + z * S;                             // 5!
    S = -1.0 / 6.0 + z * S;                              // 3!
    const double sin_y = y + (y * z) * S;
    double C = 1.0 / 2432902008176640000.0;              // 20!
    C = -1.0 / 6402373705728000.0 + z * C;               // 18!
    C = 1.0 / 20922789888000.0 + z * C;                  // 16!
    C = -1.0 / 87178291200.0 + z * C;                    // 14!
    C = 1.0 / 479001600.0 + z * C;                       // 12!
    C = -1.0 / 3628800.0 + z * C;                        // 10!
    C = 1.0 / 40320.0 + z * C;                           // 8!
    C = -1.0 / 720.0 + z * C;                            // 6!
    C = 1.0 / 24.0 + z * C;                              // 4!
    C = -1.0 / 2.0 + z * C;                              // 2!
    const double cos_y = 1.0 + z * C;
    if (q == 0.0) { sn = sin_y; cs = cos_y; }
    else if (q == 1.0) { sn = cos_y; cs = -sin_y; }
    else { sn = -sin_y; cs = -cos_y; }
}

// P(theta^2) = theta_d / theta
__device__ __forceinline__ double fe_poly(const FishCamera& c, double t2) { return 1.0 + t2 * (c.k[0] + t2 * (c.k[1] + t2 * (c.k[2] + t2 * c.k[3]))); }

// Definition 1 for one pixel.  false: (NaN, NaN).
__device__ __forceinline__ bool fe_map_pixel(const FishCamera& c, const RectRays& r, int x, int y, float& u, float& v)
{
    const double xr = ((double)x - r.cx) / r.f, yr = ((double)y - r.cy) / r.f;
    const double X = (r.M[0] * xr + r.M[1] * yr) + r.M[2];
    const double Y = (r.M[3] * xr + r.M[4] * yr) + r.M[5];
    const double Z = (r.M[6] * xr + r.M[7] * yr) + r.M[8];
    if (!(Z > 0.0)) return false;
    const double a = X / Z, b = Y / Z;
    const double rr = sqrt(a * a + b * b);
    const double theta = fe_atan(rr);
    if (!(theta <= c.theta_max)) return false;
    const double theta_d = theta * fe_poly(c, theta * theta);
    const double s = rr > 0.0 ? theta_d / rr : 1.0;
    u = (float)(c.fx * (a * s) + c.cx);
    v = (float)(c.fy * (b * s) + c.cy);
    return u == u && v == v;
}

__global__ void __launch_bounds__(kRectNT)
les_fisheye_map_kernel(FishCamera cam, RectRays rays, RectUV* __restrict__ map, int H, int W)
{
    const int x = (int)(blockIdx.x * kRectNT + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W || y >= H) return;
    float u, v;
    if (!fe_map_pixel(cam, rays, x, y, u, v)) u = v = rect_nan();
    map[(size_t)y * W + x] = RectUV{u, v};
}

// Definition 2 for one pixel.  false: (NaN, NaN).
__device__ __forceinline__ bool fe_unmap_pixel(const FishCamera& c, const UnrectView& r, int steps, double tol, int u, int v, float& xs, float& ys)
{
    const double xd = ((double)u - c.cx) / c.fx, yd = ((double)v - c.cy) / c.fy;
    const double theta_d = sqrt(xd * xd + yd * yd);
    const double q1 = 3.0 * c.k[0], q2 = 5.0 * c.k[1], q3 = 7.0 * c.k[2], q4 = 9.0 * c.k[3];
    double theta = theta_d;
    for (int i = 0; i < steps; i++) {
        const double t2 = theta * theta;
        const double P = fe_poly(c, t2);
        const double Q = 1.0 + t2 * (q1 + t2 * (q2 + t2 * (q3 + t2 * q4)));
        if (!(rect_finite(Q) && Q > 0.0)) return false;
        theta = theta - (theta * P - theta_d) / Q;
    }
    const double e = theta * fe_poly(c, theta * theta) - theta_d;
    if (!(fabs(c.fx * e) <= tol && fabs(c.fy * e) <= tol)) return false;
    if (!(theta >= 0.0 && theta <= c.theta_max)) return false;
    double sn, cs;
    fe_sincos(theta, sn, cs);
    const double g = theta_d > 0.0 ? sn / theta_d : 1.0;
    const double rx = xd * g, ry = yd * g, rz = cs;
    const double X = (r.R[0] * rx + r.R[1] * ry) + r.R[2] * rz;
    const double Y = (r.R[3] * rx + r.R[4] * ry) + r.R[5] * rz;
    const double Z = (r.R[6] * rx + r.R[7] * ry) + r.R[8] * rz;
    if (!(Z > 0.0)) return false;
    xs = (float)(r.f * (X / Z) + r.cx);
    ys = (float)(r.f * (Y / Z) + r.cy);
    return xs == xs && ys == ys;
}

__global__ void __launch_bounds__(kRectNT)
les_fisheye_unmap_kernel(FishCamera cam, UnrectView view, int steps, double tol, RectUV* __restrict__ inv, int Hs, int Ws)
{
    const int u = (int)(blockIdx.x * kRectNT + threadIdx.x), v = (int)blockIdx.y;
    if (u >= Ws || v >= Hs) return;
    float xs, ys;
    if (!fe_unmap_pixel(cam, view, steps, tol, u, v, xs, ys)) xs = ys = rect_nan();
    inv[(size_t)v * Ws + u] = RectUV{xs, ys};
}

}  // namespace les
