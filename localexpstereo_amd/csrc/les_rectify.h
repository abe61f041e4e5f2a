// les_rectify.h -- rectification of a calibrated raw stereo pair (no reference counterpart: the reference reads rectified pairs only,
// loadData, LES/main.cpp:201-268).  Two kernels: the map that says where in the raw image every rectified pixel comes from, and the sampler
// that reads a raw image through such a map.  The calibration is fixed while frames stream, so the map is built once per camera and a frame
// costs one sampling launch per image.  io.stereo_rectify (numpy fp64) makes the rotations and the new intrinsics on the host.
//
// CAMERA MODEL (stated here once; io.py, the header comment of include/localexp_hip.h and tests/rectify_cases.py use this one).  A point
// (X, Y, Z) of the raw camera's frame (X right, Y down, Z forward), pixel centres at integer coordinates, dist = (k1, k2, p1, p2, k3, k4, k5, k6):
//   x' = X / Z,  y' = Y / Z,  r2 = x'^2 + y'^2
//   rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
//   x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2)
//   y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
//   u = fx x'' + cx,  v = fy y'' + cy
//
// 1. les_rectify_map_kernel: map[y][x] = (u, v), the raw position of rectified pixel (x, y).  M (row-major 3 x 3) takes a ray of the rectified
//    frame into the raw camera's frame: the transpose of the rectifying rotation.  Every operation in fp64, rounded, in the order written, not
//    contracted; (u, v) rounded to f32 once at the end:
//      xr = (x - cx) / f                      yr = (y - cy) / f                      (f, cx, cy: the rectified intrinsics)
//      X = (M0 xr + M1 yr) + M2               Y = (M3 xr + M4 yr) + M5               Z = (M6 xr + M7 yr) + M8
//      Z > 0 or the pixel is (NaN, NaN)       (a ray that points behind the raw camera, or a NaN)
//      xp = X / Z,  yp = Y / Z,  xx = xp xp,  yy = yp yp,  xy = xp yp,  r2 = xx + yy
//      num = 1 + r2 (k1 + r2 (k2 + r2 k3))    den = 1 + r2 (k4 + r2 (k5 + r2 k6))
//      den finite and != 0 or the pixel is (NaN, NaN)
//      rad = num / den
//      xd = (xp rad + (2 p1) xy) + p2 (r2 + 2 xx)
//      yd = (yp rad + p1 (r2 + 2 yy)) + (2 p2) xy
//      u = fx xd + cxr,  v = fy yd + cyr      (fx, fy, cxr, cyr: the raw camera's)
//    A NaN in either rounded coordinate makes the pixel (NaN, NaN); every NaN stored is 0x7fc00000.
//
// 2. les_remap_kernel: dst[y][x][k] = src sampled at map[y][x] = (u, v); channels 1 or 3, bytes.
//    valid iff u and v are finite, 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1 (-0 is 0).  An invalid pixel: every channel 0, valid 0, and no
//    load from src -- the comparisons come before any conversion to an integer, so NaN, +-inf and coordinates beyond the int range never form
//    an index.  A valid pixel: valid 1, and with U = (double)u, V = (double)v (exact), every operation fp64, rounded, in the order written:
//      nearest  the tap (min(floor(U + 0.5), Ws - 1), min(floor(V + 0.5), Hs - 1))
//      linear   x0 = floor(U), tx = U - x0 (exact), x1 = min(x0 + 1, Ws - 1); y0, ty, y1 alike
//               s = (1 - ty) ((1 - tx) p00 + tx p01) + ty ((1 - tx) p10 + tx p11)          (pYX; a tap past the last column has weight tx = 0)
//      cubic    Catmull-Rom, a = -0.5: the taps x0 - 1 .. x0 + 2 and y0 - 1 .. y0 + 2, each clamped to the image, with the weights of t = tx, ty
//                 w0 = ((-0.5 t + 1) t - 0.5) t    w1 = ((1.5 t - 2.5) t) t + 1    w2 = ((-1.5 t + 2) t + 0.5) t    w3 = ((0.5 t - 0.5) t) t
//               row j:  h_j = ((wx0 p_j0 + wx1 p_j1) + wx2 p_j2) + wx3 p_j3,   s = ((wy0 h_0 + wy1 h_1) + wy2 h_2) + wy3 h_3
//               (t = 0 gives exactly (0, 1, 0, 0): integer coordinates return the source's bytes)
//      out = floor(s + 0.5) clamped to 0 .. 255  (nearest: the tap's byte)
//
// Both: grid = (ceil(W / kRectNT), H), kRectNT work-items, one pixel each, no LDS, plain loads: neighbouring work-items read neighbouring map
// entries and, for any map that is locally a small rotation, neighbouring source bytes.  Also compiled by the plain check build and by the
// CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include <cstdint>

namespace les {

constexpr int kRectNT = 256;

struct RectCamera { double fx, fy, cx, cy, dist[8]; };          // les_hip_camera
struct RectRays { double M[9], f, cx, cy; };                    // a rectified view: its rays into the raw frame, its intrinsics
struct alignas(8) RectUV { float u, v; };                       // a map entry: one 8-byte load or store

__device__ __forceinline__ float rect_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ bool rect_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }       // (false for a NaN)

// Definition 1 for one pixel.  false: (NaN, NaN).
__device__ __forceinline__ bool rect_map_pixel(const RectCamera& c, const RectRays& r, int x, int y, float& u, float& v)
{
    const double xr = ((double)x - r.cx) / r.f, yr = ((double)y - r.cy) / r.f;
    const double X = (r.M[0] * xr + r.M[1] * yr) + r.M[2];
    const double Y = (r.M[3] * xr + r.M[4] * yr) + r.M[5];
    const double Z = (r.M[6] * xr + r.M[7] * yr) + r.M[8];
    if (!(Z > 0.0)) return false;
    const double xp = X / Z, yp = Y / Z, xx = xp * xp, yy = yp * yp, xy = xp * yp, r2 = xx + yy;
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5], k5 = c.dist[6], k6 = c.dist[7];
    const double num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6));
    if (!rect_finite(den) || den == 0.0) return false;
    const double rad = num / den;
    const double xd = (xp * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx);
    const double yd = (yp * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy;
    u = (float)(c.fx * xd + c.cx);
    v = (float)(c.fy * yd + c.cy);
    return u == u && v == v;
}

__global__ void __launch_bounds__(kRectNT)
les_rectify_map_kernel(RectCamera cam, RectRays rays, RectUV* __restrict__ map, int H, int W)
{
    const int x = (int)(blockIdx.x * kRectNT + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W || y >= H) return;
    float u, v;
    if (!rect_map_pixel(cam, rays, x, y, u, v)) u = v = rect_nan();
    map[(size_t)y * W + x] = RectUV{u, v};
}

// floor(s + 0.5) clamped to 0 .. 255 (s is never a NaN: finite weights times bytes)
__device__ __forceinline__ uint8_t rect_round(double s)
{
    const double q = floor(s + 0.5);
    return (uint8_t)(int)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
}

__device__ __forceinline__ void rect_cubic_weights(double t, double w[4])
{
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = ((0.5 * t - 0.5) * t) * t;
}

__device__ __forceinline__ int rect_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// Definition 2.  C = channels, INTERP = 0 nearest, 1 linear, 2 cubic.  Source offsets fit an int: Hs Ws C < 2^31 (the launcher refuses more).
template <int C, int INTERP>
__global__ void __launch_bounds__(kRectNT)
les_remap_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, const RectUV* __restrict__ map, uint8_t* __restrict__ dst, uint8_t* __restrict__ valid, int H, int W)
{
    const int x = (int)(blockIdx.x * kRectNT + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const RectUV m = map[i];
    const double U = (double)m.u, V = (double)m.v;
    // (a NaN fails every comparison, +-inf and anything beyond the image fail one: nothing below converts such a value)
    const bool ok = U >= 0.0 && U <= (double)(Ws - 1) && V >= 0.0 && V <= (double)(Hs - 1);
    uint8_t out[C];
    for (int k = 0; k < C; k++) out[k] = 0;
    if (ok) {
        if (INTERP == 0) {
            const int xn = min((int)floor(U + 0.5), Ws - 1), yn = min((int)floor(V + 0.5), Hs - 1);
            const uint8_t* p = src + ((size_t)yn * Ws + xn) * C;
            for (int k = 0; k < C; k++) out[k] = p[k];
        } else if (INTERP == 1) {
            const double fx = floor(U), fy = floor(V), tx = U - fx, ty = V - fy;
            const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
            const uint8_t *r0 = src + (size_t)y0 * Ws * C, *r1 = src + (size_t)y1 * Ws * C;
            for (int k = 0; k < C; k++) {
                const double top = (1.0 - tx) * (double)r0[x0 * C + k] + tx * (double)r0[x1 * C + k];
                const double bot = (1.0 - tx) * (double)r1[x0 * C + k] + tx * (double)r1[x1 * C + k];
                out[k] = rect_round((1.0 - ty) * top + ty * bot);
            }
        } else {
            const double fx = floor(U), fy = floor(V);
            const int x0 = (int)fx, y0 = (int)fy;
            double wx[4], wy[4];
            rect_cubic_weights(U - fx, wx);
            rect_cubic_weights(V - fy, wy);
            int xs[4];
            for (int j = 0; j < 4; j++) xs[j] = rect_clamp(x0 - 1 + j, Ws) * C;
            double s[C];
            for (int j = 0; j < 4; j++) {
                const uint8_t* r = src + (size_t)rect_clamp(y0 - 1 + j, Hs) * Ws * C;
                for (int k = 0; k < C; k++) {
                    const double h = ((wx[0] * (double)r[xs[0] + k] + wx[1] * (double)r[xs[1] + k]) + wx[2] * (double)r[xs[2] + k]) + wx[3] * (double)r[xs[3] + k];
                    s[k] = j == 0 ? wy[0] * h : s[k] + wy[j] * h;
                }
            }
            for (int k = 0; k < C; k++) out[k] = rect_round(s[k]);
        }
    }
    for (int k = 0; k < C; k++) dst[i * C + k] = out[k];
    if (valid) valid[i] = ok ? 1 : 0;
}

}  // namespace les
