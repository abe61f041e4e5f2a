// les_view.h -- view synthesis and the photometric check: a label map turned back into an image.  The reference has neither: its two views meet
// only in the post-processing (LES/FastGCStereo.h:172-203).  Three row-local kernels on the plan of les_crossview.h (whose warp_key orders the
// candidates here too): the view of a camera anywhere on the baseline rendered from one view's labels, two such renders blended into one image
// with its holes filled, and the colour difference between every pixel and the point of the other image its label names.
//
// DEFINITIONS (stated here once; tests/view_cases.py restates them in numpy).  Every operation is f32, rounded, in the order written, not
// contracted.  sign = +1 for source view 0 (left), -1 for source view 1.  An image pixel is its three bytes (b, g, r).
//
// 1. les_render_view_kernel: labels H x W planes (a, b, c, v) and the image of view s, t in [0, 1] the fraction of the baseline from view s towards
//    the other view -> bgr H x W x 3 bytes, disp H x W floats (in view s's full-baseline disparity units), hit H x W bytes.
//    A  splat.  Source pixel (xs, y):  d = (a xs + b y) + c,  tt = (xs - (d t) sign) + 0.5.  The candidate exists iff -1e9 < tt < 1e9 and
//       rx = floor(tt) lies in [0, W) (a NaN or infinite d falls out here).  Per target column the largest d wins (-0 = +0), among equal d the
//       largest xs; disp[rx] = the winner's d, hit = 1.  (The label warp's q >= 0.125 rule is not applied: no plane is rewritten.)
//    B  cracks.  A column 0 < rx < W - 1 without a winner whose two neighbours both have hit == 1 after A and |disp[rx-1] - disp[rx+1]| <= 1 gets
//       disp = (disp[rx-1] + disp[rx+1]) * 0.5 and hit = 2.  Only winners of A count as neighbours, so the order of the columns cannot matter.
//    C  sample.  Every column with hit != 0:  xsrc = rx + (disp t) sign clamped to [0, W - 1],  x0 = floor(xsrc),  x1 = min(x0 + 1, W - 1),
//       w = xsrc - x0,  per channel val = ((1 - w) c0) + (w c1),  out = (u8)(int)(val + 0.5).  The clamp is xsrc > 0 ? (xsrc < W - 1 ? xsrc :
//       W - 1) : 0, so a NaN samples column 0 (only a crack at t = 0 between two disparities whose sum overflows has one: inf * 0).
//    A hole (hit 0): colour 0, disp NaN (0x7fc00000).
//
// 2. les_blend_views_kernel: (bgrL, dispL, hitL) = view 0 rendered at t and (bgrR, dispR, hitR) = view 1 rendered at 1 - t, either triple absent
//    as a whole -> bgr, disp, src.  Per pixel, a side counts where its hit != 0:
//       both, |dL - dR| <= tol    colour = (u8)(int)((((1 - t) cL) + (t cR)) + 0.5),  disp = ((1 - t) dL) + (t dR),  src = 3
//       both otherwise            the larger disp wins, a tie goes to the left: that side's colour and disp, src = 1 (left) or 2 (right)
//       one                       that one, src = 1 or 2
//       none                      a hole: src = 0, colour 0, disp NaN
//    fill != 0: a hole takes colour and disp of column l, the nearest column to its left that was not a hole before filling, or of r, the nearest
//    such column to its right: the one of smaller disp (the background shows through a disocclusion), equal disp goes to l; the one present when
//    only one is; the hole stays when the row has no other pixel.  A filled pixel gets src = 4.
//
// 3. les_photo_error_kernel: labels of view m and both images of the context -> err H x W floats, vis H x W bytes.  Pixel (xs, y), d as in 1:
//       vis = 0   its candidate of 1.A at t = 1 does not exist
//       vis = 2   the candidate exists and is not the winner of its landing column (the label map itself says the pixel is occluded)
//       otherwise xo = xs - d sign;  vis = 0 unless 0 <= xo <= W - 1;  else vis = 1 and, with the OTHER view's image sampled at xo as in 1.C but
//                 not rounded,  err = ((|val_b - b| + |val_g - g|) + |val_r - r|) / 3  against the pixel's own bytes
//    err = NaN (0x7fc00000) wherever vis != 1.
//
// LIMIT: rows of at most kWarpMaxW = 8192 pixels, as les_crossview.h and for its reason (render, photo error: two uint32 per column in LDS;
// blend: two uint16 per column and 2 x kViewThreads uint32); wider rows are refused with LES_HIP_ERR_UNSUPPORTED, not served slowly.
//
// All three: grid = H (one workgroup per row), block = kViewThreads.  Only LDS integer maxima and integer scans decide anything across
// columns, so the bits are a function of the inputs alone.  Also compiled by the plain check build and by the CPU fiber simulator (test
// infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_crossview.h"

namespace les {

constexpr int kViewThreads = 256;

__device__ __forceinline__ float view_nan() { return __int_as_float(0x7fc00000); }

// pixel i of an image as B | G << 8 | R << 16: of the context's packed image ipk, or of a byte image when ipk is null
__device__ __forceinline__ uint32_t view_pixel(const uint32_t* __restrict__ ipk, const uint8_t* __restrict__ bgr, size_t i)
{
    if (ipk) return ipk[i];
    const uint8_t* p = bgr + 3 * i;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ __forceinline__ float view_channel(uint32_t px, int k) { return (float)((px >> (8 * k)) & 0xffu); }

__device__ __forceinline__ float view_disparity(const float4 l, int xs, int y) { return (l.x * (float)xs + l.y * (float)y) + l.z; }

// the candidate of source pixel (xs, y) with disparity d for the camera at fraction t: its landing column; false: it does not exist
__device__ __forceinline__ bool view_candidate(float d, int xs, int W, float t, float sign, int& rx)
{
    const float tt = ((float)xs - (d * t) * sign) + 0.5f;
    if (!(tt > -1.0e9f && tt < 1.0e9f)) return false;
    rx = (int)floorf(tt);
    return rx >= 0 && rx < W;
}

// where an image row is sampled at xsrc in [0, W - 1]: the two columns and the weight of the second one
__device__ __forceinline__ void view_taps(float xsrc, int W, int& x0, int& x1, float& w)
{
    const float f = floorf(xsrc);
    x0 = (int)f;
    x1 = min(x0 + 1, W - 1);
    w = xsrc - f;
}

__device__ __forceinline__ float view_lerp(float w, float c0, float c1) { return ((1.0f - w) * c0) + (w * c1); }

__device__ __forceinline__ uint32_t view_round(float val) { return (uint32_t)(uint8_t)(int)(val + 0.5f); }

__device__ __forceinline__ void view_store_bgr(uint8_t* __restrict__ bgr, size_t i, uint32_t px)
{
    bgr[3 * i] = (uint8_t)px;
    bgr[3 * i + 1] = (uint8_t)(px >> 8);
    bgr[3 * i + 2] = (uint8_t)(px >> 16);
}

// phases 1 and 2 of les_warp_labels_kernel with this header's candidate: s_key[x] the best key that lands on column x (0: none), s_win[x] the
// winning source column.  Ends behind a barrier.
__device__ __forceinline__ void view_splat(const float4* __restrict__ lab, int y, int W, float t, float sign, uint32_t* s_key, uint32_t* s_win)
{
    const int tid = (int)threadIdx.x;
    for (int x = tid; x < W; x += kViewThreads) {
        s_key[x] = 0u;
        s_win[x] = 0u;
    }
    __syncthreads();
    for (int xs = tid; xs < W; xs += kViewThreads) {
        const float d = view_disparity(lab[xs], xs, y);
        int rx;
        if (view_candidate(d, xs, W, t, sign, rx)) atomicMax(&s_key[rx], warp_key(d));
    }
    __syncthreads();
    for (int xs = tid; xs < W; xs += kViewThreads) {
        const float d = view_disparity(lab[xs], xs, y);
        int rx;
        if (view_candidate(d, xs, W, t, sign, rx) && s_key[rx] == warp_key(d)) atomicMax(&s_win[rx], (uint32_t)xs);
    }
    __syncthreads();
}

// dynamic LDS = 8 W bytes.  After the splat every column turns its (key, winner) into (the winner's d as bits, hit) in place -- a column is
// read and written by one thread -- and phase B and C read the neighbours' words behind one more barrier.  ipk / image: view_pixel's.
__global__ void __launch_bounds__(kViewThreads)
les_render_view_kernel(const float4* __restrict__ labels, const uint32_t* __restrict__ ipk, const uint8_t* __restrict__ image, uint8_t* __restrict__ out_bgr,
                       float* __restrict__ out_disp, uint8_t* __restrict__ out_hit, int H, int W, float t, float sign)
{
#if defined(LES_SIM)
    alignas(16) static thread_local uint32_t s_dyn_view[2 * kWarpMaxW];
#else
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn_view[];
#endif
    uint32_t* s_key = s_dyn_view;
    uint32_t* s_win = s_dyn_view + W;

    const int tid = (int)threadIdx.x, y = (int)blockIdx.x;
    if (y >= H) return;
    const size_t row = (size_t)y * W;

    view_splat(labels + row, y, W, t, sign, s_key, s_win);

    for (int x = tid; x < W; x += kViewThreads) {
        const bool won = s_key[x] != 0u;
        const int xs = (int)s_win[x];
        if (won) s_key[x] = __float_as_uint(view_disparity(labels[row + xs], xs, y));
        s_win[x] = won ? 1u : 0u;
    }
    __syncthreads();

    for (int x = tid; x < W; x += kViewThreads) {
        uint32_t hit = s_win[x];
        float disp = __int_as_float((int)s_key[x]);
        if (!hit && x > 0 && x < W - 1 && s_win[x - 1] && s_win[x + 1]) {
            const float dl = __int_as_float((int)s_key[x - 1]), dr = __int_as_float((int)s_key[x + 1]);
            if (fabsf(dl - dr) <= 1.0f) {
                disp = (dl + dr) * 0.5f;
                hit = 2u;
            }
        }
        uint32_t px = 0u;
        if (hit) {
            float xsrc = (float)x + (disp * t) * sign;
            xsrc = xsrc > 0.0f ? (xsrc < (float)(W - 1) ? xsrc : (float)(W - 1)) : 0.0f;      // (written so that a NaN becomes 0)
            int x0, x1;
            float w;
            view_taps(xsrc, W, x0, x1, w);
            const uint32_t p0 = view_pixel(ipk, image, row + x0), p1 = view_pixel(ipk, image, row + x1);
            for (int k = 0; k < 3; k++) px |= view_round(view_lerp(w, view_channel(p0, k), view_channel(p1, k))) << (8 * k);
        } else {
            disp = view_nan();
        }
        view_store_bgr(out_bgr, row + x, px);
        out_disp[row + x] = disp;
        out_hit[row + x] = (uint8_t)hit;
    }
}

// one pixel of the blend before filling: its colour (packed), disp and src
struct BlendPixel { uint32_t px; float disp; uint32_t src; };

__device__ __forceinline__ uint32_t blend_src(bool hl, bool hr, float dl, float dr, float tol)
{
    if (hl && hr) return fabsf(dl - dr) <= tol ? 3u : (dr > dl ? 2u : 1u);
    return hl ? 1u : (hr ? 2u : 0u);
}

__device__ __forceinline__ BlendPixel blend_pixel(const uint8_t* __restrict__ bgrL, const float* __restrict__ dispL, const uint8_t* __restrict__ hitL,
                                                  const uint8_t* __restrict__ bgrR, const float* __restrict__ dispR, const uint8_t* __restrict__ hitR,
                                                  size_t i, float t, float tol)
{
    const bool hl = hitL && hitL[i] != 0, hr = hitR && hitR[i] != 0;
    const float dl = hl ? dispL[i] : 0.0f, dr = hr ? dispR[i] : 0.0f;
    BlendPixel o;
    o.src = blend_src(hl, hr, dl, dr, tol);
    o.px = 0u;
    o.disp = view_nan();
    if (o.src == 3u) {
        const uint32_t pl = view_pixel(nullptr, bgrL, i), pr = view_pixel(nullptr, bgrR, i);
        for (int k = 0; k < 3; k++) o.px |= view_round(((1.0f - t) * view_channel(pl, k)) + (t * view_channel(pr, k))) << (8 * k);
        o.disp = ((1.0f - t) * dl) + (t * dr);
    } else if (o.src == 1u) {
        o.px = view_pixel(nullptr, bgrL, i);
        o.disp = dl;
    } else if (o.src == 2u) {
        o.px = view_pixel(nullptr, bgrR, i);
        o.disp = dr;
    }
    return o;
}

// dynamic LDS = 4 W + 8 kViewThreads bytes: s_l[x] = 1 + the nearest column <= x that is not a hole, within the chunk of x (0: none there),
// s_r[x] = the nearest such column >= x within the chunk (W: none there); a chunk is the n = ceil(W / kViewThreads) consecutive columns one
// thread scans, and s_cl[k] / s_cr[k] carry the same over the chunks before / behind chunk k.  Integer scans: no order to depend on.  One pass
// over the renders stores every pixel that is no hole; only the holes come back after the scans.
__global__ void __launch_bounds__(kViewThreads)
les_blend_views_kernel(const uint8_t* __restrict__ bgrL, const float* __restrict__ dispL, const uint8_t* __restrict__ hitL, const uint8_t* __restrict__ bgrR,
                       const float* __restrict__ dispR, const uint8_t* __restrict__ hitR, uint8_t* __restrict__ out_bgr, float* __restrict__ out_disp,
                       uint8_t* __restrict__ out_src, int H, int W, float t, float tol, int fill)
{
#if defined(LES_SIM)
    alignas(16) static thread_local uint32_t s_dyn_blend[kWarpMaxW + 2 * kViewThreads];
#else
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn_blend[];
#endif
    uint32_t* s_cl = s_dyn_blend;
    uint32_t* s_cr = s_dyn_blend + kViewThreads;
    uint16_t* s_l = reinterpret_cast<uint16_t*>(s_dyn_blend + 2 * kViewThreads);
    uint16_t* s_r = s_l + W;

    const int tid = (int)threadIdx.x, y = (int)blockIdx.x;
    if (y >= H) return;
    const size_t row = (size_t)y * W;

    // every pixel the blend itself decides is stored here; with fill, the holes wait for the scans
    for (int x = tid; x < W; x += kViewThreads) {
        const BlendPixel o = blend_pixel(bgrL, dispL, hitL, bgrR, dispR, hitR, row + x, t, tol);
        if (fill) {
            s_l[x] = (uint16_t)(o.src ? x + 1 : 0);
            s_r[x] = (uint16_t)(o.src ? x : W);
        }
        if (o.src || !fill) {
            view_store_bgr(out_bgr, row + x, o.px);
            out_disp[row + x] = o.disp;
            out_src[row + x] = (uint8_t)o.src;
        }
    }
    if (!fill) return;
    __syncthreads();
    const int n = (W + kViewThreads - 1) / kViewThreads, x_lo = min(tid * n, W), x_hi = min(x_lo + n, W);
    uint32_t run = 0u;
    for (int x = x_lo; x < x_hi; x++) {
        run = max(run, (uint32_t)s_l[x]);
        s_l[x] = (uint16_t)run;
    }
    s_cl[tid] = run;
    run = (uint32_t)W;
    for (int x = x_hi - 1; x >= x_lo; x--) {
        run = min(run, (uint32_t)s_r[x]);
        s_r[x] = (uint16_t)run;
    }
    s_cr[tid] = run;
    __syncthreads();
    uint32_t cl = 0u, cr = (uint32_t)W;
    for (int k = 0; k < tid; k++) cl = max(cl, s_cl[k]);
    for (int k = tid + 1; k < kViewThreads; k++) cr = min(cr, s_cr[k]);
    __syncthreads();
    s_cl[tid] = cl;
    s_cr[tid] = cr;
    __syncthreads();

    // the holes (after the scan a column that is no hole finds itself: s_l[x] == x + 1): the renders are read again at the columns l and r
    for (int x = tid; x < W; x += kViewThreads) {
        if ((int)s_l[x] == x + 1) continue;
        const int k = x / n;
        const int l = (int)(s_l[x] ? (uint32_t)s_l[x] : s_cl[k]) - 1;                   // -1: none
        const int r = (int)(s_r[x] < W ? (uint32_t)s_r[x] : s_cr[k]);                   // W: none
        BlendPixel o = {0u, view_nan(), 0u};
        if (l >= 0 || r < W) {
            if (l >= 0 && r < W) {
                const BlendPixel ql = blend_pixel(bgrL, dispL, hitL, bgrR, dispR, hitR, row + l, t, tol);
                const BlendPixel qr = blend_pixel(bgrL, dispL, hitL, bgrR, dispR, hitR, row + r, t, tol);
                o = qr.disp < ql.disp ? qr : ql;
            } else {
                o = blend_pixel(bgrL, dispL, hitL, bgrR, dispR, hitR, row + (l >= 0 ? l : r), t, tol);
            }
            o.src = 4u;
        }
        view_store_bgr(out_bgr, row + x, o.px);
        out_disp[row + x] = o.disp;
        out_src[row + x] = (uint8_t)o.src;
    }
}

// dynamic LDS = 8 W bytes: the splat of 1.A at t = 1, then one thread per SOURCE pixel.  ipk_own / ipk_other: the context's packed images of the
// labels' view and of the other one.
__global__ void __launch_bounds__(kViewThreads)
les_photo_error_kernel(const float4* __restrict__ labels, const uint32_t* __restrict__ ipk_own, const uint32_t* __restrict__ ipk_other, float* __restrict__ err,
                       uint8_t* __restrict__ vis, int H, int W, float sign)
{
#if defined(LES_SIM)
    alignas(16) static thread_local uint32_t s_dyn_photo[2 * kWarpMaxW];
#else
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn_photo[];
#endif
    uint32_t* s_key = s_dyn_photo;
    uint32_t* s_win = s_dyn_photo + W;

    const int tid = (int)threadIdx.x, y = (int)blockIdx.x;
    if (y >= H) return;
    const size_t row = (size_t)y * W;

    view_splat(labels + row, y, W, 1.0f, sign, s_key, s_win);

    for (int xs = tid; xs < W; xs += kViewThreads) {
        const float d = view_disparity(labels[row + xs], xs, y);
        float e = view_nan();
        uint32_t v = 0u;
        int rx;
        if (view_candidate(d, xs, W, 1.0f, sign, rx)) {
            const float xo = (float)xs - d * sign;
            if (s_win[rx] != (uint32_t)xs) {
                v = 2u;
            } else if (xo >= 0.0f && xo <= (float)(W - 1)) {
                v = 1u;
                int x0, x1;
                float w;
                view_taps(xo, W, x0, x1, w);
                const uint32_t p0 = ipk_other[row + x0], p1 = ipk_other[row + x1], own = ipk_own[row + xs];
                float a[3];
                for (int k = 0; k < 3; k++) a[k] = fabsf(view_lerp(w, view_channel(p0, k), view_channel(p1, k)) - view_channel(own, k));
                e = ((a[0] + a[1]) + a[2]) / 3.0f;
            }
        }
        err[row + xs] = e;
        vis[row + xs] = (uint8_t)v;
    }
}

}  // namespace les
