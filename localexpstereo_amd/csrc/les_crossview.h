// les_crossview.h -- cross-view fusion: a label map of one view expressed in the coordinates of the other view (PatchMatch Stereo's "view
// propagation").  The reference has no such step: its two views meet only in the post-processing (LES/FastGCStereo.h:172-203).  The warped map
// is a second labelling for the fusion move of les_pairwise.h, so each view can take what the other one found.
//
// DEFINITION (stated here once; tests/crossview_cases.py restates it in numpy).
//   inputs    src: H x W planes (a, b, c, v) of view s (0 left, 1 right); fallback: H x W planes of the target view t = 1 - s
//   outputs   out: H x W planes of view t; hit (optional): H x W bytes
//   sign = +1 for s = 0, -1 for s = 1.  For a source pixel (xs, y), every operation in f32, in this order, not contracted:
//     d  = (a xs + b y) + c                          computeDisparities' order (les_disparity_kernel of les_post.h)
//     t  = (xs - d sign) + 0.5f
//     the candidate exists only if -1e9 < t < 1e9 (as les_lr_check_kernel: a NaN falls out here) and rx = floor(t) lies in [0, W)
//         (floor, not the check's truncation, which sends t in (-1, 0) to column 0: up to 1.5 pixels off)
//     q  = 1 - sign a;  the candidate is dropped unless q >= 0.125f and b, c, v are finite (a surface foreshortened more than 8 x in the
//         target view is not proposed)
//     the plane in the target view: a' = a / q, b' = b / q, c' = c / q (correctly rounded f32 division), v' = -v
//         (from d = a (xt + sign d) + b y + c; the candidate lands on row y: v is carried, not used in the geometry, as in the left-right
//         check, the pairwise terms and the post-processing)
//   Several candidates may land on one (rx, y): the largest d wins (the nearer surface occludes; -0 and +0 compare equal), among equal d
//   the largest xs.  A target pixel with a winner gets the winner's transformed plane and hit = 1; one without gets fallback's plane bit for
//   bit and hit = 0.  The result is a function of the inputs only, not of scheduling.
//   The transformed plane evaluated at the landing column differs from d by at most 0.5 |a'| plus rounding.
//
// LIMIT: rows of at most kWarpMaxW = 8192 pixels (two uint32 per column in LDS: 64 KB at the limit); wider rows are refused by
// les_hip_warp_labels with LES_HIP_ERR_UNSUPPORTED, not served slowly.
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_simt.h"

namespace les {

constexpr int kWarpMaxW = 8192;             // widest row: 2 x 4 bytes of LDS per column
constexpr int kWarpThreads = 256;

// order-preserving 32-bit image of a finite float (-0 counted as +0): a < b <=> key(a) < key(b); never 0, the "no candidate" value
__device__ __forceinline__ uint32_t warp_key(float d)
{
    if (d == 0.0f) d = 0.0f;
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool warp_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// the candidate of source pixel (xs, y) with label l: its landing column and the key of its disparity; false: it does not exist or is dropped
__device__ __forceinline__ bool warp_candidate(const float4 l, int xs, int y, int W, float sign, int& rx, uint32_t& key)
{
    const float d = (l.x * (float)xs + l.y * (float)y) + l.z;
    const float t = ((float)xs - d * sign) + 0.5f;
    if (!(t > -1.0e9f && t < 1.0e9f)) return false;
    rx = (int)floorf(t);
    if (rx < 0 || rx >= W) return false;
    const float q = 1.0f - sign * l.x;
    if (!(q >= 0.125f) || !warp_finite(l.y) || !warp_finite(l.z) || !warp_finite(l.w)) return false;
    key = warp_key(d);
    return true;
}

// grid = H (one workgroup per row: the problem is row-local), block = kWarpThreads, dynamic LDS = 8 W bytes: s_key[x] the best key that
// lands on target column x (0: none), s_win[x] the winning source column.
//   phase 1  every source pixel of the row (the threads stride over the columns, one 16-byte load each): atomicMax of its key at rx
//   phase 2  every candidate whose key is the best at its rx: atomicMax of xs there (the row is re-read: it was read a moment ago)
//   phase 3  one thread per target column: the winner's label is read again, transformed and stored (16 bytes + the hit byte)
// Only LDS integer maxima, which commute: the bits do not depend on the order.  out may be fallback (each target pixel is read and written by
// one thread), not src.
__global__ void __launch_bounds__(kWarpThreads)
les_warp_labels_kernel(const float4* __restrict__ src, const float4* fallback, float4* out, uint8_t* hit, int H, int W, float sign)
{
#if defined(LES_SIM)
    static thread_local uint32_t s_dyn_warp[2 * kWarpMaxW];
#else
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn_warp[];
#endif
    uint32_t* s_key = s_dyn_warp;
    uint32_t* s_win = s_dyn_warp + W;

    const int tid = (int)threadIdx.x, y = (int)blockIdx.x;
    if (y >= H) return;
    const size_t row = (size_t)y * W;

    for (int x = tid; x < W; x += kWarpThreads) {
        s_key[x] = 0u;
        s_win[x] = 0u;
    }
    __syncthreads();

    for (int xs = tid; xs < W; xs += kWarpThreads) {
        int rx;
        uint32_t key;
        if (warp_candidate(src[row + xs], xs, y, W, sign, rx, key)) atomicMax(&s_key[rx], key);
    }
    __syncthreads();

    for (int xs = tid; xs < W; xs += kWarpThreads) {
        int rx;
        uint32_t key;
        if (warp_candidate(src[row + xs], xs, y, W, sign, rx, key) && s_key[rx] == key) atomicMax(&s_win[rx], (uint32_t)xs);
    }
    __syncthreads();

    for (int x = tid; x < W; x += kWarpThreads) {
        float4 o;
        uint8_t h = 0;
        if (s_key[x] != 0u) {
            const float4 l = src[row + s_win[x]];
            const float q = 1.0f - sign * l.x;
            o = make_float4(l.x / q, l.y / q, l.z / q, -l.w);
            h = 1;
        } else {
            o = fallback[row + x];
        }
        out[row + x] = o;
        if (hit) hit[row + x] = h;
    }
}

}  // namespace les
