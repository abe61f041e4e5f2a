// les_speckle.h -- speckle filter on the device (no reference counterpart; the convention is OpenCV's filterSpeckles): connected components of a
// disparity map by union-find, their sizes, and the mask of the pixels whose component has at most max_size pixels.
//
// Definition (a function of the inputs alone):
//   * d(p) = (a x + b y) + c in float, un-fused: les_disparity_kernel's map (les_post.h)
//   * 4-neighbours p, q are connected iff both d are finite and fabsf(d(p) - d(q)) <= max_diff; a non-finite pixel is a component of its own
//   * root of a component = its smallest linear index y W + x (int32); size = its pixel count; speckle iff size <= max_size
//
// One word per pixel, parent[p] <= p at all times: it starts so, and the only writes that follow are atomicMin and "store the root".  Hence every
// walk along parents strictly decreases and ends, whatever other workgroups do meanwhile, and the root of a finished component is its minimum.
// Four launches; the launch boundary is the only ordering between them (no flags, no fences, no workgroup waits on another):
//   1. les_speckle_tile_kernel     one workgroup labels one kSpkTH x kSpkTW tile in LDS (row scan, column merge, flatten), writes the global parent of
//                                  every pixel (its tile-local root) and, at tile-local roots, the pixel count of the tile-local component (0 elsewhere)
//   2. les_speckle_merge_kernel    one work-item per connected pixel pair across a tile border unites the two components
//   3. les_speckle_flatten_kernel  every pixel walks to its root and stores it; a tile-local root that is not the root adds its count to the root's
//   4. les_speckle_mask_kernel     mask (and optionally root and size) per pixel
// Integer atomics only: roots, sizes and mask do not depend on the launch geometry or on the order in which the atomics land.
#pragma once

#include "les_simt.h"

namespace les {

constexpr int kSpkTH = 16, kSpkTW = 32;      // the tile (les_hip_speckle_tile)
constexpr int kSpkNT = 256;                  // work-items of a workgroup of every kernel here
constexpr int kSpkN = kSpkTH * kSpkTW;

__device__ __forceinline__ bool spk_finite(float d) { return (__float_as_uint(d) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool spk_connected(float a, float b, float max_diff) { return spk_finite(a) && spk_finite(b) && fabsf(a - b) <= max_diff; }

// A parent word that another work-item may update in the same launch is read and written with relaxed agent-scope atomics: a plain load may be
// served from a stale line for the whole kernel.  A stale parent is still an ancestor (parents only decrease); what an atomic RETURNS is current.
__device__ __forceinline__ int spk_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void spk_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The walk to the root.  Ends: x strictly decreases (parent[x] <= x) and is bounded by 0.  May return an ancestor that has stopped being a root.
__device__ __forceinline__ int spk_find(const int* parent, int x)
{
    for (;;) {
        const int p = spk_load(parent + x);
        if (p >= x) return x;
        x = p;
    }
}

// Unite the components of a and b, the larger root under the smaller.  atomicMin on the larger candidate a returns the word's value before:
//   old == a   a was a root and now hangs under b: done
//   old <  a   a had the parent `old` already (it was no root, or another work-item was faster); the word now holds min(old, b), so a stays
//              attached to one of the two and `old` and b are what is left to unite
// Ends: the new pair (find(old), find(b)) has old < a and b < a, so max(a, b) strictly decreases on a value the atomic returned; bounded by 0.
__device__ __forceinline__ void spk_union(int* parent, int a, int b)
{
    a = spk_find(parent, a);
    b = spk_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old >= a) break;
        a = spk_find(parent, old);
        b = spk_find(parent, b);
    }
}

// 1. grid (ceil(W / kSpkTW), ceil(H / kSpkTH)), kSpkNT work-items.  Pixels of the tile outside the image are NaN: connected to nothing, never written.
__global__ void __launch_bounds__(kSpkNT)
les_speckle_tile_kernel(const float* __restrict__ disp, int* __restrict__ parent, int* __restrict__ size, int H, int W, float max_diff)
{
    __shared__ float s_d[kSpkN];
    __shared__ int s_par[kSpkN];
    __shared__ int s_cnt[kSpkN];
    const int tid = threadIdx.x, x0 = blockIdx.x * kSpkTW, y0 = blockIdx.y * kSpkTH;
    for (int i = tid; i < kSpkN; i += kSpkNT) {
        const int x = x0 + i % kSpkTW, y = y0 + i / kSpkTW;
        s_d[i] = (x < W && y < H) ? disp[(size_t)y * W + x] : __int_as_float(0x7fc00000);
        s_cnt[i] = 0;
    }
    __syncthreads();
    // row scan: the first pixel of the run of connected neighbours that ends here (reads s_d only)
    for (int i = tid; i < kSpkN; i += kSpkNT) {
        const int row = i - i % kSpkTW;
        int j = i;
        while (j > row && spk_connected(s_d[j], s_d[j - 1], max_diff)) j--;
        s_par[i] = j;
    }
    __syncthreads();
    // column merge
    for (int i = tid; i < kSpkN; i += kSpkNT)
        if (i >= kSpkTW && spk_connected(s_d[i], s_d[i - kSpkTW], max_diff)) spk_union(s_par, i, i - kSpkTW);
    __syncthreads();
    // flatten (nobody writes s_par any more) and count
    int r[kSpkN / kSpkNT];
    for (int k = 0; k < kSpkN / kSpkNT; k++) {
        r[k] = spk_find(s_par, tid + k * kSpkNT);
        atomicAdd(&s_cnt[r[k]], 1);
    }
    __syncthreads();
    for (int k = 0; k < kSpkN / kSpkNT; k++) {
        const int i = tid + k * kSpkNT;
        const int x = x0 + i % kSpkTW, y = y0 + i / kSpkTW;
        if (x < W && y < H) {
            // the tile-local order is the order of the linear indices within the tile: the tile-local root is the smallest index
            parent[(size_t)y * W + x] = (y0 + r[k] / kSpkTW) * W + (x0 + r[k] % kSpkTW);
            size[(size_t)y * W + x] = s_cnt[i];
        }
    }
}

// 2. one work-item per pixel pair across an interior tile border: first the (W - 1) / kSpkTW vertical borders (H pairs each), then the
// (H - 1) / kSpkTH horizontal ones (W pairs each)
__global__ void __launch_bounds__(kSpkNT)
les_speckle_merge_kernel(const float* __restrict__ disp, int* parent, int H, int W, float max_diff)
{
    const long long t = (long long)blockIdx.x * kSpkNT + threadIdx.x;
    const int nbx = (W - 1) / kSpkTW, nby = (H - 1) / kSpkTH;
    const long long nv = (long long)nbx * H, nh = (long long)nby * W;
    int p, q;
    if (t < nv) {
        const int y = (int)(t / nbx), x = ((int)(t % nbx) + 1) * kSpkTW;
        p = y * W + x;
        q = p - 1;
    } else if (t < nv + nh) {
        const long long u = t - nv;
        const int y = ((int)(u / W) + 1) * kSpkTH, x = (int)(u % W);
        p = y * W + x;
        q = p - W;
    } else
        return;
    if (spk_connected(disp[p], disp[q], max_diff)) spk_union(parent, p, q);
}

// 3. every pixel to its root.  The components are final, so a root's word never changes here; a pixel whose word is rewritten meanwhile is read
// either way as an ancestor.  size[p] is read plainly: only a root's word is added to in this launch, and p is none.
__global__ void __launch_bounds__(kSpkNT)
les_speckle_flatten_kernel(int* parent, int* size, int P)
{
    const long long t = (long long)blockIdx.x * kSpkNT + threadIdx.x;
    if (t >= P) return;
    const int p = (int)t;
    const int r = spk_find(parent, p);
    if (r == p) return;
    spk_store(parent + p, r);
    const int c = size[p];
    if (c > 0) atomicAdd(size + r, c);
}

// 4. mask 255 / 0 (accumulate: 255 is OR-ed into a mask that exists), and per pixel its root and its component's size where asked for
__global__ void __launch_bounds__(kSpkNT)
les_speckle_mask_kernel(const int* __restrict__ parent, const int* __restrict__ size, uint8_t* __restrict__ mask, int* __restrict__ root_out,
                        int* __restrict__ size_out, int P, int max_size, int accumulate)
{
    const long long t = (long long)blockIdx.x * kSpkNT + threadIdx.x;
    if (t >= P) return;
    const int r = parent[t], s = size[r];
    const bool speckle = s <= max_size;
    if (!accumulate) mask[t] = speckle ? 255 : 0;
    else if (speckle) mask[t] = 255;
    if (root_out) root_out[t] = r;
    if (size_out) size_out[t] = s;
}

}  // namespace les
