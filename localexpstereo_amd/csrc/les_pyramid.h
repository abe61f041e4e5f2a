// les_pyramid.h -- the way down and the way up of a half-resolution solve: the images and matching-cost volumes of a context pooled by two
// in every dimension, and a map of slanted planes found at half resolution re-expressed at full resolution, edge-aware.  No reference
// counterpart: the reference solves at one resolution (LES/FastGCStereo.h:133-227).
//
// DEFINITION (stated here once; tests/pyramid_cases.py restates it in numpy).  Sizes: Hh = (H + 1) / 2, Wh = (W + 1) / 2, Dh = (D + 1) / 2;
// every source index clamps to its range (edge replication).  All three operations are exact -- integers, or f32 in a fixed order with
// power-of-two multipliers only, so that contracting a multiply and an add into a fused one cannot change a bit.
//
//   IMAGE POOL    u8 [H][W][3] -> [Hh][Wh][3], per channel
//                   (p(2y, 2x) + p(2y, 2x + 1) + p(2y + 1, 2x) + p(2y + 1, 2x + 1) + 2) >> 2
//   VOLUME POOL   f32 [D][H][W] -> [Dh][Hh][Wh]; half slice k is full slice 2k (half disparity d = full disparity 2d).  For each of the
//                 four pixels (2y + dy, 2x + dx), in the order (dy, dx) = (0,0), (0,1), (1,0), (1,1):
//                   t = (0.25f C[2k - 1] + 0.5f C[2k]) + 0.25f C[2k + 1]
//                 and the result is (((t00 + t01) + t10) + t11) 0.25f.  NaN and +-inf propagate by plain arithmetic.
//   LABEL UPSAMPLE  planes f32 [Hh][Wh][4] -> [H][W][4], guided by the full and the pooled image of the same view (packed B | G << 8 | R << 16).
//                 Full pixel (X, Y) has four candidates with coordinates clamped to the half image, in this order:
//                   (xh, yh) = (X >> 1, Y >> 1), (xn, yh), (xh, yn), (xn, yn)      xn = xh + (X & 1 ? 1 : -1), yn likewise
//                 The winner is the candidate of least sum_c |I_full(Y, X)_c - I_half(cand)_c| (integers); the first candidate wins ties.
//                 Its plane (a, b, c, v) becomes (a, b, (2c - 0.5f a) - 0.5f b, 2v): d_full(X, Y) = 2 d_half((X - 1/2) / 2, (Y - 1/2) / 2).
//                 It is kept -- kind 0 -- iff it is a valid label of the full context at (X, Y) (label_valid, LES/StereoEnergy.h:560-610).
//                 Otherwise with ds = ((X a + Y b) + 1 c') + 0 v' (label_valid's own value): (0, 0, clamp(ds, mind, maxd), 0) -- kind 1 --
//                 for a finite ds, (0, 0, mind, 0) -- kind 2 -- for a non-finite one.
//
// The volume pool is the hot one: it reads the whole volume once and writes an eighth of it.
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM: no non-temporal load there).
// No inline assembly.
#pragma once

#include "les_bilateral.h"

namespace les {

constexpr int kPyrTX = 128;                 // output pixels of a wave's row segment: 64 lanes x 2 (one 16-byte load per lane, input row and slice)
constexpr int kPyrRows = 4;                 // output rows of a workgroup: one per wave
constexpr int kPyrKC = 16;                  // half slices of a workgroup's chunk: 2 kPyrKC + 1 full slices are read for 2 kPyrKC owed

#if defined(LES_SIM)
template <bool NT>
__device__ inline void pyr_load4(const float* p, float* v) { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
__device__ inline void pyr_store2(float* p, float a, float b) { p[0] = a; p[1] = b; }
#else
typedef float pyr_v4f __attribute__((ext_vector_type(4)));
typedef float pyr_v2f __attribute__((ext_vector_type(2)));
// ONE global_load_dwordx4 (NT: with the non-temporal hint -- this kernel reads every entry once)
template <bool NT>
__device__ __forceinline__ void pyr_load4(const float* p, float* v)
{
    pyr_v4f q;
    if constexpr (NT) q = __builtin_nontemporal_load(reinterpret_cast<const pyr_v4f*>(p));
    else q = *reinterpret_cast<const pyr_v4f*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void pyr_store2(float* p, float a, float b)
{
    const pyr_v2f q = {a, b};
    *reinterpret_cast<pyr_v2f*>(p) = q;
}
#endif

__device__ __forceinline__ uint32_t pyr_avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

// Image pool of a u8 BGR image.  grid = (ceil(Wh / 256), Hh).  Runs once per image: one output pixel per thread, byte loads.
__global__ void les_pool_image_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W)
{
    const int Wh = (W + 1) / 2;
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (x >= Wh) return;
    const int x0 = 2 * x, x1 = min(2 * x + 1, W - 1), y0 = 2 * y, y1 = min(2 * y + 1, H - 1);
    const uint8_t *p00 = src + 3 * ((size_t)y0 * W + x0), *p01 = src + 3 * ((size_t)y0 * W + x1);
    const uint8_t *p10 = src + 3 * ((size_t)y1 * W + x0), *p11 = src + 3 * ((size_t)y1 * W + x1);
    uint8_t* o = dst + 3 * ((size_t)y * Wh + x);
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (uint8_t)pyr_avg4(p00[c], p01[c], p10[c], p11[c]);
}

// The same pool of the packed guide a context keeps (B | G << 8 | R << 16 per pixel), written as a u8 BGR image: what les_hip_create_half
// builds the half context's images from (the context does not keep the u8 images it was created from).
__global__ void les_pool_packed_kernel(const uint32_t* __restrict__ ipk, uint8_t* __restrict__ dst, int H, int W)
{
    const int Wh = (W + 1) / 2;
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (x >= Wh) return;
    const int x0 = 2 * x, x1 = min(2 * x + 1, W - 1), y0 = 2 * y, y1 = min(2 * y + 1, H - 1);
    const uint32_t a = ipk[(size_t)y0 * W + x0], b = ipk[(size_t)y0 * W + x1], c = ipk[(size_t)y1 * W + x0], d = ipk[(size_t)y1 * W + x1];
    uint8_t* o = dst + 3 * ((size_t)y * Wh + x);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (uint8_t)pyr_avg4((a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, (c >> (8 * k)) & 255u, (d >> (8 * k)) & 255u);
}

// The 2 x 4 input floats of a thread at one slice: rows y0, y1, columns x .. x + 3 (clamped on the dword path).  v[r][j].
template <bool VEC, bool NT>
__device__ __forceinline__ void pyr_load_slice(const float* __restrict__ vol, size_t row0, size_t row1, int x, int W, float v[2][4])
{
    if constexpr (VEC) {
        pyr_load4<NT>(vol + row0 + x, v[0]);
        pyr_load4<NT>(vol + row1 + x, v[1]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int xc = min(x + j, W - 1);
            v[0][j] = vol[row0 + xc];
            v[1][j] = vol[row1 + xc];
        }
    }
}

// Volume pool.  grid = (ceil(Wh / kPyrTX), ceil(Hh / kPyrRows), ceil(Dh / kPyrKC)), block = 256 = 4 waves; no LDS, no barrier.  Wave w owns
// output row kPyrRows blockIdx.y + w; lane l owns the two output pixels xh = kPyrTX blockIdx.x + 2 l, xh + 1 of that row -- input columns
// 2 xh .. 2 xh + 3 of input rows 2 yh, 2 yh + 1: one 16-byte load per lane, row and slice, 1 KB contiguous per wave -- and walks the chunk's
// half slices k in order.  The eight values of full slice 2k + 1 stay in registers and serve as slice 2(k + 1) - 1 of the next step, so every
// input float is loaded once per chunk (the slice before a chunk's first one is loaded twice: 1 / (2 kPyrKC) more).  The definition takes the
// slices' weighted sum per pixel BEFORE it adds the four pixels, so it is the loaded values that are carried, not their 2 x 2 sum.
// VEC (W % 4 == 0, the input base 16-byte aligned, the output base 8-byte aligned: every input row starts 16-byte aligned, Wh = W / 2 is even):
// 16-byte loads and one 8-byte store per lane.  Otherwise dword loads with clamped columns and dword stores with their own bounds.
// 64-bit element offsets throughout.
template <bool VEC, bool NT>
__global__ void __launch_bounds__(256)
les_pool_volume_kernel(const float* __restrict__ vol, float* __restrict__ out, int D, int H, int W)
{
    const int Dh = (D + 1) / 2, Hh = (H + 1) / 2, Wh = (W + 1) / 2;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int yh = (int)blockIdx.y * kPyrRows + wave, xh = (int)blockIdx.x * kPyrTX + 2 * lane;
    const int k_lo = (int)blockIdx.z * kPyrKC, k_hi = min(k_lo + kPyrKC, Dh);
    if (yh >= Hh || xh >= Wh) return;
    const int x = 2 * xh;                                              // (VEC: x + 3 <= W - 1, since xh is even and below Wh = W / 2)
    const size_t S = (size_t)H * W;
    const size_t r0 = (size_t)(2 * yh) * W, r1 = (size_t)min(2 * yh + 1, H - 1) * W;
    float m[2][4], c[2][4], p[2][4];                                   // slices 2k - 1, 2k, 2k + 1
    {
        const size_t s = (size_t)max(2 * k_lo - 1, 0) * S;
        pyr_load_slice<VEC, NT>(vol, s + r0, s + r1, x, W, m);
    }
    for (int k = k_lo; k < k_hi; k++) {
        const size_t sc = (size_t)(2 * k) * S, sp = (size_t)min(2 * k + 1, D - 1) * S;
        pyr_load_slice<VEC, NT>(vol, sc + r0, sc + r1, x, W, c);
        pyr_load_slice<VEC, NT>(vol, sp + r0, sp + r1, x, W, p);
        float o[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {                              // (dy, dx) = (0,0), (0,1), (1,0), (1,1)
                const int r = i >> 1, j = 2 * q + (i & 1);
                t[i] = (0.25f * m[r][j] + 0.5f * c[r][j]) + 0.25f * p[r][j];
            }
            o[q] = (((t[0] + t[1]) + t[2]) + t[3]) * 0.25f;
        }
        float* dst = out + ((size_t)k * Hh + yh) * Wh + xh;
        if constexpr (VEC) {
            pyr_store2(dst, o[0], o[1]);
        } else {
            dst[0] = o[0];
            if (xh + 1 < Wh) dst[1] = o[1];
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) m[r][j] = p[r][j];
    }
}

// Label upsample.  g: the FULL context's geometry (H, W, disparity range); Hh, Wh: the half map's size.  grid = (ceil(W / 256), H): one full
// pixel per thread; the four candidates' guide pixels and the winner's plane come through the cache (neighbouring threads share them).
__global__ void les_upsample_labels_kernel(Geom g, const uint32_t* __restrict__ ipk_full, const uint32_t* __restrict__ ipk_half,
                                           const float4* __restrict__ src, float4* __restrict__ out, uint8_t* __restrict__ kind, int Hh, int Wh)
{
    const int X = (int)(blockIdx.x * blockDim.x + threadIdx.x), Y = (int)blockIdx.y;
    if (X >= g.W) return;
    const int xh = X >> 1, yh = Y >> 1;
    const int xn = min(max(xh + ((X & 1) ? 1 : -1), 0), Wh - 1), yn = min(max(yh + ((Y & 1) ? 1 : -1), 0), Hh - 1);
    const size_t px = (size_t)Y * g.W + X;
    const uint32_t gc = ipk_full[px];
    const int cx[4] = {xh, xn, xh, xn}, cy[4] = {yh, yh, yn, yn};
    size_t win = 0;
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const size_t q = (size_t)cy[i] * Wh + cx[i];
        const uint32_t s = bf_sad(gc, ipk_half[q]);
        if (s < best) { best = s; win = q; }
    }
    const float4 l = src[win];
    float4 o = make_float4(l.x, l.y, (2.0f * l.z - 0.5f * l.x) - 0.5f * l.y, 2.0f * l.w);
    uint8_t k = 0;
    if (!label_valid(g, o.x, o.y, o.z, o.w, X, Y)) {
        const float ds = (((float)X * o.x + (float)Y * o.y) + 1.0f * o.z) + 0.0f * o.w;
        if ((__float_as_uint(ds) & 0x7f800000u) != 0x7f800000u) {
            o = make_float4(0.0f, 0.0f, ds < g.mind ? g.mind : (ds > g.maxd ? g.maxd : ds), 0.0f);
            k = 1;
        } else {
            o = make_float4(0.0f, 0.0f, g.mind, 0.0f);
            k = 2;
        }
    }
    out[px] = o;
    if (kind) kind[px] = k;
}

}  // namespace les
