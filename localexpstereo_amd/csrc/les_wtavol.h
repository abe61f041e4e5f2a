// les_wtavol.h -- winner-take-all labels of an aggregated cost volume (cost-volume filtering: the per-pixel minimum over the disparity slices,
// refined to sub-pixel).  The reference has no such step: its only start is one random plane per finest-layer cell (initCurrentFast,
// LES/FastGCStereo.h:94-115).  The slabs are what the batch path writes for fronto-parallel planes (les_hip_batch_create with out_slabs = 1: the H1
// workload); this is the streaming reduction over them.
//
// DEFINITION (stated here once; tests/wtavol_cases.py restates it in numpy).
//   A pixel has costs c_0 ... c_{K-1}, one per slab; slab k holds the aggregated cost of the fronto-parallel plane at disparity d0 + k
//   (d0 = min_disparity).  Every operation in f32, in this order, not contracted:
//     best = +inf, k* = -1; for k = 0 ... K-1: if (c_k < best) { best = c_k; k* = k; }
//         (k* is the smallest k whose c_k is the minimum: NaN never wins, of equal costs the lowest disparity wins, -0 and +0 are equal; +inf
//         never wins either)
//     c0 = c_{k*}, cm = c_{k* - 1}, cp = c_{k* + 1}
//     off = 0, unless subpixel != 0 and 0 < k* < K-1 and cm, cp are finite and den = (cm - c0) + (cp - c0) > 0: then off = 0.5f * (cm - cp) / den
//         (cm > c0 and cp >= c0 by the tie rule, so |off| <= 0.5: no clamp)
//     label (0, 0, (float(k*) + off) + d0, 0), cost c0;  without a winner (k* = -1): label (0, 0, d0, 0), cost +inf
//
// The slabs arrive in chunks (the whole volume, 256 x 1500 x 1000 floats = 1.5 GB, need never exist): the step kernel consumes n slabs [n][H][W]
// and updates a per-pixel state, the finish kernel turns the state into labels and costs.  STATE: five planes of P4 = (H W rounded up to 4) words,
//     best (f32) | k* (i32) | cm (f32) | cp (f32) | prev (f32: the cost of the last slab consumed)
// cm of a winner on the first slab of a chunk is the state's prev; cp of a winner on the last slab of a chunk is taken from the first slab of the
// next one (k* == k_first - 1 says it is still owed).  The state after slab k is a function of c_0 ... c_k alone, so the chunking cannot change a bit.
//
// SHAPE: a read-once stream, n H W 4 bytes in, 20 bytes per pixel of state in and out (the read is skipped for k_first = 0).  A thread owns four
// consecutive pixels of the flat H W index, keeps their state in registers and issues kArgminInFlight 16-byte loads (one per slab) before it
// compares any of them; a slab whose base is not 16-byte aligned (H W % 4 != 0 puts every other slab or three of four off) and the last, partial
// group are read dword by dword.  No LDS, no atomics; grid = ceil(H W / 4 / 256) workgroups (1465 at 1500 x 1000, 1 at 5 x 7).
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_simt.h"

namespace les {

constexpr int kArgminThreads = 256;
constexpr int kArgminInFlight = 8;          // slabs loaded before the first comparison
constexpr int kArgminStatePlanes = 5;

struct alignas(16) ArgminInt4 { int x, y, z, w; };

__host__ __device__ __forceinline__ size_t argmin_plane_words(size_t P) { return (P + 3) & ~(size_t)3; }

__device__ __forceinline__ bool argmin_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// the parabola offset of the winner ks of K costs: c0 its cost, cm / cp the costs of slabs ks - 1 / ks + 1 (read only when they exist); also the
// read-out of les_sgm.h
__device__ __forceinline__ float argmin_offset(int ks, int K, int subpixel, float c0, float cm, float cp)
{
    float off = 0.0f;
    if (subpixel && ks > 0 && ks < K - 1 && argmin_finite(cm) && argmin_finite(cp)) {
        const float den = (cm - c0) + (cp - c0);
        if (den > 0.0f) off = 0.5f * (cm - cp) / den;
    }
    return off;
}

// slab g (counted over the whole volume) offers cost c to a pixel
__device__ __forceinline__ void argmin_take(float c, int g, float& best, int& ks, float& cm, float& cp, float& prev)
{
    if (ks >= 0 && ks == g - 1) cp = c;                     // the slab after the winner so far
    if (c < best) { best = c; ks = g; cm = prev; cp = __builtin_nanf(""); }
    prev = c;
}

// four consecutive costs of one slab from p (pixels i ... i + 3 of P); vec: p is 16-byte aligned and the group is whole
__device__ __forceinline__ void argmin_load4(const float* p, bool vec, size_t i, size_t P, float v[4])
{
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = i + e < P ? p[e] : __builtin_nanf("");
    }
}

// grid = ceil(ceil(P / 4) / kArgminThreads), block = kArgminThreads.  slabs: [n][P] floats; state: kArgminStatePlanes planes of P4 words,
// 16-byte aligned; k_first: the index of slabs[0] in the whole volume (0: the state is initialised, not read).
// ALIGNED: slabs is 16-byte aligned and P % 4 == 0, so every load is a 16-byte one and nothing is tested per slab.
template <bool ALIGNED>
__global__ void __launch_bounds__(kArgminThreads)
les_slab_argmin_kernel(const float* __restrict__ slabs, int n, int k_first, size_t P, float* __restrict__ state)
{
    const size_t i = ((size_t)blockIdx.x * kArgminThreads + threadIdx.x) * 4;
    if (i >= P) return;
    const size_t P4 = argmin_plane_words(P);
    const bool whole = ALIGNED || i + 4 <= P;
    float4* s_best = reinterpret_cast<float4*>(state + i);
    ArgminInt4* s_ks = reinterpret_cast<ArgminInt4*>(state + P4 + i);
    float4* s_cm = reinterpret_cast<float4*>(state + 2 * P4 + i);
    float4* s_cp = reinterpret_cast<float4*>(state + 3 * P4 + i);
    float4* s_prev = reinterpret_cast<float4*>(state + 4 * P4 + i);

    float best[4], cm[4], cp[4], prev[4];
    int ks[4];
    if (k_first == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) { best[e] = __builtin_inff(); ks[e] = -1; cm[e] = cp[e] = prev[e] = __builtin_nanf(""); }
    } else {                                                // (the planes are padded to P4: the last group's state is whole)
        const float4 b = *s_best, m = *s_cm, q = *s_cp, r = *s_prev;
        const ArgminInt4 k = *s_ks;
        best[0] = b.x; best[1] = b.y; best[2] = b.z; best[3] = b.w;
        ks[0] = k.x; ks[1] = k.y; ks[2] = k.z; ks[3] = k.w;
        cm[0] = m.x; cm[1] = m.y; cm[2] = m.z; cm[3] = m.w;
        cp[0] = q.x; cp[1] = q.y; cp[2] = q.z; cp[3] = q.w;
        prev[0] = r.x; prev[1] = r.y; prev[2] = r.z; prev[3] = r.w;
    }

    const float* p = slabs + i;
    int k = 0;
    for (; k + kArgminInFlight <= n; k += kArgminInFlight) {
        float v[kArgminInFlight][4];
#pragma unroll
        for (int u = 0; u < kArgminInFlight; u++) {
            const float* q = p + (size_t)(k + u) * P;
            // (the slab's alignment is the same for every lane: i is a multiple of 4)
            argmin_load4(q, ALIGNED || (whole && ((uintptr_t)(slabs + (size_t)(k + u) * P) & 15) == 0), i, P, v[u]);
        }
#pragma unroll
        for (int u = 0; u < kArgminInFlight; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) argmin_take(v[u][e], k_first + k + u, best[e], ks[e], cm[e], cp[e], prev[e]);
    }
    for (; k < n; k++) {
        float v[4];
        argmin_load4(p + (size_t)k * P, ALIGNED || (whole && ((uintptr_t)(slabs + (size_t)k * P) & 15) == 0), i, P, v);
#pragma unroll
        for (int e = 0; e < 4; e++) argmin_take(v[e], k_first + k, best[e], ks[e], cm[e], cp[e], prev[e]);
    }

    *s_best = make_float4(best[0], best[1], best[2], best[3]);
    *s_ks = ArgminInt4{ks[0], ks[1], ks[2], ks[3]};
    *s_cm = make_float4(cm[0], cm[1], cm[2], cm[3]);
    *s_cp = make_float4(cp[0], cp[1], cp[2], cp[3]);
    *s_prev = make_float4(prev[0], prev[1], prev[2], prev[3]);
}

// grid = ceil(P / kArgminThreads), block = kArgminThreads: one pixel per thread (16 bytes of state in, a 16-byte label and a cost out)
__global__ void __launch_bounds__(kArgminThreads)
les_slab_argmin_finish_kernel(const float* __restrict__ state, size_t P, int K, int subpixel, float d0, float4* __restrict__ labels, float* __restrict__ cost)
{
    const size_t i = (size_t)blockIdx.x * kArgminThreads + threadIdx.x;
    if (i >= P) return;
    const size_t P4 = argmin_plane_words(P);
    const float c0 = state[i], cm = state[2 * P4 + i], cp = state[3 * P4 + i];
    const int ks = reinterpret_cast<const int*>(state + P4)[i];
    if (ks < 0) {
        labels[i] = make_float4(0.0f, 0.0f, d0, 0.0f);
        cost[i] = __builtin_inff();
        return;
    }
    const float off = argmin_offset(ks, K, subpixel, c0, cm, cp);
    labels[i] = make_float4(0.0f, 0.0f, ((float)ks + off) + d0, 0.0f);
    cost[i] = c0;
}

}  // namespace les
