// les_confidence.h -- the confidence of a given label map under an aggregated cost volume: per pixel, how much cheaper the aggregated cost is near
// the pixel's own disparity than anywhere else on its cost curve (the cost-margin measure of the confidence literature, taken on the filtered
// volume).  The reference has no such step: it tells nobody which pixels of its result to trust.  The slabs are what les_wtavol.h reduces (the
// batch path's output for the fronto-parallel planes, les_hip_batch_create with out_slabs = 1); this is a second streaming reduction over them.
//
// DEFINITION (stated here once; tests/confidence_cases.py restates it in numpy).
//   A pixel has costs c_0 ... c_{K-1}, one per slab; slab k holds the aggregated cost of the fronto-parallel plane at disparity d0 + k
//   (d0 = min_disparity).  Its label (a, b, c, v) gives its own disparity d = (a x + b y) + c, un-fused (les_disparity_kernel's map), and
//   u = d - d0.  Slab k is IN BAND iff fabsf((float)k - u) <= band (a NaN u is never in band).  Every operation in f32, in this order, not
//   contracted:
//     own = +inf, rival = +inf, k_r = -1; for k = 0 ... K-1:
//         in band:  if (c_k < own) own = c_k;
//         else:     if (c_k < rival) { rival = c_k; k_r = k; }
//         (NaN and +inf never win, of equal rivals the lowest k wins, -0 and +0 are equal)
//     conf = 0                       when own is still +inf (a label outside the volume's range, a NaN label, an in-band that is all NaN / +inf)
//     conf = 1                       otherwise, when k_r < 0 (nothing finite lies outside the band)
//     m = (rival - own) / scale,  conf = (m > 0) ? (m < 1 ? m : 1) : 0         otherwise (a NaN m gives 0)
//   Outputs: conf in [0, 1], and optionally own, rival (f32) and k_r (i32) as the reduction left them.
//
// The slabs arrive in chunks, as for the arg-min: the step kernel consumes n slabs [n][H][W] and updates a per-pixel state, the finish kernel turns
// the state into the outputs.  STATE: four planes of P4 = argmin_plane_words(H W) words,
//     u (f32) | own (f32) | rival (f32) | k_r (i32)
// With k_first = 0 the state is initialised from the label map (read only then); afterwards it is a function of the slabs seen alone, so the chunking
// cannot change a bit.
//
// SHAPE: the arg-min's (les_wtavol.h): a read-once stream, n H W 4 bytes in, 16 bytes per pixel of state in and out (with k_first = 0 the 16-byte label
// is read in its place).  A thread owns four consecutive pixels of the flat H W index, keeps their state in registers and issues kArgminInFlight
// 16-byte loads (one per slab) before it compares any of them; unaligned slabs and the last, partial group are read dword by dword.  Per element
// the in-band test costs a subtraction and a compare on top of the arg-min's compare and selects ((float)k is per slab, not per element).  No LDS,
// no atomics; grid = ceil(H W / 4 / 256) workgroups.
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).  No inline assembly.
#pragma once

#include "les_simt.h"
#include "les_wtavol.h"

namespace les {

constexpr int kConfStatePlanes = 4;

// slab g (counted over the whole volume) offers cost c to a pixel whose own disparity sits u slabs above the first
__device__ __forceinline__ void conf_take(float c, int g, float u, float band, float& own, float& rival, int& kr)
{
    // (selects, not branches: neighbouring pixels fall on both sides of the band)
    const bool in = fabsf((float)g - u) <= band;
    const bool to_own = in & (c < own), to_rival = !in & (c < rival);
    own = to_own ? c : own;
    rival = to_rival ? c : rival;
    kr = to_rival ? g : kr;
}

// grid = ceil(ceil(P / 4) / kArgminThreads), block = kArgminThreads.  labels: [P] planes, read only when k_first == 0 (W: the row length, for a
// pixel's x and y); slabs: [n][P] floats; state: kConfStatePlanes planes of P4 words, 16-byte aligned; k_first: the index of slabs[0] in the
// whole volume.  ALIGNED: slabs is 16-byte aligned and P % 4 == 0, so every load is a 16-byte one and nothing is tested per slab.
template <bool ALIGNED>
__global__ void __launch_bounds__(kArgminThreads)
les_slab_confidence_kernel(const float4* __restrict__ labels, const float* __restrict__ slabs, int n, int k_first, size_t P, int W, float d0, float band,
                           float* __restrict__ state)
{
    const size_t i = ((size_t)blockIdx.x * kArgminThreads + threadIdx.x) * 4;
    if (i >= P) return;
    const size_t P4 = argmin_plane_words(P);
    const bool whole = ALIGNED || i + 4 <= P;
    float4* s_u = reinterpret_cast<float4*>(state + i);
    float4* s_own = reinterpret_cast<float4*>(state + P4 + i);
    float4* s_rival = reinterpret_cast<float4*>(state + 2 * P4 + i);
    ArgminInt4* s_kr = reinterpret_cast<ArgminInt4*>(state + 3 * P4 + i);

    float u[4], own[4], rival[4];
    int kr[4];
    if (k_first == 0) {
        int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * (size_t)W);     // (one division per thread; the other three pixels step from it)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            own[e] = rival[e] = __builtin_inff();
            kr[e] = -1;
            u[e] = __builtin_nanf("");                      // (the padding of the last group: never in band, never read by the finish)
            if (ALIGNED || i + e < P) {
                const float4 l = labels[i + e];
                u[e] = ((l.x * (float)x + l.y * (float)y) + l.z) - d0;
            }
            if (++x == W) { x = 0; y++; }
        }
    } else {                                                // (the planes are padded to P4: the last group's state is whole)
        const float4 a = *s_u, b = *s_own, r = *s_rival;
        const ArgminInt4 k = *s_kr;
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
        own[0] = b.x; own[1] = b.y; own[2] = b.z; own[3] = b.w;
        rival[0] = r.x; rival[1] = r.y; rival[2] = r.z; rival[3] = r.w;
        kr[0] = k.x; kr[1] = k.y; kr[2] = k.z; kr[3] = k.w;
    }

    const float* p = slabs + i;
    int k = 0;
    for (; k + kArgminInFlight <= n; k += kArgminInFlight) {
        float v[kArgminInFlight][4];
#pragma unroll
        for (int j = 0; j < kArgminInFlight; j++) {
            const float* q = p + (size_t)(k + j) * P;
            // (the slab's alignment is the same for every lane: i is a multiple of 4)
            argmin_load4(q, ALIGNED || (whole && ((uintptr_t)(slabs + (size_t)(k + j) * P) & 15) == 0), i, P, v[j]);
        }
#pragma unroll
        for (int j = 0; j < kArgminInFlight; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) conf_take(v[j][e], k_first + k + j, u[e], band, own[e], rival[e], kr[e]);
    }
    for (; k < n; k++) {
        float v[4];
        argmin_load4(p + (size_t)k * P, ALIGNED || (whole && ((uintptr_t)(slabs + (size_t)k * P) & 15) == 0), i, P, v);
#pragma unroll
        for (int e = 0; e < 4; e++) conf_take(v[e], k_first + k, u[e], band, own[e], rival[e], kr[e]);
    }

    *s_u = make_float4(u[0], u[1], u[2], u[3]);
    *s_own = make_float4(own[0], own[1], own[2], own[3]);
    *s_rival = make_float4(rival[0], rival[1], rival[2], rival[3]);
    *s_kr = ArgminInt4{kr[0], kr[1], kr[2], kr[3]};
}

// grid = ceil(P / kArgminThreads), block = kArgminThreads: one pixel per thread (12 bytes of state in, 4 to 16 bytes out).  own_out, rival_out and
// kr_out may be null.
__global__ void __launch_bounds__(kArgminThreads)
les_slab_confidence_finish_kernel(const float* __restrict__ state, size_t P, float scale, float* __restrict__ conf, float* __restrict__ own_out,
                                  float* __restrict__ rival_out, int* __restrict__ kr_out)
{
    const size_t i = (size_t)blockIdx.x * kArgminThreads + threadIdx.x;
    if (i >= P) return;
    const size_t P4 = argmin_plane_words(P);
    const float own = state[P4 + i], rival = state[2 * P4 + i];
    const int kr = reinterpret_cast<const int*>(state + 3 * P4)[i];
    float cf;
    if (!(own < __builtin_inff())) cf = 0.0f;               // (own only ever takes a value below +inf: this is "still +inf")
    else if (kr < 0) cf = 1.0f;
    else {
        const float m = (rival - own) / scale;
        cf = (m > 0.0f) ? (m < 1.0f ? m : 1.0f) : 0.0f;
    }
    conf[i] = cf;
    if (own_out) own_out[i] = own;
    if (rival_out) rival_out[i] = rival;
    if (kr_out) kr_out[i] = kr;
}

}  // namespace les
