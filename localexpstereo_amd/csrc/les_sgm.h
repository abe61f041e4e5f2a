// les_sgm.h -- semi-global matching over a matching-cost volume: scan-line dynamic programming along 2, 4 or 8 directions, summed, read out per
// pixel.  The reference has no such step (its only start is one random plane per finest-layer cell, initCurrentFast, LES/FastGCStereo.h:94-115);
// this is the classic stage between local aggregation (les_wtavol.h) and the global graph cut: the cheapest thing that enforces smoothness across
// the whole image.
//
// DEFINITION (stated here once; tests/sgm_cases.py restates it in numpy).
//   The input is a view's own volume C, float [D][H][W], slice k = disparity d0 + k (d0 = min_disparity); K = int(max_disparity - min_disparity) + 1
//   slices are used.  Every operation in f32, in this order, not contracted; min(a, b) below is (b < a ? b : a) with the operands in the order written.
//   Truncation:  C'(p,k) = C(p,k) if C(p,k) is finite and C(p,k) < th_col, else th_col  (NaN, +-inf and everything >= th_col become th_col)
//   Directions r = (dx, dy), in this fixed order: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1); `paths` takes the first 2, 4 or 8.
//   Recurrence of one direction, q = p - r:
//     q outside the image:  L(p,k) = C'(p,k)
//     otherwise:            m = min_j L(q,j), then m = m + 0.0f  (the minimum as a value: where it is a zero it is +0)
//                           t = L(q,k)
//                           if k - 1 >= 0 or k + 1 <= K - 1:  n = min(L(q,k-1), L(q,k+1)) over the neighbours that exist, t = min(t, n + P1)
//                           t = min(t, m + P2)
//                           L(p,k) = C'(p,k) + (t - m)
//     (K = 1: L = C' + 0.)  Every L is finite as long as P2 and the costs are of a magnitude whose sums are.
//   Sum:       S = ((L_0 + L_1) + L_2) + ... in direction order.
//   Read-out:  per pixel over S(p,0..K-1) the rule of les_wtavol.h: k* the smallest k whose S is the minimum (comparison s < best from +inf), the
//              parabola offset of argmin_offset() when subpixel; label (0, 0, (float(k*) + off) + d0, 0); second output S(p,k*).
//
// SHAPE.  [D][H][W] puts a pixel's K costs H W floats apart, the wrong shape for a recurrence whose inner operation is a minimum over k:
//   les_sgm_transpose_kernel    truncates and transposes through a 64 x 64 LDS tile into Ct [H][W][Kp], Kp = 64 V with V = 1, 2, 4, 8 the smallest
//                               that holds K (K <= 512); loads run along x, stores along k.  The pad entries k >= K are written as +inf: they are
//                               never read as the cost of a disparity, never win a minimum and stay +inf in every L and in S (+inf plus
//                               a finite value), so the path kernel needs no test of k < K and lane K - 1's upper neighbour "does not exist".
//   les_sgm_path_kernel<V>      one wave per scan line (a row, a column, or a diagonal clipped to the image: H, W or W + H - 1 lines), a lane owns
//                               V consecutive disparities, so the k +- 1 neighbours are registers except at the lane edges (one lane shift each);
//                               the minimum over k is a wave reduction.  A step loads Kp floats of Ct (one contiguous piece), writes S (first
//                               direction) or reads, adds and writes it (later ones); the addresses do not depend on the recurrence, so
//                               the loads go through a ring of kSgmInFlight steps (how far ahead they really run is the compiler's schedule:
//                               DESIGN 3.2i).  Directions are successive launches: that order is the order of the sum, no atomics.
//   les_sgm_readout_kernel<V>   one wave per pixel (kSgmReadoutPixels pixels per wave, loaded before the first is reduced): lane-local first
//                               minimum, wave minimum of the values, wave minimum of the indices that hold it.
// Element offsets are 64-bit.  No LDS outside the transpose, no atomics, no inline assembly.
//
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM).
#pragma once

#include "les_simt.h"
#include "les_wtavol.h"

#include <stddef.h>

namespace les {

constexpr int kSgmThreads = 256;            // 4 waves: 4 scan lines / 4 groups of pixels per workgroup
constexpr int kSgmInFlight = 8;             // slots of the ring a scan line's loads go through
constexpr int kSgmMaxK = 512;
constexpr int kSgmTile = 64;                // transpose tile: 64 pixels of a row x 64 disparities
constexpr int kSgmReadoutPixels = 4;        // pixels per wave of the read-out

__host__ __device__ __forceinline__ int sgm_lane_vector(int K) { return K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : 8; }
__host__ __device__ __forceinline__ int sgm_padded(int K) { return 64 * sgm_lane_vector(K); }
__host__ __device__ __forceinline__ int sgm_lines(int H, int W, int dx, int dy) { return dy == 0 ? H : dx == 0 ? W : W + H - 1; }

// scan line `line` of direction (dx, dy): its first pixel (the one whose predecessor lies outside the image) and its length
__host__ __device__ __forceinline__ void sgm_line(int line, int H, int W, int dx, int dy, int& x0, int& y0, int& len)
{
    if (dy == 0) { x0 = dx > 0 ? 0 : W - 1; y0 = line; len = W; return; }
    if (dx == 0) { x0 = line; y0 = dy > 0 ? 0 : H - 1; len = H; return; }
    if (line < W) { x0 = line; y0 = dy > 0 ? 0 : H - 1; }                     // enters through the first / last row
    else { const int j = line - W + 1; x0 = dx > 0 ? 0 : W - 1; y0 = dy > 0 ? j : H - 1 - j; }      // ... through the first / last column, below / above the corner
    const int lx = dx > 0 ? W - x0 : x0 + 1, ly = dy > 0 ? H - y0 : y0 + 1;
    len = lx < ly ? lx : ly;
}

template <int V> struct alignas(4 * V) SgmVec { float v[V]; };

__device__ __forceinline__ float sgm_min(float a, float b) { return b < a ? b : a; }

// grid = (ceil(W / 64), H, Kp / 64), block = kSgmThreads.  vol: [D][H][W] (the first K slices are read); Ct: [H][W][Kp]
__global__ void __launch_bounds__(kSgmThreads)
les_sgm_transpose_kernel(const float* __restrict__ vol, float* __restrict__ Ct, int H, int W, int K, int Kp, float th_col)
{
    __shared__ float tile[kSgmTile][kSgmTile + 1];
    const int tx = threadIdx.x & 63, tw = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kSgmTile, y = blockIdx.y, k0 = blockIdx.z * kSgmTile;
    const size_t P = (size_t)H * W, row = (size_t)y * W;
    for (int r = tw; r < kSgmTile; r += kSgmThreads / 64) {
        const int k = k0 + r, x = x0 + tx;
        float v = k < K ? th_col : __builtin_inff();     // (a pad entry: never a cost, never the winner of a minimum)
        if (k < K && x < W) {
            const float c = vol[(size_t)k * P + row + x];
            if (argmin_finite(c) && c < th_col) v = c;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = tw; r < kSgmTile; r += kSgmThreads / 64) {
        const int x = x0 + r;
        if (x < W) Ct[(row + x) * Kp + k0 + tx] = tile[tx][r];
    }
}

// grid = ceil(lines / 4), block = kSgmThreads: wave w of the grid walks scan line w of direction (dx, dy).  FIRST: S is written, not added to.
template <int V, bool FIRST>
__global__ void __launch_bounds__(kSgmThreads)
les_sgm_path_kernel(const float* __restrict__ Ct, float* S, int H, int W, int dx, int dy, float P1, float P2)
{
    constexpr int Kp = 64 * V;
    constexpr int PF = kSgmInFlight;
    const int lane = threadIdx.x & 63;
    const int line = (int)blockIdx.x * (kSgmThreads / 64) + (int)(threadIdx.x >> 6);
    if (line >= sgm_lines(H, W, dx, dy)) return;            // (the whole wave)
    int x0, y0, len;
    sgm_line(line, H, W, dx, dy, x0, y0, len);
    const ptrdiff_t step = ((ptrdiff_t)dy * W + dx) * Kp;
    const size_t base = ((size_t)y0 * W + x0) * Kp + (size_t)lane * V;
    const float* pc = Ct + base;
    float* ps = S + base;
    const float inf = __builtin_inff();
    // the loads of steps 1 .. len - 1 go through a ring of PF steps: slot u holds step s with (s - 1) % PF == u.  Every load is unconditional -- past the end of
    // the line the last pixel is loaded again and never used -- so that the loop body is straight-line code the compiler can count waits in
    const int last = len - 1;
    SgmVec<V> bc[PF], bs[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) {
        const ptrdiff_t o = (ptrdiff_t)(1 + u < last ? 1 + u : last) * step;
        bc[u] = *reinterpret_cast<const SgmVec<V>*>(pc + o);
        if (!FIRST) bs[u] = *reinterpret_cast<const SgmVec<V>*>(ps + o);
    }

    // step 0: the pixel whose predecessor lies outside the image
    float lp[V];                                            // L of the previous pixel; +inf at the pad entries
    float m;                                                // its minimum over k
    {
        const SgmVec<V> c = *reinterpret_cast<const SgmVec<V>*>(pc);
        SgmVec<V> so;
        if (!FIRST) so = *reinterpret_cast<const SgmVec<V>*>(ps);
        float mn = inf;
#pragma unroll
        for (int e = 0; e < V; e++) {
            lp[e] = c.v[e];
            mn = sgm_min(mn, lp[e]);
            so.v[e] = FIRST ? lp[e] : so.v[e] + lp[e];
        }
        m = wave_min_finite(mn) + 0.0f;
        *reinterpret_cast<SgmVec<V>*>(ps) = so;
    }

    auto advance = [&](const SgmVec<V>& c, SgmVec<V> so, int s) {
        // a neighbour that does not exist reads +inf: min() then keeps the one that does, and inf + P1 never wins
        const float lo = wave_from_lower(lp[V - 1], inf), hi = wave_from_upper(lp[0], inf);
        const float mp2 = m + P2;
        float ln[V];
#pragma unroll
        for (int e = 0; e < V; e++) {
            const float a = e > 0 ? lp[e - 1] : lo, b = e < V - 1 ? lp[e + 1] : hi;
            float t = lp[e];
            t = sgm_min(t, sgm_min(a, b) + P1);
            t = sgm_min(t, mp2);
            ln[e] = c.v[e] + (t - m);                       // (a pad entry: +inf plus a finite value)
        }
        float mn = inf;
#pragma unroll
        for (int e = 0; e < V; e++) {
            mn = sgm_min(mn, ln[e]);
            lp[e] = ln[e];
            so.v[e] = FIRST ? ln[e] : so.v[e] + ln[e];
        }
        m = wave_min_finite(mn) + 0.0f;
        *reinterpret_cast<SgmVec<V>*>(ps + (ptrdiff_t)s * step) = so;
    };
    int s0 = 1;
    for (; s0 + PF <= len; s0 += PF) {                      // whole rings
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int s = s0 + u;
            SgmVec<V> so;
            if (!FIRST) so = bs[u];
            advance(bc[u], so, s);
            const ptrdiff_t o = (ptrdiff_t)(s + PF < last ? s + PF : last) * step;      // (the slot is free: its next load goes out)
            bc[u] = *reinterpret_cast<const SgmVec<V>*>(pc + o);
            if (!FIRST) bs[u] = *reinterpret_cast<const SgmVec<V>*>(ps + o);
        }
    }
#pragma unroll
    for (int u = 0; u < PF; u++)                            // the rest: everything it needs is in the ring
        if (s0 + u < len) {                                 // (wave-uniform)
            SgmVec<V> so;
            if (!FIRST) so = bs[u];
            advance(bc[u], so, s0 + u);
        }
}

// grid = ceil(ceil(P / kSgmReadoutPixels) / 4), block = kSgmThreads.  S: [P][Kp]; sum may be null
template <int V>
__global__ void __launch_bounds__(kSgmThreads)
les_sgm_readout_kernel(const float* __restrict__ S, size_t P, int K, int subpixel, float d0, float4* __restrict__ labels, float* __restrict__ sum)
{
    constexpr int Kp = 64 * V;
    constexpr int N = kSgmReadoutPixels;
    const int lane = threadIdx.x & 63;
    const size_t p0 = ((size_t)blockIdx.x * (kSgmThreads / 64) + (threadIdx.x >> 6)) * N;
    if (p0 >= P) return;                                    // (the whole wave)
    SgmVec<V> c[N];
#pragma unroll
    for (int u = 0; u < N; u++)
        if (p0 + u < P) c[u] = *reinterpret_cast<const SgmVec<V>*>(S + (p0 + u) * Kp + (size_t)lane * V);
#pragma unroll
    for (int u = 0; u < N; u++) {
        if (p0 + u >= P) break;                             // (wave-uniform)
        float best = __builtin_inff();
        int kb = K;
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int k = lane * V + e;
            if (k < K && c[u].v[e] < best) { best = c[u].v[e]; kb = k; }
        }
        const float m = wave_min_finite(best);              // (every S(p, k < K) is finite: lane 0 offers one)
        const int ks = (int)wave_min_finite(best == m ? (float)kb : (float)kSgmMaxK);
        // the costs of k* - 1, k*, k* + 1 as they lie in their owners' registers
        float got[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            int k = ks + j - 1;
            k = k < 0 ? 0 : k > K - 1 ? K - 1 : k;          // (an index outside is not used by argmin_offset)
            const int e_ = k % V;
            float v = c[u].v[0];
#pragma unroll
            for (int e = 1; e < V; e++) v = e_ == e ? c[u].v[e] : v;
            got[j] = readlane_f32(v, k / V);
        }
        const float off = argmin_offset(ks, K, subpixel, got[1], got[0], got[2]);
        if (lane == 0) {
            labels[p0 + u] = make_float4(0.0f, 0.0f, ((float)ks + off) + d0, 0.0f);
            if (sum) sum[p0 + u] = got[1];
        }
    }
}

}  // namespace les
