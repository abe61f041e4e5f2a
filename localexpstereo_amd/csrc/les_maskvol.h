// les_maskvol.h -- valid masks in the cost volumes: the nearest-valid row fill (no reference counterpart beyond fillOutOfView, LES/main.cpp:146-176,
// which it widens from "outside the image" to "outside the valid image").  A rectified view has invalid (black) pixels along its borders
// (les_rectify.h's valid bytes), a caller may have masks of their own (ego vehicle, sky, dead pixels); an entry of a view's volume that was
// matched from or against such a pixel is a cost against nothing, and fillOutOfView hands the costs of a black border column on to a whole band.
//
// THE RULE (stated here once; tests/maskvol_cases.py restates it in numpy).  One view's volume [D][H][W] of 32-bit entries: mode 0 is the left
// volume (I = L, J = R), mode 1 the right one (I = R, J = L).  validI, validJ: H x W bytes, nonzero = valid; a null pointer = all valid.  Slice k
// is disparity d = k + d0, in 64-bit arithmetic.
//   seen(x)     the reference's own test:  mode 0: x >= min(d, W - 1)      mode 1: x < max(W - d, 1)
//   partner     c = clamp(x - d, 0, W - 1) for mode 0, clamp(x + d, 0, W - 1) for mode 1
//   ok(k, y, x) = seen(x) && validI[y][x] && validJ[y][c]
//   An ok entry is never written.
//   A not-ok entry takes the 32 bits of the nearest ok entry of its own row and slice, by least |x - x'|; a tie goes right in mode 0 and left in
//   mode 1.
//   A row of a slice without an ok entry is set to `fill` (finite: the launcher refuses anything else -- a NaN would send the volume to the
//   strip kernel).
// Sources are never written, so the pass is in place, has no order and is idempotent.  With both masks null and d0 = 0 the not-ok entries are
// x < min(d, W - 1) with source min(d, W - 1) (mode 0) and x >= max(W - d, 1) with source max(W - d, 1) - 1 (mode 1): exactly the bytes of
// les_fill_out_of_view_kernel.
//
// THE KERNEL.  grid = (ceil(D / kMvDC), H), 256 work-items = 4 waves: a workgroup owns row y of a chunk of kMvDC slices.  Both mask rows are
// staged ONCE as bits (one ballot per 64 columns; the partner's row with its last bit repeated to the end of its last word).  The chunk is walked
// in rounds of four slices, one per wave.  A wave makes the ok flags of its row as ceil(W / 64) words in LDS without another ballot: word i is
//      seen_i  &  I_i  &  (64 bits of the partner's row from bit 64 i -+ d on, the row continued by its first and last bit on either side)
// -- a funnel shift of two LDS words per lane.  A wave whose words are all ones goes on without touching the volume.  Otherwise lane l takes
// the groups of four columns 4 (l + 64 t): a not-ok column finds its source by bit scans left and right over the words, loads it, and the group
// is stored with ONE 16-byte store where all four entries are written and the row is 16-byte aligned (VEC: aligned base and W % 4 == 0), with
// dword stores otherwise.  The kernel never loads an entry it does not copy: its traffic is the masks plus the entries it rewrites (the same
// source is read by many lanes: one cache line).  Entries are moved as 32-bit integers -- a NaN keeps its payload.  64-bit element offsets.
// W <= kMvMaxW (the LDS rows), H <= 65535, ceil(D / kMvDC) <= 65535: the launcher refuses more.
// Also compiled by the plain check build and by the CPU fiber simulator (test infrastructure only, LES_SIM: plain bit scans and stores there;
// the ballot is the simulator's own).  No inline assembly.
#pragma once

#include "les_simt.h"

namespace les {

constexpr int kMvNT = 256, kMvWaves = 4;
constexpr int kMvDC = 32;                   // slices of a workgroup's chunk: 8 rounds of one slice per wave
constexpr int kMvMaxW = 32768;              // widest row: 512 words per LDS row, 24 KB in all
constexpr int kMvNW = kMvMaxW / 64;

#if defined(LES_SIM)
__device__ inline int mv_lowest(unsigned long long v)            // index of the lowest set bit, v != 0
{
    int n = 0;
    while (!((v >> n) & 1ull)) n++;
    return n;
}
__device__ inline int mv_highest(unsigned long long v)           // index of the highest set bit, v != 0
{
    int n = 63;
    while (!((v >> n) & 1ull)) n--;
    return n;
}
__device__ inline void mv_store4(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
#else
__device__ __forceinline__ int mv_lowest(unsigned long long v) { return __ffsll(v) - 1; }
__device__ __forceinline__ int mv_highest(unsigned long long v) { return 63 - __clzll((long long)v); }
// ONE global_store_dwordx4
__device__ __forceinline__ void mv_store4(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = {a, b, c, d};
    *reinterpret_cast<v4u*>(p) = v;
}
#endif

// word q of the partner's row, continued to either side: by its first bit below 0, by its last bit (the top bit of the last staged word) past
// the end
__device__ __forceinline__ unsigned long long mv_partner_word(const unsigned long long* J, int nw, long long q)
{
    if (q < 0) return (J[0] & 1ull) ? ~0ull : 0ull;
    if (q >= nw) return (J[nw - 1] >> 63) ? ~0ull : 0ull;
    return J[q];
}

// ok flags of columns 64 i .. 64 i + 63 of slice d
__device__ __forceinline__ unsigned long long mv_ok_word(const unsigned long long* I, const unsigned long long* J, int nw, int W, int mode, long long d, int i)
{
    const long long x0 = 64ll * i;
    unsigned long long seen;
    if (mode == 0) {
        const long long r = (d < W - 1 ? d : (long long)(W - 1)) - x0;          // seen: x - x0 >= r
        seen = r <= 0 ? ~0ull : (r >= 64 ? 0ull : ~0ull << r);
    } else {
        const long long p = W - d, r = (p > 1 ? p : 1ll) - x0;                  // seen: x - x0 < r
        seen = r >= 64 ? ~0ull : (r <= 0 ? 0ull : (1ull << r) - 1ull);
    }
    const long long t0 = mode == 0 ? x0 - d : x0 + d;                           // partner column of bit 0, before the clamp
    const long long q = t0 >> 6;                                                // (floor: an arithmetic shift)
    const int sh = (int)(t0 & 63);
    const unsigned long long lo = mv_partner_word(J, nw, q), hi = mv_partner_word(J, nw, q + 1);
    const unsigned long long g = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return seen & I[i] & g;
}

// the source column of not-ok column x of a row that has an ok entry
__device__ __forceinline__ int mv_source(const unsigned long long* ok, int nw, int x, int mode)
{
    const int i = x >> 6, b = x & 63;
    int xr = -1, xl = -1;
    unsigned long long w = (ok[i] >> b) >> 1;                                   // the columns right of x in its word, bit 0 = x + 1
    if (w) xr = x + 1 + mv_lowest(w);
    else
        for (int j = i + 1; j < nw; j++)
            if ((w = ok[j]) != 0) { xr = 64 * j + mv_lowest(w); break; }
    w = ok[i] & ((1ull << b) - 1ull);                                           // the columns left of x in its word
    if (w) xl = 64 * i + mv_highest(w);
    else
        for (int j = i - 1; j >= 0; j--)
            if ((w = ok[j]) != 0) { xl = 64 * j + mv_highest(w); break; }
    if (xl < 0) return xr;
    if (xr < 0) return xl;
    const int dl = x - xl, dr = xr - x;
    return (dr < dl || (dr == dl && mode == 0)) ? xr : xl;
}

template <bool VEC>
__global__ void __launch_bounds__(kMvNT)
les_fill_invalid_kernel(uint32_t* __restrict__ vol, int D, int H, int W, int mode, int d0, const uint8_t* __restrict__ validI,
                        const uint8_t* __restrict__ validJ, uint32_t fill)
{
    __shared__ unsigned long long s_I[kMvNW], s_J[kMvNW], s_ok[kMvWaves][kMvNW];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y = (int)blockIdx.y, k_lo = (int)blockIdx.x * kMvDC;
    const int nw = (W + 63) >> 6;
    const size_t mrow = (size_t)y * W;

    for (int s = wave; s < nw; s += kMvWaves) {                                 // (wave-uniform: every lane reaches both ballots)
        const int x = 64 * s + lane;
        const size_t at = mrow + (size_t)(x < W ? x : W - 1);
        const bool bi = x < W && (validI == nullptr || validI[at] != 0);
        const bool bj = validJ == nullptr || validJ[at] != 0;                   // past the row's end: its last pixel
        const unsigned long long ui = __ballot(bi), uj = __ballot(bj);
        if (lane == 0) {
            s_I[s] = ui;
            s_J[s] = uj;
        }
    }
    __syncthreads();

    unsigned long long* ok = s_ok[wave];
    const unsigned long long last_full = (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
    for (int r = 0; r < kMvDC / kMvWaves; r++) {
        if (k_lo + kMvWaves * r >= D) break;                                    // (uniform over the workgroup)
        const int k = k_lo + kMvWaves * r + wave;
        const bool active = k < D;                                              // (wave-uniform)
        bool holes = false, any = false;
        if (active) {
            const long long d = (long long)k + d0;
            for (int i0 = 0; i0 < nw; i0 += 64) {
                const int i = i0 + lane;
                unsigned long long word = 0, full = 0;
                if (i < nw) {
                    word = mv_ok_word(s_I, s_J, nw, W, mode, d, i);
                    full = i == nw - 1 ? last_full : ~0ull;
                    ok[i] = word;
                }
                holes = holes | (__ballot(word != full) != 0);
                any = any | (__ballot(word != 0) != 0);
            }
        }
        __syncthreads();
        if (active && holes) {
            uint32_t* row = vol + ((size_t)k * H + y) * W;
            for (int x0 = 4 * lane; x0 < W; x0 += 4 * 64) {
                const int n = W - x0 < 4 ? W - x0 : 4;
                const unsigned nib = (unsigned)(ok[x0 >> 6] >> (x0 & 63)) & 15u;
                if (nib == (1u << n) - 1u) continue;
                uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < n && !((nib >> j) & 1u)) v[j] = any ? row[mv_source(ok, nw, x0 + j, mode)] : fill;
                if (VEC && nib == 0 && n == 4) mv_store4(row + x0, v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (j < n && !((nib >> j) & 1u)) row[x0 + j] = v[j];
                }
            }
        }
        __syncthreads();                                                        // (the words are overwritten by the next round)
    }
}

}  // namespace les
