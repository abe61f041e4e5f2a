// les_costvol.h -- AD-Census matching-cost volumes built on the device from the stereo pair: the input of the cost-volume energy that the
// reference reads from an external MC-CNN run (im0.acrt / im1.acrt, LES/main.cpp:353-357).  Absolute colour difference plus the Hamming
// distance of 9 x 7 census signatures, each through 1 - exp(-c / lambda) (Mei et al., "On building an accurate stereo matching system on
// graphics hardware", 2011, without their cross-based aggregation: the guided filter is the aggregation here).
//
// DEFINITION (stated here once; tests/costvol_cases.py restates it in numpy).  Images are H x W x 3 u8 in BGR order; every index clamps to
// the image (edge replication).
//   grey       g = (77 R + 150 G + 29 B + 128) >> 8, in integers
//   signature  window 9 wide x 7 tall (dx in -4..4, dy in -3..3), neighbours visited row-major over (dy, dx), the centre skipped: bit k
//              (k = 0..61 in visiting order) of a uint64 is 1 iff g(neighbour) < g(centre); neighbour coordinates clamped to the image
//   pair       pixel (y, x) of the view I and its partner column xp of the other view J:
//                s = sum_c |I_c(y, x) - J_c(y, xp)|  in 0..765        h = popcount(sig_I(y, x) ^ sig_J(y, xp))  in 0..62
//   tables     built on the host in double, rounded once to f32 (costvol_tables of les_hip_costvol.inc):
//                ta[s] = 0.5 (1 - exp(-(s / 3) / lambda_AD)), 766 entries      tc[h] = 0.5 (1 - exp(-h / lambda_C)), 63 entries
//   cost       ta[s] + tc[h]: one f32 add, in [0, 1)
//   slices     slice k is disparity d = k + d0
//   partner    mode 0 (left view's volume):  I = L, J = R, xp = clamp(x - d, 0, W - 1)
//              mode 1 (right view's volume): I = R, J = L, xp = clamp(x + d, 0, W - 1)
// Every entry of the [D][H][W] volume follows this rule (out-of-view entries through the clamped column; nothing special for d >= W).
//
// The simulator build (LES_SIM) has no __popcll, v_sad_u8 or non-temporal store: their plain equivalents are below.
#pragma once

#include "les_simt.h"

namespace les {

constexpr int kCvTX = 256;                  // pixels of a row segment: 64 lanes x 4 consecutive pixels (one 16-byte store per lane)
constexpr int kCvDC = 64;                   // disparities of a workgroup's chunk: 4 waves x 16
constexpr int kCvSpan = kCvTX + kCvDC;      // staged partner entries (kCvTX + kCvDC - 1 are read)
constexpr int kCvNA = 766, kCvNC = 63;      // table sizes

#if defined(LES_SIM)
__device__ inline int cv_popc64(uint64_t v)
{
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}
__device__ inline uint32_t cv_sad3(uint32_t a, uint32_t b)
{
    uint32_t s = 0;
    for (int c = 0; c < 3; c++) {
        const int p = (int)((a >> (8 * c)) & 255u), q = (int)((b >> (8 * c)) & 255u);
        s += (uint32_t)(p < q ? q - p : p - q);
    }
    return s;
}
template <bool NT>
__device__ inline void cv_store4(float* p, float a, float b, float c, float d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
#else
__device__ __forceinline__ int cv_popc64(uint64_t v) { return __popcll(v); }
// sum of the absolute differences of the four bytes in one instruction (v_sad_u8); byte 3 of a packed colour is 0
__device__ __forceinline__ uint32_t cv_sad3(uint32_t a, uint32_t b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }
// ONE global_store_dwordx4 (NT: with the non-temporal hint -- the volume is written once and not read by this kernel)
template <bool NT>
__device__ __forceinline__ void cv_store4(float* p, float a, float b, float c, float d)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = {a, b, c, d};
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
    else *reinterpret_cast<v4f*>(p) = v;
}
#endif

__device__ __forceinline__ int cv_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int cv_grey(const uint8_t* __restrict__ bgr, int H, int W, int y, int x)
{
    const uint8_t* p = bgr + 3 * ((size_t)cv_clamp(y, H - 1) * W + cv_clamp(x, W - 1));
    return (77 * (int)p[2] + 150 * (int)p[1] + 29 * (int)p[0] + 128) >> 8;
}

// One signature per pixel; packed (may be null): the pixel's colour as B | G << 8 | R << 16, the operand of cv_sad3.  grid = (ceil(W / 256), H).
// Runs once per image (the volume kernel is the hot one): every neighbour's grey is recomputed from the cached image, nothing is staged.
__global__ void les_census_kernel(const uint8_t* __restrict__ bgr, unsigned long long* __restrict__ sig, uint32_t* __restrict__ packed, int H, int W)
{
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W) return;
    const int g0 = cv_grey(bgr, H, W, y, x);
    unsigned long long s = 0;
    int k = 0;
    for (int dy = -3; dy <= 3; dy++)
        for (int dx = -4; dx <= 4; dx++) {
            if (dx == 0 && dy == 0) continue;
            if (cv_grey(bgr, H, W, y + dy, x + dx) < g0) s |= 1ull << k;
            k++;
        }
    const size_t px = (size_t)y * W + x;
    sig[px] = s;
    if (packed) {
        const uint8_t* p = bgr + 3 * px;
        packed[px] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
}

// The volume.  grid = (ceil(W / kCvTX), H, ceil(D / kCvDC)), block = 256 = 4 waves.  A workgroup owns kCvTX pixels of one row and a chunk of
// kCvDC slices.  Lane l of every wave owns the four consecutive pixels x0 + 4 l + j: their signatures and packed colours are loaded once and
// stay in registers.  The chunk is walked in steps t = 0 .. nd - 1, ordered so that the partner column of a pixel moves LEFT by one per step
// in both modes (mode 0: d = d_lo + t, mode 1: d = d_hi - 1 - t): partner column = x + off - t.  The partner view's span -- columns
// cb + i, i = 0 .. kCvTX + kCvDC - 2, clamped to the row -- is staged once in LDS, so the clamp costs nothing in the loop, and so are both
// tables; the loop itself has no global loads.  Wave w takes steps 16 w .. 16 w + 15 in groups of four: over a group a lane needs seven
// consecutive partner entries for its 16 outputs, three of them carried over from the group before -- four LDS reads of a signature and a
// colour per 16 outputs, plus two table look-ups per output.  Entry i lives at [i & 3][i >> 2]: the lanes of a wave read entries 4 apart,
// which are consecutive addresses of one of the four planes (no bank conflict).
// VEC (every row start 16-byte aligned: W % 4 == 0 and an aligned base): one 16-byte store per lane and step, 1 KB contiguous per wave.
// Otherwise four dword stores with their own bounds (a row of slice k starts at (k H + y) W floats).  64-bit element offsets throughout.
template <bool VEC, bool NT>
__global__ void __launch_bounds__(256)
les_costvol_kernel(const unsigned long long* __restrict__ sigI, const uint32_t* __restrict__ colI, const unsigned long long* __restrict__ sigJ,
                   const uint32_t* __restrict__ colJ, const float* __restrict__ tab_ad, const float* __restrict__ tab_census,
                   float* __restrict__ vol, int D, int H, int W, int mode, int d0)
{
    __shared__ unsigned long long s_sig[4][kCvSpan / 4];
    __shared__ uint32_t s_col[4][kCvSpan / 4];
    __shared__ float s_ta[kCvNA];
    __shared__ float s_tc[kCvNC];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)blockIdx.x * kCvTX, y = (int)blockIdx.y, k_lo = (int)blockIdx.z * kCvDC;
    const int nd = min(kCvDC, D - k_lo);
    // partner column of pixel x at step t: x + off - t (64-bit: d0 is the caller's)
    const long long off = mode == 0 ? -((long long)d0 + k_lo) : (long long)d0 + k_lo + nd - 1;
    const long long cb = (long long)x0 + off - (kCvDC - 1);
    const size_t row = (size_t)y * W;

    for (int i = tid; i < kCvSpan; i += 256) {
        long long c = cb + i;
        c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        s_sig[i & 3][i >> 2] = sigJ[row + (size_t)c];
        s_col[i & 3][i >> 2] = colJ[row + (size_t)c];
    }
    for (int i = tid; i < kCvNA; i += 256) s_ta[i] = tab_ad[i];
    if (tid < kCvNC) s_tc[tid] = tab_census[tid];

    const int xl = x0 + 4 * lane;
    unsigned long long own_s[4];
    uint32_t own_c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const size_t px = row + (size_t)min(xl + j, W - 1);          // (lanes past the row's end compute on its last pixel and store nothing)
        own_s[j] = sigI[px];
        own_c[j] = colI[px];
    }
    __syncthreads();

    // entry of pixel j at step t = tb + u (tb a multiple of 4): i = 4 lane + j + (kCvDC - 1) - t = 4 (lane + c) + m, c = (kCvDC - 4 - tb) / 4, m = j + 3 - u
    unsigned long long ws[7];
    uint32_t wc[7];
    int c = (kCvDC - 4 - 16 * wave) / 4;
#pragma unroll
    for (int m = 4; m < 7; m++) {                                    // what a group before the first one would have left: m - 4 = 0..2 at c + 1
        ws[m] = s_sig[m & 3][lane + c + 1];
        wc[m] = s_col[m & 3][lane + c + 1];
    }
    for (int g = 0; g < 4; g++, c--) {
        const int tb = 16 * wave + 4 * g;
        if (tb >= nd) break;                                         // (wave-uniform)
#pragma unroll
        for (int m = 0; m < 4; m++) {
            ws[m] = s_sig[m][lane + c];
            wc[m] = s_col[m][lane + c];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = tb + u;
            if (t >= nd) break;
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int m = j + 3 - u;
                const uint32_t s = cv_sad3(own_c[j], wc[m]);
                const int h = cv_popc64(own_s[j] ^ ws[m]);
                o[j] = s_ta[s] + s_tc[h];
            }
            const int k = k_lo + (mode == 0 ? t : nd - 1 - t);
            float* dst = vol + ((size_t)k * H + y) * W + xl;
            if (VEC) {
                if (xl < W) cv_store4<NT>(dst, o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (xl + j < W) dst[j] = o[j];
            }
        }
#pragma unroll
        for (int m = 0; m < 3; m++) {
            ws[m + 4] = ws[m];
            wc[m + 4] = wc[m];
        }
    }
}

}  // namespace les
