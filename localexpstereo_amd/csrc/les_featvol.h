// les_featvol.h -- correlation matching-cost volumes from per-pixel feature maps, on the matrix cores, and the ZNCC patch descriptor as a
// built-in feature map.  The route from any feature extractor (MC-CNN-fast and its successors, or a hand-made descriptor) to the optimiser:
// the cost of a pixel at disparity d is the correlation of its feature vector with the partner pixel's.
//
// DEFINITION (stated here once; tests/featvol_cases.py restates it in numpy).
// Feature maps are [C][H][W] float32, contiguous.  View I, partner view J, as in les_costvol.h:
//   partner    mode 0 (left view's volume):  I = L, J = R, xp = clamp(x - d, 0, W - 1)
//              mode 1 (right view's volume): I = R, J = L, xp = clamp(x + d, 0, W - 1)
//   slices     slice k is disparity d = k + d0
//   s          an f32 fma chain over c = 0 .. C - 1 in ascending order, starting from +0:  s <- fmaf(fI[c][y][x], fJ[c][y][xp], s)
//   cost       fmaf(-alpha, s, beta): one f32 fma.  alpha = beta = 0.5 maps unit-norm features to [0, 1]; alpha = 1, beta = 0 is the raw -dot
// Every entry of the [D][H][W] volume follows this rule (out-of-view entries through the clamped column; nothing special for d >= W).
//
// PATCH DESCRIPTOR (the ZNCC feature map; exact).  g: the grey of les_costvol.h; a window of radii ry, rx in 0 .. kFvMaxRadius has
// N = (2 ry + 1)(2 rx + 1) taps, visited row-major over (dy, dx), coordinates clamped to the image; channel c is tap c:
//   S = sum g      Q = sum g^2      V = N Q - S^2   (integers, V >= 0)
//   f_c = (float)((double)(N g_c - S) / sqrt((double)(N V)))   if V > 0,      f_c = 0   if V = 0 (a flat patch: the zero vector, cost beta)
// Numerator and N V are exact integers below 2^53, the double sqrt and division are IEEE (no fast-math, -ffp-contract=off), the cast rounds
// once: the map is a function of the image alone.  sum_c f_c^2 = 1 up to that rounding, so the correlation of two descriptors is the ZNCC
// of the two patches.
//
// NUMERICS OF THE VOLUME.  v_mfma_f32_32x32x2_f32 accumulates k = 0 then k = 1 into its C operand with one f32 rounding per product, no
// wider accumulation: over consecutive instructions that is the ascending fmaf chain of the definition.  C is padded to the instruction's
// K = 2 with one zero channel, which is exact: fmaf(0, 0, s) = s, and s is never -0 (the chain starts from +0, and a sum that cancels
// rounds to +0).  For any summation order  |cost - (beta - alpha s_exact)| <= alpha gamma_(C+1) sum_c |fI_c fJ_c| + 2^-24 |cost_exact|,
// gamma_n = n 2^-24 / (1 - n 2^-24); DESIGN 3.2k records how the MI355X's bytes compare with the chain's.
//
// The simulator build (LES_SIM) has no MFMA: fv_mac2 has a plain body that runs the same chain per accumulator element.  Everything around
// it (staging, skew, stores) is the same source.
#pragma once

#include "les_costvol.h"

namespace les {

constexpr int kFvSeg = 128;                       // pixels of a row segment: 4 waves x one 32-pixel tile
constexpr int kFvChunk = 64;                      // slices of a workgroup's chunk
constexpr int kFvKC = 32;                         // channels staged per pass
constexpr int kFvTiles = kFvChunk / 32 + 1;       // partner tiles per pixel tile: a band of kFvChunk diagonals crosses kFvChunk + 31 columns
constexpr int kFvSpan = kFvSeg + kFvChunk;        // staged partner columns (kFvSeg + kFvChunk - 1 carry a diagonal of the band)
constexpr int kFvMaxC = 512;                      // channels of a feature map (les_hip_build_feature_volume refuses more)
constexpr int kFvMaxRadius = 4;                   // patch radii: at most 9 x 9 = 81 channels
constexpr int kFvCG = kFvKC / 4;                  // staging: an item is one column and kFvCG consecutive channels; 4 items cover a column's pass
constexpr int kFvOwnItems = kFvSeg * 4 / 256;     // items per thread: the segment's own columns ...
constexpr int kFvParItems = kFvSpan * 4 / 256;    // ... and the partner span's
static_assert(kFvSeg * 4 % 256 == 0 && kFvSpan * 4 % 256 == 0 && kFvKC % 8 == 0, "256 threads cover the staged columns exactly");
static_assert(kFvKC * (kFvSeg + kFvSpan) >= kFvChunk * kFvSeg, "the skew image reuses the staging memory");

// the accumulator tile of one 32 x 32 product: element e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int fv_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

#if defined(LES_SIM)
struct fv_acc {
    float v[16];
    __device__ float& operator[](int i) { return v[i]; }
};
// acc[t][row][col] <- fmaf(A[c + 1][row], B[c + 1][col], fmaf(A[c][row], B[c][col], acc)) for the kFvTiles tiles whose A rows start at
// pa + 32 t: pa / pb point at channel c of the staged partner / own rows (channel strides lda / ldb)
__device__ inline void fv_mac2(fv_acc (&acc)[kFvTiles], const float* pa, int lda, const float* pb, int ldb, int lane)
{
    const int col = lane & 31;
    for (int t = 0; t < kFvTiles; t++)
        for (int e = 0; e < 16; e++) {
            const int row = 32 * t + fv_row(e, lane);
            acc[t][e] = fmaf(pa[lda + row], pb[ldb + col], fmaf(pa[row], pb[col], acc[t][e]));
        }
}
__device__ inline float4 fv_load4(const float* p) { return float4{p[0], p[1], p[2], p[3]}; }
#else
typedef float fv_acc __attribute__((ext_vector_type(16)));
// the same in kFvTiles v_mfma_f32_32x32x2_f32: lane l supplies A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]
__device__ __forceinline__ void fv_mac2(fv_acc (&acc)[kFvTiles], const float* pa, int lda, const float* pb, int ldb, int lane)
{
    const int i = lane & 31, k = lane >> 5;
    const float b = pb[k * ldb + i];
#pragma unroll
    for (int t = 0; t < kFvTiles; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k * lda + 32 * t + i], b, acc[t], 0, 0, 0);
}
__device__ __forceinline__ float4 fv_load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
#endif

// The descriptor.  One thread per pixel, grid = (ceil(W / 256), H): runs once per image, every tap's grey is recomputed from the cached image.
__global__ void les_patch_features_kernel(const uint8_t* __restrict__ bgr, float* __restrict__ feat, int H, int W, int ry, int rx)
{
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W) return;
    const long long N = (long long)(2 * ry + 1) * (2 * rx + 1);
    long long S = 0, Q = 0;
    for (int dy = -ry; dy <= ry; dy++)
        for (int dx = -rx; dx <= rx; dx++) {
            const long long g = cv_grey(bgr, H, W, y + dy, x + dx);
            S += g;
            Q += g * g;
        }
    const long long V = N * Q - S * S;
    const double den = sqrt((double)(N * V));
    const size_t P = (size_t)H * W;
    float* out = feat + (size_t)y * W + x;
    for (int dy = -ry; dy <= ry; dy++)
        for (int dx = -rx; dx <= rx; dx++, out += P) {
            const long long g = cv_grey(bgr, H, W, y + dy, x + dx);
            *out = V > 0 ? (float)((double)(N * g - S) / den) : 0.0f;
        }
}

// The volume.  grid = (segments x chunks, H) with the chunk running fastest (the chunks of one segment read the same feature columns at the
// same time), block = 256 = 4 waves.  A workgroup owns kFvSeg pixels x0 .. of row y and the slices k_lo .. k_lo + nd - 1 (nd <= kFvChunk).
//
// Staging, per pass of kFvKC channels: the segment's own features s_own[c][i] = fI[c][y][x0 + i] and the partner span s_par[c][i] =
// fJ[c][y][clamp(cb + i)], i = 0 .. kFvSpan - 1 -- clamped here, so the product loop has no clamp; channels past C read as zero (the K
// padding).  cb is chosen so that pixel x0 + xl at local slice dl reads staged column
//      mode 0:  i = xl - dl + kFvChunk - 1            mode 1:  i = xl + dl
// Product: wave w owns the pixel tile xl = 32 w .. 32 w + 31 as the B operand (columns of the accumulator, one pixel per lane) and the
// kFvTiles partner tiles i = 32 w + 32 t .. + 31 as the A operand (rows, in the registers): G_t[r][l] = sum_c s_par[c][32 w + 32 t + r]
// s_own[c][32 w + l].  kFvTiles x 16 accumulator registers; per channel pair one LDS read of the own operand, kFvTiles of the partner's.
// A slice is a DIAGONAL of these tiles (dl = l - r - 32 t + kFvChunk - 1, resp. r + 32 t - l), so one register across the lanes spans 32
// slices, H W floats apart.  Skew: every lane writes fmaf(-alpha, G, beta) of its in-band elements to the LDS image s_out[dl][xl] (which
// reuses the staging memory) -- lane stride kFvSeg + 1 resp. 1 - kFvSeg dwords, both odd: no bank conflict -- and the image is read back
// by rows: 16 bytes per lane, a wave stores two 512-byte runs of consecutive pixels of two slices.  Band efficiency: kFvChunk /
// (32 kFvTiles) = 2 / 3 of the issued MFMAs land in the band.
// VEC (W % 4 == 0 and a 16-byte aligned base): one non-temporal 16-byte store per lane; otherwise four dword stores with their own bounds.
// 64-bit element offsets throughout.
template <bool VEC>
__global__ void __launch_bounds__(256)
les_featvol_kernel(const float* __restrict__ fI, const float* __restrict__ fJ, float* __restrict__ vol, int C, int D, int H, int W, int mode, int d0,
                   float alpha, float beta, int nchunk)
{
    __shared__ __attribute__((aligned(16))) float s_mem[kFvKC * (kFvSeg + kFvSpan)];
    float* const s_own = s_mem;                          // [kFvKC][kFvSeg]
    float* const s_par = s_mem + kFvKC * kFvSeg;         // [kFvKC][kFvSpan]
    float* const s_out = s_mem;                          // [kFvChunk][kFvSeg], after the last product

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)(blockIdx.x / (unsigned)nchunk) * kFvSeg, k_lo = (int)(blockIdx.x % (unsigned)nchunk) * kFvChunk, y = (int)blockIdx.y;
    const int nd = min(kFvChunk, D - k_lo);
    const long long cb = mode == 0 ? (long long)x0 - ((long long)d0 + k_lo + kFvChunk - 1) : (long long)x0 + d0 + k_lo;      // (64-bit: d0 is the caller's)
    const size_t P = (size_t)H * W, row = (size_t)y * W;

    // this thread's staging items: one column of s_own (kFvOwnItems of them) or of s_par (kFvParItems) and kFvCG consecutive channels of the pass
    size_t src_own[kFvOwnItems], src_par[kFvParItems];   // element offset of the column in channel 0
    int dst_own[kFvOwnItems], dst_par[kFvParItems];      // ... and in LDS, at the item's first channel
    int ch_own[kFvOwnItems], ch_par[kFvParItems];        // the item's first channel
#pragma unroll
    for (int j = 0; j < kFvOwnItems; j++) {
        const int item = tid + 256 * j, col = item % kFvSeg;
        ch_own[j] = (item / kFvSeg) * kFvCG;
        src_own[j] = row + (size_t)min(x0 + col, W - 1);             // (columns past the row's end compute on its last pixel and are not stored)
        dst_own[j] = ch_own[j] * kFvSeg + col;
    }
#pragma unroll
    for (int j = 0; j < kFvParItems; j++) {
        const int item = tid + 256 * j, col = item % kFvSpan;
        ch_par[j] = (item / kFvSpan) * kFvCG;
        long long c = cb + col;
        c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        src_par[j] = row + (size_t)c;
        dst_par[j] = ch_par[j] * kFvSpan + col;
    }
    // a pass's operands travel through registers: fetch() issues every load of a pass back to back (unconditional: channels past C re-read
    // channel C - 1 and are zeroed in stash()), and the loads of pass n + 1 are in flight while the matrix cores work on pass n
    float pre_own[kFvOwnItems][kFvCG], pre_par[kFvParItems][kFvCG];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int j = 0; j < kFvOwnItems; j++)
#pragma unroll
            for (int u = 0; u < kFvCG; u++) pre_own[j][u] = fI[src_own[j] + (size_t)min(c0 + ch_own[j] + u, C - 1) * P];
#pragma unroll
        for (int j = 0; j < kFvParItems; j++)
#pragma unroll
            for (int u = 0; u < kFvCG; u++) pre_par[j][u] = fJ[src_par[j] + (size_t)min(c0 + ch_par[j] + u, C - 1) * P];
    };
    auto stash = [&](int c0) {
#pragma unroll
        for (int j = 0; j < kFvOwnItems; j++)
#pragma unroll
            for (int u = 0; u < kFvCG; u++) s_own[dst_own[j] + u * kFvSeg] = c0 + ch_own[j] + u < C ? pre_own[j][u] : 0.0f;
#pragma unroll
        for (int j = 0; j < kFvParItems; j++)
#pragma unroll
            for (int u = 0; u < kFvCG; u++) s_par[dst_par[j] + u * kFvSpan] = c0 + ch_par[j] + u < C ? pre_par[j][u] : 0.0f;
    };

    fv_acc acc[kFvTiles];
#pragma unroll
    for (int t = 0; t < kFvTiles; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][e] = 0.0f;

    fetch(0);
    for (int c0 = 0; c0 < C; c0 += kFvKC) {
        const int nk2 = (min(kFvKC, C - c0) + 1) & ~1;
        if (c0) __syncthreads();                         // the pass before has been consumed
        stash(c0);
        __syncthreads();
        if (c0 + kFvKC < C) fetch(c0 + kFvKC);
        for (int c = 0; c < nk2; c += 2) fv_mac2(acc, s_par + c * kFvSpan + 32 * wave, kFvSpan, s_own + c * kFvSeg + 32 * wave, kFvSeg, lane);
    }
    __syncthreads();                                     // s_out overwrites the operands

    const int l = lane & 31, xl = 32 * wave + l;
#pragma unroll
    for (int t = 0; t < kFvTiles; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int r = 32 * t + fv_row(e, lane);
            const int dl = mode == 0 ? l - r + kFvChunk - 1 : r - l;
            if (dl >= 0 && dl < nd) s_out[dl * kFvSeg + xl] = fmaf(-alpha, acc[t][e], beta);
        }
    __syncthreads();

    const int q = tid & 31, x = x0 + 4 * q;
    for (int dl = tid >> 5; dl < nd; dl += 8) {
        const float4 v = fv_load4(s_out + dl * kFvSeg + 4 * q);
        float* p = vol + ((size_t)(k_lo + dl) * H + y) * W + x;
        if (VEC) {
            if (x < W) cv_store4<true>(p, v.x, v.y, v.z, v.w);
        } else {
            if (x < W) p[0] = v.x;
            if (x + 1 < W) p[1] = v.y;
            if (x + 2 < W) p[2] = v.z;
            if (x + 3 < W) p[3] = v.w;
        }
    }
}

}  // namespace les
