// les_reproject.h -- 3D reconstruction from a label map (no reference counterpart: the reference only paints the normals as a picture,
// computeNormalMap, LES/StereoEnergy.h:274-289): per pixel the point and the exact unit normal of the label's plane in the view's camera frame,
// and the triangle mesh over the pixel grid, torn where the optimiser's own pairwise term says two pixels lie on different surfaces.
//
// Calibration (f, cx, cy, doffs, baseline), a rectified pinhole pair; view m has cx_m = cx + (m ? doffs : 0).  Camera frame of the view: X right,
// Y down, Z forward (X_left = X_right + baseline).  Per pixel (x, y) with label (a, b, c, .):
//   d = (a (float)x + b (float)y) + c                      float, un-fused: pw_getz, les_disparity_kernel's order
//   everything below in double from the float inputs, in the written order, rounded to float once at the end
//   D = d + doffs
//   valid iff d is finite, D > 0, the drop mask (if any) is zero there, and Z <= z_max when z_max > 0
//   Z = (f baseline) / D        X = ((x - cx_m) Z) / f        Y = ((y - cy) Z) / f
//   n = (a f, b f, ((a cx_m + b cy) + c) + doffs)          the label's plane is exactly n . P = f baseline
//   normal = -n / sqrt((nx nx + ny ny) + nz nz)            it faces the camera
//   invalid: NaN (0x7fc00000) in both maps and 0 in the valid map; valid: 255
//
// Mesh.  Pixels p, q are connected iff both are valid and psi(p, q) = |l_p(p) - l_q(p)| + |l_p(q) - l_q(q)| <= max_jump in float: the
// un-truncated pairwise term (LES/StereoEnergy.h:238-241), taken from pw_term with unit weights and no truncation.  A NaN psi connects nothing.
// Quad (x, y), x < W - 1, y < H - 1, has corners p00, p10, p01, p11 (first index: the x offset) and yields T0 = (p00, p01, p10) and
// T1 = (p10, p01, p11); a triangle is emitted iff all three of its edges are connected (T0: p00-p01, p00-p10, p10-p01; T1: p10-p11, p01-p11,
// p10-p01).  Vertex k is the k-th valid pixel in row-major order; the triangles are in row-major quad order, T0 before T1, and carry vertex
// numbers.  The order is a function of the inputs alone.
//
// Compaction: a three-step scan, no atomics, and NO WORKGROUP EVER WAITS ON ANOTHER (no look-back, no flags, no spins): the launch boundary is the
// only ordering.  A workgroup owns a flat run of kMeshTile pixels (the quad of a pixel is the one it is the corner p00 of).
//   1. les_mesh_count_kernel      per tile: its vertices and its triangles
//   2. les_mesh_scan_kernel       ONE workgroup: the exclusive scan of the tile counts (kMeshScanW tiles per turn of its loop) and the two totals
//   3. les_mesh_vertices_kernel   recomputes the flags, ranks them inside the workgroup, writes vertex_index and vertex_pixel
//   4. les_mesh_triangles_kernel  recomputes the flags, ranks them, writes the triangles from vertex_index
// Ranking inside a workgroup: one wave ballot and popcounts per flag, one LDS exchange of the waves' totals.  Element offsets are 64-bit.
#pragma once

#include "les_pairwise.h"
#include "les_speckle.h"

namespace les {

constexpr int kRepNT = 256;                  // work-items (= pixels) of a workgroup of les_reproject_kernel
constexpr int kMeshNT = 256;                 // work-items of a workgroup of the mesh kernels
constexpr int kMeshTile = 1024;              // pixels one workgroup owns (les_hip_mesh_tile)
constexpr int kMeshScanW = 256;              // tiles per turn of the scan's loop (les_hip_mesh_tile)
constexpr int kMeshWaves = kMeshNT / 64;
static_assert(kMeshTile % kMeshNT == 0 && kMeshNT % 64 == 0, "whole waves, whole turns");

struct Calib { float f, cx, cy, doffs, baseline; };

struct RepPixel {
    float p[3], n[3];
    bool valid;
};

// The definition above for one pixel.  dropped: the caller's drop mask at the pixel.
__device__ __forceinline__ RepPixel rep_pixel(float4 l, int x, int y, const Calib& k, int mode, float z_max, bool dropped)
{
    const float qnan = __int_as_float(0x7fc00000);
    RepPixel r = {{qnan, qnan, qnan}, {qnan, qnan, qnan}, false};
    const float d = pw_getz(l, x, y);
    const double f = (double)k.f, cy = (double)k.cy, doffs = (double)k.doffs;
    const double cxm = mode ? (double)k.cx + doffs : (double)k.cx;
    const double D = (double)d + doffs;
    if (!spk_finite(d) || !(D > 0.0) || dropped) return r;
    const double Z = (f * (double)k.baseline) / D;
    if (z_max > 0.0f && !(Z <= (double)z_max)) return r;
    const double X = (((double)x - cxm) * Z) / f;
    const double Y = (((double)y - cy) * Z) / f;
    const double a = (double)l.x, b = (double)l.y, c = (double)l.z;
    const double nx = a * f, ny = b * f, nz = ((a * cxm + b * cy) + c) + doffs;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    r.p[0] = (float)X; r.p[1] = (float)Y; r.p[2] = (float)Z;
    r.n[0] = (float)(-nx / len); r.n[1] = (float)(-ny / len); r.n[2] = (float)(-nz / len);
    r.valid = true;
    return r;
}

// grid ceil(H W / kRepNT), kRepNT work-items, one pixel each: one 16-byte label load; the two H x W x 3 maps leave through LDS so that a
// workgroup stores its 3 kRepNT floats as consecutive dwords.  points / normals may be null.
__global__ void __launch_bounds__(kRepNT)
les_reproject_kernel(const float4* __restrict__ labels, const uint8_t* __restrict__ drop, Calib k, int mode, float z_max, float* __restrict__ points,
                     float* __restrict__ normals, uint8_t* __restrict__ valid, int H, int W)
{
    __shared__ float s_p[3 * kRepNT];
    __shared__ float s_n[3 * kRepNT];
    const int tid = threadIdx.x;
    const long long P = (long long)H * W, base = (long long)blockIdx.x * kRepNT, t = base + tid;
    if (t < P) {
        const int y = (int)(t / W), x = (int)(t - (long long)y * W);
        const RepPixel r = rep_pixel(labels[t], x, y, k, mode, z_max, drop != nullptr && drop[t] != 0);
        for (int j = 0; j < 3; j++) {
            s_p[3 * tid + j] = r.p[j];
            s_n[3 * tid + j] = r.n[j];
        }
        valid[t] = r.valid ? 255 : 0;
    }
    __syncthreads();
    const long long left = P - base;
    const int n3 = 3 * (int)(left < kRepNT ? left : kRepNT);
    for (int i = tid; i < n3; i += kRepNT) {
        if (points) points[3 * base + i] = s_p[i];
        if (normals) normals[3 * base + i] = s_n[i];
    }
}

// psi(p, q) <= max_jump: pw_term with coefficient 1, lambda 1 and the truncation at +inf is psi itself, bit for bit (pw_min(d, +inf) = d, NaN included)
__device__ __forceinline__ bool mesh_connected(float4 lp, int xp, int yp, float4 lq, int xq, int yq, float max_jump)
{
    const PairwiseParams untruncated = {0, 0, 1.0f, __int_as_float(0x7f800000)};
    return pw_term(1.0f, lp, lq, xp, yp, xq, yq, untruncated) <= max_jump;
}

struct MeshFlags { bool v, t0, t1; };

// Flags of pixel t (any t; beyond the image: none): v = it is a vertex, t0 / t1 = its quad emits T0 / T1
__device__ __forceinline__ MeshFlags mesh_flags(const float4* __restrict__ labels, const uint8_t* __restrict__ valid, int H, int W, long long t, float max_jump)
{
    MeshFlags f = {false, false, false};
    if (t >= (long long)H * W) return f;
    const int y = (int)(t / W), x = (int)(t - (long long)y * W);
    f.v = valid[t] != 0;
    if (x + 1 >= W || y + 1 >= H) return f;
    const bool v10 = valid[t + 1] != 0, v01 = valid[t + W] != 0, v11 = valid[t + W + 1] != 0;
    if (!v10 || !v01) return f;                                       // both triangles hold the edge p10 - p01
    const float4 l10 = labels[t + 1], l01 = labels[t + W];
    if (!mesh_connected(l10, x + 1, y, l01, x, y + 1, max_jump)) return f;
    if (f.v) {
        const float4 l00 = labels[t];
        f.t0 = mesh_connected(l00, x, y, l01, x, y + 1, max_jump) && mesh_connected(l00, x, y, l10, x + 1, y, max_jump);
    }
    if (v11) {
        const float4 l11 = labels[t + W + 1];
        f.t1 = mesh_connected(l10, x + 1, y, l11, x + 1, y + 1, max_jump) && mesh_connected(l01, x, y + 1, l11, x + 1, y + 1, max_jump);
    }
    return f;
}

// set bits of a wave ballot below this lane: the rank of the lane's flag among its wave's
__device__ __forceinline__ int mesh_rank(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// 1. grid = tiles, kMeshNT work-items.  cnt[2 tile] = vertices, cnt[2 tile + 1] = triangles of the tile.  Every work-item reaches every ballot.
__global__ void __launch_bounds__(kMeshNT)
les_mesh_count_kernel(const float4* __restrict__ labels, const uint8_t* __restrict__ valid, int H, int W, float max_jump, int* __restrict__ cnt)
{
    __shared__ int s_v[kMeshWaves];
    __shared__ int s_t[kMeshWaves];
    const int tid = threadIdx.x;
    int nv = 0, nt = 0;                                               // (the wave's sums, the same in all of its lanes)
    for (int s = 0; s < kMeshTile / kMeshNT; s++) {
        const MeshFlags f = mesh_flags(labels, valid, H, W, (long long)blockIdx.x * kMeshTile + s * kMeshNT + tid, max_jump);
        nv += __popcll(__ballot(f.v));
        nt += __popcll(__ballot(f.t0)) + __popcll(__ballot(f.t1));
    }
    if ((tid & 63) == 0) {
        s_v[tid >> 6] = nv;
        s_t[tid >> 6] = nt;
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < kMeshWaves; w++) {
            a += s_v[w];
            b += s_t[w];
        }
        cnt[2 * (size_t)blockIdx.x] = a;
        cnt[2 * (size_t)blockIdx.x + 1] = b;
    }
}

// 2. ONE workgroup of kMeshScanW work-items: off[2 i], off[2 i + 1] = vertices, triangles of the tiles before tile i; counts[0], counts[1] = the totals.
// A Hillis-Steele scan in LDS per kMeshScanW tiles, the running totals carried from turn to turn.
__global__ void __launch_bounds__(kMeshScanW)
les_mesh_scan_kernel(const int* __restrict__ cnt, long long* __restrict__ off, long long* __restrict__ counts, int ntiles)
{
    __shared__ long long s_v[kMeshScanW];
    __shared__ long long s_t[kMeshScanW];
    const int tid = threadIdx.x;
    long long carry_v = 0, carry_t = 0;
    for (int base = 0; base < ntiles; base += kMeshScanW) {
        const int i = base + tid;
        const long long cv = i < ntiles ? cnt[2 * (size_t)i] : 0, ct = i < ntiles ? cnt[2 * (size_t)i + 1] : 0;
        s_v[tid] = cv;
        s_t[tid] = ct;
        __syncthreads();
        for (int d = 1; d < kMeshScanW; d <<= 1) {
            const long long a = tid >= d ? s_v[tid - d] : 0, b = tid >= d ? s_t[tid - d] : 0;
            __syncthreads();
            s_v[tid] += a;
            s_t[tid] += b;
            __syncthreads();
        }
        if (i < ntiles) {
            off[2 * (size_t)i] = carry_v + (s_v[tid] - cv);
            off[2 * (size_t)i + 1] = carry_t + (s_t[tid] - ct);
        }
        carry_v += s_v[kMeshScanW - 1];
        carry_t += s_t[kMeshScanW - 1];
        __syncthreads();                                              // (the next turn rewrites s_v, s_t)
    }
    if (tid == 0) {
        counts[0] = carry_v;
        counts[1] = carry_t;
    }
}

// 3. grid = tiles.  vertex_index[t] = the pixel's vertex number or -1; vertex_pixel[k] = the linear pixel index of vertex k.
__global__ void __launch_bounds__(kMeshNT)
les_mesh_vertices_kernel(const uint8_t* __restrict__ valid, int H, int W, const long long* __restrict__ off, int* __restrict__ vertex_index,
                         int* __restrict__ vertex_pixel)
{
    __shared__ int s_w[kMeshWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long P = (long long)H * W;
    long long next = off[2 * (size_t)blockIdx.x];                     // the number of the first vertex of this turn
    for (int s = 0; s < kMeshTile / kMeshNT; s++) {
        const long long t = (long long)blockIdx.x * kMeshTile + s * kMeshNT + tid;
        const bool v = t < P && valid[t] != 0;
        const unsigned long long bv = __ballot(v);
        if (lane == 0) s_w[wave] = __popcll(bv);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kMeshWaves; w++) {
            if (w < wave) before += s_w[w];
            total += s_w[w];
        }
        const long long k = next + before + mesh_rank(bv, lane);
        if (t < P) vertex_index[t] = v ? (int)k : -1;
        if (v) vertex_pixel[k] = (int)t;
        next += total;
        __syncthreads();                                              // (the next turn rewrites s_w)
    }
}

// 4. grid = tiles.  triangles[3 k .. 3 k + 2] = the vertex numbers of triangle k.
__global__ void __launch_bounds__(kMeshNT)
les_mesh_triangles_kernel(const float4* __restrict__ labels, const uint8_t* __restrict__ valid, int H, int W, float max_jump,
                          const long long* __restrict__ off, const int* __restrict__ vertex_index, int* __restrict__ triangles)
{
    __shared__ int s_w[kMeshWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long next = off[2 * (size_t)blockIdx.x + 1];                 // the number of the first triangle of this turn
    for (int s = 0; s < kMeshTile / kMeshNT; s++) {
        const long long t = (long long)blockIdx.x * kMeshTile + s * kMeshNT + tid;
        const MeshFlags f = mesh_flags(labels, valid, H, W, t, max_jump);
        const unsigned long long b0 = __ballot(f.t0), b1 = __ballot(f.t1);
        if (lane == 0) s_w[wave] = __popcll(b0) + __popcll(b1);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kMeshWaves; w++) {
            if (w < wave) before += s_w[w];
            total += s_w[w];
        }
        long long k = next + before + mesh_rank(b0, lane) + mesh_rank(b1, lane);
        if (f.t0) {
            int* o = triangles + 3 * k;
            o[0] = vertex_index[t]; o[1] = vertex_index[t + W]; o[2] = vertex_index[t + 1];
            k++;
        }
        if (f.t1) {
            int* o = triangles + 3 * k;
            o[0] = vertex_index[t + 1]; o[1] = vertex_index[t + W]; o[2] = vertex_index[t + W + 1];
        }
        next += total;
        __syncthreads();                                              // (the next turn rewrites s_w)
    }
}

}  // namespace les
