// les_eval.h -- looking at the device-resident solution on the device: the progress log of Evaluator::evaluate (LES/Evaluator.h:113-187:
// data term, smoothness term, bad-pixel rates) and the energy of the cells of a lock-step (the flow == energy self-check of
// LES/FastGCStereo.h:561-594), so that neither pulls the label and cost maps back to the host.
//
// Reference: PMStereoBase::computeCurrentEnergy (LES/PMStereoBase.h:263-270) = cv::sum(currentCost) + StereoEnergy::computeSmoothnessCost
// (LES/StereoEnergy.h:165-203: computeSmoothnessTerm over the forward pairs GE, EG, LG, GG that lie inside the image); Evaluator::quantize
// (:106-111) and the rates (:133-140).  The f32 terms are those of les_pairwise.h (pw_term with the context's coefficient table), so they are
// bit-identical to the host's (localexpstereo_amd/host/StereoEnergy.h).
//
// Summation contract: every f32 term is converted to fp64 and added in fp64, in a tree that is a function of (H, W) only -- the tile grid
// below is fixed by constants, a work-item adds its column of a tile top to bottom (per pixel: GE, EG, LG, GG), a workgroup adds its 256
// work-items in a balanced tree (the butterfly of les_simt.h's wave_sum_tree within a wave, then the four waves), the partial record of
// tile (bx, by) goes to slot by * gridDim.x + bx, and the finishing kernel (one workgroup, launched after it on the same stream: the kernel
// boundary orders the two) adds the slots in index order, a contiguous run per work-item, then a tree over the work-items.  No
// floating-point atomics, no fence, no "last block" counter.  Counts are integers.
#pragma once

#include "les_pairwise.h"

namespace les {

// a row of the device-resident log (== les_hip_eval_row of include/localexp_hip.h)
struct EvalRecord {
    int index, mode;
    double data, smooth;
    long long good_valid, good_nonocc, n_valid, n_nonocc;
};
struct EvalPartial {
    double data, smooth;
    long long good_valid, good_nonocc, n_valid, n_nonocc;
};
struct EvalParams {
    int H, W;
    float lambda, th_smooth;
    float threshold, precision;          // |d - gt| <= threshold is good; precision > 0: d quantised to multiples of it first
};

constexpr int kEvTW = 256, kEvTH = 8;                       // a workgroup's tile: one column per work-item
constexpr int kEvLW = kEvTW + 2, kEvLH = kEvTH + 1;         // ... with the halo the forward pairs reach: a column either side, a row below

// balanced tree over the 256 work-items of the workgroup, result in [0]
template <typename T>
__device__ __forceinline__ void ev_tree(T* s, int tid)
{
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) s[tid] = s[tid] + s[tid + k];
        __syncthreads();
    }
}

// grid = (ceil(W / kEvTW), ceil(H / kEvTH)); block = 256.  Labels and guide pixels of the tile and its halo come from device memory once
// (16-byte loads) and are shared through LDS: a label serves as the pixel's own and as the LG / EG / GG neighbour of three pixels of the row
// above.  Every global load of a work-item -- its share of the tile, its column of the cost / ground-truth / mask maps, the coefficient table --
// is issued before the one barrier, so a workgroup waits for memory once; 49 KB of LDS keep three workgroups on a CU.  gt / nonocc may be
// null (no ground truth: the counts are 0 / every pixel counts as non-occluded).
__global__ void __launch_bounds__(256) les_eval_kernel(const float4* __restrict__ labels, const float* __restrict__ cost, const uint32_t* __restrict__ ipk,
                                                       const float* __restrict__ wtab, const float* __restrict__ gt, const uint8_t* __restrict__ nonocc,
                                                       EvalParams p, EvalPartial* __restrict__ part)
{
    __shared__ float4 s_lab[kEvLH * kEvLW];
    __shared__ uint32_t s_ipk[kEvLH * kEvLW];
    __shared__ float s_tab[768];
    __shared__ double s_sum[2][4];
    __shared__ int s_cnt[4][4];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kEvTW, y0 = (int)blockIdx.y * kEvTH;
    const int X = x0 + tid;
    float cst[kEvTH], gtv[kEvTH];
    bool noc[kEvTH];
#pragma unroll
    for (int r = 0; r < kEvTH; r++) {
        const bool in = X < p.W && y0 + r < p.H;
        const size_t px = in ? (size_t)(y0 + r) * p.W + X : 0;
        cst[r] = in ? cost[px] : 0.0f;
        gtv[r] = (in && gt) ? gt[px] : 0.0f;
        noc[r] = (in && nonocc) ? nonocc[px] != 0 : true;
    }
#pragma unroll
    for (int j = 0; j < (kEvLH * kEvLW + 255) / 256; j++) {
        const int i = j * 256 + tid;
        const int r = i / kEvLW, c = i - r * kEvLW;
        const int Xi = x0 - 1 + c, Yi = y0 + r;
        const bool in = i < kEvLH * kEvLW && Xi >= 0 && Xi < p.W && Yi < p.H;
        const float4 l = in ? labels[(size_t)Yi * p.W + Xi] : make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t g = in ? ipk[(size_t)Yi * p.W + Xi] : 0u;
        if (i < kEvLH * kEvLW) { s_lab[i] = l; s_ipk[i] = g; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j * 256 + tid < 766) s_tab[j * 256 + tid] = wtab[j * 256 + tid];
    __syncthreads();
    const PairwiseParams pp{p.H, p.W, p.lambda, p.th_smooth};
    // forward neighbours in the order the host sums them: GE, EG, LG, GG
    const int fdx[4] = {+1, 0, -1, +1}, fdy[4] = {0, +1, +1, +1};
    double data = 0.0, smooth = 0.0;
    int gv = 0, gn = 0, nv = 0, nn = 0;
    if (X < p.W) {
#pragma unroll
        for (int r = 0; r < kEvTH; r++) {
            const int Y = y0 + r, li = r * kEvLW + tid + 1;
            if (Y >= p.H) break;
            const float4 lp = s_lab[li];
            const uint32_t ip = s_ipk[li];
            data += (double)cst[r];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xn = X + fdx[k], yn = Y + fdy[k];
                if (xn < 0 || xn >= p.W || yn >= p.H) continue;
                const int lq = li + fdy[k] * kEvLW + fdx[k];
                smooth += (double)pw_term(s_tab[pw_absdiff(ip, s_ipk[lq])], lp, s_lab[lq], X, Y, xn, yn, pp);
            }
            if (gt) {
                float d = pw_getz(lp, X, Y);
                if (p.precision > 0.0f) d = rintf(d / p.precision) * p.precision;      // Evaluator::quantize: true division, round-half-even
                const float g = gtv[r];
                const bool good = fabsf(d - g) <= p.threshold;                          // (false for NaN)
                const bool valid = g > 0.0f && g <= 3.402823466e+38f;                   // gt > 0 and finite
                nv += valid; nn += noc[r]; gv += good && valid; gn += good && noc[r];
            }
        }
    }
    // the workgroup's tree: the butterfly over the 64 lanes of each wave, then (w0 + w1) + (w2 + w3)
    data = wave_sum_tree(data); smooth = wave_sum_tree(smooth);
    gv = wave_sum_tree(gv); gn = wave_sum_tree(gn); nv = wave_sum_tree(nv); nn = wave_sum_tree(nn);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        s_sum[0][w] = data; s_sum[1][w] = smooth;
        s_cnt[0][w] = gv; s_cnt[1][w] = gn; s_cnt[2][w] = nv; s_cnt[3][w] = nn;
    }
    __syncthreads();
    if (tid == 0) {
        EvalPartial q;
        q.data = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
        q.smooth = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
        q.good_valid = (s_cnt[0][0] + s_cnt[0][1]) + (s_cnt[0][2] + s_cnt[0][3]);
        q.good_nonocc = (s_cnt[1][0] + s_cnt[1][1]) + (s_cnt[1][2] + s_cnt[1][3]);
        q.n_valid = (s_cnt[2][0] + s_cnt[2][1]) + (s_cnt[2][2] + s_cnt[2][3]);
        q.n_nonocc = (s_cnt[3][0] + s_cnt[3][1]) + (s_cnt[3][2] + s_cnt[3][3]);
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = q;
    }
}

// grid = 1, block = 256: work-item t adds the slots [t * per, (t + 1) * per) in index order, per = ceil(nslots / 256); then the tree.
__global__ void __launch_bounds__(256) les_eval_finish_kernel(const EvalPartial* __restrict__ part, int nslots, int index, int mode, EvalRecord* __restrict__ row)
{
    __shared__ double s_data[256], s_smooth[256];
    __shared__ long long s_cnt[4][256];
    const int tid = (int)threadIdx.x, per = (nslots + 255) / 256;
    double data = 0.0, smooth = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int i = tid * per; i < (tid + 1) * per && i < nslots; i++) {
        const EvalPartial q = part[i];
        data += q.data; smooth += q.smooth;
        c[0] += q.good_valid; c[1] += q.good_nonocc; c[2] += q.n_valid; c[3] += q.n_nonocc;
    }
    s_data[tid] = data; s_smooth[tid] = smooth;
    for (int j = 0; j < 4; j++) s_cnt[j][tid] = c[j];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            s_data[tid] += s_data[tid + k]; s_smooth[tid] += s_smooth[tid + k];
            for (int j = 0; j < 4; j++) s_cnt[j][tid] += s_cnt[j][tid + k];
        }
        __syncthreads();
    }
    if (tid == 0) *row = EvalRecord{index, mode, s_data[0], s_smooth[0], s_cnt[0][0], s_cnt[1][0], s_cnt[2][0], s_cnt[3][0]};
}

// ---- energy of the cells of a lock-step: fusedEnergy (localexpstereo_amd/host/ExpansionMove.h) of the CURRENT maps -- the cost of every
// pixel of the cell's region plus every forward pair term with at least one endpoint in the region and both in the image.
// A cell's pixels are those of its region grown by one (clipped to the image), row-major; chunk k of a cell is the pixels
// [k * kRegChunk, (k + 1) * kRegChunk): a work-item adds its (at most four) pixels in index order, the workgroup its work-items in the
// tree, the finishing kernel the cell's chunks in index order.  Everything is a function of the cell's rect and the maps: not of the other
// cells of the call (the grid's chunk count is the largest cell's; a cell's surplus chunks write nothing and are not read).
constexpr int kRegChunk = 1024;
struct RegionGeom { int mx, my, mw, mh; };
__device__ __forceinline__ RegionGeom region_geom(const GraphCell& c, int W, int H)
{
    RegionGeom g;
    g.mx = c.x - 1 < 0 ? 0 : c.x - 1;
    g.my = c.y - 1 < 0 ? 0 : c.y - 1;
    const int x1 = c.x + c.w + 1 > W ? W : c.x + c.w + 1, y1 = c.y + c.h + 1 > H ? H : c.y + c.h + 1;
    g.mw = (c.w > 0 && c.h > 0 && x1 > g.mx) ? x1 - g.mx : 0;
    g.mh = (c.w > 0 && c.h > 0 && y1 > g.my) ? y1 - g.my : 0;
    return g;
}

// grid = (cells, chunks); block = 256; part: cells * gridDim.y doubles
__global__ void __launch_bounds__(256) les_region_energy_kernel(const GraphCell* __restrict__ cells, const float4* __restrict__ labels, const float* __restrict__ cost,
                                                                const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, PairwiseParams p,
                                                                double* __restrict__ part)
{
    __shared__ double s_e[256];
    const GraphCell c = cells[blockIdx.x];
    const RegionGeom g = region_geom(c, p.W, p.H);
    const int N = g.mw * g.mh, tid = (int)threadIdx.x;
    if ((int)blockIdx.y * kRegChunk >= N) return;            // (uniform over the workgroup)
    const int fdx[4] = {+1, 0, -1, +1}, fdy[4] = {0, +1, +1, +1};
    double e = 0.0;
    for (int j = 0; j < kRegChunk / 256; j++) {
        const int idx = (int)blockIdx.y * kRegChunk + j * 256 + tid;
        if (idx >= N) break;
        const int yy = idx / g.mw, X = g.mx + idx - yy * g.mw, Y = g.my + yy;
        const bool in_p = X >= c.x && X < c.x + c.w && Y >= c.y && Y < c.y + c.h;
        const size_t px = (size_t)Y * p.W + X;
        if (in_p) e += (double)cost[px];
        const float4 lp = labels[px];
        for (int k = 0; k < 4; k++) {
            const int xn = X + fdx[k], yn = Y + fdy[k];
            if (xn < 0 || xn >= p.W || yn >= p.H) continue;
            const bool in_q = xn >= c.x && xn < c.x + c.w && yn >= c.y && yn < c.y + c.h;
            if (!in_p && !in_q) continue;
            e += (double)pw_term(pw_coeff(ipk, wtab, p.W, p.H, X, Y, fdx[k], fdy[k]), lp, labels[(size_t)yn * p.W + xn], X, Y, xn, yn, p);
        }
    }
    s_e[tid] = e;
    __syncthreads();
    ev_tree(s_e, tid);
    if (tid == 0) part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = s_e[0];
}

// one work-item per cell: its chunks in index order
__global__ void les_region_energy_finish_kernel(const GraphCell* __restrict__ cells, int n, int W, int H, const double* __restrict__ part, int chunks,
                                                double* __restrict__ energy)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const RegionGeom g = region_geom(cells[i], W, H);
    const int mine = (g.mw * g.mh + kRegChunk - 1) / kRegChunk;
    double e = 0.0;
    for (int k = 0; k < mine && k < chunks; k++) e += part[(size_t)i * chunks + k];
    energy[i] = e;
}

}  // namespace les
