// les_fusion.h -- fusion moves on the device: two label maps fused by graph cuts, cell by cell.  The expansion moves of les_pairwise.h try one
// plane per cell against the current labelling; a fusion move tries a whole second labelling (another seed's solution, a resumed one, a
// post-processed map), pixel by pixel.
//
// Reference: FastGCStereo::fusionMoveBK (LES/FastGCStereo.h:241-410) on StereoEnergy::computeSmoothnessTermsFusion (LES/StereoEnergy.h:331-394).
//
// DEFINITION (stated here once; tests/fusion_cases.py restates it in numpy).  Maps L0 (current) and L1 (proposal), float4 [H][W]; cur[p] the
// unary cost of L0[p], prop[p] of L1[p]; mask 255 / SOURCE = the pixel takes L1[p].
//   Pair terms of a pixel ee and its forward neighbour le (directions GE, EG, LG, GG in that order), w = pw_coeff(ee -> le),
//   T(a, b) = min(|a(ee) - b(ee)| + |a(le) - b(le)|, th_smooth) * w * lambda with the planes evaluated by pw_dot -- pw_expansion_terms' arithmetic:
//     c00 = T(L0[ee], L0[le])   c01 = T(L0[ee], L1[le])   c10 = T(L1[ee], L0[le])   c11 = T(L1[ee], L1[le])
//   Per node p, one TLink replays, in the expansion kernel's program order:
//     1. add(cur[p], prop[p])
//     2. for k = 0..7 with the neighbour pt outside the cell and inside the image:
//        add(pw_term(coeff, L0[p], L0[pt]), pw_term(coeff, L1[p], L0[pt]))                                  (LES/FastGCStereo.h:276-289)
//     3. for each forward direction d: as `j` of the preceding pixel add(c00 - c01, 0); then as `i` of its own pair
//        cap[d] = max(0, ((c10 + c01) - c11) - c00) and add(c01, c11).
//
// DEVIATION from the reference, on purpose.  The reference drops cost11 (its comment at :255), which is right only when L1 is one plane (then
// c11 = 0 and this graph is the expansion graph, bit for bit).  Here c11 enters the t-link of `i` and the arc capacity.  A pair with
// c10 + c01 < c11 + c00 is not submodular; it gets capacity 0, which represents the energy E' whose "i takes, j keeps" cost of that pair is
// raised by the deficit: E' >= E for every labelling, E' = E at "all keep" and "all take", and the cut of this graph minimises E'.  So a fusion
// move never raises the true energy, and a one-cell fusion ends at or below both inputs.  The kernel counts the truncated pairs per cell.
//
// Payload, node order and the per-chunk flow0 slots are those of les_expansion_graph_kernel: every max-flow solver takes the graphs unchanged.
#pragma once

#include "les_pairwise.h"

namespace les {

struct FuTerms { float c00, c01, c10, c11; };
// the four pair terms of pixel ee = (ex, ey) with labels (l0e, l1e) and its neighbour le = (lx, ly) with labels (l0l, l1l); w = pw_coeff(ee -> le)
__device__ __forceinline__ FuTerms fu_terms(float4 l0e, float4 l1e, float4 l0l, float4 l1l, int ex, int ey, int lx, int ly, float w, const PairwiseParams& p)
{
    const float fx = (float)ex, fy = (float)ey, gx = (float)lx, gy = (float)ly;
    const float e0_at_ee = pw_dot(l0e, fx, fy), e0_at_le = pw_dot(l0e, gx, gy), e1_at_ee = pw_dot(l1e, fx, fy), e1_at_le = pw_dot(l1e, gx, gy);
    const float n0_at_ee = pw_dot(l0l, fx, fy), n0_at_le = pw_dot(l0l, gx, gy), n1_at_ee = pw_dot(l1l, fx, fy), n1_at_le = pw_dot(l1l, gx, gy);
    FuTerms t;
    t.c00 = pw_min(fabsf(e0_at_ee - n0_at_ee) + fabsf(e0_at_le - n0_at_le), p.th_smooth) * w * p.lambda;
    t.c01 = pw_min(fabsf(e0_at_ee - n1_at_ee) + fabsf(e0_at_le - n1_at_le), p.th_smooth) * w * p.lambda;
    t.c10 = pw_min(fabsf(e1_at_ee - n0_at_ee) + fabsf(e1_at_le - n0_at_le), p.th_smooth) * w * p.lambda;
    t.c11 = pw_min(fabsf(e1_at_ee - n1_at_ee) + fabsf(e1_at_le - n1_at_le), p.th_smooth) * w * p.lambda;
    return t;
}

// grid = (cells, chunks); block = 256: one thread per node, as les_expansion_graph_kernel.  A node needs its own pair of labels and those of up
// to eight neighbours (L0 of every neighbour inside the image, L1 of those inside the cell as well): the up to 18 independent 16-byte loads are
// issued before the first term is formed and kept in registers, so each label is fetched once per node and the dependent arithmetic starts
// after one round of memory latency.  nonsub (may be null): per cell, += the pairs this block took as `i` and truncated (zeroed by the caller).
__global__ void les_fusion_graph_kernel(const GraphCell* __restrict__ cells, const long long* __restrict__ offsets, const float4* __restrict__ labels1,
                                        const float4* __restrict__ labels, const float* __restrict__ cur, const float* __restrict__ prop,
                                        const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, PairwiseParams p,
                                        float* __restrict__ payload, double* __restrict__ flow0, int* __restrict__ nonsub)
{
    const GraphCell c = cells[blockIdx.x];
    float* out = payload + 5 * offsets[blockIdx.x];
    const int N = c.w * c.h;
    // neighbour table of the reference (LES/StereoEnergy.h:99-110): LE GE EL EG LL GL LG GG
    const int nbx[8] = {-1, +1, 0, 0, -1, +1, -1, +1}, nby[8] = {0, 0, -1, +1, -1, -1, +1, +1};
    // forward directions in the order the graph is linked (GE, EG, LG, GG) as entries of that table, and the entries that point back along them
    const int kfwd[4] = {1, 3, 6, 7}, kback[4] = {0, 2, 5, 4};
    double flow_acc = 0.0;
    int truncated = 0;
    for (int idx = (int)(blockIdx.y * blockDim.x + threadIdx.x); idx < N; idx += (int)(blockDim.x * gridDim.y)) {
        const int y = idx / c.w, x = idx - y * c.w;
        const int X = c.x + x, Y = c.y + y;
        const size_t px = (size_t)Y * p.W + X;
        const float4 own0 = labels[px], own1 = labels1[px];
        float4 nb0[8], nb1[8];
        unsigned in_image = 0, in_cell = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int xt = X + nbx[k], yt = Y + nby[k];
            const bool img = xt >= 0 && xt < p.W && yt >= 0 && yt < p.H;
            const bool cell = xt >= c.x && xt < c.x + c.w && yt >= c.y && yt < c.y + c.h;      // (a cell lies inside the image)
            const size_t pt = (size_t)yt * p.W + xt;
            nb0[k] = img ? labels[pt] : make_float4(0.f, 0.f, 0.f, 0.f);
            nb1[k] = (img && cell) ? labels1[pt] : make_float4(0.f, 0.f, 0.f, 0.f);
            in_image |= (unsigned)img << k;
            in_cell |= (unsigned)(img && cell) << k;
        }
        TLink t;
        t.add(cur[px], prop[px]);                                            // LES/FastGCStereo.h:266
#pragma unroll
        for (int k = 0; k < 8; k++) {                                        // :273-290 terms towards fixed neighbours outside the region (pt keeps L0)
            if (((in_cell >> k) & 1u) || !((in_image >> k) & 1u)) continue;
            const int xt = X + nbx[k], yt = Y + nby[k];
            const float coeff = pw_coeff(ipk, wtab, p.W, p.H, X, Y, nbx[k], nby[k]);
            t.add(pw_term(coeff, own0, nb0[k], X, Y, xt, yt, p), pw_term(coeff, own1, nb0[k], X, Y, xt, yt, p));
        }
        float cap[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int kb = kback[d], kf = kfwd[d];
            // as `j` of the preceding pixel, if that pixel is in the cell (it then links in this direction)
            if ((in_cell >> kb) & 1u) {
                const int xs = X + nbx[kb], ys = Y + nby[kb];
                const float w = pw_coeff(ipk, wtab, p.W, p.H, xs, ys, nbx[kf], nby[kf]);
                const FuTerms s = fu_terms(nb0[kb], nb1[kb], own0, own1, xs, ys, X, Y, w, p);
                t.add(s.c00 - s.c01, 0.0f);                                  // add_tweights(j, D - C, 0)
            }
            // as `i`: its own pair, if the neighbour is inside the cell
            if ((in_cell >> kf) & 1u) {
                const float w = pw_coeff(ipk, wtab, p.W, p.H, X, Y, nbx[kf], nby[kf]);
                const FuTerms s = fu_terms(own0, own1, nb0[kf], nb1[kf], X, Y, X + nbx[kf], Y + nby[kf], w, p);
                const float bcd = ((s.c10 + s.c01) - s.c11) - s.c00;
                truncated += (bcd < 0.0f) ? 1 : 0;
                cap[d] = (0.0f < bcd) ? bcd : 0.0f;                          // add_edge(i, j, max(0, B + C - A - D), 0)
                t.add(s.c01, s.c11);                                         // add_tweights(i, C, A)
            }
        }
        float* o = out + 5 * (size_t)idx;
        o[0] = t.tr; o[1] = cap[0]; o[2] = cap[1]; o[3] = cap[2]; o[4] = cap[3];
        flow_acc += t.flow;
    }
    // per-cell flow already routed through the t-links, and the block's truncated pairs: one tree over both, one integer atomic per block
    __shared__ double s_red[256];
    __shared__ int s_cnt[256];
    s_red[threadIdx.x] = flow_acc;
    s_cnt[threadIdx.x] = truncated;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_red[threadIdx.x] += s_red[threadIdx.x + s];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        flow0[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = s_red[0];
        if (nonsub && s_cnt[0]) atomicAdd(&nonsub[blockIdx.x], s_cnt[0]);
    }
}

// the mask updates of a fusion move: subProposalCost.copyTo(subCurrentCost, updateMask) and the proposal map's labels copied under the same mask
// (LES/FastGCStereo.h:61-62 with a label map in the place of the one plane); masks in graph-node order.  grid = (cells, chunks)
__global__ void les_apply_masks_labels_kernel(const GraphCell* __restrict__ cells, const long long* __restrict__ offsets, const float4* labels1,
                                              const uint8_t* __restrict__ masks, float* __restrict__ cur, const float* __restrict__ prop, float4* labels, int W)
{
    const GraphCell c = cells[blockIdx.x];
    const uint8_t* m = masks + offsets[blockIdx.x];
    for (int idx = (int)(blockIdx.y * blockDim.x + threadIdx.x); idx < c.w * c.h; idx += (int)(blockDim.x * gridDim.y)) {
        if (!m[idx]) continue;
        const int y = idx / c.w, x = idx - y * c.w;
        const size_t px = (size_t)(c.y + y) * W + c.x + x;
        cur[px] = prop[px];
        labels[px] = labels1[px];
    }
}

}  // namespace les
