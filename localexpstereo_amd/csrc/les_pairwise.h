// les_pairwise.h -- the graph of a move on the device ("next" row N1 of SURVEY.md section 8(f)): for every cell of a lock-step one kernel produces
// the ready-made capacities of the cell's graph, so the D2H payload is what the max-flow consumes and the host no longer touches labels, images or
// cost maps.  An EXPANSION move tries one plane per cell against the current labelling; a FUSION move tries a whole second labelling (another
// seed's solution, a resumed one, a post-processed map), pixel by pixel.  They are one graph: the expansion is the fusion whose second map is
// constant over the cell.
//
// Reference: StereoEnergy::initSmoothnessCoeff / computeSmoothnessTerm / computeSmoothnessTermsExpansion / ...Fusion (LES/StereoEnergy.h:131-163,
// 225-230, 398-453, 331-394) and the graph construction of FastGCStereo::expansionMoveBK / fusionMoveBK (LES/FastGCStereo.h:425-551, 241-410).
//
// DEFINITION (stated here once; tests/fusion_cases.py restates it in numpy).  Maps L0 (current) and L1 (proposal), float4 [H][W] -- for an
// expansion move L1 is the cell's plane at every pixel; cur[p] the unary cost of L0[p], prop[p] of L1[p]; mask 255 / SOURCE = the pixel takes L1[p].
//   Pair terms of a pixel ee and its forward neighbour le (directions GE, EG, LG, GG in that order), w = pw_coeff(ee -> le),
//   T(a, b) = min(|a(ee) - b(ee)| + |a(le) - b(le)|, th_smooth) * w * lambda with the planes evaluated by pw_dot (pw_pair_terms):
//     c00 = T(L0[ee], L0[le])   c01 = T(L0[ee], L1[le])   c10 = T(L1[ee], L0[le])   c11 = T(L1[ee], L1[le]) for a map, the constant 0 for one plane
//   Per node p, one TLink replays, in the reference's program order, exactly the add_tweights calls that touch the node:
//     1. add(cur[p], prop[p])
//     2. for k = 0..7 with the neighbour pt outside the cell and inside the image:
//        add(pw_term(coeff, L0[p], L0[pt]), pw_term(coeff, L1[p], L0[pt]))                                  (LES/FastGCStereo.h:276-289, 455-475)
//     3. for each forward direction d: as `j` of the preceding pixel add(c00 - c01, 0); then as `i` of its own pair
//        cap[d] = max(0, ((c10 + c01) - c11) - c00) and add(c01, c11).
//   With one plane this is the host construction (localexpstereo_amd/host/ExpansionMove.h) bit for bit.  c11 of one plane P is NOT computed:
//   T(P, P) is 0 only for a finite P (inf - inf = NaN), and the reference's expansion graph never forms it.
//
// DEVIATION from the reference, on purpose (label maps only).  The reference drops cost11 (its comment at :255), which is right only when L1 is
// one plane.  Here c11 enters the t-link of `i` and the arc capacity.  A pair with c10 + c01 < c11 + c00 is not submodular; it gets capacity 0,
// which represents the energy E' whose "i takes, j keeps" cost of that pair is raised by the deficit: E' >= E for every labelling, E' = E at
// "all keep" and "all take", and the cut of this graph minimises E'.  So a fusion move never raises the true energy, and a one-cell fusion ends
// at or below both inputs.  The kernel counts the truncated pairs per cell.
//
// Payload per node (5 floats, AoS): { tr = source - sink residual, cap E, cap S, cap SW, cap SE }; cell i starts at 5 * offset[i] floats, nodes
// row-major over the cell's region: every max-flow solver takes the graphs of both moves unchanged.  flow0 (per cell and chunk, double): the flow
// already routed source -> node -> sink by the t-links (sum over nodes, in node order within a lane's partial sums -- it is only used by the
// optional flow == energy self-check).
#pragma once

#include "les_simt.h"

namespace les {

struct PairwiseParams {
    int H, W;
    float lambda, th_smooth;
};

// smoothness coefficient of pixel (x, y) towards neighbour k: max(epsilon, exp(-|dI|_1 / omega)) via the 766-entry table
// (|dI|_1 of 8-bit colours is an integer), 0 for pairs that leave the image  (LES/StereoEnergy.h:131-163)
// |dI|_1 of two packed guide pixels: the index into the table
__device__ __forceinline__ int pw_absdiff(uint32_t a, uint32_t b)
{
    return abs((int)(a & 255) - (int)(b & 255)) + abs((int)((a >> 8) & 255) - (int)((b >> 8) & 255)) + abs((int)((a >> 16) & 255) - (int)((b >> 16) & 255));
}
__device__ __forceinline__ float pw_coeff(const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, int W, int H, int x, int y, int dx, int dy)
{
    const int xn = x + dx, yn = y + dy;
    if (xn < 0 || xn >= W || yn < 0 || yn >= H) return 0.0f;
    return wtab[pw_absdiff(ipk[(size_t)y * W + x], ipk[(size_t)yn * W + xn])];
}
// std::min(a, b) of the reference / host code: (b < a) ? b : a  -- NaN in `a` propagates, unlike fminf
__device__ __forceinline__ float pw_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float pw_getz(float4 l, int x, int y) { return (l.x * (float)x + l.y * (float)y) + l.z; }          // Plane::GetZ
__device__ __forceinline__ float pw_dot(float4 l, float x, float y) { return ((l.x * x + l.y * y) + l.z * 1.0f) + l.w * 0.0f; }   // channelDot order

// computeSmoothnessTerm (LES/StereoEnergy.h:225-230)
__device__ __forceinline__ float pw_term(float coeff, float4 ls, float4 lt, int x, int y, int xt, int yt, const PairwiseParams& p)
{
    const float d = fabsf(pw_getz(ls, x, y) - pw_getz(lt, x, y)) + fabsf(pw_getz(ls, xt, yt) - pw_getz(lt, xt, yt));
    return coeff * pw_min(d, p.th_smooth) * p.lambda;
}

struct PairTerms { float c00, c01, c10, c11; };
// the four pair terms of pixel ee = (ex, ey) with labels (l0e, l1e) and its neighbour le = (lx, ly) with labels (l0l, l1l); w = pw_coeff(ee -> le).
// kMap: L1 is a label map; otherwise one plane (l1e == l1l) and c11 is the constant 0  (LES/StereoEnergy.h:331-394, 398-453)
template <bool kMap>
__device__ __forceinline__ PairTerms pw_pair_terms(float4 l0e, float4 l1e, float4 l0l, float4 l1l, int ex, int ey, int lx, int ly, float w, const PairwiseParams& p)
{
    const float fx = (float)ex, fy = (float)ey, gx = (float)lx, gy = (float)ly;
    const float e0_at_ee = pw_dot(l0e, fx, fy), e0_at_le = pw_dot(l0e, gx, gy), e1_at_ee = pw_dot(l1e, fx, fy), e1_at_le = pw_dot(l1e, gx, gy);
    const float n0_at_ee = pw_dot(l0l, fx, fy), n0_at_le = pw_dot(l0l, gx, gy), n1_at_ee = pw_dot(l1l, fx, fy), n1_at_le = pw_dot(l1l, gx, gy);
    PairTerms t;
    t.c00 = pw_min(fabsf(e0_at_ee - n0_at_ee) + fabsf(e0_at_le - n0_at_le), p.th_smooth) * w * p.lambda;
    t.c01 = pw_min(fabsf(e0_at_ee - n1_at_ee) + fabsf(e0_at_le - n1_at_le), p.th_smooth) * w * p.lambda;
    t.c10 = pw_min(fabsf(e1_at_ee - n0_at_ee) + fabsf(e1_at_le - n0_at_le), p.th_smooth) * w * p.lambda;
    t.c11 = 0.0f;
    if constexpr (kMap) t.c11 = pw_min(fabsf(e1_at_ee - n1_at_ee) + fabsf(e1_at_le - n1_at_le), p.th_smooth) * w * p.lambda;
    return t;
}

struct TLink {
    float tr = 0.0f;
    double flow = 0.0;
    // MaxFlow add_tweights: capacities accumulate; the common part of source and sink capacity is flow
    __device__ __forceinline__ void add(float cap_source, float cap_sink)
    {
        const float delta = tr;
        if (delta > 0) cap_source += delta;
        else cap_sink -= delta;
        flow += (double)((cap_source < cap_sink) ? cap_source : cap_sink);
        tr = cap_source - cap_sink;
    }
};

struct GraphCell { int x, y, w, h; };      // a cell of a lock-step: its region of the image (the layout of les_hip_rect)

// grid = (cells, chunks); block = 256: one thread per node.  kMap: `proposal` is the label map L1 [H][W]; otherwise one plane per cell.
// A node needs its own labels and those of up to eight neighbours (L0 of every neighbour inside the image, for a map L1 of those inside the
// cell as well).  For a map the up to 18 independent 16-byte loads are issued before the first term is formed and kept in registers, so each
// label is fetched once per node and the dependent arithmetic starts after one round of memory latency (124 VGPRs, 4 waves per SIMD).  With one
// plane the neighbours' L0 are read where they are used (through L1/L2): 66 VGPRs and 7 waves per SIMD against 102 and 4 with the nine L0 labels
// preloaded, which measured a quarter slower.  nonsub (kMap only; may be null): per cell, += the pairs this block took as `i`
// and truncated (zeroed by the caller).
template <bool kMap>
__global__ void les_move_graph_kernel(const GraphCell* __restrict__ cells, const long long* __restrict__ offsets, const float4* __restrict__ proposal,
                                      const float4* __restrict__ labels, const float* __restrict__ cur, const float* __restrict__ prop,
                                      const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, PairwiseParams p,
                                      float* __restrict__ payload, double* __restrict__ flow0, int* __restrict__ nonsub)
{
    const GraphCell c = cells[blockIdx.x];
    const float4 plane = kMap ? make_float4(0.f, 0.f, 0.f, 0.f) : proposal[blockIdx.x];
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
        const float4 own0 = labels[px], own1 = kMap ? proposal[px] : plane;
        float4 nb0[8], nb1[8];                                               // (the map instance's preloaded neighbours)
        unsigned in_image = 0, in_cell = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int xt = X + nbx[k], yt = Y + nby[k];
            const bool img = xt >= 0 && xt < p.W && yt >= 0 && yt < p.H;
            const bool cell = xt >= c.x && xt < c.x + c.w && yt >= c.y && yt < c.y + c.h;      // (a cell lies inside the image)
            const size_t pt = (size_t)yt * p.W + xt;                                           // (zeros as prvalues: a named zero is selected by address and costs scratch)
            if constexpr (kMap) nb0[k] = img ? labels[pt] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (kMap) nb1[k] = (img && cell) ? proposal[pt] : make_float4(0.f, 0.f, 0.f, 0.f);
            in_image |= (unsigned)img << k;
            in_cell |= (unsigned)(img && cell) << k;
        }
        // L0 / L1 of neighbour k; asked only for neighbours inside the image / inside the cell
        auto l0 = [&](int k) { if constexpr (kMap) return nb0[k]; else return labels[(size_t)(Y + nby[k]) * p.W + (X + nbx[k])]; };
        auto l1 = [&](int k) { if constexpr (kMap) return nb1[k]; else return plane; };
        TLink t;
        t.add(cur[px], prop[px]);                                            // LES/FastGCStereo.h:266, 433
#pragma unroll
        for (int k = 0; k < 8; k++) {                                        // :273-290, 455-475 terms towards fixed neighbours outside the region (pt keeps L0)
            if (((in_cell >> k) & 1u) || !((in_image >> k) & 1u)) continue;
            const int xt = X + nbx[k], yt = Y + nby[k];
            const float coeff = pw_coeff(ipk, wtab, p.W, p.H, X, Y, nbx[k], nby[k]);
            const float4 lpt = l0(k);
            t.add(pw_term(coeff, own0, lpt, X, Y, xt, yt, p), pw_term(coeff, own1, lpt, X, Y, xt, yt, p));
        }
        float cap[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int kb = kback[d], kf = kfwd[d];
            // as `j` of the preceding pixel, if that pixel is in the cell (it then links in this direction)
            if ((in_cell >> kb) & 1u) {
                const int xs = X + nbx[kb], ys = Y + nby[kb];
                const float w = pw_coeff(ipk, wtab, p.W, p.H, xs, ys, nbx[kf], nby[kf]);
                const PairTerms s = pw_pair_terms<kMap>(l0(kb), l1(kb), own0, own1, xs, ys, X, Y, w, p);
                t.add(s.c00 - s.c01, 0.0f);                                  // add_tweights(j, D - C, 0)
            }
            // as `i`: its own pair, if the neighbour is inside the cell
            if ((in_cell >> kf) & 1u) {
                const float w = pw_coeff(ipk, wtab, p.W, p.H, X, Y, nbx[kf], nby[kf]);
                const PairTerms s = pw_pair_terms<kMap>(own0, own1, l0(kf), l1(kf), X, Y, X + nbx[kf], Y + nby[kf], w, p);
                const float bcd = ((s.c10 + s.c01) - s.c11) - s.c00;
                if constexpr (kMap) truncated += (bcd < 0.0f) ? 1 : 0;
                cap[d] = (0.0f < bcd) ? bcd : 0.0f;                          // add_edge(i, j, max(0, B + C - A - D), 0)
                t.add(s.c01, s.c11);                                         // add_tweights(i, C, A)
            }
        }
        float* o = out + 5 * (size_t)idx;
        o[0] = t.tr; o[1] = cap[0]; o[2] = cap[1]; o[3] = cap[2]; o[4] = cap[3];
        flow_acc += t.flow;
    }
    // per-cell flow already routed through the t-links and, for a map, the block's truncated pairs: one tree over both, one integer atomic per block
    __shared__ double s_red[256];
    __shared__ int s_cnt[256];                                               // (referenced, so allocated, only for a map)
    s_red[threadIdx.x] = flow_acc;
    if constexpr (kMap) s_cnt[threadIdx.x] = truncated;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_red[threadIdx.x] += s_red[threadIdx.x + s];
            if constexpr (kMap) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        flow0[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = s_red[0];
        if constexpr (kMap)
            if (nonsub && s_cnt[0]) atomicAdd(&nonsub[blockIdx.x], s_cnt[0]);
    }
}

// The mask updates of a lock-step: subProposalCost.copyTo(subCurrentCost, updateMask) and the proposal's label -- the cell's plane, or for kMap the
// map's label at the pixel -- written under the same mask  (LES/FastGCStereo.h:61-62); masks in graph-node order (cell i at offsets[i], row-major
// over its region).  grid = (cells, chunks)
template <bool kMap>
__global__ void les_apply_masks_kernel(const GraphCell* __restrict__ cells, const long long* __restrict__ offsets, const float4* proposal,
                                       const uint8_t* __restrict__ masks, float* __restrict__ cur, const float* __restrict__ prop, float4* labels, int W)
{
    const GraphCell c = cells[blockIdx.x];
    const float4 plane = kMap ? make_float4(0.f, 0.f, 0.f, 0.f) : proposal[blockIdx.x];
    const uint8_t* m = masks + offsets[blockIdx.x];
    for (int idx = (int)(blockIdx.y * blockDim.x + threadIdx.x); idx < c.w * c.h; idx += (int)(blockDim.x * gridDim.y)) {
        if (!m[idx]) continue;
        const int y = idx / c.w, x = idx - y * c.w;
        const size_t px = (size_t)(c.y + y) * W + c.x + x;
        cur[px] = prop[px];
        labels[px] = kMap ? proposal[px] : plane;
    }
}

}  // namespace les
