// les_bilateral.h -- HIP kernels of the joint bilateral ("BF") and the unfiltered ("") cost aggregation (gfx950 / CDNA4, wave64).
//
// What is computed (reference: BilateralFilter::filter, LES/GuidedFilter.h:329-374, built on the sub-region I(filterRect) by
// createSubregionFilter; raw costs LES/CostVolumeEnergy.h:70-98 and LES/StereoEnergy.h:702-742):
//   raw(s)  = the truncated matching cost of the plane at pixel s of the filterRect                       (pre-pass, one patch per call)
//   q(p)    = sum over s in [p - R, p + R]^2 clipped to the filterRect of w(p, s) raw(s),                 (les_bf_kernel)
//   w(p, s) = exp(-(|dB| + |dG| + |dR|) / sig2) of the 8-bit guide colours, NOT normalised by sum w,
//   R = windR (the guided filter uses windR / 2).  q is written for the target pixels only; invalid labels get 1e6.
//   The unfiltered energy ("") is the same kernel at R = 0: q = raw exactly.
//
// |dI|_1 of two 8-bit colours is an integer in 0 .. 765, so w comes from a 766-entry table built on the host in double
// (les_hip_bilateral.inc) and held in LDS; |dI|_1 of two packed B | G << 8 | R << 16 words is one v_sad_u8.
//
// Kernel structure: a workgroup owns a tile of BF_TY x BF_TX outputs of up to NP calls that share the filterRect and the
// target rect (the planes of a slot batch or of a whole-image slab batch): w(p, s) does not depend on the plane, so every
// weight is computed once and used for NP accumulators.  A thread owns 4 horizontally adjacent outputs of one row, so
// every (guide, raw) pair it loads serves up to 4 windows.  The window rows are marched in lock-step: at step dy thread row
// ty reads halo row ty + dy, so the workgroup needs halo rows dy .. dy + BF_TY - 1 only -- a ring of BF_TY + 1 rows in LDS
// (the next row is loaded from global memory into registers before the step's arithmetic and stored after it).
// Numerics: every window row is summed in f32 (at most 2R + 1 = 63 terms), the row sums are added in f32 -- a two-level
// sum whose error stays below (2R + 1 + 2R + 1) u sum w |raw| (4.9e-6 of it at R = 20); the reference sums in double.
//
// Also compiled by the CPU fiber simulator (test infrastructure only) with LES_SIM defined: bf_sad has a portable form there.
#pragma once

#include "les_kernels.h"

namespace les {

constexpr int kBfMaxR = 31;          // largest supported radius (LDS ring width BF_TX + 2 kBfMaxR)
constexpr int kBfTabSize = 766;      // |dI|_1 = 0 .. 3 * 255
constexpr int BF_TX = 32, BF_TY = 16, BF_OX = 4;
constexpr int BF_NT = (BF_TX / BF_OX) * BF_TY;      // 128 threads
constexpr int BF_WMAX = BF_TX + 2 * kBfMaxR;        // 94 halo columns at most
constexpr int BF_NPMAX = 4;

// One tile of outputs of up to BF_NPMAX calls with the same filterRect and target rect.
struct BfJob {
    int tx0, ty0, tw, th;              // tile (image coordinates), tw <= BF_TX, th <= BF_TY
    int fx, fy, fw, fh;                // filterRect == the domain of the sub-region filter
    int np, out_stride;                // calls in the tile; floats per output row
    int call[BF_NPMAX];                // call indices: plane, raw-cost patch (RawCall table)
    long long out_off[BF_NPMAX];       // float offset of output element (ty0, tx0) of each call
};

// L1 distance of two packed 8-bit BGR words (the top byte is 0 in both): v_sad_u8
__device__ __forceinline__ uint32_t bf_sad(uint32_t a, uint32_t b)
{
#if defined(LES_SIM)
    uint32_t s = 0;
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 0xffu) - (int)((b >> k) & 0xffu);
        s += (uint32_t)(d < 0 ? -d : d);
    }
    return s;
#else
    return __builtin_amdgcn_sad_u8(a, b, 0u);
#endif
}

// Raw cost of a cost-volume context over whole filterRects (LES/CostVolumeEnergy.h:70-98, interpolate == 1): call i evaluates its
// plane on every pixel of its filterRect and stores min(C, th_col) compactly at raw + calls[i].off (the image-based energy fills the
// same patches with les_naive_raw_kernel).
__global__ void les_bf_volume_raw_kernel(Geom g, const float* __restrict__ vol, const RawCall* __restrict__ calls, const float4* __restrict__ planes,
                                         float* __restrict__ raw)
{
    const RawCall rc = calls[blockIdx.x];
    const float4 plane = planes[blockIdx.x];
    const long long area = (long long)rc.fw * rc.fh;
    const long long per = (area + gridDim.y - 1) / gridDim.y;
    const long long p0 = per * blockIdx.y, p1 = p0 + per < area ? p0 + per : area;
    for (long long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const int yy = (int)(p / rc.fw), xx = (int)(p - (long long)yy * rc.fw);
        raw[rc.off + p] = gather_cost(g, vol, plane.x, plane.y, plane.z, rc.fx + xx, rc.fy + yy);
    }
}

template <int NP>
__global__ void __launch_bounds__(BF_NT)
les_bf_kernel(Geom g, const uint32_t* __restrict__ ipk, const float* __restrict__ wtab, const BfJob* __restrict__ jobs,
              const RawCall* __restrict__ calls, const float4* __restrict__ planes, const float* __restrict__ raw,
              float* __restrict__ out, int R, int njobs, int check)
{
    __shared__ float s_tab[kBfTabSize];
    __shared__ uint32_t s_g[BF_TY + 1][BF_WMAX];        // guide ring (0 outside the filterRect)
    __shared__ float s_r[BF_TY + 1][BF_WMAX][NP];       // raw-cost ring of the NP calls (0 outside the filterRect)

    const int job_id = (int)blockIdx.x;
    if (job_id >= njobs) return;
    const BfJob job = jobs[job_id];
    const int tid = (int)threadIdx.x;
    const int WH = BF_TX + 2 * R;                       // halo columns
    for (int i = tid; i < kBfTabSize; i += BF_NT) s_tab[i] = wtab[i];

    long long roff[NP];
    int rstride[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const RawCall rc = calls[job.call[p < job.np ? p : 0]];
        roff[p] = rc.off - (long long)rc.fy * rc.fw - rc.fx;     // raw of image pixel (y, x) at roff + y * fw + x
        rstride[p] = rc.fw;
    }
    // halo loader: thread `tid` owns halo column tid of every ring row it fills
    const int lx = job.tx0 - R + tid;
    const bool lcol = tid < WH && lx >= job.fx && lx < job.fx + job.fw;
    auto load_row = [&](int r, uint32_t& gv, float (&rv)[NP]) {
        const int y = job.ty0 - R + r;
        const bool in = lcol && y >= job.fy && y < job.fy + job.fh;
        gv = in ? ipk[(size_t)y * g.W + lx] : 0u;
#pragma unroll
        for (int p = 0; p < NP; p++) rv[p] = in ? raw[roff[p] + (long long)y * rstride[p] + lx] : 0.0f;
    };
    auto store_row = [&](int r, uint32_t gv, const float (&rv)[NP]) {
        if (tid < WH) {
            const int slot = r % (BF_TY + 1);
            s_g[slot][tid] = gv;
#pragma unroll
            for (int p = 0; p < NP; p++) s_r[slot][tid][p] = rv[p];
        }
    };
    for (int r = 0; r < BF_TY; r++) {
        uint32_t gv;
        float rv[NP];
        load_row(r, gv, rv);
        store_row(r, gv, rv);
    }

    // output identity: row ty, columns 4 tq .. 4 tq + 3 of the tile
    const int ty = tid / (BF_TX / BF_OX), tq = tid - ty * (BF_TX / BF_OX);
    const int oy = job.ty0 + ty, ox0 = job.tx0 + BF_OX * tq;
    uint32_t gc[BF_OX];
#pragma unroll
    for (int o = 0; o < BF_OX; o++) {
        const int x = min(ox0 + o, job.tx0 + job.tw - 1), y = min(oy, job.ty0 + job.th - 1);
        gc[o] = ipk[(size_t)y * g.W + x];
    }
    float tot[BF_OX][NP];
#pragma unroll
    for (int o = 0; o < BF_OX; o++)
#pragma unroll
        for (int p = 0; p < NP; p++) tot[o][p] = 0.0f;
    float centre[BF_OX][NP];                            // R == 0: the raw cost itself
#pragma unroll
    for (int o = 0; o < BF_OX; o++)
#pragma unroll
        for (int p = 0; p < NP; p++) centre[o][p] = 0.0f;
    __syncthreads();

    for (int dy = 0; dy <= 2 * R; dy++) {
        // next ring row (halo row dy + BF_TY) into registers before the arithmetic of the step
        uint32_t ngv = 0;
        float nrv[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) nrv[p] = 0.0f;
        const bool more = dy + BF_TY < BF_TY + 2 * R;
        if (more) load_row(dy + BF_TY, ngv, nrv);
        const int slot = (ty + dy) % (BF_TY + 1);
        const uint32_t* grow = &s_g[slot][BF_OX * tq];
        const float (*rrow)[NP] = &s_r[slot][BF_OX * tq];
        float acc[BF_OX][NP];
#pragma unroll
        for (int o = 0; o < BF_OX; o++)
#pragma unroll
            for (int p = 0; p < NP; p++) acc[o][p] = 0.0f;
        // halo column j of this thread's row feeds output o as window column j - o (0 .. 2R)
        for (int j = 0; j < 2 * R + BF_OX; j++) {
            const uint32_t gs = grow[j];
            float rs[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) rs[p] = rrow[j][p];
#pragma unroll
            for (int o = 0; o < BF_OX; o++) {
                if (j >= o && j - o <= 2 * R) {
                    const float w = s_tab[bf_sad(gs, gc[o])];
#pragma unroll
                    for (int p = 0; p < NP; p++) acc[o][p] = fmaf(w, rs[p], acc[o][p]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < BF_OX; o++)
#pragma unroll
            for (int p = 0; p < NP; p++) tot[o][p] += acc[o][p];
        if (R == 0) {
#pragma unroll
            for (int o = 0; o < BF_OX; o++)
#pragma unroll
                for (int p = 0; p < NP; p++) centre[o][p] = rrow[o][p];
        }
        // the slot of halo row dy - 1, which no thread reads at step dy; every thread finished step dy - 1 before the barrier below
        // ended the previous iteration, and row dy + BF_TY is first read at step dy + 1, after the next barrier
        if (more) store_row(dy + BF_TY, ngv, nrv);
        __syncthreads();
    }

    if (ty >= job.th) return;
#pragma unroll
    for (int o = 0; o < BF_OX; o++) {
        const int xo = BF_OX * tq + o;
        if (xo >= job.tw) continue;
        const int x = job.tx0 + xo;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (p >= job.np) continue;
            const float4 pl = planes[job.call[p]];
            // R == 0 (the unfiltered energy): w = exp(0) = 1 and q = raw bit for bit (the sum 0 + 1 * raw would turn -0 into +0)
            float q = R == 0 ? centre[o][p] : tot[o][p];
            if (check && !label_valid(g, pl.x, pl.y, pl.z, pl.w, x, oy)) q = LES_COST_INVALID;
            out[job.out_off[p] + (long long)ty * job.out_stride + xo] = q;
        }
    }
}

}  // namespace les
