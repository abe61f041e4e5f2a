// les_vdisp.h -- vertical disparity (Plane::v, LES/Plane.h:4-40) in the image-based matching cost (NaiveStereoEnergy,
// LES/StereoEnergy.h:704-742): the other view's feature image is sampled at (x - sign d(x, y), y + v) with the bilinear
// interpolation of cv::warpAffine (INTER_LINEAR, BORDER_REPLICATE).  Calls with v == 0 (-0.0 included: the reference only adds v
// when plane.v != 0) keep the one-row gather of les_kernels.h (naive_prepare / naive_finish) bit for bit.  CostVolumeEnergy
// ignores v (LES/CostVolumeEnergy.h:64-98): nothing here touches a cost volume.
//
// Source coordinate, defined once ([recollection] of OpenCV 3.1's warpAffine, extended from the x axis to the y axis):
//   xs = (double)X - (double)sign * (double)z,  z = (a X + b Y) + c in f32          (as naive_prepare)
//   ys = (double)((float)Y + v)                                                      (the reference's float add `y += v`)
//   each quantised to 1/32 pixel: q = floor(s * 32 + 0.5) / 32 in double; fraction f = (float)(q - floor(q)); the integer part is
//   clamped to [-2, size + 1] (NaN -> -2) and its two taps to [0, size - 1] (replicated border)
//   weights w00 = (1 - fy)(1 - fx), w01 = (1 - fy) fx, w10 = fy (1 - fx), w11 = fy fx (f32 products),
//   sample = ((t00 w00 + t01 w01) + t10 w10) + t11 w11 per channel, in f32 (compiled with -ffp-contract=off).
#pragma once

#include "les_kernels.h"

namespace les {

struct VAxis { int i0, i1; float f; };      // the two clamped taps of one axis and the weight of the second
__device__ __forceinline__ VAxis vdisp_axis(double s, int n)
{
    VAxis r;
    const double q = floor(s * 32.0 + 0.5) / 32.0;
    const double fl = floor(q);
    r.f = (float)(q - fl);
    const double flc = fmin(fmax(fl, -2.0), (double)n + 1.0);         // NaN -> -2: defined conversion, weights stay NaN
    const int k = (int)flc;
    r.i0 = min(max(k, 0), n - 1);
    r.i1 = min(max(k + 1, 0), n - 1);
    return r;
}

// Raw cost of pixel (gx, gy) of view `view` for a plane with v != 0: four feature taps over two rows
__device__ __forceinline__ float vdisp_raw(const Geom& g, const View& view, float4 plane, int gx, int gy)
{
    const float z = (plane.x * (float)gx + plane.y * (float)gy) + plane.z;
    const VAxis ax = vdisp_axis((double)gx - (double)view.sign * (double)z, g.W);
    const VAxis ay = vdisp_axis((double)((float)gy + plane.w), g.H);
    const float fx0 = 1.0f - ax.f, fy0 = 1.0f - ay.f;
    const float w00 = fy0 * fx0, w01 = fy0 * ax.f, w10 = ay.f * fx0, w11 = ay.f * ax.f;
    const uint32_t r0 = (uint32_t)ay.i0 * (uint32_t)g.W, r1 = (uint32_t)ay.i1 * (uint32_t)g.W;
    const float4 t00 = view.feat_other[r0 + (uint32_t)ax.i0], t01 = view.feat_other[r0 + (uint32_t)ax.i1];
    const float4 t10 = view.feat_other[r1 + (uint32_t)ax.i0], t11 = view.feat_other[r1 + (uint32_t)ax.i1];
    const float4 own = view.feat_self[(uint32_t)gy * (uint32_t)g.W + (uint32_t)gx];
    const float v0 = ((t00.x * w00 + t01.x * w01) + t10.x * w10) + t11.x * w11;
    const float v1 = ((t00.y * w00 + t01.y * w01) + t10.y * w10) + t11.y * w11;
    const float v2 = ((t00.z * w00 + t01.z * w01) + t10.z * w10) + t11.z * w11;
    const float v3 = ((t00.w * w00 + t01.w * w01) + t10.w * w10) + t11.w * w11;
    const float col = (fabsf(own.x - v0) + fabsf(own.y - v1)) + fabsf(own.z - v2);
    const float grad = fabsf(own.w - v3);
    return ((col < view.th_color) ? col : view.th_color) + ((grad < view.th_grad) ? grad : view.th_grad);      // std::min(th, x)
}

// The raw-cost pre-pass of the image-based energy with v (replaces les_naive_raw_kernel's launches; same grid: call x chunk).
// Call i writes its filterRect at raw + off, row y at off + y * (row_stride ? row_stride : fw).  A call with v == 0 runs
// les_naive_raw_kernel's loop body unchanged.  only_v != 0: calls with v == 0 write nothing (the strip-kernel recompute below).
// flags (may be null): flags[i] = (v != 0), written by chunk 0 -- the calls the strip path recomputes.
__global__ void les_naive_raw_v_kernel(Geom g, View view, const RawCall* __restrict__ calls, const float4* __restrict__ planes,
                                       float* __restrict__ raw, int row_stride, int only_v, unsigned* __restrict__ flags)
{
    const RawCall rc = calls[blockIdx.x];
    const float4 plane = planes[blockIdx.x];
    const bool vd = plane.w != 0.0f;
    if (flags && blockIdx.y == 0 && threadIdx.x == 0) flags[blockIdx.x] = vd ? 1u : 0u;
    if (only_v && !vd) return;
    const long long stride = row_stride ? row_stride : rc.fw;
    const long long area = (long long)rc.fw * rc.fh;
    const long long per = (area + gridDim.y - 1) / gridDim.y;
    const long long p0 = per * blockIdx.y, p1 = p0 + per < area ? p0 + per : area;
    for (long long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const int yy = (int)(p / rc.fw), xx = (int)(p - (long long)yy * rc.fw);
        const int gx = rc.fx + xx, gy = rc.fy + yy;
        float r;
        if (vd) r = vdisp_raw(g, view, plane, gx, gy);
        else {
            const NaivePrep np = naive_prepare(g, view.sign, plane.x, plane.y, plane.z, gx, gy);
            const uint32_t px = (uint32_t)gy * (uint32_t)g.W + (uint32_t)gx;
            r = naive_finish(view, np, view.feat_self[px], view.feat_other[np.ia], view.feat_other[np.ib]);
        }
        raw[rc.off + (long long)yy * stride + xx] = r;
    }
}

// Strip-kernel path (no march kernel for the call): the flagged calls' raw costs are laid out as slices of an H x W "volume" and
// re-read by the nearest-slice strip kernel through a stand-in plane (0, 0, slice) -- the same guided filter as the image-based
// strip kernel, fed the 2-D samples.  That launch runs without check; this kernel then applies the validity rule of the real
// plane (LES/StereoEnergy.h:560-610, which ignores v) over the same jobs.
__global__ void les_vdisp_check_kernel(Geom g, const Job* __restrict__ jobs, const float4* __restrict__ planes, float* __restrict__ out, int njobs)
{
    const int j = (int)blockIdx.x;
    if (j >= njobs) return;
    const Job job = jobs[j];
    if (job.tw <= 0 || job.th <= 0) return;
    const float4 pl = planes[job.plane_idx];
    for (int idx = (int)threadIdx.x; idx < job.tw * job.th; idx += (int)blockDim.x) {
        const int yy = idx / job.tw, xx = idx - yy * job.tw;
        if (!label_valid(g, pl.x, pl.y, pl.z, pl.w, job.tx0 + xx, job.ty0 + yy))
            out[job.out_off + (long long)yy * job.out_stride + xx] = LES_COST_INVALID;
    }
}

}  // namespace les
