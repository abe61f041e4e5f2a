// les_hip_vdisp.inc -- part of the single translation unit les_hip.hip: launches of the image-based cost with vertical disparity
// (Plane::v, csrc/les_vdisp.h).  Every path of an image-based context honours v:
//   - the march kernel and the bilateral / unfiltered kernel read raw-cost patches: les_naive_raw_v_kernel fills them;
//   - the strip kernel gathers in-kernel along one row: after it, the calls with v != 0 are recomputed on the device (launch_vdisp_strips).
// Calls with v == 0 keep their kernels and their bits.

// The raw-cost pre-pass of an image-based context into per-call patches (rp: call table, patch buffer)
void launch_naive_raw(les_hip_ctx* c, int mode, const les::RawCall* calls, int n, int chunks, const float4* d_planes, float* raw, hipStream_t stream)
{
    hipLaunchKernelGGL(les::les_naive_raw_v_kernel, dim3(n, chunks), dim3(256), 0, stream, c->geom, strip_view(c, mode), calls, d_planes, raw, 0, 0,
                       (unsigned*)nullptr);
}

// launch_march of an image-based context: the pre-pass above, then the march kernel on the patches (role A's KIND 3)
int launch_naive_march(les_hip_ctx* c, const MarchEntry* m, int mode, const les::Job* d_mjobs, int ngroups, const float4* d_planes, float* d_out, int check,
                       hipStream_t stream, const RawPatches& rp)
{
    if (ngroups <= 0) return LES_HIP_OK;
    if (!rp.raw || !c->v[1 - mode].feat) return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    launch_naive_raw(c, mode, rp.calls, rp.n, rp.chunks, d_planes, rp.raw, stream);
    les::MarchView mv = c->v[mode].mv;
    mv.vol = rp.raw; mv.raw_off = rp.off;
    hipLaunchKernelGGL(m->fn, dim3(ngroups), dim3(m->NT), 0, stream, c->geom, mv, d_mjobs, d_planes, d_out, ngroups, check);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

// The strip path's recompute of the calls with v != 0.  Their raw costs are written as slices of an H x W stand-in volume (calls whose
// filterRects do not overlap share a slice) and read back by the nearest-slice strip kernel through the stand-in plane (0, 0, slice):
// the image-based strip kernel's guided filter, fed the 2-D samples.  The calls are cut into groups of at most kVdispMaxSlices slices,
// one pass per group.
constexpr long long kVdispVolCapFloats = 1ll << 28;      // 1 GB of stand-in volume per view

struct VdispGroup { int c0, c1, slices; };
struct VdispStrip {
    std::vector<VdispGroup> groups;
    les::RawCall* d_calls = nullptr;       // per call: its filterRect at its slice (offset slice * H * W + y * W + x)
    float4* d_stand_in = nullptr;          // per call: (0, 0, slice, 0)
    int max_slices = 0;
    float* d_vol[2] = {nullptr, nullptr};  // per view, max_slices * H * W floats (allocated on the view's first recompute)
    unsigned* d_flags[2] = {nullptr, nullptr};
    les::Job* d_rjobs[2] = {nullptr, nullptr};
    int n = 0, chunks = 1;
};

void vdisp_free(VdispStrip* v)
{
    if (!v) return;
    if (v->d_calls) (void)hipFree(v->d_calls);
    if (v->d_stand_in) (void)hipFree(v->d_stand_in);
    for (int m = 0; m < 2; m++) {
        if (v->d_vol[m]) (void)hipFree(v->d_vol[m]);
        if (v->d_flags[m]) (void)hipFree(v->d_flags[m]);
        if (v->d_rjobs[m]) (void)hipFree(v->d_rjobs[m]);
    }
    delete v;
}

// The slice layout of n calls (host), uploaded once
int vdisp_build(const les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, VdispStrip** out)
{
    const long long HW = (long long)c->p.H * c->p.W;
    const int cap = (int)std::max<long long>(1, kVdispVolCapFloats / std::max<long long>(HW, 1));
    VdispStrip* v = new VdispStrip();
    v->n = n;
    std::vector<les::RawCall> calls((size_t)n);
    std::vector<float4> stand((size_t)n);
    std::vector<std::vector<les_hip_rect>> used;          // rects of each slice of the current group
    VdispGroup g{0, 0, 0};
    long long amax = 1;
    for (int i = 0; i < n; i++) {
        const les_hip_rect f = frs[i];
        const bool live = trs[i].w > 0 && trs[i].h > 0 && f.w > 0 && f.h > 0;
        int s = 0;
        if (live) {
            auto overlaps = [&](const les_hip_rect& r) { return f.x < r.x + r.w && r.x < f.x + f.w && f.y < r.y + r.h && r.y < f.y + f.h; };
            for (s = 0; s < (int)used.size(); s++) {
                bool free_ = true;
                for (const auto& r : used[s]) if (overlaps(r)) { free_ = false; break; }
                if (free_) break;
            }
            if (s == (int)used.size()) {
                if (s == cap) {                         // the group is full: start the next one at this call
                    g.c1 = i; g.slices = s; v->groups.push_back(g);
                    g = VdispGroup{i, i, 0};
                    used.clear(); s = 0;
                }
                used.emplace_back();
            }
            used[s].push_back(f);
            amax = std::max(amax, (long long)f.w * f.h);
        }
        calls[i] = les::RawCall{f.x, f.y, live ? f.w : 0, live ? f.h : 0, (long long)s * HW + (long long)f.y * c->p.W + f.x};
        stand[i] = make_float4(0.0f, 0.0f, (float)s, 0.0f);
    }
    g.c1 = n; g.slices = (int)used.size(); v->groups.push_back(g);
    for (const auto& gg : v->groups) v->max_slices = std::max(v->max_slices, gg.slices);
    v->chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
    if (n > 0) {
        if (hipMalloc((void**)&v->d_calls, (size_t)n * sizeof(les::RawCall)) != hipSuccess ||
            hipMemcpy(v->d_calls, calls.data(), (size_t)n * sizeof(les::RawCall), hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc((void**)&v->d_stand_in, (size_t)n * sizeof(float4)) != hipSuccess ||
            hipMemcpy(v->d_stand_in, stand.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess) {
            vdisp_free(v);
            return fail(LES_HIP_ERR_DEVICE, "upload of the vertical-disparity call table failed");
        }
    }
    *out = v;
    return LES_HIP_OK;
}

// After the strip kernel served the jobs d_jobs (njobs, plane_idx = call index) of an image-based context: recompute the calls with v != 0.
// Stream-ordered; the per-view buffers of v are allocated here, under the context's lock.
int launch_vdisp_strips(les_hip_ctx* c, VdispStrip* v, int mode, const les::Job* d_jobs, int njobs, const float4* d_planes, float* d_out, int check,
                        hipStream_t stream)
{
    if (njobs <= 0 || v->n <= 0 || v->max_slices <= 0) return LES_HIP_OK;
    const StripEntry* se = find_interp_strip(c->R, 0);
    if (!se || se->TW < c->strip->TW)
        return fail(LES_HIP_ERR_UNSUPPORTED, "no nearest-slice strip kernel for guided-filter radius %d (vertical disparity on the strip path)", c->R);
    const size_t HW = (size_t)c->p.H * c->p.W;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!v->d_vol[mode]) HIPCHECK(hipMalloc((void**)&v->d_vol[mode], (size_t)v->max_slices * HW * sizeof(float)));
        if (!v->d_flags[mode]) HIPCHECK(hipMalloc((void**)&v->d_flags[mode], (size_t)v->n * sizeof(unsigned)));
        if (!v->d_rjobs[mode]) HIPCHECK(hipMalloc((void**)&v->d_rjobs[mode], (size_t)njobs * sizeof(les::Job)));
    }
    les::Geom g = c->geom;
    g.D0 = 0; g.th_col = INFINITY;                  // slice k of the stand-in volume holds raw costs as they are
    les::View view = strip_view(c, mode);
    view.vol = v->d_vol[mode];
    for (const auto& gr : v->groups) {
        if (gr.c1 <= gr.c0 || gr.slices <= 0) continue;
        g.D = gr.slices;
        if (v->groups.size() > 1) HIPCHECK(hipMemsetAsync(v->d_flags[mode], 0, (size_t)v->n * sizeof(unsigned), stream));
        hipLaunchKernelGGL(les::les_naive_raw_v_kernel, dim3(gr.c1 - gr.c0, v->chunks), dim3(256), 0, stream, c->geom, strip_view(c, mode),
                           (const les::RawCall*)(v->d_calls + gr.c0), d_planes + gr.c0, v->d_vol[mode], c->p.W, 1, v->d_flags[mode] + gr.c0);
        hipLaunchKernelGGL(les::les_mask_jobs_kernel, dim3((njobs + 255) / 256), dim3(256), 0, stream, d_jobs, v->d_rjobs[mode],
                           (const unsigned*)v->d_flags[mode], njobs);
        hipLaunchKernelGGL(se->fn, dim3(njobs), dim3(se->NT), 0, stream, g, view, (const les::Job*)v->d_rjobs[mode], (const float4*)v->d_stand_in, d_out,
                           njobs, 0);
        if (check)
            hipLaunchKernelGGL(les::les_vdisp_check_kernel, dim3(njobs), dim3(256), 0, stream, c->geom, (const les::Job*)v->d_rjobs[mode], d_planes, d_out,
                               njobs);
        HIPCHECK(hipGetLastError());
    }
    return LES_HIP_OK;
}
