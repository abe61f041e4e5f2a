// les_hip_vdisp.inc -- part of the single translation unit les_hip.hip: launches of the image-based cost with vertical disparity
// (Plane::v, csrc/les_vdisp.h).  Every path of an image-based context honours v:
//   - the march kernel and the bilateral / unfiltered kernel read raw-cost patches: les_naive_raw_v_kernel fills them;
//   - the strip kernel gathers in-kernel along one row: after it, the calls with v != 0 are recomputed on the device (launch_vdisp_strips).
// Calls with v == 0 keep their kernels and their bits.  run_unary (les_hip_unary.inc) picks the path; the recompute's slice layout is part
// of the calls' UnaryTables (vdisp_layout), its stand-in volume, flags and masked jobs are workspace.

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

// The slice layout of n calls: t's groups, max_slices and chunks, and the host tables behind t.d_vd_calls / t.d_vd_stand_in
void vdisp_layout(const les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, UnaryTables& t, std::vector<les::RawCall>& calls,
                  std::vector<float4>& stand)
{
    const long long HW = (long long)c->p.H * c->p.W;
    const int cap = (int)std::max<long long>(1, kVdispVolCapFloats / std::max<long long>(HW, 1));
    calls.resize((size_t)n);
    stand.resize((size_t)n);
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
                    g.c1 = i; g.slices = s; t.vd_groups.push_back(g);
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
    g.c1 = n; g.slices = (int)used.size(); t.vd_groups.push_back(g);
    for (const auto& gg : t.vd_groups) t.vd_max_slices = std::max(t.vd_max_slices, gg.slices);
    t.vd_chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
}

// After the strip kernel served the strip jobs of t (plane_idx = call index) of an image-based context: recompute the calls with v != 0.
// Stream-ordered; vol (t.vd_max_slices * H * W floats), flags (t.n) and rjobs (t.njobs) are the caller's workspace.
int launch_vdisp_strips(les_hip_ctx* c, const UnaryTables& t, float* vol, unsigned* flags, les::Job* rjobs, int mode, const float4* d_planes,
                        float* d_out, int check, hipStream_t stream)
{
    const int njobs = t.njobs;
    if (njobs <= 0 || t.n <= 0 || t.vd_max_slices <= 0) return LES_HIP_OK;
    const StripEntry* se = find_interp_strip(c->R, 0);
    if (!se || se->TW < c->strip->TW)
        return fail(LES_HIP_ERR_UNSUPPORTED, "no nearest-slice strip kernel for guided-filter radius %d (vertical disparity on the strip path)", c->R);
    les::Geom g = c->geom;
    g.D0 = 0; g.th_col = INFINITY;                  // slice k of the stand-in volume holds raw costs as they are
    les::View view = strip_view(c, mode);
    view.vol = vol;
    const les::RawCall* vd_calls = t.d_vd_calls;      // (launches take raw pointers, not t: les_hip_mem.h)
    const les::Job* jobs = t.d_jobs;
    const float4* stand_in = t.d_vd_stand_in;
    for (const auto& gr : t.vd_groups) {
        if (gr.c1 <= gr.c0 || gr.slices <= 0) continue;
        g.D = gr.slices;
        if (t.vd_groups.size() > 1) HIPCHECK(hipMemsetAsync(flags, 0, (size_t)t.n * sizeof(unsigned), stream));
        hipLaunchKernelGGL(les::les_naive_raw_v_kernel, dim3(gr.c1 - gr.c0, t.vd_chunks), dim3(256), 0, stream, c->geom, strip_view(c, mode),
                           vd_calls + gr.c0, d_planes + gr.c0, vol, c->p.W, 1, flags + gr.c0);
        hipLaunchKernelGGL(les::les_mask_jobs_kernel, dim3((njobs + 255) / 256), dim3(256), 0, stream, jobs, rjobs, (const unsigned*)flags, njobs);
        hipLaunchKernelGGL(se->fn, dim3(njobs), dim3(se->NT), 0, stream, g, view, (const les::Job*)rjobs, stand_in, d_out, njobs, 0);
        if (check)
            hipLaunchKernelGGL(les::les_vdisp_check_kernel, dim3(njobs), dim3(256), 0, stream, c->geom, (const les::Job*)rjobs, d_planes, d_out, njobs);
        HIPCHECK(hipGetLastError());
    }
    return LES_HIP_OK;
}
