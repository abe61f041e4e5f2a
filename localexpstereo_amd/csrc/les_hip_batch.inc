// les_hip_batch.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): prepared batches -- creation, proposals, winner-take-all, unary-cost launches -- and the per-call operator with its scratch
extern "C" {

int les_hip_batch_create(les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, int out_slabs, les_hip_batch** out)
{
    if (!c || !out || n < 0 || (n > 0 && (!frs || !trs))) return fail(LES_HIP_ERR_ARG, "null argument");
    if (out_slabs < 0) return fail(LES_HIP_ERR_ARG, "out_slabs must be 0 (one map) or the number of consecutive calls that share a slab");
    // (since round 4 out_slabs = k means "call i writes slab i / k"; before, any non-zero value meant k = 1.  A caller that still passes another
    // non-zero constant for "one slab per call" would get overlapping writes: only a k that divides n is a well-formed request)
    if (out_slabs > 1 && n % out_slabs != 0) return fail(LES_HIP_ERR_ARG, "out_slabs = %d does not divide the %d calls of the batch (slab i / out_slabs holds out_slabs consecutive calls; pass 1 for one slab per call)", out_slabs, n);
    *out = nullptr;
    std::vector<les::Job> jobs;
    int rc = LES_HIP_OK;
    if (c->filter == LES_HIP_FILTER_GF) rc = build_jobs(c, n, frs, trs, out_slabs, jobs);
    else for (int i = 0; i < n && !rc; i++) rc = check_rects(c, frs[i], trs[i]);      // (the bilateral / unfiltered tiles are cut below)
    if (rc) return rc;
    les_hip_batch* b = new les_hip_batch();
    b->n = n; b->njobs = (int)jobs.size(); b->out_slabs = out_slabs; b->R = c->R; b->device = c->p.device;
    b->targets.assign(trs, trs + n);
    if (c->filter == LES_HIP_FILTER_GF) b->filters.assign(frs, frs + n);     // (the raw-cost patch table of interpolation 0 / 2; the vertical-disparity recompute)
    {
        int max_area = 1;
        for (int i = 0; i < n; i++) max_area = std::max(max_area, trs[i].w * trs[i].h);
        b->wta_chunks = std::min(32, std::max(1, (max_area + 4095) / 4096));
        b->graph_chunks = std::min(256, std::max(1, (max_area + 255) / 256));
    }
    b->graph_off.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        b->graph_off[i] = b->graph_nodes;
        b->graph_nodes += (long long)std::max(0, trs[i].w) * std::max(0, trs[i].h);
    }
    if (n > 0) {
        static_assert(sizeof(les::WtaJob) == sizeof(les_hip_rect), "rect layout");
        static_assert(sizeof(les::GraphCell) == sizeof(les_hip_rect), "rect layout");
        if (hipMalloc((void**)&b->d_graph_off, (size_t)n * sizeof(long long)) != hipSuccess ||
            hipMemcpy(b->d_graph_off, b->graph_off.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc((void**)&b->d_flow0, (size_t)n * b->graph_chunks * sizeof(double)) != hipSuccess) {
            les_hip_batch_destroy(b);
            return fail(LES_HIP_ERR_DEVICE, "upload of the graph offset table failed");
        }
        if (hipMalloc((void**)&b->d_targets, (size_t)n * sizeof(les::WtaJob)) != hipSuccess ||
            hipMemcpy(b->d_targets, trs, (size_t)n * sizeof(les::WtaJob), hipMemcpyHostToDevice) != hipSuccess) {
            les_hip_batch_destroy(b);
            return fail(LES_HIP_ERR_DEVICE, "upload of the target table failed");
        }
    }
    {
        std::vector<les::Job> mjobs;
        bool mok = false;
        build_march_jobs(c, n, frs, trs, out_slabs, mjobs, mok, b->mentry);
        if (mok && !mjobs.empty()) {
            if (hipMalloc((void**)&b->d_mjobs, mjobs.size() * sizeof(les::Job)) != hipSuccess ||
                hipMemcpy(b->d_mjobs, mjobs.data(), mjobs.size() * sizeof(les::Job), hipMemcpyHostToDevice) != hipSuccess) {
                les_hip_batch_destroy(b);
                return fail(LES_HIP_ERR_DEVICE, "upload of the march job table failed");
            }
            b->nmgroups = (int)(mjobs.size() / b->mentry->NJ);
            b->march_ok = true;
        }
        if (b->march_ok && c->naive) {
            // raw-cost patches: one per call, the size of its filterRect.  Batches whose patches would not fit the cap stay on the strip kernel.
            std::vector<les::RawCall> calls((size_t)n);
            std::vector<long long> offs((size_t)n);
            long long tot = 0, amax = 1;
            for (int i = 0; i < n; i++) {
                const bool live = trs[i].w > 0 && trs[i].h > 0;
                const long long a = live ? (long long)frs[i].w * frs[i].h : 0;
                calls[i] = les::RawCall{frs[i].x, frs[i].y, live ? frs[i].w : 0, live ? frs[i].h : 0, tot};
                offs[i] = tot;
                tot += a; amax = std::max(amax, a);
            }
            if (tot > kRawPatchCapFloats) {
                b->march_ok = false;
                note_fallback(c->fallback_seen, FB_PATCHES, "the raw-cost patches of one batch of the image-based energy exceed 4 GB");
            }
            else {
                b->raw_floats = tot;
                b->raw_chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
                if (hipMalloc((void**)&b->d_rawcalls, (size_t)n * sizeof(les::RawCall)) != hipSuccess ||
                    hipMemcpy(b->d_rawcalls, calls.data(), (size_t)n * sizeof(les::RawCall), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMalloc((void**)&b->d_raw_off, (size_t)n * sizeof(long long)) != hipSuccess ||
                    hipMemcpy(b->d_raw_off, offs.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess) {
                    les_hip_batch_destroy(b);
                    return fail(LES_HIP_ERR_DEVICE, "upload of the raw-cost call table failed");
                }
            }
        }
    }
    if (c->filter != LES_HIP_FILTER_GF) {
        rc = build_bf_batch(c, b, n, frs, trs, out_slabs);
        if (rc) { les_hip_batch_destroy(b); return rc; }
    }
    if (!jobs.empty()) {
        if (hipMalloc((void**)&b->d_jobs, jobs.size() * sizeof(les::Job)) != hipSuccess) { les_hip_batch_destroy(b); return fail(LES_HIP_ERR_DEVICE, "hipMalloc(jobs) failed"); }
        if (hipMemcpy(b->d_jobs, jobs.data(), jobs.size() * sizeof(les::Job), hipMemcpyHostToDevice) != hipSuccess) {
            les_hip_batch_destroy(b); return fail(LES_HIP_ERR_DEVICE, "hipMemcpy(jobs) failed");
        }
    }
    *out = b;
    return LES_HIP_OK;
}

void les_hip_batch_destroy(les_hip_batch* b)
{
    if (!b) return;
    if (b->d_jobs) (void)hipFree(b->d_jobs);
    if (b->d_mjobs) (void)hipFree(b->d_mjobs);
    if (b->d_rawcalls) (void)hipFree(b->d_rawcalls);
    if (b->d_bfjobs) (void)hipFree(b->d_bfjobs);
    if (b->d_raw_off) (void)hipFree(b->d_raw_off);
    for (int m = 0; m < 2; m++) if (b->d_raw[m]) (void)hipFree(b->d_raw[m]);
    for (int m = 0; m < 2; m++) if (b->d_flags[m]) (void)hipFree(b->d_flags[m]);
    if (b->d_out_off) (void)hipFree(b->d_out_off);
    for (int m = 0; m < 2; m++) if (b->d_rjobs[m]) (void)hipFree(b->d_rjobs[m]);
    vdisp_free(b->vd);
    if (b->d_units) (void)hipFree(b->d_units);
    if (b->d_targets) (void)hipFree(b->d_targets);
    if (b->d_graph_off) (void)hipFree(b->d_graph_off);
    if (b->d_flow0) (void)hipFree(b->d_flow0);
    if (b->d_mt_tiles) (void)hipFree(b->d_mt_tiles);
    if (b->d_mt_tiles_per_cell) (void)hipFree(b->d_mt_tiles_per_cell);
    if (b->d_mf_list) (void)hipFree(b->d_mf_list);
    if (b->rs.disp) (void)hipFree(b->rs.disp);
    if (b->rs.idx) (void)hipFree(b->rs.idx);
    if (b->rs.state) (void)hipFree(b->rs.state);
    if (b->rs.noi) (void)hipFree(b->rs.noi);
    if (b->rs.no) (void)hipFree(b->rs.no);
    if (b->rs.refit) (void)hipFree(b->rs.refit);
    if (b->rs.cell) (void)hipFree(b->rs.cell);
    delete b;
}

int les_hip_batch_set_units(les_hip_ctx* c, les_hip_batch* b, const les_hip_rect* units)
{
    if (!c || !b || (b->n > 0 && !units)) return fail(LES_HIP_ERR_ARG, "null argument");
    int maxlen = 1;
    for (int i = 0; i < b->n; i++) {
        const les_hip_rect& u = units[i];
        if (u.w <= 0 || u.h <= 0 || u.x < 0 || u.y < 0 || u.x + u.w > c->p.W || u.y + u.h > c->p.H)
            return fail(LES_HIP_ERR_ARG, "unit rect %d empty or outside the image", i);
        maxlen = std::max(maxlen, u.w * u.h);
    }
    if (b->n == 0) return LES_HIP_OK;
    static_assert(sizeof(les::Rect4) == sizeof(les_hip_rect), "rect layout");
    if (!b->d_units) HIPCHECK(hipMalloc((void**)&b->d_units, (size_t)b->n * sizeof(les::Rect4)));
    HIPCHECK(hipMemcpy(b->d_units, units, (size_t)b->n * sizeof(les::Rect4), hipMemcpyHostToDevice));
    if (!b->rs.idx) {
        const size_t n = (size_t)b->n, S = kRansacMaxSam;
        HIPCHECK(hipMalloc((void**)&b->rs.idx, n * S * 3 * sizeof(int)));
        HIPCHECK(hipMalloc((void**)&b->rs.state, n * (S + 1) * sizeof(uint64_t)));
        HIPCHECK(hipMalloc((void**)&b->rs.noi, n * S * sizeof(int)));
        HIPCHECK(hipMalloc((void**)&b->rs.no, n * S * sizeof(int)));
        HIPCHECK(hipMalloc((void**)&b->rs.refit, n * S * 3 * sizeof(float)));
        HIPCHECK(hipMalloc((void**)&b->rs.cell, n * sizeof(les::RansacCell)));
    }
    if (b->rs.disp) HIPCHECK(hipFree(b->rs.disp));
    b->rs.disp = nullptr;
    b->rs.stride = maxlen;
    HIPCHECK(hipMalloc((void**)&b->rs.disp, (size_t)b->n * maxlen * sizeof(float)));
    return LES_HIP_OK;
}

int les_hip_batch_propose(les_hip_ctx* c, const les_hip_batch* b, int kind, int m, les_hip_plane* labels, uint64_t* rng,
                          les_hip_plane* planes)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !labels || !rng || !planes) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    if (!b->d_units) return fail(LES_HIP_ERR_ARG, "les_hip_batch_set_units was not called for this batch");
    float4* lab = reinterpret_cast<float4*>(labels);
    float4* pl = reinterpret_cast<float4*>(planes);
    const int n = b->n, W = c->p.W;
    const float mind = c->p.min_disparity, maxd = c->p.max_disparity;
    switch (kind) {
    case LES_HIP_PROPOSE_EXPANSION:
        hipLaunchKernelGGL(les::les_expansion_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units, lab, W, rng, pl, n);
        break;
    case LES_HIP_PROPOSE_RANDOM:
        hipLaunchKernelGGL(les::les_random_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units, lab, W, rng, pl, n, m, mind, maxd, c->random_vdisp);
        break;
    case LES_HIP_PROPOSE_RANSAC:
        // RansacProposer(K, MAX_SAM = 500, conf = 0.95), threshold 1.0 (LES/Proposer.h:265,305)
        hipLaunchKernelGGL(les::les_ransac_snapshot_kernel, dim3(n), dim3(256), 0, cur_stream(c), b->d_units, lab, W, b->rs);
        // the reference's adaptive schedule (:193, :229-236): candidates in chunks, a cell whose loop has ended ignores the later launches
        // (no host round trip: the launches of dead chunks return at once)
        hipLaunchKernelGGL(les::les_ransac_begin_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units, rng, b->rs, n, kRansacMaxSam, kRansacChunkEnds[0]);
        for (int k = 0, j0 = 0; k < kRansacChunks; k++) {
            const int j1 = kRansacChunkEnds[k], j2 = k + 1 < kRansacChunks ? kRansacChunkEnds[k + 1] : kRansacMaxSam;
            hipLaunchKernelGGL(les::les_ransac_eval_kernel, dim3(n, (j1 - j0 + les::kRansacCandPerBlock - 1) / les::kRansacCandPerBlock), dim3(64 * les::kRansacCandPerBlock), 0, cur_stream(c), b->d_units, b->rs, kRansacMaxSam, 1.0f, j0, j1);
            hipLaunchKernelGGL(les::les_ransac_walk_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units, rng, pl, b->rs, n, kRansacMaxSam, 0.95f, j0, j1, j2);
            j0 = j1;
        }
        break;
    case LES_HIP_PROPOSE_INIT:
        hipLaunchKernelGGL(les::les_init_labels_kernel, dim3(n), dim3(64), 0, cur_stream(c), b->d_units, lab, W, rng, pl, mind, maxd, c->max_vdisp);
        break;
    default:
        return fail(LES_HIP_ERR_ARG, "unknown proposer kind %d", kind);
    }
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_batch_wta(les_hip_ctx* c, const les_hip_batch* b, const les_hip_plane* planes, float* cur, const float* prop,
                      les_hip_plane* labels)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !planes || !cur || !prop || !labels) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    if (!b->d_targets) return fail(LES_HIP_ERR_ARG, "batch has no target table");
    hipLaunchKernelGGL(les::les_wta_kernel, dim3(b->n, b->wta_chunks), dim3(256), 0, cur_stream(c), b->d_targets, reinterpret_cast<const float4*>(planes),
                       cur, prop, reinterpret_cast<float4*>(labels), c->p.W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_batch_num_jobs(const les_hip_batch* b) { return b ? (b->march_ok ? b->nmgroups : b->njobs) : 0; }

int les_hip_batch_kernel_kind(const les_hip_ctx* c, const les_hip_batch* b, int mode)
{
    if (!c || !b || mode < 0 || mode > 1) return -1;
    if (c->filter != LES_HIP_FILTER_GF) return 2;
    if (!c->naive && c->interp != 1) return (b->march_ok && interp_march_ok(c, mode) && b->raw_floats <= kRawPatchCapFloats) ? 1 : 0;
    return (b->march_ok && c->march && c->v[mode].march_ok) ? 1 : 0;
}

// The raw-cost patch table of a cost-volume batch (interpolation 0 / 2 on the march kernel), built on the batch's first such run
int ensure_interp_tables(les_hip_ctx* c, const les_hip_batch* b_)
{
    les_hip_batch* b = const_cast<les_hip_batch*>(b_);
    if (b->interp_tables) return LES_HIP_OK;
    std::vector<les::RawCall> calls;
    long long tot = 0, amax = 1;
    build_bf_raw_calls(b->n, b->filters.data(), b->targets.data(), calls, tot, amax);
    b->raw_floats = tot;
    std::vector<long long> offs((size_t)b->n), outs((size_t)b->n);
    const long long P = (long long)c->p.H * c->p.W;
    for (int i = 0; i < b->n; i++) {
        offs[i] = calls[i].off;
        outs[i] = (b->out_slabs ? (long long)(i / b->out_slabs) * P : 0) + (long long)b->targets[i].y * c->p.W + b->targets[i].x;
    }
    b->raw_chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
    if (b->n > 0) {
        HIPCHECK(hipMalloc((void**)&b->d_rawcalls, (size_t)b->n * sizeof(les::RawCall)));
        HIPCHECK(hipMemcpy(b->d_rawcalls, calls.data(), (size_t)b->n * sizeof(les::RawCall), hipMemcpyHostToDevice));
        HIPCHECK(hipMalloc((void**)&b->d_raw_off, (size_t)b->n * sizeof(long long)));
        HIPCHECK(hipMemcpy(b->d_raw_off, offs.data(), (size_t)b->n * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHECK(hipMalloc((void**)&b->d_out_off, (size_t)b->n * sizeof(long long)));
        HIPCHECK(hipMemcpy(b->d_out_off, outs.data(), (size_t)b->n * sizeof(long long), hipMemcpyHostToDevice));
    }
    b->interp_tables = true;
    return LES_HIP_OK;
}

int les_hip_batch_run(les_hip_ctx* c, const les_hip_batch* b, int mode, const les_hip_plane* planes, int planes_on_device,
                      float* out_dev, int check)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !out_dev || (b->n > 0 && !planes)) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->R != c->R) return fail(LES_HIP_ERR_ARG, "batch was prepared for a different context");
    const float4* d_planes = reinterpret_cast<const float4*>(planes);
    if (!planes_on_device) {
        int rc = ensure_planes(c, (size_t)b->n);
        if (rc) return rc;
        HIPCHECK(hipMemcpyAsync(c->d_planes, planes, (size_t)b->n * sizeof(float4), hipMemcpyHostToDevice, cur_stream(c)));
        d_planes = c->d_planes;
    }
    if (c->filter != LES_HIP_FILTER_GF) return run_bf_batch(c, b, mode, d_planes, out_dev, check);
    if (!c->naive && c->interp != 1 && mode >= 0 && mode <= 1 && b->march_ok && interp_march_ok(c, mode)) {
        {
            std::lock_guard<std::mutex> lk(c->mu);
            int rc = ensure_interp_tables(c, b);
            if (rc) return rc;
            if (b->raw_floats <= kRawPatchCapFloats) {
                if (!b->d_raw[mode]) HIPCHECK(hipMalloc((void**)&b->d_raw[mode], (size_t)std::max<long long>(b->raw_floats, 1) * sizeof(float)));
                if (c->interp == 2 && !b->d_flags[mode]) HIPCHECK(hipMalloc((void**)&b->d_flags[mode], (size_t)std::max(b->n, 1) * sizeof(unsigned)));
                if (c->interp == 2 && !b->d_rjobs[mode]) HIPCHECK(hipMalloc((void**)&b->d_rjobs[mode], (size_t)std::max(b->njobs, 1) * sizeof(les::Job)));
            }
        }
        if (b->raw_floats <= kRawPatchCapFloats) {
            const RawPatches rp{b->d_rawcalls, b->d_raw_off, b->d_raw[mode], b->n, b->raw_chunks};
            return launch_interp_march(c, b->mentry, mode, b->d_mjobs, b->nmgroups, rp, b->d_flags[mode], b->d_jobs, b->d_rjobs[mode], b->njobs,
                                       b->d_targets, b->d_out_off, c->p.W, d_planes, out_dev, check, cur_stream(c));
        }
        note_fallback(c->fallback_seen, FB_PATCHES, "the raw-cost patches of one batch at interpolation %d exceed 4 GB", c->interp);
    }
    if (b->march_ok && mode >= 0 && mode <= 1 && c->march && c->v[mode].march_ok && (c->naive || c->interp == 1)) {
        if (!c->naive) return launch_march(c, b->mentry, mode, b->d_mjobs, b->nmgroups, d_planes, out_dev, check, cur_stream(c));
        {
            std::lock_guard<std::mutex> lk(c->mu);
            if (!b->d_raw[mode]) HIPCHECK(hipMalloc((void**)&b->d_raw[mode], (size_t)std::max<long long>(b->raw_floats, 1) * sizeof(float)));
        }
        const RawPatches rp{b->d_rawcalls, b->d_raw_off, b->d_raw[mode], b->n, b->raw_chunks};
        return launch_naive_march(c, b->mentry, mode, b->d_mjobs, b->nmgroups, d_planes, out_dev, check, cur_stream(c), rp);
    }
    if (!c->naive && c->interp != 1) {
        {
            std::lock_guard<std::mutex> lk(c->mu);
            int rc = ensure_interp_tables(c, b);
            if (rc) return rc;
        }
        int rc = launch_strips(c, mode, b->d_jobs, b->njobs, d_planes, out_dev, check, cur_stream(c));
        if (rc) return rc;
        return launch_nan_spread(c, mode, b->n, b->d_rawcalls, b->d_targets, b->d_out_off, c->p.W, d_planes, nullptr, out_dev, check, cur_stream(c));
    }
    int rc = launch_strips(c, mode, b->d_jobs, b->njobs, d_planes, out_dev, check, cur_stream(c));
    if (rc || !c->naive) return rc;
    // image-based context: the strip kernel gathers along one row; the calls with v != 0 are recomputed after it
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!b->vd) rc = vdisp_build(c, b->n, b->filters.data(), b->targets.data(), &b->vd);
        if (rc) return rc;
    }
    return launch_vdisp_strips(c, b->vd, mode, b->d_jobs, b->njobs, d_planes, out_dev, check, cur_stream(c));
}

int les_hip_unary_batch(les_hip_ctx* c, int mode, int n, const les_hip_rect* frs, const les_hip_rect* trs,
                        const les_hip_plane* planes, float* cost_map, int check)
{
    if (!c || !cost_map) return fail(LES_HIP_ERR_ARG, "null argument");
    les_hip_batch* b = nullptr;
    int rc = les_hip_batch_create(c, n, frs, trs, 0, &b);
    if (rc) return rc;
    rc = les_hip_batch_run(c, b, mode, planes, 0, c->d_map, check);
    if (rc == LES_HIP_OK) {
        // copy back only the target rects (the reference writes nothing else, LES/CostVolumeEnergy.h:169-171)
        for (int i = 0; i < n && rc == LES_HIP_OK; i++) {
            const les_hip_rect& t = trs[i];
            if (t.w <= 0 || t.h <= 0) continue;
            size_t off = (size_t)t.y * c->p.W + t.x;
            hipError_t e = hipMemcpy2DAsync(cost_map + off, (size_t)c->p.W * sizeof(float), c->d_map + off, (size_t)c->p.W * sizeof(float),
                                            (size_t)t.w * sizeof(float), (size_t)t.h, hipMemcpyDeviceToHost, cur_stream(c));
            if (e != hipSuccess) rc = fail(LES_HIP_ERR_DEVICE, "hipMemcpy2DAsync failed: %s", hipGetErrorString(e));
        }
        if (rc == LES_HIP_OK && hipStreamSynchronize(cur_stream(c)) != hipSuccess) rc = fail(LES_HIP_ERR_DEVICE, "stream synchronize failed");
    }
    les_hip_batch_destroy(b);
    return rc;
}

int les_hip_scratch_create(les_hip_ctx* c, les_hip_scratch** out)
{
    if (!c || !out) return fail(LES_HIP_ERR_ARG, "null argument");
    *out = nullptr;
    HIPCHECK(hipSetDevice(c->p.device));
    les_hip_scratch* s = new les_hip_scratch();
    s->c = c;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&s->d_plane, sizeof(float4)) != hipSuccess || hipHostMalloc((void**)&s->h_plane, sizeof(float4), hipHostMallocDefault) != hipSuccess) {
        les_hip_scratch_destroy(s);
        return fail(LES_HIP_ERR_DEVICE, "scratch allocation failed");
    }
    *out = s;
    return LES_HIP_OK;
}

void les_hip_scratch_destroy(les_hip_scratch* s)
{
    if (!s) return;
    if (s->c) (void)hipSetDevice(s->c->p.device);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    for (auto& e : s->cache) if (e.d_jobs) (void)hipFree(e.d_jobs);
    for (auto& e : s->cache) if (e.d_sjobs) (void)hipFree(e.d_sjobs);
    if (s->d_flag) (void)hipFree(s->d_flag);
    if (s->d_target) (void)hipFree(s->d_target);
    if (s->d_zero) (void)hipFree(s->d_zero);
    if (s->d_rjobs) (void)hipFree(s->d_rjobs);
    vdisp_free(s->vd);
    if (s->d_tile) (void)hipFree(s->d_tile);
    if (s->h_tile) (void)hipHostFree(s->h_tile);
    if (s->d_raw) (void)hipFree(s->d_raw);
    if (s->d_rawcall) (void)hipFree(s->d_rawcall);
    if (s->d_bfjobs) (void)hipFree(s->d_bfjobs);
    if (s->d_raw_off) (void)hipFree(s->d_raw_off);
    if (s->d_plane) (void)hipFree(s->d_plane);
    if (s->h_plane) (void)hipHostFree(s->h_plane);
    delete s;
}

int les_hip_unary_one_scratch(les_hip_ctx* c, les_hip_scratch* s, int mode, const les_hip_rect* fr, const les_hip_rect* tr,
                              const les_hip_plane* plane, float* costs, int row_stride, int check)
{
    if (!c || !s || !fr || !tr || !plane || !costs) return fail(LES_HIP_ERR_ARG, "null argument");
    if (s->c != c) return fail(LES_HIP_ERR_ARG, "scratch belongs to another context");
    if (c->filter != LES_HIP_FILTER_GF) return bf_unary_one(c, s, mode, fr, tr, plane, costs, row_stride, check);
    if (mode < 0 || mode > 1 || !c->v[mode].stats || (c->naive ? !c->v[1 - mode].feat : !c->v[mode].vol))
        return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    HIPCHECK(hipSetDevice(c->p.device));                  // HIP's current device is per host thread
    int rc = check_rects(c, *fr, *tr);
    if (rc) return rc;
    if (tr->w <= 0 || tr->h <= 0) return LES_HIP_OK;
    // ---- job table of this rect pair (built and uploaded the first time it is seen; 16 pairs are remembered)
    const bool lin = c->naive || c->interp == 1;
    const int want_march = (lin ? (c->march && c->v[mode].march_ok) : interp_march_ok(c, mode)) ? 1 : 0;      // per view: the march kernel needs a finite, bounded volume
    les_hip_scratch::Entry* e = nullptr;
    for (auto& x : s->cache)
        if (x.want_march == want_march && !memcmp(&x.f, fr, sizeof *fr) && !memcmp(&x.t, tr, sizeof *tr)) { e = &x; break; }
    if (!e) {
        std::vector<les::Job> jobs;
        bool mok = false;
        const MarchEntry* me = nullptr;
        if (want_march) build_march_jobs(c, 1, fr, tr, 0, jobs, mok, me);
        const bool use_march = want_march && mok && !jobs.empty();
        if (!use_march) {
            rc = build_jobs(c, 1, fr, tr, 0, jobs);
            if (rc) return rc;
            me = nullptr;
        }
        for (auto& j : jobs) {                           // compact tile: row stride = target width, origin = target corner
            j.out_off = (long long)(j.ty0 - tr->y) * tr->w + (j.tx0 - tr->x);
            j.out_stride = tr->w;
        }
        les_hip_scratch::Entry ne{*fr, *tr, want_march, me, (int)jobs.size(), me ? (int)(jobs.size() / me->NJ) : 0, nullptr, 0};
        if (s->cache.size() >= 16) {                     // evict the least recently used pair
            size_t k = 0;
            for (size_t i = 1; i < s->cache.size(); i++) if (s->cache[i].stamp < s->cache[k].stamp) k = i;
            HIPCHECK(hipStreamSynchronize(s->stream));
            if (s->cache[k].d_jobs) HIPCHECK(hipFree(s->cache[k].d_jobs));
            if (s->cache[k].d_sjobs) HIPCHECK(hipFree(s->cache[k].d_sjobs));
            s->cache.erase(s->cache.begin() + (long)k);
        }
        HIPCHECK(hipMalloc((void**)&ne.d_jobs, jobs.size() * sizeof(les::Job)));
        if (hipMemcpy(ne.d_jobs, jobs.data(), jobs.size() * sizeof(les::Job), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(ne.d_jobs);
            return fail(LES_HIP_ERR_DEVICE, "upload of the job table failed");
        }
        s->cache.push_back(ne);
        e = &s->cache.back();
    }
    e->stamp = ++s->clock;
    const size_t need = (size_t)tr->w * tr->h;
    if (need > s->tile_cap) {
        HIPCHECK(hipStreamSynchronize(s->stream));
        if (s->d_tile) HIPCHECK(hipFree(s->d_tile));
        if (s->h_tile) HIPCHECK(hipHostFree(s->h_tile));
        s->d_tile = nullptr; s->h_tile = nullptr; s->tile_cap = 0;
        const size_t cap = std::max(need, (size_t)256 * 256);
        HIPCHECK(hipMalloc((void**)&s->d_tile, cap * sizeof(float)));
        HIPCHECK(hipHostMalloc((void**)&s->h_tile, cap * sizeof(float), hipHostMallocDefault));
        s->tile_cap = cap;
    }
    *s->h_plane = make_float4(plane->a, plane->b, plane->c, plane->v);
    HIPCHECK(hipMemcpyAsync(s->d_plane, s->h_plane, sizeof(float4), hipMemcpyHostToDevice, s->stream));
    if (e->march && !lin && c->interp == 2 && !e->d_sjobs) {
        // the strip jobs of the recompute launch of this rect pair, and room for their masked copy
        std::vector<les::Job> sj;
        rc = build_jobs(c, 1, fr, tr, 0, sj);
        if (rc) return rc;
        for (auto& j : sj) { j.out_off = (long long)(j.ty0 - tr->y) * tr->w + (j.tx0 - tr->x); j.out_stride = tr->w; }
        HIPCHECK(hipStreamSynchronize(s->stream));
        HIPCHECK(hipMalloc((void**)&e->d_sjobs, sj.size() * sizeof(les::Job)));
        HIPCHECK(hipMemcpy(e->d_sjobs, sj.data(), sj.size() * sizeof(les::Job), hipMemcpyHostToDevice));
        e->nsjobs = (int)sj.size();
        if (sj.size() > s->rjobs_cap) {
            if (s->d_rjobs) HIPCHECK(hipFree(s->d_rjobs));
            s->d_rjobs = nullptr; s->rjobs_cap = 0;
            HIPCHECK(hipMalloc((void**)&s->d_rjobs, std::max<size_t>(sj.size(), 64) * sizeof(les::Job)));
            s->rjobs_cap = std::max<size_t>(sj.size(), 64);
        }
        if (!s->d_flag) HIPCHECK(hipMalloc((void**)&s->d_flag, sizeof(unsigned)));
    }
    if ((e->march && c->naive) || !lin) {
        // raw-cost patch of this filterRect (the one-entry call table is rewritten when the rect changes; everything is ordered on the scratch's stream)
        const size_t rneed = (size_t)fr->w * fr->h;
        if (rneed > s->raw_cap || !s->d_rawcall) {
            HIPCHECK(hipStreamSynchronize(s->stream));
            if (s->d_raw) HIPCHECK(hipFree(s->d_raw));
            s->d_raw = nullptr; s->raw_cap = 0;
            const size_t cap = std::max(rneed, (size_t)256 * 256);
            HIPCHECK(hipMalloc((void**)&s->d_raw, cap * sizeof(float)));
            s->raw_cap = cap;
            if (!s->d_rawcall) {
                HIPCHECK(hipMalloc((void**)&s->d_rawcall, sizeof(les::RawCall)));
                HIPCHECK(hipMalloc((void**)&s->d_raw_off, sizeof(long long)));
                const long long zero = 0;
                HIPCHECK(hipMemcpy(s->d_raw_off, &zero, sizeof zero, hipMemcpyHostToDevice));
            }
            s->raw_f = les_hip_rect{-1, -1, -1, -1};
        }
        if (memcmp(&s->raw_f, fr, sizeof *fr)) {
            const les::RawCall call{fr->x, fr->y, fr->w, fr->h, 0};
            HIPCHECK(hipStreamSynchronize(s->stream));
            HIPCHECK(hipMemcpy(s->d_rawcall, &call, sizeof call, hipMemcpyHostToDevice));
            s->raw_f = *fr;
        }
        const RawPatches rp{s->d_rawcall, s->d_raw_off, s->d_raw, 1, (int)std::min<size_t>(1024, (rneed + 4095) / 4096)};
        if (!c->naive) {
            // (interpolation 0 / 2: the target rect of les_nan_spread_kernel)
            if (!s->d_target) {
                HIPCHECK(hipMalloc((void**)&s->d_target, sizeof(les::WtaJob)));
                HIPCHECK(hipMalloc((void**)&s->d_zero, sizeof(long long)));
                const long long zero = 0;
                HIPCHECK(hipMemcpy(s->d_zero, &zero, sizeof zero, hipMemcpyHostToDevice));
            }
            const les::WtaJob tj{tr->x, tr->y, tr->w, tr->h};
            HIPCHECK(hipStreamSynchronize(s->stream));
            HIPCHECK(hipMemcpy(s->d_target, &tj, sizeof tj, hipMemcpyHostToDevice));
        }
        if (c->naive) rc = launch_naive_march(c, static_cast<const MarchEntry*>(e->march), mode, e->d_jobs, e->ngroups, s->d_plane, s->d_tile, check, s->stream, rp);
        else if (e->march) rc = launch_interp_march(c, static_cast<const MarchEntry*>(e->march), mode, e->d_jobs, e->ngroups, rp, s->d_flag, e->d_sjobs, s->d_rjobs,
                                                    c->interp == 2 ? e->nsjobs : 0, s->d_target, s->d_zero, tr->w, s->d_plane, s->d_tile, check, s->stream);
        else {
            rc = launch_strips(c, mode, e->d_jobs, e->njobs, s->d_plane, s->d_tile, check, s->stream);
            if (!rc) rc = launch_nan_spread(c, mode, 1, s->d_rawcall, s->d_target, s->d_zero, tr->w, s->d_plane, nullptr, s->d_tile, check, s->stream);
        }
    }
    else if (e->march) rc = launch_march(c, static_cast<const MarchEntry*>(e->march), mode, e->d_jobs, e->ngroups, s->d_plane, s->d_tile, check, s->stream);
    else {
        rc = launch_strips(c, mode, e->d_jobs, e->njobs, s->d_plane, s->d_tile, check, s->stream);
        if (!rc && c->naive) {
            // image-based context: a call with v != 0 is recomputed after the strip kernel (les_hip_vdisp.inc); the call table follows the rect
            // pair, the stand-in volume (one slice) and the flag stay
            if (!s->vd || memcmp(&s->vd_f, fr, sizeof *fr) || memcmp(&s->vd_t, tr, sizeof *tr)) {
                VdispStrip* nv = nullptr;
                HIPCHECK(hipStreamSynchronize(s->stream));
                rc = vdisp_build(c, 1, fr, tr, &nv);
                if (rc) return rc;
                if (s->vd) for (int m = 0; m < 2; m++) { std::swap(nv->d_vol[m], s->vd->d_vol[m]); std::swap(nv->d_flags[m], s->vd->d_flags[m]); }
                vdisp_free(s->vd);
                s->vd = nv; s->vd_f = *fr; s->vd_t = *tr;
            }
            rc = launch_vdisp_strips(c, s->vd, mode, e->d_jobs, e->njobs, s->d_plane, s->d_tile, check, s->stream);
        }
    }
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(s->h_tile, s->d_tile, need * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHECK(hipStreamSynchronize(s->stream));
    // costs(targetRect - filterRect.tl()), LES/CostVolumeEnergy.h:169
    float* dst = costs + (size_t)(tr->y - fr->y) * row_stride + (tr->x - fr->x);
    for (int y = 0; y < tr->h; y++) memcpy(dst + (size_t)y * row_stride, s->h_tile + (size_t)y * tr->w, (size_t)tr->w * sizeof(float));
    return LES_HIP_OK;
}

int les_hip_unary_one(les_hip_ctx* c, int mode, const les_hip_rect* fr, const les_hip_rect* tr, const les_hip_plane* plane,
                      float* costs, int row_stride, int check)
{
    if (!c || !fr || !tr || !plane || !costs) return fail(LES_HIP_ERR_ARG, "null argument");
    // One scratch per (calling thread, context), created on the thread's first call and owned by the context.  The thread-local entry
    // is keyed by the context's generation id (never by its address); when the thread exits, its scratches go back to their contexts'
    // idle lists -- if those contexts are still alive -- so short-lived caller threads recycle a bounded set instead of piling up.
    struct Mine {
        std::vector<std::pair<unsigned long long, les_hip_scratch*>> v;
        ~Mine() { for (auto& e : v) release_hidden_scratch(e.first, e.second); }
    };
    thread_local Mine mine;
    les_hip_scratch* s = nullptr;
    for (auto& e : mine.v) if (e.first == c->gen) { s = e.second; break; }
    if (!s) {
        {
            std::lock_guard<std::mutex> lk(c->mu);
            if (!c->idle_scratch.empty()) { s = c->idle_scratch.back(); c->idle_scratch.pop_back(); }
        }
        if (!s) {
            int rc = les_hip_scratch_create(c, &s);
            if (rc) return rc;
            std::lock_guard<std::mutex> lk(c->mu);
            c->own_scratch.push_back(s);
        }
        mine.v.emplace_back(c->gen, s);
    }
    return les_hip_unary_one_scratch(c, s, mode, fr, tr, plane, costs, row_stride, check);
}

int les_hip_wta_update(les_hip_ctx* c, int n, const les_hip_rect* rects, const les_hip_plane* planes, int planes_on_device,
                       float* cur, const float* prop, les_hip_plane* labels)
{
    if (!c || n < 0 || (n > 0 && (!rects || !planes || !cur || !prop || !labels))) return fail(LES_HIP_ERR_ARG, "null argument");
    if (n == 0) return LES_HIP_OK;
    for (int i = 0; i < n; i++)
        if (rects[i].x < 0 || rects[i].y < 0 || rects[i].w < 0 || rects[i].h < 0 || rects[i].x + rects[i].w > c->p.W || rects[i].y + rects[i].h > c->p.H)
            return fail(LES_HIP_ERR_ARG, "rect outside the image");
    if ((size_t)n > c->wta_cap) {
        if (c->d_wta) HIPCHECK(hipFree(c->d_wta));
        c->d_wta = nullptr; c->wta_cap = 0;
        HIPCHECK(hipMalloc((void**)&c->d_wta, std::max<size_t>(n, 1024) * sizeof(les::WtaJob)));
        c->wta_cap = std::max<size_t>(n, 1024);
    }
    static_assert(sizeof(les::WtaJob) == sizeof(les_hip_rect), "rect layout");
    HIPCHECK(hipMemcpyAsync(c->d_wta, rects, (size_t)n * sizeof(les::WtaJob), hipMemcpyHostToDevice, cur_stream(c)));
    const float4* d_planes = reinterpret_cast<const float4*>(planes);
    if (!planes_on_device) {
        if ((size_t)n > c->wta_planes_cap) {
            if (c->d_wta_planes) HIPCHECK(hipFree(c->d_wta_planes));
            c->d_wta_planes = nullptr; c->wta_planes_cap = 0;
            HIPCHECK(hipMalloc((void**)&c->d_wta_planes, std::max<size_t>(n, 1024) * sizeof(float4)));
            c->wta_planes_cap = std::max<size_t>(n, 1024);
        }
        HIPCHECK(hipMemcpyAsync(c->d_wta_planes, planes, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, cur_stream(c)));
        d_planes = c->d_wta_planes;
    }
    int max_area = 1;
    for (int i = 0; i < n; i++) max_area = std::max(max_area, rects[i].w * rects[i].h);
    const int chunks = std::min(32, std::max(1, (max_area + 4095) / 4096));
    hipLaunchKernelGGL(les::les_wta_kernel, dim3(n, chunks), dim3(256), 0, cur_stream(c), c->d_wta, d_planes, cur, prop,
                       reinterpret_cast<float4*>(labels), c->p.W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
