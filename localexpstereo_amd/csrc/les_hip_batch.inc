// les_hip_batch.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): prepared batches -- creation, proposals, winner-take-all, unary costs -- and the per-call operator with its scratch; both run their unary costs through run_unary (les_hip_unary.inc)
extern "C" {

int les_hip_batch_create(les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, int out_slabs, les_hip_batch** out)
{
    if (!c || !out || n < 0 || (n > 0 && (!frs || !trs))) return fail(LES_HIP_ERR_ARG, "null argument");
    if (out_slabs < 0) return fail(LES_HIP_ERR_ARG, "out_slabs must be 0 (one map) or the number of consecutive calls that share a slab");
    // (since round 4 out_slabs = k means "call i writes slab i / k"; before, any non-zero value meant k = 1.  A caller that still passes another
    // non-zero constant for "one slab per call" would get overlapping writes: only a k that divides n is a well-formed request)
    if (out_slabs > 1 && n % out_slabs != 0) return fail(LES_HIP_ERR_ARG, "out_slabs = %d does not divide the %d calls of the batch (slab i / out_slabs holds out_slabs consecutive calls; pass 1 for one slab per call)", out_slabs, n);
    *out = nullptr;
    les_hip_batch* b = new les_hip_batch();
    int rc = build_unary_tables(c, n, frs, trs, out_slabs, false, b->tab);
    if (rc) { les_hip_batch_destroy(b); return rc; }
    b->ws.shared = true;
    b->n = n; b->R = c->R; b->device = c->p.device;
    b->targets.assign(trs, trs + n);
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
        if (b->d_graph_off.alloc((size_t)n) ||
            hipMemcpy(b->d_graph_off.p, b->graph_off.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess ||
            b->d_flow0.alloc((size_t)n * b->graph_chunks)) {
            les_hip_batch_destroy(b);
            return fail(LES_HIP_ERR_DEVICE, "upload of the graph offset table failed");
        }
        if (b->d_targets.alloc((size_t)n) ||
            hipMemcpy(b->d_targets.p, trs, (size_t)n * sizeof(les::WtaJob), hipMemcpyHostToDevice) != hipSuccess) {
            les_hip_batch_destroy(b);
            return fail(LES_HIP_ERR_DEVICE, "upload of the target table failed");
        }
    }
    *out = b;
    return LES_HIP_OK;
}

void les_hip_batch_destroy(les_hip_batch* b)
{
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
    int rc = b->d_units.grow((size_t)b->n, 0, cur_stream(c));
    if (rc) return rc;
    HIPCHECK(hipMemcpy(b->d_units.p, units, (size_t)b->n * sizeof(les::Rect4), hipMemcpyHostToDevice));
    // (sized by b->n, which is fixed: allocated by the first call; the snapshot follows the largest unit seen)
    const size_t n = (size_t)b->n, S = kRansacMaxSam;
    hipStream_t st = cur_stream(c);
    rc = b->rs_idx.grow(n * S * 3, 0, st);
    if (!rc) rc = b->rs_state.grow(n * (S + 1), 0, st);
    if (!rc) rc = b->rs_noi.grow(n * S, 0, st);
    if (!rc) rc = b->rs_no.grow(n * S, 0, st);
    if (!rc) rc = b->rs_refit.grow(n * S * 3, 0, st);
    if (!rc) rc = b->rs_cell.grow(n, 0, st);
    if (!rc) rc = b->rs_disp.grow(n * maxlen, 0, st);
    // (after a failure too: a grow that failed has freed its old buffer, which must not stay in the kernels' argument)
    b->rs = les::RansacScratch{b->rs_disp.p, b->rs_idx.p, b->rs_state.p, b->rs_noi.p, b->rs_no.p, b->rs_refit.p, maxlen, b->rs_cell.p};
    return rc;
}

int les_hip_batch_propose(les_hip_ctx* c, const les_hip_batch* b, int kind, int m, les_hip_plane* labels, uint64_t* rng,
                          les_hip_plane* planes)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !labels || !rng || !planes) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    if (!b->d_units.p) return fail(LES_HIP_ERR_ARG, "les_hip_batch_set_units was not called for this batch");
    float4* lab = reinterpret_cast<float4*>(labels);
    float4* pl = reinterpret_cast<float4*>(planes);
    const int n = b->n, W = c->p.W;
    const float mind = c->p.min_disparity, maxd = c->p.max_disparity;
    switch (kind) {
    case LES_HIP_PROPOSE_EXPANSION:
        hipLaunchKernelGGL(les::les_expansion_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units.p, lab, W, rng, pl, n);
        break;
    case LES_HIP_PROPOSE_RANDOM:
        hipLaunchKernelGGL(les::les_random_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units.p, lab, W, rng, pl, n, m, mind, maxd, c->random_vdisp);
        break;
    case LES_HIP_PROPOSE_RANSAC:
        // RansacProposer(K, MAX_SAM = 500, conf = 0.95), threshold 1.0 (LES/Proposer.h:265,305)
        hipLaunchKernelGGL(les::les_ransac_snapshot_kernel, dim3(n), dim3(256), 0, cur_stream(c), b->d_units.p, lab, W, b->rs);
        // the reference's adaptive schedule (:193, :229-236): candidates in chunks, a cell whose loop has ended ignores the later launches
        // (no host round trip: the launches of dead chunks return at once)
        hipLaunchKernelGGL(les::les_ransac_begin_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units.p, rng, b->rs, n, kRansacMaxSam, kRansacChunkEnds[0]);
        for (int k = 0, j0 = 0; k < kRansacChunks; k++) {
            const int j1 = kRansacChunkEnds[k], j2 = k + 1 < kRansacChunks ? kRansacChunkEnds[k + 1] : kRansacMaxSam;
            hipLaunchKernelGGL(les::les_ransac_eval_kernel, dim3(n, (j1 - j0 + les::kRansacCandPerBlock - 1) / les::kRansacCandPerBlock), dim3(64 * les::kRansacCandPerBlock), 0, cur_stream(c), b->d_units.p, b->rs, kRansacMaxSam, 1.0f, j0, j1);
            hipLaunchKernelGGL(les::les_ransac_walk_kernel, dim3((n + 63) / 64), dim3(64), 0, cur_stream(c), b->d_units.p, rng, pl, b->rs, n, kRansacMaxSam, 0.95f, j0, j1, j2);
            j0 = j1;
        }
        break;
    case LES_HIP_PROPOSE_INIT:
        hipLaunchKernelGGL(les::les_init_labels_kernel, dim3(n), dim3(64), 0, cur_stream(c), b->d_units.p, lab, W, rng, pl, mind, maxd, c->max_vdisp);
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
    if (!b->d_targets.p) return fail(LES_HIP_ERR_ARG, "batch has no target table");
    hipLaunchKernelGGL(les::les_wta_kernel, dim3(b->n, b->wta_chunks), dim3(256), 0, cur_stream(c), b->d_targets.p, reinterpret_cast<const float4*>(planes),
                       cur, prop, reinterpret_cast<float4*>(labels), c->p.W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

// (a guided-filter batch has strip jobs, a bilateral / unfiltered one tiles)
int les_hip_batch_num_jobs(const les_hip_batch* b) { return b ? (b->tab.march_ok ? b->tab.nmgroups : b->tab.njobs + b->tab.nbfjobs) : 0; }

int les_hip_batch_kernel_kind(const les_hip_ctx* c, const les_hip_batch* b, int mode)
{
    if (!c || !b || mode < 0 || mode > 1) return -1;
    return unary_kind(c, b->tab, mode);
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
    return run_unary(c, b->tab, b->ws, mode, d_planes, out_dev, check, cur_stream(c));
}

int les_hip_unary_batch(les_hip_ctx* c, int mode, int n, const les_hip_rect* frs, const les_hip_rect* trs,
                        const les_hip_plane* planes, float* cost_map, int check)
{
    if (!c || !cost_map) return fail(LES_HIP_ERR_ARG, "null argument");
    les_hip_batch* b = nullptr;
    int rc = les_hip_batch_create(c, n, frs, trs, 0, &b);
    if (rc) return rc;
    rc = les_hip_batch_run(c, b, mode, planes, 0, c->d_map.p, check);
    if (rc == LES_HIP_OK) {
        // copy back only the target rects (the reference writes nothing else, LES/CostVolumeEnergy.h:169-171)
        for (int i = 0; i < n && rc == LES_HIP_OK; i++) {
            const les_hip_rect& t = trs[i];
            if (t.w <= 0 || t.h <= 0) continue;
            size_t off = (size_t)t.y * c->p.W + t.x;
            hipError_t e = hipMemcpy2DAsync(cost_map + off, (size_t)c->p.W * sizeof(float), c->d_map.p + off, (size_t)c->p.W * sizeof(float),
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
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess || s->d_plane.alloc(1) || s->h_plane.alloc(1)) {
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
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }      // drained before the buffers go
    delete s;
}

int les_hip_unary_one_scratch(les_hip_ctx* c, les_hip_scratch* s, int mode, const les_hip_rect* fr, const les_hip_rect* tr,
                              const les_hip_plane* plane, float* costs, int row_stride, int check)
{
    if (!c || !s || !fr || !tr || !plane || !costs) return fail(LES_HIP_ERR_ARG, "null argument");
    if (s->c != c) return fail(LES_HIP_ERR_ARG, "scratch belongs to another context");
    int rc = view_ok(c, mode);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(c->p.device));                  // HIP's current device is per host thread
    rc = check_rects(c, *fr, *tr);
    if (rc) return rc;
    if (tr->w <= 0 || tr->h <= 0) return LES_HIP_OK;
    // ---- compact-layout tables of this rect pair (built the first time it is seen; 16 pairs are remembered)
    les_hip_scratch::Entry* e = nullptr;
    for (auto& x : s->cache)
        if (!memcmp(&x.f, fr, sizeof *fr) && !memcmp(&x.t, tr, sizeof *tr)) { e = &x; break; }
    if (!e) {
        if (s->cache.size() >= 16) {                     // evict the least recently used pair
            size_t k = 0;
            for (size_t i = 1; i < s->cache.size(); i++) if (s->cache[i].stamp < s->cache[k].stamp) k = i;
            HIPCHECK(hipStreamSynchronize(s->stream));      // (launches in flight may still read its tables, which go with the entry)
            s->cache.erase(s->cache.begin() + (long)k);
        }
        UnaryTables tab;
        rc = build_unary_tables(c, 1, fr, tr, 0, true, tab);
        if (rc) return rc;
        s->cache.push_back(les_hip_scratch::Entry{*fr, *tr, std::move(tab), 0});
        e = &s->cache.back();
    }
    e->stamp = ++s->clock;
    const size_t need = (size_t)tr->w * tr->h;
    if ((rc = s->d_tile.grow(need, (size_t)256 * 256, s->stream)) || (rc = s->h_tile.grow(need, (size_t)256 * 256, s->stream))) return rc;
    *s->h_plane.p = make_float4(plane->a, plane->b, plane->c, plane->v);
    HIPCHECK(hipMemcpyAsync(s->d_plane.p, s->h_plane.p, sizeof(float4), hipMemcpyHostToDevice, s->stream));
    rc = run_unary(c, e->tab, s->ws, mode, s->d_plane.p, s->d_tile.p, check, s->stream);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(s->h_tile.p, s->d_tile.p, need * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHECK(hipStreamSynchronize(s->stream));
    // costs(targetRect - filterRect.tl()), LES/CostVolumeEnergy.h:169
    float* dst = costs + (size_t)(tr->y - fr->y) * row_stride + (tr->x - fr->x);
    for (int y = 0; y < tr->h; y++) memcpy(dst + (size_t)y * row_stride, s->h_tile.p + (size_t)y * tr->w, (size_t)tr->w * sizeof(float));
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
    int rc = c->d_wta.grow((size_t)n, 1024, cur_stream(c));
    if (rc) return rc;
    static_assert(sizeof(les::WtaJob) == sizeof(les_hip_rect), "rect layout");
    HIPCHECK(hipMemcpyAsync(c->d_wta.p, rects, (size_t)n * sizeof(les::WtaJob), hipMemcpyHostToDevice, cur_stream(c)));
    const float4* d_planes = reinterpret_cast<const float4*>(planes);
    if (!planes_on_device) {
        if ((rc = c->d_wta_planes.grow((size_t)n, 1024, cur_stream(c)))) return rc;
        HIPCHECK(hipMemcpyAsync(c->d_wta_planes.p, planes, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, cur_stream(c)));
        d_planes = c->d_wta_planes.p;
    }
    int max_area = 1;
    for (int i = 0; i < n; i++) max_area = std::max(max_area, rects[i].w * rects[i].h);
    const int chunks = std::min(32, std::max(1, (max_area + 4095) / 4096));
    hipLaunchKernelGGL(les::les_wta_kernel, dim3(n, chunks), dim3(256), 0, cur_stream(c), c->d_wta.p, d_planes, cur, prop,
                       reinterpret_cast<float4*>(labels), c->p.W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
