// les_hip_bilateral.inc -- part of the single translation unit les_hip.hip (inside its anonymous namespace): the joint bilateral ("BF") and
// the unfiltered ("") aggregation of contexts made by les_hip_create_filtered / les_hip_create_naive_filtered -- per-view set-up, weight
// table, job tables and launches of csrc/les_bilateral.h.  Guided-filter contexts never reach this file.

// Per-view set-up of a bilateral / unfiltered context: the volume (as build_view keeps it), the packed guide (the weights' operand, and the
// pairwise terms' and the post-processing's input) and, for the image-based energy, the feature images.  No guided-filter statistics.
int build_bf_view(les_hip_ctx* c, int m, const uint8_t* im, const float* vol)
{
    const size_t P = (size_t)c->p.H * c->p.W;
    ViewData& v = c->v[m];
    if (vol) {
        if (c->p.volumes_on_device) { v.vol = const_cast<float*>(vol); v.own_vol = false; }
        else {
            HIPCHECK(hipMalloc((void**)&v.vol, P * c->p.D * sizeof(float)));
            v.own_vol = true;
            HIPCHECK(hipMemcpy(v.vol, vol, P * c->p.D * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (!im) return LES_HIP_OK;
    uint8_t* d_img = nullptr;
    HIPCHECK(hipMalloc((void**)&d_img, P * 3));
    HIPCHECK(hipMemcpy(d_img, im, P * 3, hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc((void**)&v.ipk, P * sizeof(uint32_t)));
    HIPCHECK(hipMalloc((void**)&v.ipk10, P * sizeof(uint32_t)));
    if (c->naive) {
        HIPCHECK(hipMalloc((void**)&v.feat, P * sizeof(float4)));
        hipLaunchKernelGGL(les::les_naive_features_kernel, dim3((c->p.W + 255) / 256, c->p.H), dim3(256), 0, cur_stream(c), d_img, v.feat, c->p.H, c->p.W, naive_alpha(c));
    }
    hipLaunchKernelGGL(les::les_pack_guide_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, cur_stream(c), d_img, v.ipk, v.ipk10, (int)P);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    HIPCHECK(hipFree(d_img));
    return LES_HIP_OK;
}

// w[s] = exp(-s / sig2) for s = |dI|_1 = 0 .. 765, in double, stored as float (BilateralFilter::filter: cv::exp(-channelSum(w) / sig2),
// LES/GuidedFilter.h:366).  The unfiltered context gets the same table; it only ever reads w[0] = 1.
int build_bf_table(les_hip_ctx* c)
{
    std::vector<float> tab(les::kBfTabSize);
    const double sig2 = c->filter == LES_HIP_FILTER_BILATERAL ? c->p.eps : 1.0;
    for (int s = 0; s < les::kBfTabSize; s++) tab[s] = (float)std::exp(-(double)s / sig2);
    HIPCHECK(hipMalloc((void**)&c->d_bf_tab, tab.size() * sizeof(float)));
    HIPCHECK(hipMemcpy(c->d_bf_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return LES_HIP_OK;
}

// Raw-cost patch table of n calls: one patch per call with a non-empty target, the size of its filterRect.
void build_bf_raw_calls(int n, const les_hip_rect* frs, const les_hip_rect* trs, std::vector<les::RawCall>& calls, long long& tot, long long& amax)
{
    calls.resize((size_t)n);
    tot = 0; amax = 1;
    for (int i = 0; i < n; i++) {
        const bool live = trs[i].w > 0 && trs[i].h > 0;
        const long long a = live ? (long long)frs[i].w * frs[i].h : 0;
        calls[i] = les::RawCall{frs[i].x, frs[i].y, live ? frs[i].w : 0, live ? frs[i].h : 0, tot};
        tot += a; amax = std::max(amax, a);
    }
}

// Tiles of BF_TY x BF_TX outputs.  Calls with the same filterRect and target rect (the cells of one slot in a slot batch, the planes of a
// whole-image slab batch) share their tiles, up to BF_NPMAX calls per tile.  compact: outputs go to a tile of the target rect's size
// (row stride = its width: the scratch of the one-call operator), otherwise to map / slab coordinates as in les_hip_batch_create.
int build_bf_jobs(const les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, int out_slabs, bool compact,
                  std::vector<les::BfJob>& jobs, int& np_max)
{
    jobs.clear();
    np_max = 1;
    const long long P = (long long)c->p.H * c->p.W;
    std::vector<int> order;
    for (int i = 0; i < n; i++) {
        int rc = check_rects(c, frs[i], trs[i]);
        if (rc) return rc;
        if (trs[i].w > 0 && trs[i].h > 0) order.push_back(i);
    }
    auto key = [&](int i) { return std::array<int, 8>{frs[i].x, frs[i].y, frs[i].w, frs[i].h, trs[i].x, trs[i].y, trs[i].w, trs[i].h}; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
    for (size_t g0 = 0; g0 < order.size();) {
        size_t g1 = g0 + 1;
        while (g1 < order.size() && g1 - g0 < (size_t)les::BF_NPMAX && key(order[g1]) == key(order[g0])) g1++;
        const les_hip_rect &f = frs[order[g0]], &t = trs[order[g0]];
        const int np = (int)(g1 - g0);
        np_max = std::max(np_max, np);
        for (int sy = 0; sy < t.h; sy += les::BF_TY)
            for (int sx = 0; sx < t.w; sx += les::BF_TX) {
                les::BfJob j = {};
                j.tx0 = t.x + sx; j.ty0 = t.y + sy;
                j.tw = std::min(les::BF_TX, t.w - sx); j.th = std::min(les::BF_TY, t.h - sy);
                j.fx = f.x; j.fy = f.y; j.fw = f.w; j.fh = f.h;
                j.np = np;
                j.out_stride = compact ? t.w : c->p.W;
                for (int k = 0; k < les::BF_NPMAX; k++) {
                    const int i = order[g0 + std::min<size_t>(k, np - 1)];
                    j.call[k] = i;
                    j.out_off[k] = compact ? (long long)sy * t.w + sx
                                           : (out_slabs ? (long long)(i / out_slabs) * P : 0) + (long long)j.ty0 * c->p.W + j.tx0;
                }
                jobs.push_back(j);
            }
        g0 = g1;
    }
    return LES_HIP_OK;
}

int bf_view_ok(const les_hip_ctx* c, int mode)
{
    if (mode < 0 || mode > 1 || !c->v[mode].ipk || (c->naive ? !c->v[1 - mode].feat : !c->v[mode].vol))
        return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    return LES_HIP_OK;
}

// raw-cost pre-pass of every call, then the aggregation (both on `stream`)
int launch_bf(les_hip_ctx* c, int mode, const les::BfJob* d_jobs, int njobs, int np, const les::RawCall* d_calls, int ncalls, int chunks,
              float* d_raw, const float4* d_planes, float* d_out, int check, hipStream_t stream)
{
    int rc = bf_view_ok(c, mode);
    if (rc) return rc;
    if (njobs <= 0) return LES_HIP_OK;
    if (c->naive)
        launch_naive_raw(c, mode, d_calls, ncalls, chunks, d_planes, d_raw, stream);          // (honours Plane::v: les_vdisp.h)
    else if (c->interp == 0)
        hipLaunchKernelGGL(les::les_interp_raw_kernel<0>, dim3(ncalls, chunks), dim3(256), 0, stream, c->geom, (const float*)c->v[mode].vol, d_calls, d_planes, d_raw,
                           (unsigned*)nullptr, 0.0f);
    else if (c->interp == 2)
        hipLaunchKernelGGL(les::les_interp_raw_kernel<2>, dim3(ncalls, chunks), dim3(256), 0, stream, c->geom, (const float*)c->v[mode].vol, d_calls, d_planes, d_raw,
                           (unsigned*)nullptr, 0.0f);
    else
        hipLaunchKernelGGL(les::les_bf_volume_raw_kernel, dim3(ncalls, chunks), dim3(256), 0, stream, c->geom, (const float*)c->v[mode].vol, d_calls, d_planes, d_raw);
    HIPCHECK(hipGetLastError());
    if (np > 1)
        hipLaunchKernelGGL(les::les_bf_kernel<les::BF_NPMAX>, dim3(njobs), dim3(les::BF_NT), 0, stream, c->geom, (const uint32_t*)c->v[mode].ipk,
                           (const float*)c->d_bf_tab, d_jobs, d_calls, d_planes, (const float*)d_raw, d_out, c->R, njobs, check);
    else
        hipLaunchKernelGGL(les::les_bf_kernel<1>, dim3(njobs), dim3(les::BF_NT), 0, stream, c->geom, (const uint32_t*)c->v[mode].ipk,
                           (const float*)c->d_bf_tab, d_jobs, d_calls, d_planes, (const float*)d_raw, d_out, c->R, njobs, check);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

// les_hip_batch_create's part for a bilateral / unfiltered context: tiles and raw-cost patch table (the patch buffers are allocated on a
// view's first run, as for the image-based energy on the march kernel)
int build_bf_batch(les_hip_ctx* c, les_hip_batch* b, int n, const les_hip_rect* frs, const les_hip_rect* trs, int out_slabs)
{
    std::vector<les::BfJob> jobs;
    int rc = build_bf_jobs(c, n, frs, trs, out_slabs, false, jobs, b->bf_np);
    if (rc) return rc;
    std::vector<les::RawCall> calls;
    long long tot = 0, amax = 1;
    build_bf_raw_calls(n, frs, trs, calls, tot, amax);
    if (tot > kRawPatchCapFloats)
        return fail(LES_HIP_ERR_UNSUPPORTED, "the raw-cost patches of one batch exceed 4 GB (%lld floats): split the batch", tot);
    b->raw_floats = tot;
    b->raw_chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
    b->njobs = (int)jobs.size();
    if (n > 0) {
        HIPCHECK(hipMalloc((void**)&b->d_rawcalls, (size_t)n * sizeof(les::RawCall)));
        HIPCHECK(hipMemcpy(b->d_rawcalls, calls.data(), (size_t)n * sizeof(les::RawCall), hipMemcpyHostToDevice));
    }
    if (!jobs.empty()) {
        HIPCHECK(hipMalloc((void**)&b->d_bfjobs, jobs.size() * sizeof(les::BfJob)));
        HIPCHECK(hipMemcpy(b->d_bfjobs, jobs.data(), jobs.size() * sizeof(les::BfJob), hipMemcpyHostToDevice));
    }
    return LES_HIP_OK;
}

int run_bf_batch(les_hip_ctx* c, const les_hip_batch* b, int mode, const float4* d_planes, float* out_dev, int check)
{
    int rc = bf_view_ok(c, mode);
    if (rc) return rc;
    if (b->njobs == 0) return LES_HIP_OK;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!b->d_raw[mode]) HIPCHECK(hipMalloc((void**)&b->d_raw[mode], (size_t)std::max<long long>(b->raw_floats, 1) * sizeof(float)));
    }
    return launch_bf(c, mode, b->d_bfjobs, b->njobs, b->bf_np, b->d_rawcalls, b->n, b->raw_chunks, b->d_raw[mode], d_planes, out_dev, check, cur_stream(c));
}

// les_hip_unary_one_scratch for a bilateral / unfiltered context: the scratch keeps the tiles and the one-entry patch table of the last
// rect pair, its raw-cost patch and its output tile
int bf_unary_one(les_hip_ctx* c, les_hip_scratch* s, int mode, const les_hip_rect* fr, const les_hip_rect* tr, const les_hip_plane* plane,
                 float* costs, int row_stride, int check)
{
    int rc = bf_view_ok(c, mode);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(c->p.device));
    rc = check_rects(c, *fr, *tr);
    if (rc) return rc;
    if (tr->w <= 0 || tr->h <= 0) return LES_HIP_OK;
    if (memcmp(&s->bf_f, fr, sizeof *fr) || memcmp(&s->bf_t, tr, sizeof *tr)) {
        std::vector<les::BfJob> jobs;
        int np = 1;
        rc = build_bf_jobs(c, 1, fr, tr, 0, true, jobs, np);
        if (rc) return rc;
        HIPCHECK(hipStreamSynchronize(s->stream));
        if (jobs.size() > s->bf_cap) {
            if (s->d_bfjobs) HIPCHECK(hipFree(s->d_bfjobs));
            s->d_bfjobs = nullptr; s->bf_cap = 0;
            HIPCHECK(hipMalloc((void**)&s->d_bfjobs, jobs.size() * sizeof(les::BfJob)));
            s->bf_cap = jobs.size();
        }
        HIPCHECK(hipMemcpy(s->d_bfjobs, jobs.data(), jobs.size() * sizeof(les::BfJob), hipMemcpyHostToDevice));
        const size_t rneed = (size_t)fr->w * fr->h;
        if (rneed > s->raw_cap) {
            if (s->d_raw) HIPCHECK(hipFree(s->d_raw));
            s->d_raw = nullptr; s->raw_cap = 0;
            const size_t cap = std::max(rneed, (size_t)256 * 256);
            HIPCHECK(hipMalloc((void**)&s->d_raw, cap * sizeof(float)));
            s->raw_cap = cap;
        }
        if (!s->d_rawcall) HIPCHECK(hipMalloc((void**)&s->d_rawcall, sizeof(les::RawCall)));
        const les::RawCall call{fr->x, fr->y, fr->w, fr->h, 0};
        HIPCHECK(hipMemcpy(s->d_rawcall, &call, sizeof call, hipMemcpyHostToDevice));
        s->raw_f = les_hip_rect{-1, -1, -1, -1};           // (the guided filter's patch table of this scratch is stale now)
        s->bf_f = *fr; s->bf_t = *tr; s->bf_njobs = (int)jobs.size();
    }
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
    const int chunks = (int)std::min<size_t>(1024, std::max<size_t>(1, ((size_t)fr->w * fr->h + 4095) / 4096));
    rc = launch_bf(c, mode, s->d_bfjobs, s->bf_njobs, 1, s->d_rawcall, 1, chunks, s->d_raw, s->d_plane, s->d_tile, check, s->stream);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(s->h_tile, s->d_tile, need * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHECK(hipStreamSynchronize(s->stream));
    float* dst = costs + (size_t)(tr->y - fr->y) * row_stride + (tr->x - fr->x);
    for (int y = 0; y < tr->h; y++) memcpy(dst + (size_t)y * row_stride, s->h_tile + (size_t)y * tr->w, (size_t)tr->w * sizeof(float));
    return LES_HIP_OK;
}
