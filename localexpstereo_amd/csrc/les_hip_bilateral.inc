// les_hip_bilateral.inc -- part of the single translation unit les_hip.hip (inside its anonymous namespace): the joint bilateral ("BF") and
// the unfiltered ("") aggregation of contexts made by les_hip_create_filtered / les_hip_create_naive_filtered -- per-view set-up, weight
// table, tiles and launch of csrc/les_bilateral.h.  Batches and single calls reach launch_bf through run_unary (les_hip_unary.inc), with
// the tiles and raw-cost patch table of their UnaryTables.  Guided-filter contexts never launch this file's kernels.

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
    DevBuf<uint8_t> img;                  // freed on every return below
    const int rc = img.alloc(P * 3);
    if (rc) return rc;
    const uint8_t* d_img = img.p;
    HIPCHECK(hipMemcpy(img.p, im, P * 3, hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc((void**)&v.ipk, P * sizeof(uint32_t)));
    HIPCHECK(hipMalloc((void**)&v.ipk10, P * sizeof(uint32_t)));
    if (c->naive) {
        HIPCHECK(hipMalloc((void**)&v.feat, P * sizeof(float4)));
        hipLaunchKernelGGL(les::les_naive_features_kernel, dim3((c->p.W + 255) / 256, c->p.H), dim3(256), 0, cur_stream(c), d_img, v.feat, c->p.H, c->p.W, naive_alpha(c));
    }
    hipLaunchKernelGGL(les::les_pack_guide_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, cur_stream(c), d_img, v.ipk, v.ipk10, (int)P);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

// w[s] = exp(-s / sig2) for s = |dI|_1 = 0 .. 765, in double, stored as float (BilateralFilter::filter: cv::exp(-channelSum(w) / sig2),
// LES/GuidedFilter.h:366).  The unfiltered context gets the same table; it only ever reads w[0] = 1.
int build_bf_table(les_hip_ctx* c)
{
    std::vector<float> tab(les::kBfTabSize);
    const double sig2 = c->filter == LES_HIP_FILTER_BILATERAL ? c->p.eps : 1.0;
    for (int s = 0; s < les::kBfTabSize; s++) tab[s] = (float)std::exp(-(double)s / sig2);
    const int rc = c->d_bf_tab.alloc(tab.size());
    if (rc) return rc;
    HIPCHECK(hipMemcpy(c->d_bf_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return LES_HIP_OK;
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

// The views a call of view `mode` reads were supplied at creation (every filter: each view's packed guide is built with it)
int view_ok(const les_hip_ctx* c, int mode)
{
    if (mode < 0 || mode > 1 || !c->v[mode].ipk || (c->naive ? !c->v[1 - mode].feat : !c->v[mode].vol))
        return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    return LES_HIP_OK;
}

// raw-cost pre-pass of every call, then the aggregation (both on `stream`)
int launch_bf(les_hip_ctx* c, int mode, const les::BfJob* d_jobs, int njobs, int np, const les::RawCall* d_calls, int ncalls, int chunks,
              float* d_raw, const float4* d_planes, float* d_out, int check, hipStream_t stream)
{
    int rc = view_ok(c, mode);
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
                           (const float*)c->d_bf_tab.p, d_jobs, d_calls, d_planes, (const float*)d_raw, d_out, c->R, njobs, check);
    else
        hipLaunchKernelGGL(les::les_bf_kernel<1>, dim3(njobs), dim3(les::BF_NT), 0, stream, c->geom, (const uint32_t*)c->v[mode].ipk,
                           (const float*)c->d_bf_tab.p, d_jobs, d_calls, d_planes, (const float*)d_raw, d_out, c->R, njobs, check);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}
