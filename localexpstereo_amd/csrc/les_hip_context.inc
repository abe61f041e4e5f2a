// les_hip_context.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): context life cycle, streams, volume refresh, device-memory helpers, calibration copies of the C ABI (include/localexp_hip.h)
extern "C" {

const char* les_hip_last_error(void) { return g_err.c_str(); }

#if defined(LES_PHASE_TIMING)
int les_hip_debug_phases(unsigned long long* out)          // experiment builds only (tools/phase_probe.py); not part of the ABI header
{
    (void)hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(les::les_dbg), 12 * sizeof(unsigned long long)) != hipSuccess) return 1;
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(les::les_dbg), z, sizeof z);
    return 0;
}
#endif

int les_hip_strip_width(int R)
{
    const StripEntry* e = find_strip(R);
    return e ? e->TW : 0;
}

static int create_common(les_hip_ctx** out, const les_hip_params* params, const uint8_t* imL, const uint8_t* imR,
                         const float* volL, const float* volR, int naive, float alpha, float th_grad, int filter = LES_HIP_FILTER_GF)
{
    if (!out || !params) return fail(LES_HIP_ERR_ARG, "null argument");
    *out = nullptr;
    les_hip_params p = *params;
    if (naive) { p.D = 1; p.volumes_on_device = 0; }
    const bool gf = filter == LES_HIP_FILTER_GF;
    if (!gf && filter != LES_HIP_FILTER_BILATERAL && filter != LES_HIP_FILTER_NONE) return fail(LES_HIP_ERR_ARG, "unknown filter %d", filter);
    if (p.H <= 0 || p.W <= 0 || p.D <= 0 || p.windR < (gf ? 2 : 0)) return fail(LES_HIP_ERR_ARG, "bad dimensions");
    if (filter == LES_HIP_FILTER_BILATERAL && p.windR > les::kBfMaxR)
        return fail(LES_HIP_ERR_UNSUPPORTED, "bilateral filter radius windR = %d (supported: 0 .. %d)", p.windR, les::kBfMaxR);
    if (filter == LES_HIP_FILTER_BILATERAL && !(p.eps > 0.0)) return fail(LES_HIP_ERR_ARG, "the bilateral filter needs sig2 = eps > 0 (got %g)", p.eps);
    if (naive && (!imL || !imR)) return fail(LES_HIP_ERR_ARG, "the image-based matching cost needs both views");
    if ((unsigned long long)p.H * p.W * p.D >= (1ull << 32)) return fail(LES_HIP_ERR_UNSUPPORTED, "volumes of 2^32 or more floats are not supported (32-bit element offsets)");
    const StripEntry* strip = !gf ? nullptr : naive ? find_naive_strip(p.windR / 2) : find_strip(p.windR / 2);
    if (gf && !strip) return fail(LES_HIP_ERR_UNSUPPORTED, "no kernel instantiated for guided-filter radius %d (windR %d)", p.windR / 2, p.windR);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(LES_HIP_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (p.device < 0 || p.device >= ndev) return fail(LES_HIP_ERR_ARG, "device %d out of range (%d devices)", p.device, ndev);
    HIPCHECK(hipSetDevice(p.device));
    les_hip_ctx* c = new les_hip_ctx();
    c->gen = ++g_ctx_gen;
    { std::lock_guard<std::mutex> lk(g_live_mu); g_live.emplace_back(c->gen, c); }
    c->p = p;
    c->filter = filter;
    c->R = gf ? p.windR / 2 : (filter == LES_HIP_FILTER_BILATERAL ? p.windR : 0);
    c->strip = strip;
    if (gf && !naive)
        for (int k = 0; k < 2; k++) {
            const StripEntry* e = find_interp_strip(p.windR / 2, k == 0 ? 0 : 2);
            c->istrip[k] = e && e->TW >= strip->TW ? e : nullptr;       // (the job tables are cut for c->strip's width)
        }
    c->march = gf ? find_march(p.windR / 2) : nullptr;
    if (gf && !c->march && !(getenv("LES_HIP_KERNEL") && !strcmp(getenv("LES_HIP_KERNEL"), "strip")))
        note_fallback(c->fallback_seen, FB_RADIUS, "no march kernel for guided-filter radius %d (windR %d; instantiated: 2 .. 10)", p.windR / 2, p.windR);
#if !defined(LES_SIM)
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, p.device) == hipSuccess && v > 0) c->ncu = v;
    }
#endif
    c->stream = nullptr;
    c->geom.H = p.H; c->geom.W = p.W; c->geom.D = p.D;
    c->geom.D0 = (int)(-p.min_disparity);                       // LES/CostVolumeEnergy.h:67
    c->geom.th_col = p.th_col; c->geom.pad_ = 0.0f;
    c->geom.maxd = p.max_disparity; c->geom.mind = p.min_disparity;
    c->naive = naive;
    if (naive) {
        c->th_color = p.th_col * (1.0f - alpha);                 // LES/StereoEnergy.h:662
        c->th_grad = th_grad * alpha;                            // LES/StereoEnergy.h:663
        c->naive_alpha = alpha;
        c->naive_th_grad = th_grad;
    }
    const uint8_t* ims[2] = {imL, imR};
    const float* vols[2] = {volL, volR};
    for (int m = 0; m < 2; m++) {
        int rc = gf ? build_view(c, m, ims[m], vols[m]) : build_bf_view(c, m, ims[m], vols[m]);
        if (rc) { les_hip_destroy(c); return rc; }
    }
    if (!gf) {
        int rc = build_bf_table(c);
        if (rc) { les_hip_destroy(c); return rc; }
    }
    if (c->d_map.alloc((size_t)p.H * p.W)) {
        les_hip_destroy(c);
        return fail(LES_HIP_ERR_DEVICE, "hipMalloc of the scratch cost map failed");
    }
    *out = c;
    return LES_HIP_OK;
}

int les_hip_create(les_hip_ctx** out, const les_hip_params* params, const uint8_t* imL, const uint8_t* imR,
                   const float* volL, const float* volR)
{
    return create_common(out, params, imL, imR, volL, volR, 0, 0.0f, 0.0f);
}

int les_hip_create_naive(les_hip_ctx** out, const les_hip_params* params, const uint8_t* imL, const uint8_t* imR, float alpha, float th_grad)
{
    return create_common(out, params, imL, imR, nullptr, nullptr, 1, alpha, th_grad);
}

int les_hip_create_filtered(les_hip_ctx** out, const les_hip_params* params, int filter, const uint8_t* imL, const uint8_t* imR,
                            const float* volL, const float* volR)
{
    return create_common(out, params, imL, imR, volL, volR, 0, 0.0f, 0.0f, filter);
}

int les_hip_create_naive_filtered(les_hip_ctx** out, const les_hip_params* params, int filter, const uint8_t* imL, const uint8_t* imR,
                                  float alpha, float th_grad)
{
    return create_common(out, params, imL, imR, nullptr, nullptr, 1, alpha, th_grad, filter);
}

void les_hip_destroy(les_hip_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (tl_stream_gen == c->gen) { tl_stream_gen = 0; tl_stream = nullptr; }     // the destroying thread's own binding (other threads' bindings die with the id)
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.erase(std::remove_if(g_live.begin(), g_live.end(), [c](const std::pair<unsigned long long, les_hip_ctx*>& e) { return e.second == c; }), g_live.end());
    }
    for (les_hip_scratch* sc : c->own_scratch) les_hip_scratch_destroy(sc);
    c->own_scratch.clear();
    for (MtHost* m : c->mt_idle) mt_host_free(m);
    c->mt_idle.clear();
    wtavol_free(c->wtavol);                                     // (its batches go before the context they were prepared on)
    c->wtavol = nullptr;
    sgm_free(c->sgm);
    c->sgm = nullptr;
    fit_tables_free(c->fit_tables);
    c->fit_tables = nullptr;
    delete c;                                                   // the views' buffers and every owned table
}

int les_hip_set_stream(les_hip_ctx* c, void* s)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    c->stream = (hipStream_t)s;
    return LES_HIP_OK;
}

int les_hip_set_thread_stream(les_hip_ctx* c, void* s, int bind)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    if (bind) { tl_stream_gen = c->gen; tl_stream = (hipStream_t)s; }
    else if (tl_stream_gen == c->gen) { tl_stream_gen = 0; tl_stream = nullptr; }
    return LES_HIP_OK;
}

int les_hip_synchronize(les_hip_ctx* c)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

int les_hip_refresh_volume(les_hip_ctx* c, int mode)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null argument");
    if (mode < 0 || mode > 1 || !c->v[mode].vol) return fail(LES_HIP_ERR_ARG, "view %d has no cost volume", mode);
    HIPCHECK(hipSetDevice(c->p.device));
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    if (!c->march || !c->v[mode].mstats) return LES_HIP_OK;          // radius without a march kernel / image too large for it: the strip kernel keeps nothing derived from the volume
    const int rc = build_march_view(c, mode, nullptr);             // cost range -> fixed-point scales, tiled copy rebuilt; the guide's tables stay
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

int les_hip_set_interpolation(les_hip_ctx* c, int none_lin_quad)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    if (c->naive) return fail(LES_HIP_ERR_ARG, "the image-based energy has no cost volume to interpolate");
    if (none_lin_quad < 0 || none_lin_quad > 2) return fail(LES_HIP_ERR_ARG, "interpolation %d (0: nearest, 1: linear, 2: quadratic)", none_lin_quad);
    c->interp = none_lin_quad;
    return LES_HIP_OK;
}

int les_hip_set_max_vdisparity(les_hip_ctx* c, float max_vdisp)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    if (!(max_vdisp >= 0.0f) || max_vdisp == INFINITY) return fail(LES_HIP_ERR_ARG, "MAX_VDISPARITY %g (a finite value >= 0)", (double)max_vdisp);
    c->max_vdisp = max_vdisp;
    return LES_HIP_OK;
}

int les_hip_set_random_vdisparity(les_hip_ctx* c, float max_vdisp)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null context");
    if (!(max_vdisp >= 0.0f) || max_vdisp == INFINITY) return fail(LES_HIP_ERR_ARG, "maxVDisp %g (a finite value >= 0)", (double)max_vdisp);
    c->random_vdisp = max_vdisp;
    return LES_HIP_OK;
}

int les_hip_calib_copy(const float* d_src, float* d_dst, size_t n, int device, void* stream)
{
    if (!d_src || !d_dst || n == 0) return fail(LES_HIP_ERR_ARG, "bad argument");
    HIPCHECK(hipSetDevice(device));
    hipLaunchKernelGGL(les::les_calib_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_src, d_dst, n);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_calib_copy_wide(const float* d_src, float* d_dst, size_t n, int device, void* stream)
{
    if (!d_src || !d_dst || n == 0 || (n & 3) || (((uintptr_t)d_src | (uintptr_t)d_dst) & 15)) return fail(LES_HIP_ERR_ARG, "bad argument (n must be a multiple of 4, pointers 16-byte aligned)");
    HIPCHECK(hipSetDevice(device));
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(les::les_calib_copy_wide_kernel, dim3((unsigned)((n4 + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(d_src), reinterpret_cast<float4*>(d_dst), n4);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_malloc(les_hip_ctx* c, void** p, size_t bytes)
{
    if (!c || !p) return fail(LES_HIP_ERR_ARG, "null argument");
    HIPCHECK(hipMalloc(p, bytes));
    return LES_HIP_OK;
}
int les_hip_free(les_hip_ctx* c, void* p)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null argument");
    if (p) HIPCHECK(hipFree(p));
    return LES_HIP_OK;
}
int les_hip_memcpy_h2d(les_hip_ctx* c, void* d, const void* s, size_t bytes)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null argument");
    HIPCHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}
int les_hip_memcpy_d2h(les_hip_ctx* c, void* d, const void* s, size_t bytes)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null argument");
    HIPCHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}
int les_hip_memset(les_hip_ctx* c, void* d, int value, size_t bytes)
{
    if (!c) return fail(LES_HIP_ERR_ARG, "null argument");
    HIPCHECK(hipMemsetAsync(d, value, bytes, cur_stream(c)));
    return LES_HIP_OK;
}

size_t les_hip_tiled_volume_bytes(les_hip_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 1 || !c->v[mode].vol_t) return 0;
    return (size_t)c->p.H * (size_t)((c->p.W + 7) / 8) * 8u * (size_t)c->p.D * sizeof(float);
}

int les_hip_get_stats(les_hip_ctx* c, int mode, float* out)
{
    if (!c || !out || mode < 0 || mode > 1 || !c->v[mode].stats) return fail(LES_HIP_ERR_ARG, "bad argument");
    HIPCHECK(hipMemcpy(out, c->v[mode].stats, (size_t)c->p.H * c->p.W * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return LES_HIP_OK;
}

}  // extern "C"
