// les_hip_wtavol.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): winner-take-all labels of the aggregated cost volume (les_wtavol.h holds the definition and the kernels) -- the reduction's two entry points and the whole operation for one view
// What les_hip_wta_labels keeps on its context, built on first use and freed with the context: the K fronto-parallel planes, one prepared batch
// per chunk length seen (n calls with filterRect = targetRect = the image, one slab each), the slab workspace and the reduction's state.
// les_hip_confidence (les_hip_confidence.inc) shares all of it but the state.
struct WtaVol {
    int K = 0; float d0 = 0.0f;                 // what d_planes holds: (0, 0, d0 + k, 0) for k < K
    DevBuf<float4> d_planes;
    std::vector<std::pair<int, les_hip_batch*>> batches;
    DevBuf<float> d_slabs, d_state;
    DevBuf<float> d_conf_state;                 // les_hip_confidence's own state (les_hip_confidence.inc): a confidence call leaves the arg-min's alone
    ~WtaVol() { for (auto& b : batches) les_hip_batch_destroy(b.second); }
};

namespace {

void wtavol_free(WtaVol* w) { delete w; }

int launch_slab_argmin(const float* d_slabs, int n, int k_first, size_t P, float* d_state, hipStream_t stream)
{
    const unsigned grid = (unsigned)(((P + 3) / 4 + les::kArgminThreads - 1) / les::kArgminThreads);
    if ((P & 3) == 0 && ((uintptr_t)d_slabs & 15) == 0)
        hipLaunchKernelGGL(les::les_slab_argmin_kernel<true>, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_slabs, n, k_first, P, d_state);
    else
        hipLaunchKernelGGL(les::les_slab_argmin_kernel<false>, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_slabs, n, k_first, P, d_state);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int launch_slab_argmin_finish(const float* d_state, size_t P, int K, int subpixel, float d0, float4* d_labels, float* d_cost, hipStream_t stream)
{
    const unsigned grid = (unsigned)((P + les::kArgminThreads - 1) / les::kArgminThreads);
    hipLaunchKernelGGL(les::les_slab_argmin_finish_kernel, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_state, P, K, subpixel, d0, d_labels, d_cost);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

// the prepared batch of n whole-image calls (created once per n)
int wtavol_batch(les_hip_ctx* c, WtaVol* w, int n, les_hip_batch** out)
{
    for (auto& b : w->batches)
        if (b.first == n) { *out = b.second; return LES_HIP_OK; }
    const std::vector<les_hip_rect> rects((size_t)n, les_hip_rect{0, 0, c->p.W, c->p.H});
    int rc = les_hip_batch_create(c, n, rects.data(), rects.data(), 1, out);
    if (rc) return rc;
    w->batches.emplace_back(n, *out);
    return LES_HIP_OK;
}

// K = int(max_disparity - min_disparity) + 1, or the refusal of a range that is negative, NaN or 65536 and more
int wtavol_range(const les_hip_ctx* c, const char* who, int* K)
{
    const float range = c->p.max_disparity - c->p.min_disparity;
    if (!(range >= 0.0f) || range >= 65536.0f) return fail(LES_HIP_ERR_ARG, "%s: disparity range [%g, %g]", who, (double)c->p.min_disparity, (double)c->p.max_disparity);
    *K = (int)range + 1;
    return LES_HIP_OK;
}

// What les_hip_wta_labels and les_hip_confidence share, on the calling thread's stream: the disparity range checked (*K planes), *chunk resolved
// (<= 0: 32; clamped to K), the context's WtaVol with its K planes uploaded and its slab workspace grown to *chunk slabs.  Launches nothing.
int wtavol_prepare(les_hip_ctx* c, const char* who, int* chunk, int* Kout)
{
    int K = 0;
    int rc = wtavol_range(c, who, &K);
    if (rc) return rc;
    const float d0 = c->p.min_disparity;
    if (*chunk <= 0) *chunk = 32;
    *chunk = std::min(*chunk, K);
    hipStream_t stream = cur_stream(c);
    const size_t P = (size_t)c->p.H * c->p.W;
    if (!c->wtavol) c->wtavol = new WtaVol();
    WtaVol* w = c->wtavol;
    if (w->K != K || w->d0 != d0) {
        std::vector<float4> planes((size_t)K);
        for (int k = 0; k < K; k++) planes[(size_t)k] = make_float4(0.0f, 0.0f, d0 + (float)k, 0.0f);
        if ((rc = w->d_planes.grow((size_t)K, 0, stream))) return rc;
        HIPCHECK(hipStreamSynchronize(stream));              // (an earlier call's launches may still read the old planes)
        HIPCHECK(hipMemcpy(w->d_planes.p, planes.data(), (size_t)K * sizeof(float4), hipMemcpyHostToDevice));
        w->K = K; w->d0 = d0;
    }
    if ((rc = w->d_slabs.grow((size_t)*chunk * P, 0, stream))) return rc;
    *Kout = K;
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

size_t les_hip_slab_argmin_state_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return les::kArgminStatePlanes * les::argmin_plane_words((size_t)H * W) * sizeof(float);
}

int les_hip_slab_argmin(les_hip_ctx* c, const float* d_slabs, int n, int k_first, void* d_state)
{
    if (!c || !d_slabs || !d_state) return fail(LES_HIP_ERR_ARG, "les_hip_slab_argmin: null argument");
    if (n < 0 || k_first < 0 || n > INT32_MAX - k_first) return fail(LES_HIP_ERR_ARG, "les_hip_slab_argmin: n %d, k_first %d", n, k_first);
    if ((uintptr_t)d_state & 15) return fail(LES_HIP_ERR_ARG, "les_hip_slab_argmin: d_state must be 16-byte aligned");
    if (n == 0 && k_first > 0) return LES_HIP_OK;
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    return launch_slab_argmin(d_slabs, n, k_first, (size_t)c->p.H * c->p.W, static_cast<float*>(d_state), cur_stream(c));
}

int les_hip_slab_argmin_finish(les_hip_ctx* c, const void* d_state, int K, int subpixel, les_hip_plane* d_labels, float* d_cost)
{
    if (!c || !d_state || !d_labels || !d_cost) return fail(LES_HIP_ERR_ARG, "les_hip_slab_argmin_finish: null argument");
    if (K < 0) return fail(LES_HIP_ERR_ARG, "les_hip_slab_argmin_finish: K %d", K);
    (void)hipSetDevice(c->p.device);
    return launch_slab_argmin_finish(static_cast<const float*>(d_state), (size_t)c->p.H * c->p.W, K, subpixel, c->p.min_disparity,
                                     reinterpret_cast<float4*>(d_labels), d_cost, cur_stream(c));
}

int les_hip_wta_labels(les_hip_ctx* c, int mode, int chunk, int subpixel, les_hip_plane* d_labels, float* d_cost)
{
    if (!c || !d_labels || !d_cost) return fail(LES_HIP_ERR_ARG, "les_hip_wta_labels: null argument");
    int rc = view_ok(c, mode);
    if (rc) return rc;
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    int K = 0;
    if ((rc = wtavol_prepare(c, "les_hip_wta_labels", &chunk, &K))) return rc;
    const float d0 = c->p.min_disparity;
    hipStream_t stream = cur_stream(c);
    const size_t P = (size_t)c->p.H * c->p.W;
    WtaVol* w = c->wtavol;
    if ((rc = w->d_state.grow(les::kArgminStatePlanes * les::argmin_plane_words(P), 0, stream))) return rc;
    const float4* d_planes = w->d_planes.p;
    float* d_slabs = w->d_slabs.p;
    float* d_state = w->d_state.p;
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int n = std::min(chunk, K - k0);
        les_hip_batch* b = nullptr;
        if ((rc = wtavol_batch(c, w, n, &b))) return rc;
        if ((rc = run_unary(c, b->tab, b->ws, mode, d_planes + k0, d_slabs, 0, stream))) return rc;
        if ((rc = launch_slab_argmin(d_slabs, n, k0, P, d_state, stream))) return rc;
    }
    return launch_slab_argmin_finish(d_state, P, K, subpixel, d0, reinterpret_cast<float4*>(d_labels), d_cost, stream);
}

}  // extern "C"
