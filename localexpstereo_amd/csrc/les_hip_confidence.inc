// les_hip_confidence.inc -- part of the single translation unit les_hip.hip (included there, after les_hip_wtavol.inc; not compiled on its own): the confidence of a label map under the aggregated cost volume (les_confidence.h holds the definition and the kernels) -- the reduction's two entry points and the whole operation for one view
namespace {

int launch_slab_confidence(const float4* d_labels, const float* d_slabs, int n, int k_first, size_t P, int W, float d0, float band, float* d_state,
                           hipStream_t stream)
{
    const unsigned grid = (unsigned)(((P + 3) / 4 + les::kArgminThreads - 1) / les::kArgminThreads);
    if ((P & 3) == 0 && ((uintptr_t)d_slabs & 15) == 0)
        hipLaunchKernelGGL(les::les_slab_confidence_kernel<true>, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_labels, d_slabs, n, k_first, P, W, d0, band, d_state);
    else
        hipLaunchKernelGGL(les::les_slab_confidence_kernel<false>, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_labels, d_slabs, n, k_first, P, W, d0, band, d_state);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int launch_slab_confidence_finish(const float* d_state, size_t P, float scale, float* d_conf, float* d_own, float* d_rival, int* d_krival, hipStream_t stream)
{
    const unsigned grid = (unsigned)((P + les::kArgminThreads - 1) / les::kArgminThreads);
    hipLaunchKernelGGL(les::les_slab_confidence_finish_kernel, dim3(grid), dim3(les::kArgminThreads), 0, stream, d_state, P, scale, d_conf, d_own, d_rival, d_krival);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

bool conf_band_ok(float band) { return band >= 0.0f; }                                   // (false for NaN)
bool conf_scale_ok(float scale) { return scale > 0.0f && scale < __builtin_inff(); }     // (false for NaN)

}  // namespace

extern "C" {

size_t les_hip_slab_confidence_state_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return les::kConfStatePlanes * les::argmin_plane_words((size_t)H * W) * sizeof(float);
}

int les_hip_slab_confidence(les_hip_ctx* c, const les_hip_plane* d_labels, const float* d_slabs, int n, int k_first, float band, void* d_state)
{
    if (!c || !d_slabs || !d_state || (k_first == 0 && !d_labels)) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence: null argument");
    if (n < 0 || k_first < 0 || n > INT32_MAX - k_first) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence: n %d, k_first %d", n, k_first);
    if (!conf_band_ok(band)) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence: band %g (>= 0)", (double)band);
    if ((uintptr_t)d_state & 15) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence: d_state must be 16-byte aligned");
    if (n == 0 && k_first > 0) return LES_HIP_OK;
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    return launch_slab_confidence(reinterpret_cast<const float4*>(d_labels), d_slabs, n, k_first, (size_t)c->p.H * c->p.W, c->p.W, c->p.min_disparity, band,
                                  static_cast<float*>(d_state), cur_stream(c));
}

int les_hip_slab_confidence_finish(les_hip_ctx* c, const void* d_state, float scale, float* d_conf, float* d_own, float* d_rival, int* d_krival)
{
    if (!c || !d_state || !d_conf) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence_finish: null argument");
    if (!conf_scale_ok(scale)) return fail(LES_HIP_ERR_ARG, "les_hip_slab_confidence_finish: scale %g (positive and finite)", (double)scale);
    (void)hipSetDevice(c->p.device);
    return launch_slab_confidence_finish(static_cast<const float*>(d_state), (size_t)c->p.H * c->p.W, scale, d_conf, d_own, d_rival, d_krival, cur_stream(c));
}

int les_hip_confidence(les_hip_ctx* c, int mode, const les_hip_plane* d_labels, int chunk, float band, float scale, float* d_conf, float* d_own,
                       float* d_rival, int* d_krival)
{
    if (!c || !d_labels || !d_conf) return fail(LES_HIP_ERR_ARG, "les_hip_confidence: null argument");
    int rc = view_ok(c, mode);
    if (rc) return rc;
    if (!conf_band_ok(band)) return fail(LES_HIP_ERR_ARG, "les_hip_confidence: band %g (>= 0)", (double)band);
    if (!conf_scale_ok(scale)) return fail(LES_HIP_ERR_ARG, "les_hip_confidence: scale %g (positive and finite)", (double)scale);
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    int K = 0;
    if ((rc = wtavol_prepare(c, "les_hip_confidence", &chunk, &K))) return rc;
    hipStream_t stream = cur_stream(c);
    const size_t P = (size_t)c->p.H * c->p.W;
    WtaVol* w = c->wtavol;
    if ((rc = w->d_conf_state.grow(les::kConfStatePlanes * les::argmin_plane_words(P), 0, stream))) return rc;
    const float4* d_planes = w->d_planes.p;
    float* d_slabs = w->d_slabs.p;
    float* d_state = w->d_conf_state.p;
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int n = std::min(chunk, K - k0);
        les_hip_batch* b = nullptr;
        if ((rc = wtavol_batch(c, w, n, &b))) return rc;
        if ((rc = run_unary(c, b->tab, b->ws, mode, d_planes + k0, d_slabs, 0, stream))) return rc;
        if ((rc = launch_slab_confidence(reinterpret_cast<const float4*>(d_labels), d_slabs, n, k0, P, c->p.W, c->p.min_disparity, band, d_state, stream))) return rc;
    }
    return launch_slab_confidence_finish(d_state, P, scale, d_conf, d_own, d_rival, d_krival, stream);
}

}  // extern "C"
