// les_hip_crossview.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): cross-view fusion's warp of a label map into the other view (les_crossview.h holds the definition and the kernel)
extern "C" {

int les_hip_warp_labels(les_hip_ctx* c, int src_mode, const les_hip_plane* d_src, const les_hip_plane* d_fallback, les_hip_plane* d_out, unsigned char* d_hit)
{
    if (!c || !d_src || !d_fallback || !d_out) return fail(LES_HIP_ERR_ARG, "les_hip_warp_labels: null argument");
    if (src_mode < 0 || src_mode > 1) return fail(LES_HIP_ERR_ARG, "les_hip_warp_labels: src_mode %d (0 left, 1 right)", src_mode);
    if ((const void*)d_out == (const void*)d_src) return fail(LES_HIP_ERR_ARG, "les_hip_warp_labels: d_out may be d_fallback, not d_src");
    const int H = c->p.H, W = c->p.W;
    if (W > les::kWarpMaxW) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_warp_labels: rows of %d pixels, at most %d are supported", W, les::kWarpMaxW);
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    const float sign = src_mode ? -1.0f : 1.0f;
    hipLaunchKernelGGL(les::les_warp_labels_kernel, dim3((unsigned)H), dim3(les::kWarpThreads), 2 * sizeof(uint32_t) * (size_t)W, cur_stream(c),
                       reinterpret_cast<const float4*>(d_src), reinterpret_cast<const float4*>(d_fallback), reinterpret_cast<float4*>(d_out), d_hit, H, W, sign);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
