// les_hip_featvol.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): correlation cost volumes from feature maps and the ZNCC patch descriptor (les_featvol.h holds the definitions and the kernels)
namespace {

// LES_HIP_FEATVOL_TIMING=1: each of the two calls brackets its launch with events and waits for it; the calling thread reads the device
// milliseconds of its last descriptor launch and its last volume launch with les_hip_featvol_last_times (tools/featvol_timing.py)
thread_local float tl_fv_ms[2] = {-1.0f, -1.0f};

// launch() between two events when timing is on (then the stream is synchronised and *ms set); plain otherwise
template <typename Launch>
int fv_timed(hipStream_t st, float* ms, Launch launch)
{
#if !defined(LES_SIM)
    if (cv_env_flag("LES_HIP_FEATVOL_TIMING", false)) {
        struct Events {                                    // (destroyed on every return path)
            hipEvent_t e[2] = {nullptr, nullptr};
            ~Events() { for (hipEvent_t q : e) if (q) (void)hipEventDestroy(q); }
        } ev;
        for (hipEvent_t& q : ev.e) HIPCHECK(hipEventCreate(&q));
        HIPCHECK(hipEventRecord(ev.e[0], st));
        launch();
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev.e[1], st));
        HIPCHECK(hipStreamSynchronize(st));
        HIPCHECK(hipEventElapsedTime(ms, ev.e[0], ev.e[1]));
        return LES_HIP_OK;
    }
#endif
    launch();
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_patch_features(const uint8_t* d_bgr, float* d_feat, int H, int W, int ry, int rx, int device, void* stream)
{
    if (!d_bgr || !d_feat || H <= 0 || W <= 0 || ry < 0 || rx < 0) return fail(LES_HIP_ERR_ARG, "les_hip_patch_features: bad argument");
    if (ry > les::kFvMaxRadius || rx > les::kFvMaxRadius)
        return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_patch_features: radii %d x %d (at most %d each)", ry, rx, les::kFvMaxRadius);
    if (H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "image height %d exceeds the launch grid", H);
    HIPCHECK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    return fv_timed(st, &tl_fv_ms[0], [&] {
        hipLaunchKernelGGL(les::les_patch_features_kernel, dim3((W + 255) / 256, H), dim3(256), 0, st, d_bgr, d_feat, H, W, ry, rx);
    });
}

int les_hip_build_feature_volume(const float* d_featL, const float* d_featR, float* d_vol, int C, int D, int H, int W, int mode, int d0, float alpha,
                                 float beta, int device, void* stream)
{
    if (!d_featL || !d_featR || !d_vol || C <= 0 || D <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 1)
        return fail(LES_HIP_ERR_ARG, "les_hip_build_feature_volume: bad argument");
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return fail(LES_HIP_ERR_ARG, "les_hip_build_feature_volume: alpha %g, beta %g (finite)", (double)alpha, (double)beta);
    if ((unsigned long long)D * H * W >= (1ull << 32)) return fail(LES_HIP_ERR_UNSUPPORTED, "volumes of 2^32 or more floats are not supported");
    if (H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "image height %d exceeds the launch grid", H);
    if (C > les::kFvMaxC) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_build_feature_volume: %d channels (at most %d)", C, les::kFvMaxC);
    HIPCHECK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    // mode 0: the left view's pixels against the right view's row; mode 1: the other way round
    const float *fI = mode == 0 ? d_featL : d_featR, *fJ = mode == 0 ? d_featR : d_featL;
    const int nchunk = (D + les::kFvChunk - 1) / les::kFvChunk;
    const dim3 grid((unsigned)((W + les::kFvSeg - 1) / les::kFvSeg) * (unsigned)nchunk, H), block(256);
    const bool vec = (W % 4 == 0) && (((uintptr_t)d_vol & 15) == 0);           // every row of every slice starts 16-byte aligned
    return fv_timed(st, &tl_fv_ms[1], [&] {
        if (vec) hipLaunchKernelGGL((les::les_featvol_kernel<true>), grid, block, 0, st, fI, fJ, d_vol, C, D, H, W, mode, d0, alpha, beta, nchunk);
        else hipLaunchKernelGGL((les::les_featvol_kernel<false>), grid, block, 0, st, fI, fJ, d_vol, C, D, H, W, mode, d0, alpha, beta, nchunk);
    });
}

int les_hip_featvol_last_times(float* features_ms, float* volume_ms)
{
    if (!features_ms || !volume_ms) return fail(LES_HIP_ERR_ARG, "les_hip_featvol_last_times: null argument");
    if (tl_fv_ms[0] < 0.0f && tl_fv_ms[1] < 0.0f)
        return fail(LES_HIP_ERR_ARG, "les_hip_featvol_last_times: this thread has run neither call with LES_HIP_FEATVOL_TIMING=1");
    *features_ms = tl_fv_ms[0];
    *volume_ms = tl_fv_ms[1];
    return LES_HIP_OK;
}

}  // extern "C"
