// les_hip_sgm.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): semi-global matching over a view's cost volume (les_sgm.h holds the definition and the kernels) -- the workspace, the launches and the two entry points
// What les_hip_sgm_labels keeps on its context, built on first use, regrown when the disparity range grows, freed with the context: Ct and S,
// [H][W][Kp] floats each
struct SgmWork {
    DevBuf<float> ws;
};

namespace {

void sgm_free(SgmWork* w) { delete w; }

constexpr int kSgmDirs[8][2] = {{+1, 0}, {-1, 0}, {0, +1}, {0, -1}, {+1, +1}, {-1, -1}, {-1, +1}, {+1, -1}};

// LES_HIP_SGM_TIMING=1: the call brackets every kernel with events and waits for the last one; the calling thread reads the device milliseconds of
// its last call with les_hip_sgm_last_times (tools/sgm_timing.py): transpose, one per direction, read-out
constexpr int kSgmMaxTimes = 10;
thread_local float tl_sgm_ms[kSgmMaxTimes];
thread_local int tl_sgm_n = -1;

// Whether les_hip_sgm_labels serves the context: K of its disparity range, or the error code of the refusal (*K untouched).  The one validation
// of both entry points
int sgm_check(const les_hip_ctx* c, int* K)
{
    if (c->naive) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_sgm_labels: the image-based energy holds no cost volume");
    const float range = c->p.max_disparity - c->p.min_disparity;
    if (!(range >= 0.0f) || range >= 65536.0f)
        return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: disparity range [%g, %g]", (double)c->p.min_disparity, (double)c->p.max_disparity);
    const int k = (int)range + 1;
    if (k > les::kSgmMaxK) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_sgm_labels: %d disparities (supported: 1 .. %d)", k, les::kSgmMaxK);
    if (k > c->p.D) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: the disparity range needs %d slices, the volume has %d", k, c->p.D);
    const float th = c->p.th_col;
    if (!(th == th) || th == INFINITY || th == -INFINITY) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: th_col %g (a finite truncation value)", (double)th);
    if (c->p.H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_sgm_labels: image height %d exceeds the launch grid", c->p.H);
    *K = k;
    return LES_HIP_OK;
}

template <int V>
int sgm_launch(const float* vol, float* Ct, float* S, int H, int W, int K, float th_col, int paths, float p1, float p2, int subpixel, float d0,
               float4* d_labels, float* d_sum, hipStream_t stream, void* const* events)
{
    const int Kp = 64 * V;
    const size_t P = (size_t)H * W;
    int ne = 0;
#if !defined(LES_SIM)
#define LES_SGM_MARK() do { if (events) HIPCHECK(hipEventRecord((hipEvent_t)events[ne++], stream)); } while (0)
#else
#define LES_SGM_MARK() do { (void)events; (void)ne; } while (0)
#endif
    LES_SGM_MARK();
    hipLaunchKernelGGL(les::les_sgm_transpose_kernel, dim3((W + les::kSgmTile - 1) / les::kSgmTile, H, Kp / les::kSgmTile), dim3(les::kSgmThreads), 0, stream,
                       vol, Ct, H, W, K, Kp, th_col);
    LES_SGM_MARK();
    for (int i = 0; i < paths; i++) {
        const int dx = kSgmDirs[i][0], dy = kSgmDirs[i][1];
        const dim3 grid((les::sgm_lines(H, W, dx, dy) + les::kSgmThreads / 64 - 1) / (les::kSgmThreads / 64));
        if (i == 0) hipLaunchKernelGGL((les::les_sgm_path_kernel<V, true>), grid, dim3(les::kSgmThreads), 0, stream, Ct, S, H, W, dx, dy, p1, p2);
        else hipLaunchKernelGGL((les::les_sgm_path_kernel<V, false>), grid, dim3(les::kSgmThreads), 0, stream, Ct, S, H, W, dx, dy, p1, p2);
        LES_SGM_MARK();
    }
    const size_t waves = (P + les::kSgmReadoutPixels - 1) / les::kSgmReadoutPixels;
    const float* Sc = S;
    hipLaunchKernelGGL((les::les_sgm_readout_kernel<V>), dim3((unsigned)((waves + les::kSgmThreads / 64 - 1) / (les::kSgmThreads / 64))), dim3(les::kSgmThreads), 0,
                       stream, Sc, P, K, subpixel, d0, d_labels, d_sum);
    LES_SGM_MARK();
#undef LES_SGM_MARK
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

size_t les_hip_sgm_workspace_bytes(const les_hip_ctx* c)
{
    int K = 0;
    if (!c || sgm_check(c, &K)) return 0;
    return 2 * (size_t)c->p.H * c->p.W * (size_t)les::sgm_padded(K) * sizeof(float);
}

int les_hip_sgm_labels(les_hip_ctx* c, int mode, int paths, float p1, float p2, int subpixel, les_hip_plane* d_labels, float* d_sum)
{
    if (!c || !d_labels) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: null argument");
    if (paths != 2 && paths != 4 && paths != 8) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: paths %d (2, 4 or 8)", paths);
    if (!(p1 >= 0.0f) || !(p2 >= p1) || p1 == INFINITY || p2 == INFINITY)
        return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: penalties P1 %g, P2 %g (finite, 0 <= P1 <= P2)", (double)p1, (double)p2);
    int K = 0;
    int rc = sgm_check(c, &K);
    if (rc) return rc;
    if (mode < 0 || mode > 1 || !c->v[mode].vol) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_labels: view %d was not supplied at creation", mode);
    const float th = c->p.th_col;
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    hipStream_t stream = cur_stream(c);
    const int H = c->p.H, W = c->p.W, Kp = les::sgm_padded(K);
    const size_t n = (size_t)H * W * Kp;
    if (!c->sgm) c->sgm = new SgmWork();
    if ((rc = c->sgm->ws.grow(2 * n, 0, stream))) return rc;
    float *Ct = c->sgm->ws.p, *S = Ct + n;
    const float* vol = c->v[mode].vol;
    float4* lab = reinterpret_cast<float4*>(d_labels);
    void* const* events = nullptr;
#if !defined(LES_SIM)
    struct Events {                                         // (destroyed on every return path)
        hipEvent_t e[kSgmMaxTimes + 1] = {};
        ~Events() { for (hipEvent_t q : e) if (q) (void)hipEventDestroy(q); }
    } ev;
    const bool timing = cv_env_flag("LES_HIP_SGM_TIMING", false);
    if (timing) {
        for (int i = 0; i < paths + 3; i++) HIPCHECK(hipEventCreate(&ev.e[i]));
        events = reinterpret_cast<void* const*>(ev.e);
    }
#endif
    const float d0 = c->p.min_disparity;
    switch (les::sgm_lane_vector(K)) {
    case 1: rc = sgm_launch<1>(vol, Ct, S, H, W, K, th, paths, p1, p2, subpixel, d0, lab, d_sum, stream, events); break;
    case 2: rc = sgm_launch<2>(vol, Ct, S, H, W, K, th, paths, p1, p2, subpixel, d0, lab, d_sum, stream, events); break;
    case 4: rc = sgm_launch<4>(vol, Ct, S, H, W, K, th, paths, p1, p2, subpixel, d0, lab, d_sum, stream, events); break;
    default: rc = sgm_launch<8>(vol, Ct, S, H, W, K, th, paths, p1, p2, subpixel, d0, lab, d_sum, stream, events); break;
    }
    if (rc) return rc;
#if !defined(LES_SIM)
    if (timing) {
        HIPCHECK(hipStreamSynchronize(stream));
        for (int i = 0; i < paths + 2; i++) HIPCHECK(hipEventElapsedTime(&tl_sgm_ms[i], ev.e[i], ev.e[i + 1]));
        tl_sgm_n = paths + 2;
    }
#endif
    return LES_HIP_OK;
}

int les_hip_sgm_last_times(float* ms, int cap, int* n)
{
    if (!ms || !n || cap < 0) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_last_times: bad argument");
    if (tl_sgm_n < 0) return fail(LES_HIP_ERR_ARG, "les_hip_sgm_last_times: this thread has run no les_hip_sgm_labels with LES_HIP_SGM_TIMING=1");
    *n = tl_sgm_n;
    for (int i = 0; i < tl_sgm_n && i < cap; i++) ms[i] = tl_sgm_ms[i];
    return LES_HIP_OK;
}

}  // extern "C"
