// les_hip_ingest_post.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): volume ingest (fillOutOfView, convertVolumeL2R) and the dual-view post-processing
extern "C" {

int les_hip_fill_out_of_view(float* vol, int D, int H, int W, int mode, int device, void* stream)
{
    if (!vol || D <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 1) return fail(LES_HIP_ERR_ARG, "bad argument");
    HIPCHECK(hipSetDevice(device));
    hipLaunchKernelGGL(les::les_fill_out_of_view_kernel, dim3((W + 255) / 256, H, D), dim3(256), 0, (hipStream_t)stream, vol, D, H, W, mode);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_convert_volume_l2r(const float* src, float* dst, int D, int H, int W, int device, void* stream)
{
    if (!src || !dst || src == dst || D <= 0 || H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "bad argument");
    HIPCHECK(hipSetDevice(device));
    hipLaunchKernelGGL(les::les_convert_l2r_kernel, dim3((W + 255) / 256, H, D), dim3(256), 0, (hipStream_t)stream, src, dst, D, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

// ---- dual-view post-processing (LES/PMStereoBase.h:111-256)
namespace {
struct PostScratch {                                       // (launches take the raw pointers, never the owners)
    DevBuf<float> disp[2];
    DevBuf<uint8_t> fail, failb, fail2;
    DevBuf<float4> copy;
    DevBuf<float> wtab;
};
int post_disparities(les_hip_ctx* c, PostScratch& ps, const les_hip_plane* const labels[2])
{
    const int H = c->p.H, W = c->p.W;
    const size_t P = (size_t)H * W;
    for (int m = 0; m < 2; m++) {
        if (!labels[m]) continue;                          // (the one-view form of les_hip_post_process_speckle)
        const int rc = ps.disp[m].alloc(P);
        if (rc) return rc;
        const float4* lab = (const float4*)labels[m];
        float* disp = ps.disp[m].p;
        hipLaunchKernelGGL(les::les_disparity_kernel, dim3((W + 255) / 256, H), dim3(256), 0, cur_stream(c), lab, disp, H, W);
    }
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

struct SpeckleParams { int max_size; float max_diff; };

// The body of les_hip_post_process, les_hip_post_process_speckle and les_hip_post_process_masked: per view present, the failure mask -- the
// left-right check when both views are there, OR the speckle mask when `sp` asks for one, OR the caller's own mask user[m] (H x W bytes on the
// device, nonzero = failed; `user` or either entry may be null) -- its dilation and the fill; then per view the weighted median.
int post_process_body(les_hip_ctx* c, les_hip_plane* const labels[2], float threshold, float omega, const SpeckleParams* sp,
                      const unsigned char* const* user = nullptr)
{
    const bool both = labels[0] && labels[1];
    for (int m = 0; m < 2; m++)
        if (labels[m] && !c->v[m].ipk) return fail(LES_HIP_ERR_ARG, both ? "post-processing needs both views' images" : "post-processing needs the view's image");
    const int windR = c->p.windR;
    if (windR > 31) return fail(LES_HIP_ERR_UNSUPPORTED, "weighted median window radius %d > 31", windR);
    HIPCHECK(hipSetDevice(c->p.device));
    const int H = c->p.H, W = c->p.W;
    const size_t P = (size_t)H * W;
    PostScratch ps;
    SpeckleScratch ss;
    int rc = post_disparities(c, ps, labels);
    if (rc) return rc;
    if ((rc = ps.fail.alloc(P)) || (rc = ps.failb.alloc(2 * P)) || (rc = ps.fail2.alloc(P)) || (rc = ps.copy.alloc(P))) return rc;
    {
        // computePatchWeight (LES/StereoEnergy.h:251-257): exp(-|dI|_1 / omega) in float; |dI|_1 of 8-bit colours is an integer
        std::vector<float> tab(766);
        for (int k = 0; k < 766; k++) tab[k] = std::exp(-(float)k / omega);
        if ((rc = ps.wtab.alloc(tab.size()))) return rc;
        HIPCHECK(hipMemcpyAsync(ps.wtab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream(c)));
        HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    }
    const dim3 g((W + 255) / 256, H), b(256);
    // both fail masks come from the labels before any of them is modified (LES/PMStereoBase.h:158-164): from the disparities above
    uint8_t *failm = ps.fail.p, *fail2 = ps.fail2.p;
    const float* wtab = ps.wtab.p;
    float4* copy = ps.copy.p;
    for (int m = 0; m < 2; m++) {
        if (!labels[m]) continue;
        const float *d_self = ps.disp[m].p, *d_other = ps.disp[1 - m].p;
        uint8_t* failb = ps.failb.p + m * P;
        float4* lab = (float4*)labels[m];
        const float sign = m ? -1.0f : 1.0f;
        if (both) hipLaunchKernelGGL(les::les_lr_check_kernel, g, b, 0, cur_stream(c), d_self, d_other, failm, H, W, sign, threshold);
        else HIPCHECK(hipMemsetAsync(failm, 0, P, cur_stream(c)));
        if (sp && sp->max_size > 0 && (rc = speckle_launch(c, ss, d_self, sp->max_size, sp->max_diff, failm, nullptr, nullptr, 1))) return rc;
        if (user && user[m]) hipLaunchKernelGGL(les::les_fail_or_kernel, g, b, 0, cur_stream(c), (const uint8_t*)user[m], failm, H, W);
        hipLaunchKernelGGL(les::les_fail_dilate_kernel, g, b, 0, cur_stream(c), failm, failb, fail2, H, W);
        hipLaunchKernelGGL(les::les_nn_fill_kernel, g, b, 0, cur_stream(c), failb, fail2, lab, H, W);
    }
    for (int m = 0; m < 2; m++) {
        if (!labels[m]) continue;
        HIPCHECK(hipMemcpyAsync(ps.copy.p, labels[m], P * sizeof(float4), hipMemcpyDeviceToDevice, cur_stream(c)));
        const dim3 gp(W, H);
        const int area = (2 * windR + 1) * (2 * windR + 1);
        const uint8_t* failb = ps.failb.p + m * P;
        float4* lab = (float4*)labels[m];
        const uint32_t* ipk = c->v[m].ipk;
        if (area <= 256)
            hipLaunchKernelGGL((les::les_weighted_median_kernel<256, 64>), gp, dim3(64), 0, cur_stream(c), failb, copy, lab, ipk, wtab, H, W, windR);
        else if (area <= 1024)
            hipLaunchKernelGGL((les::les_weighted_median_kernel<1024, 256>), gp, dim3(256), 0, cur_stream(c), failb, copy, lab, ipk, wtab, H, W, windR);
        else if (area <= 2048)
            hipLaunchKernelGGL((les::les_weighted_median_kernel<2048, 256>), gp, dim3(256), 0, cur_stream(c), failb, copy, lab, ipk, wtab, H, W, windR);
        else
            hipLaunchKernelGGL((les::les_weighted_median_kernel<4096, 256>), gp, dim3(256), 0, cur_stream(c), failb, copy, lab, ipk, wtab, H, W, windR);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}
}  // namespace

int les_hip_consistency_check(les_hip_ctx* c, const les_hip_plane* d_labelsL, const les_hip_plane* d_labelsR, float threshold,
                              unsigned char* d_failL, unsigned char* d_failR)
{
    if (!c || !d_labelsL || !d_labelsR || !d_failL || !d_failR) return fail(LES_HIP_ERR_ARG, "null argument");
    HIPCHECK(hipSetDevice(c->p.device));
    const int H = c->p.H, W = c->p.W;
    PostScratch ps;
    const les_hip_plane* labels[2] = {d_labelsL, d_labelsR};
    int rc = post_disparities(c, ps, labels);
    if (rc) return rc;
    unsigned char* out[2] = {d_failL, d_failR};
    for (int m = 0; m < 2; m++) {
        const float *d_self = ps.disp[m].p, *d_other = ps.disp[1 - m].p;
        unsigned char* o = out[m];
        const float sign = m ? -1.0f : 1.0f;
        hipLaunchKernelGGL(les::les_lr_check_kernel, dim3((W + 255) / 256, H), dim3(256), 0, cur_stream(c), d_self, d_other, o, H, W, sign, threshold);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

int les_hip_post_process(les_hip_ctx* c, les_hip_plane* d_labelsL, les_hip_plane* d_labelsR, float threshold, float omega)
{
    if (!c || !d_labelsL || !d_labelsR) return fail(LES_HIP_ERR_ARG, "null argument");
    les_hip_plane* labels[2] = {d_labelsL, d_labelsR};
    return post_process_body(c, labels, threshold, omega, nullptr);
}

int les_hip_post_process_speckle(les_hip_ctx* c, les_hip_plane* d_labelsL, les_hip_plane* d_labelsR, float threshold, float omega, int max_size,
                                 float max_diff)
{
    if (!c || (!d_labelsL && !d_labelsR)) return fail(LES_HIP_ERR_ARG, "null argument");
    const int rc = speckle_check_args(c, max_size, max_diff);
    if (rc) return rc;
    les_hip_plane* labels[2] = {d_labelsL, d_labelsR};
    const SpeckleParams sp = {max_size, max_diff};
    return post_process_body(c, labels, threshold, omega, &sp);
}

int les_hip_post_process_masked(les_hip_ctx* c, les_hip_plane* d_labelsL, les_hip_plane* d_labelsR, float threshold, float omega, int max_size,
                                float max_diff, const unsigned char* d_failL, const unsigned char* d_failR)
{
    if (!c || (!d_labelsL && !d_labelsR)) return fail(LES_HIP_ERR_ARG, "null argument");
    const int rc = speckle_check_args(c, max_size, max_diff);
    if (rc) return rc;
    les_hip_plane* labels[2] = {d_labelsL, d_labelsR};
    const unsigned char* user[2] = {d_failL, d_failR};
    const SpeckleParams sp = {max_size, max_diff};
    return post_process_body(c, labels, threshold, omega, &sp, user);
}

}  // extern "C"
