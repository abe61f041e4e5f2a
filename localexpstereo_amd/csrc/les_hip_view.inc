// les_hip_view.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launches of view synthesis and
// of the photometric check (csrc/les_view.h holds the definitions and the kernels) -- les_hip_render_view, les_hip_blend_views, les_hip_photo_error.
namespace {

int view_check_width(const les_hip_ctx* c, const char* who)
{
    if (c->p.W > les::kWarpMaxW) return fail(LES_HIP_ERR_UNSUPPORTED, "%s: rows of %d pixels, at most %d are supported", who, c->p.W, les::kWarpMaxW);
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_render_view(les_hip_ctx* c, int src_mode, const les_hip_plane* d_labels, const unsigned char* d_image, float t, unsigned char* d_out_bgr,
                        float* d_out_disp, unsigned char* d_out_hit)
{
    if (!c || !d_labels || !d_out_bgr || !d_out_disp || !d_out_hit) return fail(LES_HIP_ERR_ARG, "les_hip_render_view: null argument");
    if (src_mode < 0 || src_mode > 1) return fail(LES_HIP_ERR_ARG, "les_hip_render_view: src_mode %d (0 left, 1 right)", src_mode);
    if (!d_image && !c->v[src_mode].ipk) return fail(LES_HIP_ERR_ARG, "les_hip_render_view: view %d was not supplied at creation and no image is given", src_mode);
    if (!(t >= 0.0f && t <= 1.0f)) return fail(LES_HIP_ERR_ARG, "les_hip_render_view: t %g (a fraction of the baseline in [0, 1])", (double)t);      // (written so that a NaN is refused)
    if ((const void*)d_out_bgr == (const void*)d_image) return fail(LES_HIP_ERR_ARG, "les_hip_render_view: d_out_bgr may not be the image that is read");
    int rc = view_check_width(c, "les_hip_render_view");
    if (rc) return rc;
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    const int H = c->p.H, W = c->p.W;
    const uint32_t* ipk = d_image ? nullptr : c->v[src_mode].ipk;
    const uint8_t* image = d_image;
    hipLaunchKernelGGL(les::les_render_view_kernel, dim3((unsigned)H), dim3(les::kViewThreads), 2 * sizeof(uint32_t) * (size_t)W, cur_stream(c),
                       reinterpret_cast<const float4*>(d_labels), ipk, image, d_out_bgr, d_out_disp, d_out_hit, H, W, t, src_mode ? -1.0f : 1.0f);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_blend_views(les_hip_ctx* c, float t, float tol, int fill, const unsigned char* d_bgrL, const float* d_dispL, const unsigned char* d_hitL,
                        const unsigned char* d_bgrR, const float* d_dispR, const unsigned char* d_hitR, unsigned char* d_out_bgr, float* d_out_disp,
                        unsigned char* d_out_src)
{
    if (!c || !d_out_bgr || !d_out_disp || !d_out_src) return fail(LES_HIP_ERR_ARG, "les_hip_blend_views: null argument");
    const int nl = (d_bgrL != nullptr) + (d_dispL != nullptr) + (d_hitL != nullptr), nr = (d_bgrR != nullptr) + (d_dispR != nullptr) + (d_hitR != nullptr);
    if ((nl != 0 && nl != 3) || (nr != 0 && nr != 3) || nl + nr == 0)
        return fail(LES_HIP_ERR_ARG, "les_hip_blend_views: a render is (bgr, disp, hit), given or null as a whole, and at least one is given");
    if (!(t >= 0.0f && t <= 1.0f)) return fail(LES_HIP_ERR_ARG, "les_hip_blend_views: t %g (a fraction of the baseline in [0, 1])", (double)t);
    if (!(tol >= 0.0f)) return fail(LES_HIP_ERR_ARG, "les_hip_blend_views: tol %g (>= 0)", (double)tol);
    if (d_out_bgr == d_bgrL || d_out_bgr == d_bgrR || d_out_disp == d_dispL || d_out_disp == d_dispR || d_out_src == d_hitL || d_out_src == d_hitR)
        return fail(LES_HIP_ERR_ARG, "les_hip_blend_views: the outputs may not be the renders (the hole fill reads other columns)");
    int rc = view_check_width(c, "les_hip_blend_views");
    if (rc) return rc;
    (void)hipSetDevice(c->p.device);
    const int H = c->p.H, W = c->p.W;
    const uint8_t *bl = d_bgrL, *hl = d_hitL, *br = d_bgrR, *hr = d_hitR;
    hipLaunchKernelGGL(les::les_blend_views_kernel, dim3((unsigned)H), dim3(les::kViewThreads), 2 * sizeof(uint16_t) * (size_t)W + 2 * sizeof(uint32_t) * les::kViewThreads,
                       cur_stream(c), bl, d_dispL, hl, br, d_dispR, hr, d_out_bgr, d_out_disp, d_out_src, H, W, t, tol, fill ? 1 : 0);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_photo_error(les_hip_ctx* c, int mode, const les_hip_plane* d_labels, float* d_err, unsigned char* d_vis)
{
    if (!c || !d_labels || !d_err || !d_vis) return fail(LES_HIP_ERR_ARG, "les_hip_photo_error: null argument");
    if (mode < 0 || mode > 1) return fail(LES_HIP_ERR_ARG, "les_hip_photo_error: mode %d (0 left, 1 right)", mode);
    if (!c->v[0].ipk || !c->v[1].ipk) return fail(LES_HIP_ERR_ARG, "les_hip_photo_error: the context was created with one image; the photometric error compares the two");
    int rc = view_check_width(c, "les_hip_photo_error");
    if (rc) return rc;
    (void)hipSetDevice(c->p.device);
    const int H = c->p.H, W = c->p.W;
    hipLaunchKernelGGL(les::les_photo_error_kernel, dim3((unsigned)H), dim3(les::kViewThreads), 2 * sizeof(uint32_t) * (size_t)W, cur_stream(c),
                       reinterpret_cast<const float4*>(d_labels), (const uint32_t*)c->v[mode].ipk, (const uint32_t*)c->v[1 - mode].ipk, d_err, d_vis, H, W,
                       mode ? -1.0f : 1.0f);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
