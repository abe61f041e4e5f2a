// les_hip_rectify.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launches of the
// rectification front end (csrc/les_rectify.h holds the camera model, the definitions and the kernels) -- les_hip_rectify_map, les_hip_remap.
namespace {

// grid.y is the image height
int rect_check_size(const char* who, int H, int W)
{
    if (H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "%s: bad size %d x %d", who, W, H);
    if (H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "%s: image height %d exceeds the launch grid", who, H);
    return LES_HIP_OK;
}

template <int C>
void remap_launch(int interp, dim3 grid, hipStream_t st, const uint8_t* src, int Hs, int Ws, const les::RectUV* map, uint8_t* dst, uint8_t* valid, int H, int W)
{
    const dim3 block(les::kRectNT);
    if (interp == 0)
        hipLaunchKernelGGL((les::les_remap_kernel<C, 0>), grid, block, 0, st, src, Hs, Ws, map, dst, valid, H, W);
    else if (interp == 1)
        hipLaunchKernelGGL((les::les_remap_kernel<C, 1>), grid, block, 0, st, src, Hs, Ws, map, dst, valid, H, W);
    else
        hipLaunchKernelGGL((les::les_remap_kernel<C, 2>), grid, block, 0, st, src, Hs, Ws, map, dst, valid, H, W);
}

}  // namespace

extern "C" {

int les_hip_rectify_map(const les_hip_camera* raw, const double* M, double f, double cx, double cy, float* d_map, int H, int W, int device, void* stream)
{
    if (!raw || !M || !d_map) return fail(LES_HIP_ERR_ARG, "les_hip_rectify_map: null argument");
    if (((uintptr_t)d_map & 7) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_rectify_map: d_map is not 8-byte aligned");
    int rc = rect_check_size("les_hip_rectify_map", H, W);
    if (rc) return rc;
    // (written so that a NaN is refused)
    if (!(f > 0.0 && f < (double)INFINITY) || !(raw->fx > 0.0 && raw->fx < (double)INFINITY) || !(raw->fy > 0.0 && raw->fy < (double)INFINITY))
        return fail(LES_HIP_ERR_ARG, "les_hip_rectify_map: f %g, fx %g, fy %g (all finite and > 0)", f, raw->fx, raw->fy);
    HIPCHECK(hipSetDevice(device));
    les::RectCamera cam;
    cam.fx = raw->fx; cam.fy = raw->fy; cam.cx = raw->cx; cam.cy = raw->cy;
    for (int k = 0; k < 8; k++) cam.dist[k] = raw->dist[k];
    les::RectRays rays;
    for (int k = 0; k < 9; k++) rays.M[k] = M[k];
    rays.f = f; rays.cx = cx; rays.cy = cy;
    hipLaunchKernelGGL(les::les_rectify_map_kernel, dim3((unsigned)((W + les::kRectNT - 1) / les::kRectNT), (unsigned)H), dim3(les::kRectNT), 0, (hipStream_t)stream,
                       cam, rays, reinterpret_cast<les::RectUV*>(d_map), H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_remap(const uint8_t* d_src, int Hs, int Ws, int channels, const float* d_map, uint8_t* d_dst, unsigned char* d_valid, int H, int W, int interp,
                  int device, void* stream)
{
    if (!d_src || !d_map || !d_dst) return fail(LES_HIP_ERR_ARG, "les_hip_remap: null argument");
    if (((uintptr_t)d_map & 7) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_remap: d_map is not 8-byte aligned");
    if (Hs <= 0 || Ws <= 0) return fail(LES_HIP_ERR_ARG, "les_hip_remap: bad source size %d x %d", Ws, Hs);
    if (channels != 1 && channels != 3) return fail(LES_HIP_ERR_ARG, "les_hip_remap: channels %d (1 or 3)", channels);
    if (interp < 0 || interp > 2) return fail(LES_HIP_ERR_ARG, "les_hip_remap: interp %d (0 nearest, 1 linear, 2 cubic)", interp);
    int rc = rect_check_size("les_hip_remap", H, W);
    if (rc) return rc;
    if ((long long)Hs * Ws * channels >= (1ll << 31))
        return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_remap: a source of %d x %d x %d bytes does not fit 31-bit offsets", Ws, Hs, channels);
    if ((const void*)d_dst == (const void*)d_src) return fail(LES_HIP_ERR_ARG, "les_hip_remap: d_dst may not be d_src");
    HIPCHECK(hipSetDevice(device));
    const dim3 grid((unsigned)((W + les::kRectNT - 1) / les::kRectNT), (unsigned)H);
    const les::RectUV* map = reinterpret_cast<const les::RectUV*>(d_map);
    if (channels == 1)
        remap_launch<1>(interp, grid, (hipStream_t)stream, d_src, Hs, Ws, map, d_dst, d_valid, H, W);
    else
        remap_launch<3>(interp, grid, (hipStream_t)stream, d_src, Hs, Ws, map, d_dst, d_valid, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
