// les_hip_fisheye.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launches of the fisheye
// camera's two maps (csrc/les_fisheye.h holds the camera model, the definitions and the kernels) -- les_hip_rectify_map_fisheye,
// les_hip_unrectify_map_fisheye.
namespace {

// The checks both entries share; `who` names the entry.  (written so that a NaN is refused)
int fisheye_check(const char* who, const les_hip_fisheye* raw, const double* rot, double f, const float* d_map, int H, int W)
{
    if (!raw || !rot || !d_map) return fail(LES_HIP_ERR_ARG, "%s: null argument", who);
    if (((uintptr_t)d_map & 7) != 0) return fail(LES_HIP_ERR_ARG, "%s: d_map is not 8-byte aligned", who);
    int rc = rect_check_size(who, H, W);
    if (rc) return rc;
    if (!unrect_positive(f) || !unrect_positive(raw->fx) || !unrect_positive(raw->fy))
        return fail(LES_HIP_ERR_ARG, "%s: f %g, fx %g, fy %g (all finite and > 0)", who, f, raw->fx, raw->fy);
    for (int k = 0; k < 4; k++)
        if (!(raw->k[k] >= -1.7976931348623157e308 && raw->k[k] <= 1.7976931348623157e308))
            return fail(LES_HIP_ERR_ARG, "%s: k%d is %g (finite)", who, k + 1, raw->k[k]);
    if (!(raw->theta_max > 0.0 && raw->theta_max <= 3.141592653589793))
        return fail(LES_HIP_ERR_ARG, "%s: theta_max %g (in (0, pi])", who, raw->theta_max);
    return LES_HIP_OK;
}

les::FishCamera fisheye_camera(const les_hip_fisheye* raw)
{
    les::FishCamera cam;
    cam.fx = raw->fx; cam.fy = raw->fy; cam.cx = raw->cx; cam.cy = raw->cy;
    for (int k = 0; k < 4; k++) cam.k[k] = raw->k[k];
    cam.theta_max = raw->theta_max;
    return cam;
}

}  // namespace

extern "C" {

int les_hip_rectify_map_fisheye(const les_hip_fisheye* raw, const double* M, double f, double cx, double cy, float* d_map, int H, int W, int device, void* stream)
{
    int rc = fisheye_check("les_hip_rectify_map_fisheye", raw, M, f, d_map, H, W);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    les::RectRays rays;
    for (int k = 0; k < 9; k++) rays.M[k] = M[k];
    rays.f = f; rays.cx = cx; rays.cy = cy;
    hipLaunchKernelGGL(les::les_fisheye_map_kernel, dim3((unsigned)((W + les::kRectNT - 1) / les::kRectNT), (unsigned)H), dim3(les::kRectNT), 0, (hipStream_t)stream,
                       fisheye_camera(raw), rays, reinterpret_cast<les::RectUV*>(d_map), H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_unrectify_map_fisheye(const les_hip_fisheye* raw, const double* R, double f, double cx, double cy, int steps, double tol, float* d_map, int Hs, int Ws,
                                  int device, void* stream)
{
    int rc = fisheye_check("les_hip_unrectify_map_fisheye", raw, R, f, d_map, Hs, Ws);
    if (rc) return rc;
    if (steps < 1 || steps > 64) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map_fisheye: steps %d (1 .. 64)", steps);
    if (!(tol > 0.0)) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map_fisheye: tol %g (> 0)", tol);
    HIPCHECK(hipSetDevice(device));
    les::UnrectView view;
    for (int k = 0; k < 9; k++) view.R[k] = R[k];
    view.f = f; view.cx = cx; view.cy = cy;
    hipLaunchKernelGGL(les::les_fisheye_unmap_kernel, dim3((unsigned)((Ws + les::kRectNT - 1) / les::kRectNT), (unsigned)Hs), dim3(les::kRectNT), 0,
                       (hipStream_t)stream, fisheye_camera(raw), view, steps, tol, reinterpret_cast<les::RectUV*>(d_map), Hs, Ws);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
