// les_hip_unrectify.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launches of the way
// back to the raw camera (csrc/les_unrectify.h holds the definitions and the kernels) -- les_hip_unrectify_map, les_hip_unrectify_labels.
namespace {

// (written so that a NaN is refused)
bool unrect_positive(double x) { return x > 0.0 && x < (double)INFINITY; }

}  // namespace

extern "C" {

int les_hip_unrectify_map(const les_hip_camera* raw, const double* R, double f, double cx, double cy, int steps, double tol, float* d_map, int Hs, int Ws,
                          int device, void* stream)
{
    if (!raw || !R || !d_map) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map: null argument");
    if (((uintptr_t)d_map & 7) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map: d_map is not 8-byte aligned");
    int rc = rect_check_size("les_hip_unrectify_map", Hs, Ws);
    if (rc) return rc;
    if (!unrect_positive(f) || !unrect_positive(raw->fx) || !unrect_positive(raw->fy))
        return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map: f %g, fx %g, fy %g (all finite and > 0)", f, raw->fx, raw->fy);
    if (steps < 1 || steps > 64) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map: steps %d (1 .. 64)", steps);
    if (!(tol > 0.0)) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_map: tol %g (> 0)", tol);
    HIPCHECK(hipSetDevice(device));
    les::RectCamera cam;
    cam.fx = raw->fx; cam.fy = raw->fy; cam.cx = raw->cx; cam.cy = raw->cy;
    for (int k = 0; k < 8; k++) cam.dist[k] = raw->dist[k];
    les::UnrectView view;
    for (int k = 0; k < 9; k++) view.R[k] = R[k];
    view.f = f; view.cx = cx; view.cy = cy;
    hipLaunchKernelGGL(les::les_unrectify_map_kernel, dim3((unsigned)((Ws + les::kRectNT - 1) / les::kRectNT), (unsigned)Hs), dim3(les::kRectNT), 0,
                       (hipStream_t)stream, cam, view, steps, tol, reinterpret_cast<les::RectUV*>(d_map), Hs, Ws);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_unrectify_labels(const les_hip_plane* d_labels, int H, int W, const unsigned char* d_drop, const float* d_invmap, int Hs, int Ws, const double* M,
                             double f, double cx, double cy, double doffs, double baseline, float z_max, float* d_points, float* d_normals, float* d_disparity,
                             unsigned char* d_valid, int device, void* stream)
{
    if (!d_labels || !d_invmap || !M || !d_valid) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_labels: null argument");
    if (((uintptr_t)d_invmap & 7) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_labels: d_invmap is not 8-byte aligned");
    if (((uintptr_t)d_labels & 15) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_labels: d_labels is not 16-byte aligned");
    if (H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_labels: bad label map size %d x %d", W, H);
    int rc = rect_check_size("les_hip_unrectify_labels", Hs, Ws);
    if (rc) return rc;
    if ((long long)H * W >= (1ll << 31))
        return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_unrectify_labels: a label map of %d x %d does not fit 31-bit offsets", W, H);
    if (!unrect_positive(f) || !unrect_positive(baseline))
        return fail(LES_HIP_ERR_ARG, "les_hip_unrectify_labels: f %g, baseline %g (both finite and > 0)", f, baseline);
    HIPCHECK(hipSetDevice(device));
    les::UnrectGeom g;
    for (int k = 0; k < 9; k++) g.M[k] = M[k];
    g.f = f; g.cx = cx; g.cy = cy; g.doffs = doffs; g.baseline = baseline;
    hipLaunchKernelGGL(les::les_unrectify_labels_kernel, dim3((unsigned)((Ws + les::kRectNT - 1) / les::kRectNT), (unsigned)Hs), dim3(les::kRectNT), 0,
                       (hipStream_t)stream, reinterpret_cast<const float4*>(d_labels), H, W, d_drop, reinterpret_cast<const les::RectUV*>(d_invmap), g, z_max,
                       d_points, d_normals, d_disparity, d_valid, Hs, Ws);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
