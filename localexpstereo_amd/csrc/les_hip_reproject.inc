// les_hip_reproject.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launches of the 3D
// reconstruction (csrc/les_reproject.h) -- les_hip_reproject, les_hip_mesh, les_hip_mesh_tile.
namespace {

int reproject_check_view(const les_hip_ctx* c, int mode, const char* who)
{
    if (mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "%s: view %d was not supplied at creation", who, mode);
    if ((long long)c->p.H * c->p.W >= (1ll << 31)) return fail(LES_HIP_ERR_UNSUPPORTED, "%s: %d x %d pixels do not fit 31-bit indices", who, c->p.H, c->p.W);
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_mesh_tile(int* pixels, int* scan_width)
{
    if (!pixels || !scan_width) return fail(LES_HIP_ERR_ARG, "null argument");
    *pixels = les::kMeshTile;
    *scan_width = les::kMeshScanW;
    return LES_HIP_OK;
}

int les_hip_reproject(les_hip_ctx* c, int mode, const les_hip_plane* d_labels, const unsigned char* d_drop_mask, const les_hip_calib* calib, float z_max,
                      float* d_points, float* d_normals, unsigned char* d_valid)
{
    if (!c || !d_labels || !calib || !d_valid) return fail(LES_HIP_ERR_ARG, "les_hip_reproject: null argument");
    int rc = reproject_check_view(c, mode, "les_hip_reproject");
    if (rc) return rc;
    // (written so that a NaN is refused)
    if (!(calib->f > 0.0f && calib->f < INFINITY) || !(calib->baseline > 0.0f && calib->baseline < INFINITY))
        return fail(LES_HIP_ERR_ARG, "les_hip_reproject: f %g, baseline %g (both finite and > 0)", (double)calib->f, (double)calib->baseline);
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    const int H = c->p.H, W = c->p.W;
    const les::Calib k = {calib->f, calib->cx, calib->cy, calib->doffs, calib->baseline};
    const float4* lab = reinterpret_cast<const float4*>(d_labels);
    const uint8_t* drop = d_drop_mask;
    hipLaunchKernelGGL(les::les_reproject_kernel, dim3((unsigned)(((long long)H * W + les::kRepNT - 1) / les::kRepNT)), dim3(les::kRepNT), 0, cur_stream(c), lab,
                       drop, k, mode, z_max, d_points, d_normals, d_valid, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_mesh(les_hip_ctx* c, int mode, const les_hip_plane* d_labels, const unsigned char* d_valid, float max_jump, int* d_vertex_index,
                 int* d_vertex_pixel, int* d_triangles, long long* d_counts)
{
    if (!c || !d_labels || !d_valid || !d_vertex_index || !d_vertex_pixel || !d_triangles || !d_counts)
        return fail(LES_HIP_ERR_ARG, "les_hip_mesh: null argument");
    int rc = reproject_check_view(c, mode, "les_hip_mesh");
    if (rc) return rc;
    if (!(max_jump >= 0.0f)) return fail(LES_HIP_ERR_ARG, "les_hip_mesh: max_jump %g (>= 0; +inf connects every valid neighbour)", (double)max_jump);
    (void)hipSetDevice(c->p.device);
    const int H = c->p.H, W = c->p.W;
    const int ntiles = (int)(((long long)H * W + les::kMeshTile - 1) / les::kMeshTile);
    // the workspace of the view, kept by the context: [2 ntiles] offsets (long long), then [2 ntiles] counts (int)
    long long* off = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if ((rc = c->mesh_ws[mode].grow(3 * (size_t)ntiles, 0, cur_stream(c)))) return rc;
        off = c->mesh_ws[mode].p;
    }
    int* cnt = reinterpret_cast<int*>(off + 2 * (size_t)ntiles);
    const float4* lab = reinterpret_cast<const float4*>(d_labels);
    const uint8_t* valid = d_valid;
    const dim3 grid((unsigned)ntiles), block(les::kMeshNT);
    hipLaunchKernelGGL(les::les_mesh_count_kernel, grid, block, 0, cur_stream(c), lab, valid, H, W, max_jump, cnt);
    hipLaunchKernelGGL(les::les_mesh_scan_kernel, dim3(1), dim3(les::kMeshScanW), 0, cur_stream(c), (const int*)cnt, off, d_counts, ntiles);
    hipLaunchKernelGGL(les::les_mesh_vertices_kernel, grid, block, 0, cur_stream(c), valid, H, W, (const long long*)off, d_vertex_index, d_vertex_pixel);
    hipLaunchKernelGGL(les::les_mesh_triangles_kernel, grid, block, 0, cur_stream(c), lab, valid, H, W, max_jump, (const long long*)off,
                       (const int*)d_vertex_index, d_triangles);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
