// les_hip_speckle.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the speckle filter's launches
// (csrc/les_speckle.h) and les_hip_speckle_mask / les_hip_speckle_tile.  les_hip_post_process_speckle is with the post-processing it widens
// (les_hip_ingest_post.inc).
namespace {
struct SpeckleScratch {                                    // (launches take the raw pointers, never the owners)
    DevBuf<int> parent, size;
    DevBuf<float> disp;                                    // les_hip_speckle_mask's own disparities (the post-processing has them already)
};

int speckle_check_args(const les_hip_ctx* c, int max_size, float max_diff)
{
    if (max_size < 0 || !(max_diff >= 0.0f)) return fail(LES_HIP_ERR_ARG, "speckle filter: max_size %d, max_diff %g (both >= 0)", max_size, (double)max_diff);
    if ((long long)c->p.H * c->p.W >= (1ll << 31)) return fail(LES_HIP_ERR_UNSUPPORTED, "speckle filter: %d x %d pixels do not fit 31-bit indices", c->p.H, c->p.W);
    return LES_HIP_OK;
}

// The speckle mask of the device disparity map d_disp on the calling thread's stream (enqueue only).  accumulate: 255 is OR-ed into d_mask.
int speckle_launch(les_hip_ctx* c, SpeckleScratch& ss, const float* d_disp, int max_size, float max_diff, uint8_t* d_mask, int* d_root, int* d_size,
                   int accumulate)
{
    const int H = c->p.H, W = c->p.W, P = H * W;
    int rc;
    if ((rc = ss.parent.grow((size_t)P, 0, cur_stream(c))) || (rc = ss.size.grow((size_t)P, 0, cur_stream(c)))) return rc;
    int *parent = ss.parent.p, *size = ss.size.p;
    const dim3 b(les::kSpkNT), gp((unsigned)(((long long)P + les::kSpkNT - 1) / les::kSpkNT));
    hipLaunchKernelGGL(les::les_speckle_tile_kernel, dim3((W + les::kSpkTW - 1) / les::kSpkTW, (H + les::kSpkTH - 1) / les::kSpkTH), b, 0, cur_stream(c),
                       d_disp, parent, size, H, W, max_diff);
    const long long pairs = (long long)((W - 1) / les::kSpkTW) * H + (long long)((H - 1) / les::kSpkTH) * W;
    if (pairs > 0)
        hipLaunchKernelGGL(les::les_speckle_merge_kernel, dim3((unsigned)((pairs + les::kSpkNT - 1) / les::kSpkNT)), b, 0, cur_stream(c), d_disp, parent, H, W,
                           max_diff);
    hipLaunchKernelGGL(les::les_speckle_flatten_kernel, gp, b, 0, cur_stream(c), parent, size, P);
    hipLaunchKernelGGL(les::les_speckle_mask_kernel, gp, b, 0, cur_stream(c), (const int*)parent, (const int*)size, d_mask, d_root, d_size, P, max_size,
                       accumulate);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}
}  // namespace

extern "C" {

int les_hip_speckle_tile(int* th, int* tw)
{
    if (!th || !tw) return fail(LES_HIP_ERR_ARG, "null argument");
    *th = les::kSpkTH;
    *tw = les::kSpkTW;
    return LES_HIP_OK;
}

int les_hip_speckle_mask(les_hip_ctx* c, const les_hip_plane* d_labels, int max_size, float max_diff, unsigned char* d_mask, int* d_root, int* d_size)
{
    if (!c || !d_labels || !d_mask) return fail(LES_HIP_ERR_ARG, "null argument");
    int rc = speckle_check_args(c, max_size, max_diff);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(c->p.device));
    const int H = c->p.H, W = c->p.W;
    SpeckleScratch ss;
    if ((rc = ss.disp.alloc((size_t)H * W))) return rc;
    const float4* lab = (const float4*)d_labels;
    float* disp = ss.disp.p;
    hipLaunchKernelGGL(les::les_disparity_kernel, dim3((W + 255) / 256, H), dim3(256), 0, cur_stream(c), lab, disp, H, W);
    if ((rc = speckle_launch(c, ss, disp, max_size, max_diff, d_mask, d_root, d_size, 0))) return rc;
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

}  // extern "C"
