// les_hip_pyramid.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the half-resolution solve's way down and way up (les_pyramid.h holds the definitions and the kernels) -- the stateless pools, the half context, the label upsample
namespace {

// non-temporal loads in the volume pool: LES_HIP_PYRAMID_NT=1 / 0 overrides the default; read per call (tools/pyramid_timing.py measures both)
constexpr bool kPyrNontemporalDefault = true;

int pyr_check_dims(const char* who, int D, int H, int W)
{
    if (D <= 0 || H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "%s: bad dimensions %d x %d x %d", who, D, H, W);
    if ((unsigned long long)D * H * W >= (1ull << 32)) return fail(LES_HIP_ERR_UNSUPPORTED, "%s: volumes of 2^32 or more floats are not supported", who);
    if ((H + 1) / 2 > 65535 || ((D + 1) / 2 + les::kPyrKC - 1) / les::kPyrKC > 65535)
        return fail(LES_HIP_ERR_UNSUPPORTED, "%s: image height %d / %d slices exceed the launch grid", who, H, D);
    return LES_HIP_OK;
}

// enqueue only
int pyr_pool_volume(const float* d_src, float* d_dst, int D, int H, int W, hipStream_t st)
{
    const int Dh = (D + 1) / 2, Hh = (H + 1) / 2, Wh = (W + 1) / 2;
    const dim3 grid((unsigned)((Wh + les::kPyrTX - 1) / les::kPyrTX), (unsigned)((Hh + les::kPyrRows - 1) / les::kPyrRows), (unsigned)((Dh + les::kPyrKC - 1) / les::kPyrKC));
    const dim3 block(256);
    // every input row 16-byte aligned, every output row 8-byte aligned (Wh = W / 2 is even)
    const bool vec = (W % 4 == 0) && (((uintptr_t)d_src & 15) == 0) && (((uintptr_t)d_dst & 7) == 0);
    if (!vec)
        hipLaunchKernelGGL((les::les_pool_volume_kernel<false, false>), grid, block, 0, st, d_src, d_dst, D, H, W);
    else if (cv_env_flag("LES_HIP_PYRAMID_NT", kPyrNontemporalDefault))
        hipLaunchKernelGGL((les::les_pool_volume_kernel<true, true>), grid, block, 0, st, d_src, d_dst, D, H, W);
    else
        hipLaunchKernelGGL((les::les_pool_volume_kernel<true, false>), grid, block, 0, st, d_src, d_dst, D, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_pool_image(const uint8_t* d_src, uint8_t* d_dst, int H, int W, int device, void* stream)
{
    if (!d_src || !d_dst || H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "les_hip_pool_image: bad argument");
    if ((H + 1) / 2 > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_pool_image: image height %d exceeds the launch grid", H);
    HIPCHECK(hipSetDevice(device));
    const int Hh = (H + 1) / 2, Wh = (W + 1) / 2;
    hipLaunchKernelGGL(les::les_pool_image_kernel, dim3((unsigned)((Wh + 255) / 256), (unsigned)Hh), dim3(256), 0, (hipStream_t)stream, d_src, d_dst, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_pool_volume(const float* d_src, float* d_dst, int D, int H, int W, int device, void* stream)
{
    if (!d_src || !d_dst) return fail(LES_HIP_ERR_ARG, "les_hip_pool_volume: null argument");
    const int rc = pyr_check_dims("les_hip_pool_volume", D, H, W);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    return pyr_pool_volume(d_src, d_dst, D, H, W, (hipStream_t)stream);
}

int les_hip_upsample_labels(les_hip_ctx* full, const les_hip_ctx* half, int mode, const les_hip_plane* d_src, les_hip_plane* d_out, unsigned char* d_kind)
{
    if (!full || !half || !d_src || !d_out) return fail(LES_HIP_ERR_ARG, "les_hip_upsample_labels: null argument");
    if (mode < 0 || mode > 1 || !full->v[mode].ipk || !half->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "les_hip_upsample_labels: view %d was not supplied at creation", mode);
    const int Hh = (full->p.H + 1) / 2, Wh = (full->p.W + 1) / 2;
    if (half->p.H != Hh || half->p.W != Wh || half->p.device != full->p.device)
        return fail(LES_HIP_ERR_ARG, "les_hip_upsample_labels: a %d x %d context on device %d is not the half of a %d x %d one on device %d", half->p.W, half->p.H,
                    half->p.device, full->p.W, full->p.H, full->p.device);
    if ((const void*)d_src == (const void*)d_out) return fail(LES_HIP_ERR_ARG, "les_hip_upsample_labels: d_out may not be d_src");
    if (full->p.H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_upsample_labels: image height %d exceeds the launch grid", full->p.H);
    (void)hipSetDevice(full->p.device);                     // HIP's current device is per host thread
    const uint32_t *ipk_full = full->v[mode].ipk, *ipk_half = half->v[mode].ipk;
    hipLaunchKernelGGL(les::les_upsample_labels_kernel, dim3((unsigned)((full->p.W + 255) / 256), (unsigned)full->p.H), dim3(256), 0, cur_stream(full), full->geom,
                       ipk_full, ipk_half, reinterpret_cast<const float4*>(d_src), reinterpret_cast<float4*>(d_out), d_kind, Hh, Wh);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_create_half(les_hip_ctx** out, const les_hip_ctx* src)
{
    if (!out || !src) return fail(LES_HIP_ERR_ARG, "null argument");
    *out = nullptr;
    const float half_min = 0.5f * src->p.min_disparity;
    if (!(half_min == std::floor(half_min)))                // (also refuses a non-finite one)
        return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_create_half: min_disparity %g is not an even integer (half slice k would not sit on an integer disparity)",
                    (double)src->p.min_disparity);
    const int H = src->p.H, W = src->p.W, D = src->p.D;
    int rc = pyr_check_dims("les_hip_create_half", D, H, W);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(src->p.device));
    const int Hh = (H + 1) / 2, Wh = (W + 1) / 2, Dh = (D + 1) / 2;
    const size_t Ph = (size_t)Hh * Wh;
    hipStream_t st = cur_stream(src);
    // the pooled images: from the packed guide the source keeps, to the host (the constructors take host images)
    std::vector<uint8_t> h_im[2];
    DevBuf<uint8_t> d_im;
    if ((rc = d_im.alloc(Ph * 3))) return rc;
    for (int m = 0; m < 2; m++) {
        const uint32_t* ipk = src->v[m].ipk;
        if (!ipk) continue;
        uint8_t* dst = d_im.p;
        hipLaunchKernelGGL(les::les_pool_packed_kernel, dim3((unsigned)((Wh + 255) / 256), (unsigned)Hh), dim3(256), 0, st, ipk, dst, H, W);
        HIPCHECK(hipGetLastError());
        h_im[m].resize(Ph * 3);
        HIPCHECK(hipMemcpyAsync(h_im[m].data(), d_im.p, Ph * 3, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
    }
    // the pooled volumes: owned here until the new context takes them over
    DevBuf<float> d_vol[2];
    for (int m = 0; m < 2 && !src->naive; m++) {
        if (!src->v[m].vol) continue;
        if ((rc = d_vol[m].alloc(Ph * Dh))) return rc;
        if ((rc = pyr_pool_volume(src->v[m].vol, d_vol[m].p, D, H, W, st))) return rc;
    }
    HIPCHECK(hipStreamSynchronize(st));
    les_hip_params p = src->p;
    p.H = Hh; p.W = Wh; p.D = Dh;
    p.max_disparity = 0.5f * src->p.max_disparity;
    p.min_disparity = half_min;
    p.windR = std::max(1, (src->p.windR + 1) / 2);
    p.volumes_on_device = src->naive ? 0 : 1;
    les_hip_ctx* c = nullptr;
    rc = create_common(&c, &p, h_im[0].empty() ? nullptr : h_im[0].data(), h_im[1].empty() ? nullptr : h_im[1].data(), d_vol[0].p, d_vol[1].p, src->naive,
                       src->naive_alpha, src->naive_th_grad, src->filter);
    if (rc) return rc;
    for (int m = 0; m < 2; m++)
        if (d_vol[m].p) {                                   // the context now owns the volume (freed by ~les_hip_ctx)
            c->v[m].own_vol = true;
            d_vol[m].p = nullptr; d_vol[m].cap = 0;
        }
    c->stream = src->stream;
    c->interp = src->interp;
    c->max_vdisp = 0.5f * src->max_vdisp;
    c->random_vdisp = 0.5f * src->random_vdisp;
    *out = c;
    return LES_HIP_OK;
}

int les_hip_get_image(les_hip_ctx* c, int mode, uint8_t* out_host)
{
    if (!c || !out_host || mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "les_hip_get_image: bad argument");
    HIPCHECK(hipSetDevice(c->p.device));
    const size_t P = (size_t)c->p.H * c->p.W;
    std::vector<uint32_t> pk(P);
    HIPCHECK(hipMemcpyAsync(pk.data(), c->v[mode].ipk, P * sizeof(uint32_t), hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    for (size_t i = 0; i < P; i++) {
        out_host[3 * i] = (uint8_t)(pk[i] & 255u);
        out_host[3 * i + 1] = (uint8_t)((pk[i] >> 8) & 255u);
        out_host[3 * i + 2] = (uint8_t)((pk[i] >> 16) & 255u);
    }
    return LES_HIP_OK;
}

}  // extern "C"
