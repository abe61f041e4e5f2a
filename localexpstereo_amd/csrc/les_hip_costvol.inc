// les_hip_costvol.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): AD-Census matching-cost volumes built from the stereo pair (les_costvol.h holds the definition and the kernels)
namespace {

bool cv_lambda_ok(float l) { return l > 0.0f && l < INFINITY; }

// the two tables of the definition: double arithmetic, one rounding to f32
void cv_tables(float lambda_ad, float lambda_census, float* ad, float* census)
{
    for (int s = 0; s < les::kCvNA; s++) ad[s] = (float)(0.5 * (1.0 - std::exp(-((double)s / 3.0) / (double)lambda_ad)));
    for (int h = 0; h < les::kCvNC; h++) census[h] = (float)(0.5 * (1.0 - std::exp(-(double)h / (double)lambda_census)));
}

// non-temporal stores in the volume kernel: LES_HIP_COSTVOL_NT=1 / 0 overrides the default; read per call.  Measured (DESIGN 3.2f): the medians
// with the hint are 0.2 .. 3.6 % below those without it in all four shape / mode pairs, inside the spread of the runs -- the hint stays on
constexpr bool kCvNontemporalDefault = true;
bool cv_env_flag(const char* name, bool dflt)
{
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

// LES_HIP_COSTVOL_TIMING=1: the call brackets its census launches and its volume launch with events; the calling thread reads the device
// milliseconds of its last build with les_hip_costvol_last_times (tools/costvol_timing.py: the call as a whole also allocates and frees)
thread_local float tl_cv_ms[2] = {-1.0f, -1.0f};

}  // namespace

extern "C" {

int les_hip_costvol_tables(float lambda_ad, float lambda_census, float* ad766_host, float* census63_host)
{
    if (!ad766_host || !census63_host) return fail(LES_HIP_ERR_ARG, "les_hip_costvol_tables: null table");
    if (!cv_lambda_ok(lambda_ad) || !cv_lambda_ok(lambda_census))
        return fail(LES_HIP_ERR_ARG, "les_hip_costvol_tables: lambda_ad %g, lambda_census %g (positive and finite)", (double)lambda_ad, (double)lambda_census);
    cv_tables(lambda_ad, lambda_census, ad766_host, census63_host);
    return LES_HIP_OK;
}

int les_hip_census(const uint8_t* d_bgr, unsigned long long* d_sig, int H, int W, int device, void* stream)
{
    if (!d_bgr || !d_sig || H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "les_hip_census: bad argument");
    HIPCHECK(hipSetDevice(device));
    uint32_t* no_packed = nullptr;
    hipLaunchKernelGGL(les::les_census_kernel, dim3((W + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, d_bgr, d_sig, no_packed, H, W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

int les_hip_build_cost_volume(const uint8_t* d_imL, const uint8_t* d_imR, float* d_vol, int D, int H, int W, int mode, int d0, float lambda_ad,
                              float lambda_census, int device, void* stream)
{
    if (!d_imL || !d_imR || !d_vol || D <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 1) return fail(LES_HIP_ERR_ARG, "les_hip_build_cost_volume: bad argument");
    if (!cv_lambda_ok(lambda_ad) || !cv_lambda_ok(lambda_census))
        return fail(LES_HIP_ERR_ARG, "les_hip_build_cost_volume: lambda_ad %g, lambda_census %g (positive and finite)", (double)lambda_ad, (double)lambda_census);
    if ((unsigned long long)D * H * W >= (1ull << 32)) return fail(LES_HIP_ERR_UNSUPPORTED, "volumes of 2^32 or more floats are not supported");
    if (H > 65535 || (D + les::kCvDC - 1) / les::kCvDC > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "image height %d / %d slices exceed the launch grid", H, D);
    HIPCHECK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)H * W;
#if !defined(LES_SIM)
    struct Events {                                        // (destroyed on every return path)
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t q : e) if (q) (void)hipEventDestroy(q); }
    } ev;
    const bool timing = cv_env_flag("LES_HIP_COSTVOL_TIMING", false);
    if (timing)
        for (hipEvent_t& q : ev.e) HIPCHECK(hipEventCreate(&q));
#endif
    DevBuf<unsigned long long> sig;                        // both views' signatures, [2][H][W]
    DevBuf<uint32_t> col;                                  // ... and packed colours
    DevBuf<float> tab;                                     // ta, tc
    int rc;
    if ((rc = sig.alloc(2 * P)) || (rc = col.alloc(2 * P)) || (rc = tab.alloc(les::kCvNA + les::kCvNC))) return rc;
    std::vector<float> h_tab(les::kCvNA + les::kCvNC);
    cv_tables(lambda_ad, lambda_census, h_tab.data(), h_tab.data() + les::kCvNA);
    HIPCHECK(hipMemcpyAsync(tab.p, h_tab.data(), h_tab.size() * sizeof(float), hipMemcpyHostToDevice, st));
#if !defined(LES_SIM)
    if (timing) HIPCHECK(hipEventRecord(ev.e[0], st));
#endif
    const uint8_t* im[2] = {d_imL, d_imR};
    for (int v = 0; v < 2; v++) {
        const uint8_t* bgr = im[v];
        unsigned long long* s = sig.p + v * P;
        uint32_t* c = col.p + v * P;
        hipLaunchKernelGGL(les::les_census_kernel, dim3((W + 255) / 256, H), dim3(256), 0, st, bgr, s, c, H, W);
    }
    // mode 0: the left view's pixels against the right view's row; mode 1: the other way round
    const unsigned long long *sigI = sig.p + mode * P, *sigJ = sig.p + (1 - mode) * P;
    const uint32_t *colI = col.p + mode * P, *colJ = col.p + (1 - mode) * P;
    const float *ta = tab.p, *tc = tab.p + les::kCvNA;
    const dim3 grid((W + les::kCvTX - 1) / les::kCvTX, H, (D + les::kCvDC - 1) / les::kCvDC), block(256);
#if !defined(LES_SIM)
    if (timing) HIPCHECK(hipEventRecord(ev.e[1], st));
#endif
    const bool vec = (W % 4 == 0) && (((uintptr_t)d_vol & 15) == 0);           // every row of every slice starts 16-byte aligned
    if (!vec)
        hipLaunchKernelGGL((les::les_costvol_kernel<false, false>), grid, block, 0, st, sigI, colI, sigJ, colJ, ta, tc, d_vol, D, H, W, mode, d0);
    else if (cv_env_flag("LES_HIP_COSTVOL_NT", kCvNontemporalDefault))
        hipLaunchKernelGGL((les::les_costvol_kernel<true, true>), grid, block, 0, st, sigI, colI, sigJ, colJ, ta, tc, d_vol, D, H, W, mode, d0);
    else
        hipLaunchKernelGGL((les::les_costvol_kernel<true, false>), grid, block, 0, st, sigI, colI, sigJ, colJ, ta, tc, d_vol, D, H, W, mode, d0);
    HIPCHECK(hipGetLastError());
#if !defined(LES_SIM)
    if (timing) HIPCHECK(hipEventRecord(ev.e[2], st));
#endif
    HIPCHECK(hipStreamSynchronize(st));                    // the scratch above is freed on return
#if !defined(LES_SIM)
    if (timing) {
        HIPCHECK(hipEventElapsedTime(&tl_cv_ms[0], ev.e[0], ev.e[1]));
        HIPCHECK(hipEventElapsedTime(&tl_cv_ms[1], ev.e[1], ev.e[2]));
    }
#endif
    return LES_HIP_OK;
}

int les_hip_costvol_last_times(float* census_ms, float* volume_ms)
{
    if (!census_ms || !volume_ms) return fail(LES_HIP_ERR_ARG, "les_hip_costvol_last_times: null argument");
    if (tl_cv_ms[1] < 0.0f) return fail(LES_HIP_ERR_ARG, "les_hip_costvol_last_times: this thread has run no build with LES_HIP_COSTVOL_TIMING=1");
    *census_ms = tl_cv_ms[0];
    *volume_ms = tl_cv_ms[1];
    return LES_HIP_OK;
}

}  // extern "C"
