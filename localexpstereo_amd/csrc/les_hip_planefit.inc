// les_hip_planefit.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): slanted planes fitted to a disparity map (les_planefit.h holds the definition and the kernel) -- the weight tables the context keeps per sig, and the entry point
// The tables of les_hip_fit_planes, one per sig seen, never rewritten: a launch in flight on another stream keeps reading its own.
struct FitTables {
    struct Entry { float sig; DevBuf<float> tab; };
    std::vector<Entry> entries;
};

namespace {

constexpr size_t kFitTabCache = 8;          // tables kept; one more distinct sig waits for the device and starts over

void fit_tables_free(FitTables* t) { delete t; }

// wtab[k] = (float)exp(-k / sig) in double, k = 0 .. 765; sig == 0: all ones.  A new sig uploads on the calling thread's stream and waits for it.
int fit_table(les_hip_ctx* c, float sig, const float** d_tab)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->fit_tables) c->fit_tables = new FitTables();
    FitTables* t = c->fit_tables;
    for (auto& e : t->entries)
        if (e.sig == sig) { *d_tab = e.tab.p; return LES_HIP_OK; }
    if (t->entries.size() >= kFitTabCache) {
        HIPCHECK(hipDeviceSynchronize());                    // (launches on any stream may still read the tables that go)
        t->entries.clear();
    }
    std::vector<float> tab(les::kBfTabSize);
    for (int k = 0; k < les::kBfTabSize; k++) tab[(size_t)k] = sig == 0.0f ? 1.0f : (float)std::exp(-(double)k / (double)sig);
    FitTables::Entry e;
    e.sig = sig;
    const int rc = e.tab.alloc(tab.size());
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(e.tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    *d_tab = e.tab.p;
    t->entries.push_back(std::move(e));
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_fit_planes(les_hip_ctx* c, int mode, const les_hip_plane* d_labels, const float* d_disp, const les_hip_plane* d_fallback, les_hip_plane* d_out,
                       unsigned char* d_kind, int radius, float sig, float gate0, float gate_slope, float max_slope, int min_support)
{
    if (!c || !d_out) return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: null argument");
    if ((d_labels != nullptr) == (d_disp != nullptr)) return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: give a label map or a disparity map, exactly one");
    if (mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: view %d was not supplied at creation", mode);
    if ((const void*)d_out == (const void*)d_labels || (const void*)d_out == (const void*)d_disp)
        return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: d_out may be d_fallback, not the input map");
    if (radius < 1) return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: radius %d", radius);
    if (radius > les::kFitMaxR) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_fit_planes: radius %d, at most %d is supported", radius, les::kFitMaxR);
    // (written so that a NaN is refused)
    if (!(sig >= 0.0f && sig < INFINITY) || !(gate0 > 0.0f && gate0 < INFINITY) || !(gate_slope >= 0.0f && gate_slope < INFINITY) ||
        !(max_slope > 0.0f && max_slope < INFINITY) || min_support < 3)
        return fail(LES_HIP_ERR_ARG, "les_hip_fit_planes: sig %g (>= 0), gate0 %g (> 0), gate_slope %g (>= 0), max_slope %g (> 0), min_support %d (>= 3)", (double)sig,
                    (double)gate0, (double)gate_slope, (double)max_slope, min_support);
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    const float* d_tab = nullptr;
    const int rc = fit_table(c, sig, &d_tab);
    if (rc) return rc;
    const les::FitParams fp = {radius, min_support, gate0, gate_slope, max_slope};
    const dim3 grid((unsigned)((c->p.W + les::kFitTX - 1) / les::kFitTX), (unsigned)((c->p.H + les::kFitTY - 1) / les::kFitTY));
    const uint32_t* d_ipk = c->v[mode].ipk;
    hipLaunchKernelGGL(les::les_plane_fit_kernel, grid, dim3(les::kFitThreads), 0, cur_stream(c), c->geom, d_ipk, d_tab, reinterpret_cast<const float4*>(d_labels),
                       d_disp, reinterpret_cast<const float4*>(d_fallback), reinterpret_cast<float4*>(d_out), d_kind, fp);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
