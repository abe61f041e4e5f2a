// les_hip_dense.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the unary costs of a whole
// label map in one dense pass (csrc/les_dense.h) -- which instantiations exist, the launch, and the two entry points of the C ABI
namespace {

typedef void (*DenseKernel)(les::Geom, les::View, les::DenseArgs, const float*, const float4*, float*);
// guided filter: one entry per radius, its four raw-cost sources (cost volume linear, image-based, cost volume at interpolation 0 / 2)
struct DenseEntry { int R, NT, TX, TY; DenseKernel fn[4]; };
#define LES_DENSE_ENTRY(R_) \
    { R_, les::DenseCfg<R_>::NT, les::DenseCfg<R_>::TX, les::DenseCfg<R_>::TY, \
      { les::les_dense_kernel<R_, 0, 0>, les::les_dense_kernel<R_, 1, 0>, les::les_dense_kernel<R_, 2, 0>, les::les_dense_kernel<R_, 3, 0> } }
// every radius kStrips / kNaiveStrips / the interpolation tables serve (les_hip_march_tables.inc), so no context falls back to per-pixel jobs
const DenseEntry kDense[] = {
    LES_DENSE_ENTRY(1), LES_DENSE_ENTRY(2), LES_DENSE_ENTRY(3), LES_DENSE_ENTRY(4), LES_DENSE_ENTRY(5), LES_DENSE_ENTRY(6),
    LES_DENSE_ENTRY(7), LES_DENSE_ENTRY(8), LES_DENSE_ENTRY(9), LES_DENSE_ENTRY(10), LES_DENSE_ENTRY(12), LES_DENSE_ENTRY(15),
};
// bilateral / unfiltered: the direct form, radius at run time
const DenseKernel kDenseDirect[4] = { les::les_dense_kernel<0, 0, 1>, les::les_dense_kernel<0, 1, 1>, les::les_dense_kernel<0, 2, 1>, les::les_dense_kernel<0, 3, 1> };

const DenseEntry* find_dense(int R)
{
    for (const auto& e : kDense)
        if (e.R == R) return &e;
    return nullptr;
}

// what a dense pass of view `mode` reads was supplied at creation
int dense_view_ok(const les_hip_ctx* c, int mode)
{
    int rc = view_ok(c, mode);
    if (rc) return rc;
    if (c->filter == LES_HIP_FILTER_GF && !c->v[mode].stats) return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    return LES_HIP_OK;
}

}  // namespace

extern "C" {

int les_hip_unary_labels_kind(const les_hip_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 1) return -1;
    if (c->filter != LES_HIP_FILTER_GF) return 1;
    return find_dense(c->R) ? 1 : 0;
}

int les_hip_unary_labels(les_hip_ctx* c, int mode, const les_hip_rect* region, const les_hip_plane* d_labels, float* d_cost, int check)
{
    if (!c || !d_labels || !d_cost) return fail(LES_HIP_ERR_ARG, "null argument");
    (void)hipSetDevice(c->p.device);                        // HIP's current device is per host thread
    int rc = dense_view_ok(c, mode);
    if (rc) return rc;
    les_hip_rect r{0, 0, c->p.W, c->p.H};
    if (region) r = *region;
    if (r.w < 0 || r.h < 0) return fail(LES_HIP_ERR_ARG, "negative region size");
    if (r.w == 0 || r.h == 0) return LES_HIP_OK;
    if (r.x < 0 || r.y < 0 || r.x > c->p.W - r.w || r.y > c->p.H - r.h)
        return fail(LES_HIP_ERR_ARG, "region (%d, %d, %d x %d) outside the %d x %d image", r.x, r.y, r.w, r.h, c->p.W, c->p.H);
    const int src = c->naive ? 1 : (c->interp == 1 ? 0 : (c->interp == 0 ? 2 : 3));
    const les::View view = strip_view(c, mode);
    const float4* labels = reinterpret_cast<const float4*>(d_labels);
    if (c->filter == LES_HIP_FILTER_GF) {
        const DenseEntry* e = find_dense(c->R);
        if (!e) return fail(LES_HIP_ERR_UNSUPPORTED, "no dense kernel for guided-filter radius %d (windR %d)", c->R, c->p.windR);
        const les::DenseArgs a{r.x, r.y, r.w, r.h, c->p.windR, check};
        const long long tiles = (long long)((r.w + e->TX - 1) / e->TX) * ((r.h + e->TY - 1) / e->TY);
        hipLaunchKernelGGL(e->fn[src], dim3((unsigned)tiles), dim3(e->NT), 0, cur_stream(c), c->geom, view, a, (const float*)nullptr, labels, d_cost);
    } else {
        const les::DenseArgs a{r.x, r.y, r.w, r.h, c->R, check};      // (c->R: windR of the bilateral filter, 0 without aggregation)
        const long long tiles = (long long)((r.w + les::DENSE_BF_T - 1) / les::DENSE_BF_T) * ((r.h + les::DENSE_BF_T - 1) / les::DENSE_BF_T);
        hipLaunchKernelGGL(kDenseDirect[src], dim3((unsigned)tiles), dim3(64 * les::DENSE_BF_NW), 0, cur_stream(c), c->geom, view, a, (const float*)c->d_bf_tab.p,
                           labels, d_cost);
    }
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
