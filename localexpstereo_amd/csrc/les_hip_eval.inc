// les_hip_eval.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): evaluation of the device-resident
// solution on the device (les_eval.h) -- the progress log of the Evaluator and the region energies of the flow == energy self-check
struct les_hip_evaluator {
    les_hip_ctx* c = nullptr;
    DevBuf<float> d_gt;                  // H * W floats, or empty: no ground truth
    DevBuf<uint8_t> d_nonocc;            // H * W bytes, or empty: every pixel counts as non-occluded
    float threshold = 0.5f, precision = -1.0f;
    int max_rows = 0, rows = 0;          // rows: enqueued so far (host count; the device has written them once its stream has run)
    DevBuf<les::EvalRecord> d_log;
    DevBuf<les::EvalPartial> d_part;     // one slot per tile of les_eval_kernel
    dim3 grid;
};

static_assert(sizeof(les_hip_eval_row) == sizeof(les::EvalRecord) && sizeof(les::EvalRecord) == 56, "les_hip_eval_row and les::EvalRecord are one layout");

extern "C" {

int les_hip_evaluator_create(les_hip_ctx* c, const float* gt_host, const unsigned char* nonocc_host, float error_threshold, float precision, int max_rows,
                             les_hip_evaluator** out)
{
    if (!c || !out) return fail(LES_HIP_ERR_ARG, "null argument");
    *out = nullptr;
    if (max_rows <= 0) return fail(LES_HIP_ERR_ARG, "max_rows %d (at least 1)", max_rows);
    if (nonocc_host && !gt_host) return fail(LES_HIP_ERR_ARG, "a non-occlusion mask without ground truth");
    HIPCHECK(hipSetDevice(c->p.device));
    les_hip_evaluator* ev = new les_hip_evaluator();
    ev->c = c;
    ev->threshold = error_threshold; ev->precision = precision; ev->max_rows = max_rows;
    ev->grid = dim3((unsigned)((c->p.W + les::kEvTW - 1) / les::kEvTW), (unsigned)((c->p.H + les::kEvTH - 1) / les::kEvTH));
    const size_t P = (size_t)c->p.H * c->p.W, slots = (size_t)ev->grid.x * ev->grid.y;
    bool ok = !ev->d_log.alloc((size_t)max_rows) && !ev->d_part.alloc(slots);
    if (ok && gt_host) ok = !ev->d_gt.alloc(P) && hipMemcpy(ev->d_gt.p, gt_host, P * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && nonocc_host) ok = !ev->d_nonocc.alloc(P) && hipMemcpy(ev->d_nonocc.p, nonocc_host, P, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        delete ev;
        return fail(LES_HIP_ERR_DEVICE, "les_hip_evaluator_create: device allocation or upload failed");
    }
    *out = ev;
    return LES_HIP_OK;
}

void les_hip_evaluator_destroy(les_hip_evaluator* ev)
{
    delete ev;
}

int les_hip_evaluate(les_hip_ctx* c, les_hip_evaluator* ev, int mode, const les_hip_plane* d_labels, const float* d_cost, float lambda, float th_smooth,
                     float omega, float epsilon, int index)
{
    if (!c || !ev || !d_labels || !d_cost) return fail(LES_HIP_ERR_ARG, "null argument");
    if (ev->c != c) return fail(LES_HIP_ERR_ARG, "the evaluator belongs to another context");
    if (mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    if (ev->rows >= ev->max_rows) return fail(LES_HIP_ERR_ARG, "les_hip_evaluate: the log is full (%d rows)", ev->max_rows);
    HIPCHECK(hipSetDevice(c->p.device));                     // the calling host thread may be new (one thread per view)
    const int trc = pw_table(c, omega, epsilon);             // (first call, or other parameters than the last one: builds the table)
    if (trc) return trc;
    const les::EvalParams p{c->p.H, c->p.W, lambda, th_smooth, ev->threshold, ev->precision};
    const float4* lab = reinterpret_cast<const float4*>(d_labels);
    const uint32_t* ipk = c->v[mode].ipk;
    const float *wtab = c->d_pw_tab.p, *gt = ev->d_gt.p;
    const uint8_t* nonocc = ev->d_nonocc.p;
    les::EvalPartial* part = ev->d_part.p;
    les::EvalRecord* row = ev->d_log.p + ev->rows;
    const int nslots = (int)(ev->grid.x * ev->grid.y);
    hipLaunchKernelGGL(les::les_eval_kernel, ev->grid, dim3(256), 0, cur_stream(c), lab, d_cost, ipk, wtab, gt, nonocc, p, part);
    hipLaunchKernelGGL(les::les_eval_finish_kernel, dim3(1), dim3(256), 0, cur_stream(c), part, nslots, index, mode, row);
    HIPCHECK(hipGetLastError());
    ev->rows++;
    return LES_HIP_OK;
}

int les_hip_evaluator_rows(les_hip_ctx* c, les_hip_evaluator* ev, les_hip_eval_row* rows_host, int capacity, int* n)
{
    if (!c || !ev || !n) return fail(LES_HIP_ERR_ARG, "null argument");
    if (ev->c != c) return fail(LES_HIP_ERR_ARG, "the evaluator belongs to another context");
    *n = ev->rows;
    if (ev->rows == 0) return LES_HIP_OK;
    if (!rows_host || capacity < ev->rows) return fail(LES_HIP_ERR_ARG, "les_hip_evaluator_rows: room for %d rows, %d written", rows_host ? capacity : 0, ev->rows);
    HIPCHECK(hipSetDevice(c->p.device));
    HIPCHECK(hipMemcpyAsync(rows_host, ev->d_log.p, (size_t)ev->rows * sizeof(les::EvalRecord), hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    return LES_HIP_OK;
}

int les_hip_batch_region_energy(les_hip_ctx* c, const les_hip_batch* b, int mode, const les_hip_plane* d_labels, const float* d_cost, float lambda,
                                float th_smooth, float omega, float epsilon, double* d_energy)
{
    if (!c || !b || !d_labels || !d_cost || !d_energy) return fail(LES_HIP_ERR_ARG, "null argument");
    if (mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    if (b->n == 0) return LES_HIP_OK;
    HIPCHECK(hipSetDevice(c->p.device));
    const int trc = pw_table(c, omega, epsilon);
    if (trc) return trc;
    {
        std::lock_guard<std::mutex> lk(b->re_mu);
        if (b->region_chunks < 0) {
            long long most = 1;                              // pixels of the largest cell's region grown by one
            for (const les_hip_rect& t : b->targets) most = std::max(most, (long long)(std::max(0, t.w) + 2) * (std::max(0, t.h) + 2));
            b->region_chunks = (int)((most + les::kRegChunk - 1) / les::kRegChunk);
        }
        if (!b->d_region_part[mode].p) {
            const int rc = b->d_region_part[mode].alloc((size_t)b->n * b->region_chunks);
            if (rc) return rc;
        }
    }
    const les::PairwiseParams pp{c->p.H, c->p.W, lambda, th_smooth};
    const les::GraphCell* cells = reinterpret_cast<const les::GraphCell*>(b->d_targets.p);
    const float4* lab = reinterpret_cast<const float4*>(d_labels);
    const uint32_t* ipk = c->v[mode].ipk;
    const float* wtab = c->d_pw_tab.p;
    double* part = b->d_region_part[mode].p;
    const int n = b->n, chunks = b->region_chunks, W = c->p.W, H = c->p.H;
    hipLaunchKernelGGL(les::les_region_energy_kernel, dim3(n, chunks), dim3(256), 0, cur_stream(c), cells, lab, d_cost, ipk, wtab, pp, part);
    hipLaunchKernelGGL(les::les_region_energy_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, cur_stream(c), cells, n, W, H, (const double*)part, chunks, d_energy);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
