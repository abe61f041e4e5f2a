// les_hip_unary.inc -- part of the single translation unit les_hip.hip (inside its anonymous namespace): the unary costs of a list of
// calls.  build_unary_tables builds a UnaryTables (les_hip.hip) once per batch (les_hip_batch_create) or per rect pair of a scratch
// (les_hip_unary_one_scratch); run_unary is the one router both run through, and unary_kind the one place that decides which kernel serves
// a run.  The launches themselves are les_hip_march.inc's, les_hip_vdisp.inc's and les_hip_bilateral.inc's.

// compact: one call, its outputs in a tile of its target rect's size (row stride = target width, origin = target corner); otherwise map /
// slab coordinates (out_slabs as for les_hip_batch_create)
int build_unary_tables(les_hip_ctx* c, int n, const les_hip_rect* frs, const les_hip_rect* trs, int out_slabs, bool compact, UnaryTables& t)
{
    for (int i = 0; i < n; i++) {
        int rc = check_rects(c, frs[i], trs[i]);
        if (rc) return rc;
    }
    t.n = n;
    const long long P = (long long)c->p.H * c->p.W;
    // raw-cost patches of the calls with a non-empty target, and where each target rect is written
    std::vector<les::RawCall> calls((size_t)n);
    std::vector<long long> raw_off((size_t)n), out_off((size_t)n);
    long long amax = 1;
    for (int i = 0; i < n; i++) {
        const les_hip_rect &f = frs[i], &r = trs[i];
        const bool live = r.w > 0 && r.h > 0;
        const long long a = live ? (long long)f.w * f.h : 0;
        calls[i] = les::RawCall{f.x, f.y, live ? f.w : 0, live ? f.h : 0, t.raw_floats};
        raw_off[i] = t.raw_floats;
        out_off[i] = compact ? 0 : (out_slabs ? (long long)(i / out_slabs) * P : 0) + (long long)r.y * c->p.W + r.x;
        t.raw_floats += a; amax = std::max(amax, a);
    }
    t.raw_chunks = (int)std::min<long long>(1024, std::max<long long>(1, (amax + 4095) / 4096));
    t.out_stride = compact ? trs[0].w : c->p.W;
    std::vector<les::Job> jobs, mjobs;
    std::vector<les::BfJob> bfjobs;
    std::vector<les::RawCall> vd_calls;
    std::vector<float4> vd_stand;
    if (c->filter == LES_HIP_FILTER_GF) {
        int rc = build_jobs(c, n, frs, trs, out_slabs, jobs);
        if (rc) return rc;
        bool mok = false;
        build_march_jobs(c, n, frs, trs, out_slabs, mjobs, mok, t.mentry);
        t.march_ok = mok && !mjobs.empty();
        if (t.march_ok && c->naive && t.raw_floats > kRawPatchCapFloats) {
            t.march_ok = false;
            note_fallback(c->fallback_seen, FB_PATCHES, "the raw-cost patches of one batch of the image-based energy exceed 4 GB");
        }
        if (!t.march_ok) mjobs.clear();
        if (compact)
            for (auto* v : {&jobs, &mjobs})
                for (les::Job& j : *v) { j.out_off = (long long)(j.ty0 - trs[0].y) * trs[0].w + (j.tx0 - trs[0].x); j.out_stride = trs[0].w; }
        if (c->naive) vdisp_layout(c, n, frs, trs, t, vd_calls, vd_stand);
    } else {
        if (t.raw_floats > kRawPatchCapFloats)
            return fail(LES_HIP_ERR_UNSUPPORTED, "the raw-cost patches of one batch exceed 4 GB (%lld floats): split the batch", t.raw_floats);
        int rc = build_bf_jobs(c, n, frs, trs, out_slabs, compact, bfjobs, t.bf_np);
        if (rc) return rc;
    }
    t.njobs = (int)jobs.size();
    t.nmgroups = t.march_ok ? (int)(mjobs.size() / t.mentry->NJ) : 0;
    t.nbfjobs = (int)bfjobs.size();
    // one upload: every table at a 256-byte aligned offset of one allocation
    std::vector<char> blob;
    auto put = [&](const auto& v) -> size_t {
        if (v.empty()) return SIZE_MAX;
        const size_t off = (blob.size() + 255) & ~(size_t)255, bytes = v.size() * sizeof(v[0]);
        blob.resize(off + bytes);
        memcpy(blob.data() + off, v.data(), bytes);
        return off;
    };
    static_assert(sizeof(les::WtaJob) == sizeof(les_hip_rect), "rect layout");
    const std::vector<les_hip_rect> targets(trs, trs + n);
    const size_t o_jobs = put(jobs), o_mjobs = put(mjobs), o_calls = put(calls), o_raw_off = put(raw_off), o_targets = put(targets),
                 o_out_off = put(out_off), o_bfjobs = put(bfjobs), o_vd_calls = put(vd_calls), o_vd_stand = put(vd_stand);
    if (blob.empty()) return LES_HIP_OK;
    int rc = t.mem.alloc(blob.size());
    if (rc) return rc;
    HIPCHECK(hipMemcpy(t.mem.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    auto at = [&](size_t off) -> const void* { return off == SIZE_MAX ? nullptr : t.mem.p + off; };
    t.d_jobs = static_cast<const les::Job*>(at(o_jobs));
    t.d_mjobs = static_cast<const les::Job*>(at(o_mjobs));
    t.d_rawcalls = static_cast<const les::RawCall*>(at(o_calls));
    t.d_raw_off = static_cast<const long long*>(at(o_raw_off));
    t.d_targets = static_cast<const les::WtaJob*>(at(o_targets));
    t.d_out_off = static_cast<const long long*>(at(o_out_off));
    t.d_bfjobs = static_cast<const les::BfJob*>(at(o_bfjobs));
    t.d_vd_calls = static_cast<const les::RawCall*>(at(o_vd_calls));
    t.d_vd_stand_in = static_cast<const float4*>(at(o_vd_stand));
    return LES_HIP_OK;
}

// Which kernel serves the calls of t for view `mode` (the view checked by the caller): 2 the bilateral / unfiltered kernel; 1 the march kernel
// (behind a raw-cost pre-pass for the image-based energy and at interpolation 0 / 2; at 2 the flagged calls are recomputed on the strip
// kernel); 0 the strip kernel
int unary_kind(const les_hip_ctx* c, const UnaryTables& t, int mode)
{
    if (c->filter != LES_HIP_FILTER_GF) return 2;
    if (!t.march_ok) return 0;
    if (c->naive || c->interp == 1) return c->march && c->v[mode].march_ok ? 1 : 0;
    return interp_march_ok(c, mode) && t.raw_floats <= kRawPatchCapFloats ? 1 : 0;
}

// The unary costs of the calls of t for view `mode` into d_out (t's layout), on `stream`
int run_unary(les_hip_ctx* c, const UnaryTables& t, UnaryWorkspace& w, int mode, const float4* d_planes, float* d_out, int check, hipStream_t stream)
{
    int rc = view_ok(c, mode);
    if (rc) return rc;
    const int kind = unary_kind(c, t, mode);
    const bool patches = kind == 2 || (kind == 1 && (c->naive || c->interp != 1));
    const bool vdisp = kind == 0 && c->naive;
    const bool masked = vdisp || (kind == 1 && !c->naive && c->interp == 2);      // flags and masked strip jobs of a recompute launch
    UnaryWorkspace::Slot& s = w.slot[w.shared ? mode : 0];
    if (patches || masked) {
        std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
        if (w.shared) lk.lock();
        // (a batch's tables are fixed: exact sizes; a scratch's change with its rect pairs: room for the usual ones at once)
        const size_t min_raw = w.shared ? 1 : 256 * 256, min_jobs = w.shared ? 1 : 64;
        if (patches) rc = s.raw.grow((size_t)std::max<long long>(t.raw_floats, 1), min_raw, stream);
        if (!rc && masked) rc = s.flags.grow((size_t)std::max(t.n, 1), 1, stream);
        if (!rc && masked) rc = s.rjobs.grow((size_t)std::max(t.njobs, 1), min_jobs, stream);
        if (!rc && vdisp) rc = s.vol.grow(std::max<size_t>((size_t)t.vd_max_slices * c->p.H * c->p.W, 1), 1, stream);
        if (rc) return rc;
    }
    const RawPatches rp{t.d_rawcalls, t.d_raw_off, s.raw.p, t.n, t.raw_chunks};
    if (kind == 2) return launch_bf(c, mode, t.d_bfjobs, t.nbfjobs, t.bf_np, t.d_rawcalls, t.n, t.raw_chunks, s.raw.p, d_planes, d_out, check, stream);
    if (kind == 1) {
        if (c->naive) return launch_naive_march(c, t.mentry, mode, t.d_mjobs, t.nmgroups, d_planes, d_out, check, stream, rp);
        if (c->interp == 1) return launch_march(c, t.mentry, mode, t.d_mjobs, t.nmgroups, d_planes, d_out, check, stream);
        return launch_interp_march(c, t.mentry, mode, t.d_mjobs, t.nmgroups, rp, s.flags.p, t.d_jobs, s.rjobs.p, t.njobs, t.d_targets, t.d_out_off,
                                   t.out_stride, d_planes, d_out, check, stream);
    }
    if (!c->naive && c->interp != 1 && t.march_ok && interp_march_ok(c, mode))
        note_fallback(c->fallback_seen, FB_PATCHES, "the raw-cost patches of one batch at interpolation %d exceed 4 GB", c->interp);
    rc = launch_strips(c, mode, t.d_jobs, t.njobs, d_planes, d_out, check, stream);
    if (rc) return rc;
    if (vdisp) return launch_vdisp_strips(c, t, s.vol.p, s.flags.p, s.rjobs.p, mode, d_planes, d_out, check, stream);
    if (!c->naive && c->interp != 1)
        return launch_nan_spread(c, mode, t.n, t.d_rawcalls, t.d_targets, t.d_out_off, t.out_stride, d_planes, nullptr, d_out, check, stream);
    return LES_HIP_OK;
}
