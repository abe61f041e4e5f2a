// les_hip_cuts.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the expansion and fusion moves on the device -- graph capacities, the LDS max-flow, the tiled max-flow with its hand-over to the host cores, mask application
// Host side of one tiled solve in flight: the host-mapped words the kernels report through (pinned, fine-grained: the kernel adds to them with
// system-scope atomics, the host reads them after synchronising its stream -- the progress check of a lock-step costs no copy) and the pinned
// staging of the hand-over (les_maxflow_tiled.h: residual graphs out, masks and flow values back).  A context keeps a pool of them: a call
// takes one, returns it at the end; they are freed with the context (round 5 kept two words per host THREAD for ever).
struct MtHost {
    // (h_*: the pinned owners; d_*: the addresses the device reaches them at)
    PinnedBuf<int> h_flags; int* d_flags = nullptr;                    // [0] cells finished, [1] of them: gave up, [2] cells handed over, [3] their nodes
    PinnedBuf<char> h_stage; char* d_stage = nullptr;                  // rc8 [cap_nodes][8] floats | ex [cap_nodes] floats | masks [cap_nodes] bytes | list [cap_cells] | flows [cap_cells]
    long long cap_nodes = 0;
    int cap_cells = 0;
    size_t off_ex() const { return (size_t)cap_nodes * 32; }
    size_t off_masks() const { return (size_t)cap_nodes * 36; }
    size_t off_list() const { return ((size_t)cap_nodes * 37 + 255) & ~(size_t)255; }
    size_t off_flows() const { return off_list() + (size_t)cap_cells * sizeof(les::MtHandCell); }
    size_t bytes() const { return off_flows() + (size_t)cap_cells * sizeof(double); }
};
namespace {
void mt_host_free(MtHost* m) { delete m; }                 // (les_hip_destroy sees MtHost only declared)
#if defined(LES_SIM)
constexpr unsigned kMtHostFlags = 0;
#else
constexpr unsigned kMtHostFlags = hipHostMallocMapped | hipHostMallocCoherent;
#endif
int mt_host_acquire(les_hip_ctx* c, MtHost** out)
{
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->mt_idle.empty()) { *out = c->mt_idle.back(); c->mt_idle.pop_back(); return LES_HIP_OK; }
    }
    MtHost* m = new MtHost();
    int rc = m->h_flags.alloc(16, kMtHostFlags);
    if (!rc) rc = m->h_flags.dev(&m->d_flags);
    if (rc) { delete m; return rc; }
    *out = m;
    return LES_HIP_OK;
}
void mt_host_release(les_hip_ctx* c, MtHost* m)
{
    std::lock_guard<std::mutex> lk(c->mu);
    c->mt_idle.push_back(m);
}
// staging for `nodes` graph nodes (37 bytes each) of `cells` cells, grown on demand
int mt_host_stage(MtHost* m, long long nodes, int cells, hipStream_t stream)
{
    if (m->cap_nodes >= nodes && m->cap_cells >= cells) return LES_HIP_OK;
    m->cap_nodes = std::max(m->cap_nodes, (nodes + 4095) & ~4095ll);
    m->cap_cells = std::max(m->cap_cells, (cells + 15) & ~15);
    int rc = m->h_stage.grow(m->bytes(), 0, stream, kMtHostFlags);      // (bytes() has grown: always a new buffer)
    if (!rc) rc = m->h_stage.dev(&m->d_stage);
    if (rc) { m->h_stage.reset(); m->cap_nodes = 0; m->cap_cells = 0; return rc; }
    return LES_HIP_OK;
}
// The context's smoothness-coefficient table for (omega, epsilon), rebuilt (and the calling thread's stream synchronised) only when they change:
// initSmoothnessCoeff (LES/StereoEnergy.h:131-163), max(epsilon, exp(-|dI|_1 / omega)) in float.  Shared by the graph construction and the
// evaluation kernels (les_hip_eval.inc).
int pw_table(les_hip_ctx* c, float omega, float epsilon)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->pw_omega == omega && c->pw_epsilon == epsilon && c->d_pw_tab.p) return LES_HIP_OK;
    std::vector<float> tab(766);
    for (int k = 0; k < 766; k++) tab[k] = std::max(epsilon, std::exp(-(float)k / omega));
    if (!c->d_pw_tab.p) {
        const int rc = c->d_pw_tab.alloc(tab.size());
        if (rc) return rc;
    }
    HIPCHECK(hipMemcpyAsync(c->d_pw_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream(c)));
    HIPCHECK(hipStreamSynchronize(cur_stream(c)));
    c->pw_omega = omega; c->pw_epsilon = epsilon;
    return LES_HIP_OK;
}
struct MtHostLease {                       // returns the MtHost to the pool on every exit path
    les_hip_ctx* c; MtHost* m;
    ~MtHostLease() { if (m) mt_host_release(c, m); }
};
// the cells of a lock-step as the kernels take them (les_hip_rect has GraphCell's layout: les_hip_batch.inc)
const les::GraphCell* graph_cells(const les_hip_batch* b) { return reinterpret_cast<const les::GraphCell*>(b->d_targets.p); }
// The graphs of one lock-step of moves (les_pairwise.h).  map: d_proposal is a label map [H][W] (fusion); otherwise one plane per cell (expansion).
// flow0_host (may be null): per cell, the chunks' t-link flows summed in chunk order after a synchronise.
int move_graph(bool map, les_hip_ctx* c, const les_hip_batch* b, int mode, const les_hip_plane* d_proposal, const les_hip_plane* d_labels, const float* d_cur,
               const float* d_prop, float lambda, float th_smooth, float omega, float epsilon, float* d_payload, double* flow0_host, int* d_nonsubmodular)
{
    if (!c || !b || !d_proposal || !d_labels || !d_cur || !d_prop || !d_payload) return fail(LES_HIP_ERR_ARG, "null argument");
    if (mode < 0 || mode > 1 || !c->v[mode].ipk) return fail(LES_HIP_ERR_ARG, "view %d was not supplied at creation", mode);
    if (b->n == 0) return LES_HIP_OK;
    HIPCHECK(hipSetDevice(c->p.device));                     // the calling host thread may be new (one thread per view)
    const int trc = pw_table(c, omega, epsilon);
    if (trc) return trc;
    const les::PairwiseParams pp{c->p.H, c->p.W, lambda, th_smooth};
    const float4 *pro = reinterpret_cast<const float4*>(d_proposal), *lab = reinterpret_cast<const float4*>(d_labels);
    if (d_nonsubmodular) HIPCHECK(hipMemsetAsync(d_nonsubmodular, 0, (size_t)b->n * sizeof(int), cur_stream(c)));
    auto* kernel = map ? les::les_move_graph_kernel<true> : les::les_move_graph_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(b->n, b->graph_chunks), dim3(256), 0, cur_stream(c), graph_cells(b), b->d_graph_off.p, pro, lab, d_cur, d_prop,
                       c->v[mode].ipk, c->d_pw_tab.p, pp, d_payload, b->d_flow0.p, d_nonsubmodular);
    HIPCHECK(hipGetLastError());
    if (flow0_host) {
        std::vector<double> part((size_t)b->n * b->graph_chunks);
        HIPCHECK(hipMemcpyAsync(part.data(), b->d_flow0.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, cur_stream(c)));
        HIPCHECK(hipStreamSynchronize(cur_stream(c)));
        for (int i = 0; i < b->n; i++) {
            double s = 0;
            for (int k = 0; k < b->graph_chunks; k++) s += part[(size_t)i * b->graph_chunks + k];
            flow0_host[i] = s;
        }
    }
    return LES_HIP_OK;
}
// the mask updates of that lock-step, with the same `map`
int apply_masks(bool map, les_hip_ctx* c, const les_hip_batch* b, const les_hip_plane* d_proposal, const unsigned char* d_masks, float* d_cur, const float* d_prop,
                les_hip_plane* d_labels)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !d_proposal || !d_masks || !d_cur || !d_prop || !d_labels) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    auto* kernel = map ? les::les_apply_masks_kernel<true> : les::les_apply_masks_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(b->n, b->wta_chunks), dim3(256), 0, cur_stream(c), graph_cells(b), b->d_graph_off.p, reinterpret_cast<const float4*>(d_proposal),
                       d_masks, d_cur, d_prop, reinterpret_cast<float4*>(d_labels), c->p.W);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}
}  // namespace

extern "C" {

long long les_hip_batch_graph_nodes(const les_hip_batch* b) { return b ? b->graph_nodes : 0; }

int les_hip_batch_graph_offsets(const les_hip_batch* b, long long* offsets)
{
    if (!b || !offsets) return fail(LES_HIP_ERR_ARG, "null argument");
    std::copy(b->graph_off.begin(), b->graph_off.end(), offsets);
    return LES_HIP_OK;
}

int les_hip_batch_expansion_graph(les_hip_ctx* c, const les_hip_batch* b, int mode, const les_hip_plane* d_planes, const les_hip_plane* d_labels,
                                  const float* d_cur, const float* d_prop, float lambda, float th_smooth, float omega, float epsilon,
                                  float* d_payload, double* flow0_host)
{
    return move_graph(false, c, b, mode, d_planes, d_labels, d_cur, d_prop, lambda, th_smooth, omega, epsilon, d_payload, flow0_host, nullptr);
}

int les_hip_batch_fusion_graph(les_hip_ctx* c, const les_hip_batch* b, int mode, const les_hip_plane* d_labels1, const les_hip_plane* d_labels,
                               const float* d_cur, const float* d_prop, float lambda, float th_smooth, float omega, float epsilon,
                               float* d_payload, double* flow0_host, int* d_nonsubmodular)
{
    return move_graph(true, c, b, mode, d_labels1, d_labels, d_cur, d_prop, lambda, th_smooth, omega, epsilon, d_payload, flow0_host, d_nonsubmodular);
}

long long les_hip_batch_max_cell_nodes(const les_hip_batch* b)
{
    long long m = 0;
    if (b) for (const les_hip_rect& t : b->targets) m = std::max(m, (long long)std::max(0, t.w) * std::max(0, t.h));
    return m;
}

// One workgroup per cell either way, and the kernel is chosen for every cell on its own shape -- never on the other cells of the lock-step: the kernels
// agree only up to nodes on float ties, and a cell's cut must not depend on the cells it shares a lock-step with (an N-rank run gives each rank
// another band of a set's cells than one rank has).  A cell that fits it runs the kernel with the tiled solver's two-barrier iteration and the
// residuals in registers (les_maxflow_cell.h: 0); any other cell -- or every cell with LES_HIP_MAXFLOW_CELL_KERNEL=0 (A/B, tests of the other
// path) -- runs les_maxflow.h with two nodes per thread (1) or five (2).
namespace {
bool mf_cell_kernel_enabled()
{
    if (const char* ev = getenv("LES_HIP_MAXFLOW_CELL_KERNEL")) return atoi(ev) != 0;
    return true;
}
int mf_cell_kind(const les_hip_rect& t, bool cell_kernel)
{
    if (t.w <= 0 || t.h <= 0) return 0;                      // (an empty cell is closed by whichever kernel gets it)
    if (cell_kernel && les::mc_fits(t.w, t.h)) return 0;
    return (long long)t.w * t.h <= 2048 ? 1 : 2;
}
// the batch's cells grouped by kernel (kind 0, then 1, then 2, batch order inside a group) on the device; mf_count[k]: the size of group k
int mf_build_lists(const les_hip_batch* b, bool cell_kernel)
{
    std::lock_guard<std::mutex> lk(b->mf_mu);
    const int key = cell_kernel ? 1 : 0;
    if (b->mf_list_key == key) return LES_HIP_OK;
    std::vector<int> list;
    list.reserve((size_t)b->n);
    int count[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < b->n; i++)
            if (mf_cell_kind(b->targets[i], cell_kernel) == k) { list.push_back(i); count[k]++; }
    if (!b->d_mf_list.p && b->d_mf_list.alloc(std::max<size_t>(1, list.size())))
        return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs: cell list allocation failed");
    if (!list.empty() && hipMemcpy(b->d_mf_list.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs: cell list upload failed");
    std::copy(count, count + 3, b->mf_count);
    b->mf_list_key = key;
    return LES_HIP_OK;
}
}  // namespace

int les_hip_batch_graph_solver_kind(const les_hip_batch* b)
{
    if (!b) return -1;
    if (les_hip_batch_max_cell_nodes(b) > LES_HIP_MAXFLOW_MAX_NODES) return -1;
    const bool cell_kernel = mf_cell_kernel_enabled();
    int kind = 0;
    for (const les_hip_rect& t : b->targets) kind = std::max(kind, mf_cell_kind(t, cell_kernel));
    return kind;
}

int les_hip_batch_solve_graphs(les_hip_ctx* c, const les_hip_batch* b, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows)
{
    return les_hip_batch_solve_graphs_counted(c, b, d_payload, d_masks, d_status, d_flows, nullptr);
}

int les_hip_batch_solve_graphs_counted(les_hip_ctx* c, const les_hip_batch* b, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows,
                                       int* d_unsolved_total)
{
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !d_payload || !d_masks || !d_status) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    const long long maxn = les_hip_batch_max_cell_nodes(b);
    if (maxn > LES_HIP_MAXFLOW_MAX_NODES) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs: a cell of %lld nodes exceeds the limit of %d", maxn, LES_HIP_MAXFLOW_MAX_NODES);
    static_assert(LES_HIP_MAXFLOW_MAX_NODES == les::kMfMaxNodes, "header constant out of date");
#if !defined(LES_SIM)
    // The opt-in to more than 64 KB of dynamic LDS is a per-DEVICE function attribute: it is set once per context (a context is bound
    // to one device), under the context's mutex, with that device current -- a process-wide flag would leave the second GPU of a
    // process that drives two without it.  A failure is reported with its own message so that callers can cut on the host instead.
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->maxflow_lds_ready) {
            HIPCHECK(hipSetDevice(c->p.device));
            hipError_t arc = hipFuncSetAttribute(reinterpret_cast<const void*>(les::les_maxflow_kernel<2, 1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)les::mf_lds_bytes(les::kMfMaxNodes));
            if (arc == hipSuccess)
                arc = hipFuncSetAttribute(reinterpret_cast<const void*>(les::les_maxflow_kernel<5, 512>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)les::mf_lds_bytes(les::kMfMaxNodes));
            if (arc == hipSuccess)
                arc = hipFuncSetAttribute(reinterpret_cast<const void*>(les::les_maxflow_cell_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)les::kMcLdsBytes);
            if (arc != hipSuccess) return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs: device max-flow unavailable on device %d (hipFuncSetAttribute max dynamic LDS: %s); cut on the host",
                                               c->p.device, hipGetErrorString(arc));
            c->maxflow_lds_ready = true;
        }
    }
#endif
    const les::GraphCell* cells = graph_cells(b);
    int max_iter = les::kMfMaxIter;
    if (const char* ev = getenv("LES_HIP_MAXFLOW_MAX_ITER")) max_iter = std::max(0, atoi(ev));      // tests of the callers' host fall-back
    int round_iters = 16;                                   // (8 ... 64 measured on whole runs: flat within 3 %, tools/lab/ab_cell_kernel.sh)
    if (const char* ev = getenv("LES_HIP_MAXFLOW_ROUND_ITERS")) round_iters = std::max(1, atoi(ev));
    const bool cell_kernel = mf_cell_kernel_enabled();
    const int kind = les_hip_batch_graph_solver_kind(b);
    // up to three launches on the same stream over disjoint groups of cells; a lock-step whose cells all go to one kernel is one launch over the
    // whole batch (no list), as before
    bool uniform = true;
    for (const les_hip_rect& t : b->targets) uniform = uniform && mf_cell_kind(t, cell_kernel) == kind;
    int count[3] = {0, 0, 0};
    const int* lists[3] = {nullptr, nullptr, nullptr};
    long long group_max[3] = {0, 0, 0};
    if (uniform) count[kind] = b->n;
    else {
        const int rc = mf_build_lists(b, cell_kernel);
        if (rc) return rc;
        std::copy(b->mf_count, b->mf_count + 3, count);
        lists[0] = b->d_mf_list.p; lists[1] = lists[0] + count[0]; lists[2] = lists[1] + count[1];
    }
    for (const les_hip_rect& t : b->targets) {
        const int k = uniform ? kind : mf_cell_kind(t, cell_kernel);
        group_max[k] = std::max(group_max[k], (long long)std::max(0, t.w) * std::max(0, t.h));
    }
    for (int k = 0; k < 3; k++) {
        if (count[k] == 0) continue;
        // the LDS pitch of les_maxflow.h is the largest cell of the launch: it places the arrays, it does not change the arithmetic
        const int np = (int)((std::max<long long>(group_max[k], 1) + 7) / 8) * 8;
        const size_t lds = les::mf_lds_bytes(np);
        if (k == 0)
            hipLaunchKernelGGL(les::les_maxflow_cell_kernel, dim3(count[k]), dim3(les::kMcThreads), les::kMcLdsBytes, cur_stream(c), cells, b->d_graph_off.p, d_payload, max_iter,
                               round_iters, d_masks, d_status, d_flows, d_unsolved_total, lists[k]);
        else if (k == 1)
            hipLaunchKernelGGL((les::les_maxflow_kernel<2, 1024>), dim3(count[k]), dim3(1024), lds, cur_stream(c), cells, b->d_graph_off.p, d_payload, np, max_iter, d_masks, d_status,
                               d_flows, d_unsolved_total, lists[k]);
        else
            hipLaunchKernelGGL((les::les_maxflow_kernel<5, 512>), dim3(count[k]), dim3(512), lds, cur_stream(c), cells, b->d_graph_off.p, d_payload, np, max_iter, d_masks, d_status,
                               d_flows, d_unsolved_total, lists[k]);
        HIPCHECK(hipGetLastError());
    }
    return LES_HIP_OK;
}

// ---- tiled device max-flow: cells of any size (les_maxflow_tiled.h) ------------------------------------------------------------
namespace {
// Cuts a w x h cell into tiles of at most kMtMaxTileNodes nodes and kMtMaxSide a side: the fewest tiles, then the most square ones.
void mt_partition(int w, int h, int& tw, int& th)
{
    long long best = -1;
    tw = th = 1;
    for (int ntx = (w + les::kMtMaxSide - 1) / les::kMtMaxSide; ntx <= w; ntx++) {
        const int cw = (w + ntx - 1) / ntx;
        const int chmax = std::min(les::kMtMaxSide, les::kMtMaxTileNodes / cw);
        if (chmax < 1) continue;
        const int nty = (h + chmax - 1) / chmax;
        const int ch = (h + nty - 1) / nty;
        const long long tiles = (long long)ntx * nty;
        const long long score = tiles * 1000 + std::abs(cw - ch);            // fewest tiles first
        if (best < 0 || score < best) { best = score; tw = cw; th = ch; }
        if (cw * 2 < ch) break;                                              // narrower tiles only get worse from here
    }
}
int mt_build_tiles(const les_hip_batch* b)
{
    std::lock_guard<std::mutex> lk(b->mt_mu);
    if (b->mt_ntiles >= 0) return LES_HIP_OK;
    std::vector<les::MtTile> tiles;
    std::vector<int> per_cell((size_t)std::max(1, b->n), 0);
    // tiles of one cell are neighbours in the launch order (they share halos in L2), cells in batch order
    for (int i = 0; i < b->n; i++) {
        const int w = std::max(0, b->targets[i].w), h = std::max(0, b->targets[i].h);
        if (w == 0 || h == 0) continue;
        int tw, th;
        mt_partition(w, h, tw, th);
        for (int y0 = 0; y0 < h; y0 += th)
            for (int x0 = 0; x0 < w; x0 += tw) {
                tiles.push_back(les::MtTile{i, x0, y0, std::min(tw, w - x0), std::min(th, h - y0), w, h, 0, b->graph_off[i], 0});
                per_cell[i]++;
            }
    }
    DevBuf<les::MtTile> d_t;
    DevBuf<int> d_p;
    if (d_t.alloc(std::max<size_t>(1, tiles.size())) || d_p.alloc(per_cell.size()) ||
        (tiles.size() && hipMemcpy(d_t.p, tiles.data(), tiles.size() * sizeof(les::MtTile), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(d_p.p, per_cell.data(), per_cell.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: tile table allocation failed");
    b->d_mt_tiles = std::move(d_t);
    b->d_mt_tiles_per_cell = std::move(d_p);
    b->mt_ntiles = (int)tiles.size();
    return LES_HIP_OK;
}
}  // namespace

long long les_hip_batch_tiled_workspace_bytes(const les_hip_batch* b)
{
    if (!b) return 0;
    return (long long)les::mt_layout(std::max<long long>(1, b->graph_nodes), std::max(1, b->n)).total;
}

int les_hip_batch_solve_graphs_tiled(les_hip_ctx* c, const les_hip_batch* b, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows,
                                     void* d_workspace, long long workspace_bytes, int* launches_out, int* unsolved_out)
{
    les_hip_tiled_stats st;
    const int rc = les_hip_batch_solve_graphs_tiled_stats(c, b, d_payload, d_masks, d_status, d_flows, d_workspace, workspace_bytes, &st);
    if (launches_out) *launches_out = st.launches;
    if (unsolved_out) *unsolved_out = st.unsolved;
    return rc;
}

int les_hip_batch_solve_graphs_tiled_stats(les_hip_ctx* c, const les_hip_batch* b, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows,
                                           void* d_workspace, long long workspace_bytes, les_hip_tiled_stats* stats)
{
    int launches_tmp = 0, unsolved_tmp = 0, handed_tmp = 0;
    int *launches_out = &launches_tmp, *unsolved_out = &unsolved_tmp, *handed_out = &handed_tmp;
    long long handed_nodes = 0;
    double host_ms = 0.0;
    struct Report {                                       // fills *stats on every exit path
        les_hip_tiled_stats* s; int *l, *u, *h; long long* hn; double* ms;
        ~Report() { if (s) { s->launches = *l; s->unsolved = *u; s->handed_cells = *h; s->handed_nodes = *hn; s->host_ms = *ms; } }
    } report{stats, launches_out, unsolved_out, handed_out, &handed_nodes, &host_ms};
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !d_payload || !d_masks || !d_status || !d_workspace) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    if (workspace_bytes < les_hip_batch_tiled_workspace_bytes(b))
        return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: workspace of %lld bytes, %lld needed (les_hip_batch_tiled_workspace_bytes)", workspace_bytes,
                    les_hip_batch_tiled_workspace_bytes(b));
    if (((uintptr_t)d_workspace & 255) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: the workspace must be 256-byte aligned");
    if (b->graph_nodes >= (1ll << 31) - 16) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: %lld graph nodes exceed the 32-bit height range", b->graph_nodes);
    int rc = mt_build_tiles(b);
    if (rc) return rc;
#if !defined(LES_SIM)
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->maxflow_tiled_lds_ready) {
            HIPCHECK(hipSetDevice(c->p.device));
            const hipError_t arc = hipFuncSetAttribute(reinterpret_cast<const void*>(les::les_maxflow_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)les::kMtLdsBytes);
            if (arc != hipSuccess) return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: device max-flow unavailable on device %d (hipFuncSetAttribute max dynamic LDS: %s); cut on the host",
                                               c->p.device, hipGetErrorString(arc));
            c->maxflow_tiled_lds_ready = true;
        }
    }
#endif
    hipStream_t st = cur_stream(c);
    les::MtArgs a;
    a.cells = graph_cells(b);
    a.offsets = b->d_graph_off.p;
    a.payload = d_payload;
    a.tiles = b->d_mt_tiles.p;
    a.ws = reinterpret_cast<char*>(d_workspace);
    a.nodes = b->graph_nodes;
    a.ncells = b->n;
    a.K = 8; a.S = 12;                                     // short sweeps, a dozen of them between exact relabellings (measured: K = 8 / 16 / 32 / 64 -> 4.5 / 5.2 / 6.8 / 9.7 ms on a hard layer-1 lock-step)
    a.max_launches = 2000;
    a.K2 = a.K; a.S2 = a.S;
    if (const char* ev = getenv("LES_HIP_MAXFLOW_TILED_K")) a.K = a.K2 = std::max(1, atoi(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_TILED_S")) a.S = a.S2 = std::max(1, atoi(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_TILED_K2")) a.K2 = std::max(1, atoi(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_TILED_S2")) a.S2 = std::max(1, atoi(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_MAX_ITER")) a.max_launches = std::max(1, atoi(ev));      // tests of the callers' host fall-back
    a.masks = d_masks;
    a.status = d_status;
    a.flows = d_flows;
    MtHostLease lease{c, nullptr};
    rc = mt_host_acquire(c, &lease.m);
    if (rc) return rc;
    MtHost& hf = *lease.m;
    volatile int* flags = hf.h_flags.p;
    for (int i = 0; i < 6; i++) flags[i] = 0;   // (nothing in flight writes them: the previous user of this MtHost has synchronised)
    a.host_flags = hf.d_flags;
    hipLaunchKernelGGL(les::les_maxflow_tiled_init_kernel, dim3((b->n + 255) / 256), dim3(256), 0, st, a.ws, a.nodes, a.ncells, b->d_mt_tiles_per_cell.p, d_status, d_flows, a.host_flags);
    HIPCHECK(hipGetLastError());
    if (b->mt_ntiles == 0) {                                // every target rect is empty: the init kernel has closed all cells
        HIPCHECK(hipStreamSynchronize(st));
        return LES_HIP_OK;
    }
    // Hand-over policy (les_maxflow_tiled.h, host/ResidualCut.h): at the progress checks -- after launch 12 and then every 16 launches, the same
    // schedule in every lock-step -- the host cores finish from its residual graph every open cell that has had `hand_after` launches and has at
    // most `hand_cell_nodes` nodes, and after `hand_late_after` launches every open cell whatever its size.  The decision looks at nothing but the
    // cell itself (its launch count, its size, its phase): the host finisher and the launches may pick different minimum cuts where float capacities
    // tie, so a rule that looked at the other cells of the lock-step -- how many are open, how large they are together, whether any finished lately
    // (round 6) -- made a cell's mask depend on its neighbours in the lock-step, and an N-rank run, whose ranks hold other bands of a set's cells,
    // differ from a single-rank run.  Cell size matters: a coarsest-layer cell (150 000 nodes) costs the host 3 ... 10 ms, more than the further
    // launches an ordinary straggler of that layer needs, so early on only small cells go (<= hand_cell_nodes: layer-1 cells of 129 x 129).
    // LES_HIP_MAXFLOW_HANDOVER=0 switches it off (every cell is then cut by launches alone, as in round 5); ..._AFTER / _CELL_NODES / _LATE_AFTER
    // override the thresholds (A/B measurements, tests; ..._NODES sets the node limit as well).
    int hand_after = 60, hand_late_after = 220;
    long long hand_cell_nodes = 40000;
    bool hand = true;
    if (const char* ev = getenv("LES_HIP_MAXFLOW_HANDOVER")) hand = atoi(ev) != 0;
    if (const char* ev = getenv("LES_HIP_MAXFLOW_HANDOVER_AFTER")) hand_after = std::max(1, atoi(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_HANDOVER_NODES")) hand_cell_nodes = std::max(1ll, atoll(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_HANDOVER_CELL_NODES")) hand_cell_nodes = std::max(1ll, atoll(ev));
    if (const char* ev = getenv("LES_HIP_MAXFLOW_HANDOVER_LATE_AFTER")) hand_late_after = std::max(1, atoi(ev));
    long long smallest = b->graph_nodes;                    // (the host skips the check while no cell of the batch could qualify)
    for (const les_hip_rect& t : b->targets)
        if (t.w > 0 && t.h > 0) smallest = std::min(smallest, (long long)t.w * t.h);
    // Launches are enqueued in groups; after each group the host reads "cells done" (the only synchronisation).  Launches that come
    // after the last cell finished return at once.
    int total = 0, group = 12, handed = 0;
    for (;;) {
        for (int i = 0; i < group; i++)
            hipLaunchKernelGGL(les::les_maxflow_tiled_kernel, dim3(b->mt_ntiles), dim3(les::kMtThreads), les::kMtLdsBytes, st, a);
        total += group;
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(st));
        const int done = flags[0];                          // (cells closed by the launches; the `handed` ones are closed as well)
        if (done + handed >= b->n) break;
        if (hand && total >= hand_after && (total >= hand_late_after || smallest <= hand_cell_nodes)) {
            les::MtHandArgs ha;
            ha.tiles = b->d_mt_tiles.p; ha.ws = a.ws; ha.nodes = a.nodes; ha.ncells = a.ncells; ha.cells = a.cells;
            ha.hand_after = hand_after; ha.late_after = hand_late_after; ha.cell_nodes = hand_cell_nodes;
            ha.masks = d_masks; ha.status = d_status; ha.flows = d_flows; ha.host_flags = hf.d_flags;
            // the staging holds what the collect kernel selects; when it reports more than fits, it has parked nothing: grow the staging, collect again
            // (nothing has run in between, the selection is the same)
            for (int attempt = 0;; attempt++) {
                if (attempt == 0 && hf.cap_nodes == 0) {
                    rc = mt_host_stage(&hf, std::min<long long>(b->graph_nodes, 140000), std::min(b->n, 16), st);
                    if (rc) return rc;
                }
                ha.cap_nodes = hf.cap_nodes; ha.cap_cells = hf.cap_cells;
                ha.list = reinterpret_cast<les::MtHandCell*>(hf.d_stage + hf.off_list());
                ha.rc8 = reinterpret_cast<float*>(hf.d_stage);
                ha.ex = reinterpret_cast<float*>(hf.d_stage + hf.off_ex());
                ha.hmasks = reinterpret_cast<const uint8_t*>(hf.d_stage + hf.off_masks());
                ha.hflows = reinterpret_cast<const double*>(hf.d_stage + hf.off_flows());
                hipLaunchKernelGGL(les::les_maxflow_tiled_collect_kernel, dim3(1), dim3(64), 0, st, ha);
                hipLaunchKernelGGL(les::les_maxflow_tiled_pack_kernel, dim3(b->mt_ntiles), dim3(les::kMtThreads), 0, st, ha);      // (nothing to pack when no cell qualified)
                HIPCHECK(hipGetLastError());
                HIPCHECK(hipStreamSynchronize(st));
                const int want_cells = flags[4], want_nodes = flags[5];
                if (flags[2] > 0 || want_cells == 0) break;
                if (attempt > 0) return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: hand-over staging of %lld nodes refused %d cells of %d nodes", hf.cap_nodes, want_cells, want_nodes);
                rc = mt_host_stage(&hf, want_nodes, want_cells, st);
                if (rc) return rc;
            }
            const int now = flags[2];
            if (now > 0) {
                handed += now;
                handed_nodes += flags[3];
                const auto h0 = std::chrono::steady_clock::now();
                const float* h_rc8 = reinterpret_cast<const float*>(hf.h_stage.p);
                const float* h_ex = reinterpret_cast<const float*>(hf.h_stage.p + hf.off_ex());
                uint8_t* h_masks = reinterpret_cast<uint8_t*>(hf.h_stage.p + hf.off_masks());
                const les::MtHandCell* list = reinterpret_cast<const les::MtHandCell*>(hf.h_stage.p + hf.off_list());
                double* hflows = reinterpret_cast<double*>(hf.h_stage.p + hf.off_flows());
                const std::vector<les_hip_rect>& tg = b->targets;
                const char* sev = getenv("LES_HIP_MAXFLOW_HANDOVER_SOLVER");      // 1 (default): FIFO push-relabel; 0: search trees with the push-relabel continuation (measured slower on what is handed over: tools/residual_probe.py)
                const int solver = sev ? atoi(sev) : 1;
                if (const char* dump = getenv("LES_HIP_MAXFLOW_HANDOVER_DUMP")) {      // tooling: the residual graphs as handed over (tools/residual_probe.py)
                    if (FILE* f = fopen(dump, "wb")) {
                        const long long hn = flags[3];
                        fwrite(&now, sizeof(int), 1, f); fwrite(&hn, sizeof(long long), 1, f);
                        for (int q = 0; q < now; q++) { const int wh[2] = {tg[(size_t)list[q].cell].w, tg[(size_t)list[q].cell].h}; fwrite(wh, sizeof(int), 2, f); fwrite(&list[q].hoff, sizeof(long long), 1, f); }
                        fwrite(h_rc8, sizeof(float), (size_t)hn * 8, f); fwrite(h_ex, sizeof(float), (size_t)hn, f);
                        fclose(f);
                    }
                }
                // one host thread per cell, at most as many as the process may keep busy (a persistent team owned by the calling thread); the large
                // cells split their phases over row bands as the host cuts do
                const int team = std::max(1, std::min(now, les_host::cpuBudget()));
                std::atomic<int> next{0};
                les_host::BandPool::outer().run(team, [&](int) {
                    for (int q = next.fetch_add(1); q < now; q = next.fetch_add(1)) {
                        const int cell = list[q].cell;
                        const int w = tg[(size_t)cell].w, h = tg[(size_t)cell].h;
                        hflows[q] = les_host::finishResidualCut(h_rc8 + 8 * list[q].hoff, h_ex + list[q].hoff, w, h, h_masks + list[q].hoff, les_host::residualBands(w, h), solver);
                    }
                });
                host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
                hipLaunchKernelGGL(les::les_maxflow_tiled_unpack_kernel, dim3(b->mt_ntiles), dim3(256), 0, st, ha);
                HIPCHECK(hipGetLastError());
                // the staging belongs to the next caller (and the next check) as soon as the unpack kernel has read it
                HIPCHECK(hipStreamSynchronize(st));
                if (done + handed >= b->n) break;
            }
        }
        if (total >= a.max_launches + group) return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: %d of %d cells still open after %d launches", b->n - done - handed, b->n, total);
        group = 16;
    }
    *launches_out = total;
    *unsolved_out = flags[1];
    *handed_out = handed;
    return LES_HIP_OK;
}

#if defined(LES_MT_PROBE) && !defined(LES_SIM)
// lab build only (tools/lab/mt_probe.py): where the clock stamps of les_maxflow_tiled_kernel go ([launches][tiles][16] 64-bit words of device memory)
int les_hip_debug_mt_probe(void* d_buf, int launches)
{
    unsigned long long* p = static_cast<unsigned long long*>(d_buf);
    if (hipMemcpyToSymbol(HIP_SYMBOL(les::g_mt_probe), &p, sizeof(p)) != hipSuccess) return LES_HIP_ERR_DEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(les::g_mt_probe_launches), &launches, sizeof(launches)) != hipSuccess) return LES_HIP_ERR_DEVICE;
    return LES_HIP_OK;
}
#endif

int les_hip_batch_apply_masks(les_hip_ctx* c, const les_hip_batch* b, const les_hip_plane* d_planes, const unsigned char* d_masks, float* d_cur,
                              const float* d_prop, les_hip_plane* d_labels)
{
    return apply_masks(false, c, b, d_planes, d_masks, d_cur, d_prop, d_labels);
}

int les_hip_batch_apply_masks_labels(les_hip_ctx* c, const les_hip_batch* b, const les_hip_plane* d_labels1, const unsigned char* d_masks, float* d_cur,
                                     const float* d_prop, les_hip_plane* d_labels)
{
    return apply_masks(true, c, b, d_labels1, d_masks, d_cur, d_prop, d_labels);
}

}  // extern "C"
