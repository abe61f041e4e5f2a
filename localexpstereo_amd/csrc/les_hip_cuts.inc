// les_hip_cuts.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the expansion and fusion moves on the device -- graph capacities, the LDS max-flow, the tiled max-flow with its hand-over to the host cores, mask application
// Host side of one tiled solve in flight: the host-mapped words the kernels report through (pinned, fine-grained: the kernel adds to them with
// system-scope atomics, the host reads them after synchronising its stream -- the progress check of a lock-step costs no copy) and the pinned
// staging of the hand-over (les_maxflow_tiled.h: residual graphs out, masks and flow values back).  A context keeps a pool of them: a call
// takes one, returns it at the end; they are freed with the context (round 5 kept two words per host THREAD for ever).
struct MtStage { float* rc8; float* ex; uint8_t* masks; les::MtHandCell* list; double* flows; };       // the staging's five arrays at one of its two addresses
struct MtHost {
    // (h_*: the pinned owners; d_*: the addresses the device reaches them at)
    PinnedBuf<int> h_flags; int* d_flags = nullptr;                    // les::MtFlag
    PinnedBuf<char> h_stage; char* d_stage = nullptr;                  // rc8 [cap_nodes][8] floats | ex [cap_nodes] floats | masks [cap_nodes] bytes | list [cap_cells] | flows [cap_cells]
    long long cap_nodes = 0;
    int cap_cells = 0;
    size_t off_list() const { return ((size_t)cap_nodes * 37 + 255) & ~(size_t)255; }
    size_t off_flows() const { return off_list() + (size_t)cap_cells * sizeof(les::MtHandCell); }
    size_t bytes() const { return off_flows() + (size_t)cap_cells * sizeof(double); }
    // that layout at `base`: d_stage for the kernels (MtHandArgs), h_stage.p for the host finish
    MtStage stage_at(char* base) const
    {
        return {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + (size_t)cap_nodes * 32), reinterpret_cast<uint8_t*>(base + (size_t)cap_nodes * 36),
                reinterpret_cast<les::MtHandCell*>(base + off_list()), reinterpret_cast<double*>(base + off_flows())};
    }
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
    static_assert(les::kMtFlagCount <= 16, "the flag words fit the allocation");
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
// The staging is made at a solve's first hand-over check for at most kMtStageFirstNodes nodes of kMtStageFirstCells cells (what the product's checks hand
// over), and grows, rounded up to kMtStageNodeStep / kMtStageCellStep, when a check selects more.
constexpr long long kMtStageFirstNodes = 140000, kMtStageNodeStep = 4096;
constexpr int kMtStageFirstCells = 16, kMtStageCellStep = 16;
// staging for `nodes` graph nodes (37 bytes each) of `cells` cells, grown on demand
int mt_host_stage(MtHost* m, long long nodes, int cells, hipStream_t stream)
{
    if (m->cap_nodes >= nodes && m->cap_cells >= cells) return LES_HIP_OK;
    m->cap_nodes = std::max(m->cap_nodes, (nodes + kMtStageNodeStep - 1) & ~(kMtStageNodeStep - 1));
    m->cap_cells = std::max(m->cap_cells, (cells + kMtStageCellStep - 1) & ~(kMtStageCellStep - 1));
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
// The opt-in to more than 64 KB of dynamic LDS is a per-DEVICE function attribute: it is set once per context (a context is bound to one device;
// `ready` is the context's flag for these kernels), under the context's mutex, with that device current -- a process-wide flag would leave the second
// GPU of a process that drives two without it.  A failure is reported with its own message (`who`: the entry point) so that callers can cut on the host.
struct LdsKernel { const void* fn; size_t bytes; };
int ensure_dynamic_lds(les_hip_ctx* c, bool& ready, std::initializer_list<LdsKernel> kernels, const char* who)
{
#if !defined(LES_SIM)
    std::lock_guard<std::mutex> lk(c->mu);
    if (ready) return LES_HIP_OK;
    HIPCHECK(hipSetDevice(c->p.device));
    for (const LdsKernel& k : kernels) {
        const hipError_t arc = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
        if (arc != hipSuccess) return fail(LES_HIP_ERR_DEVICE, "%s: device max-flow unavailable on device %d (hipFuncSetAttribute max dynamic LDS: %s); cut on the host", who,
                                           c->p.device, hipGetErrorString(arc));
    }
    ready = true;
#endif
    return LES_HIP_OK;
}
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

// The environment variables of the two device max-flows: THE table (include/localexp_hip.h, INTEGRATION.md and DESIGN.md point here).  Each entry point reads
// its struct once, at its top, on every call (tests change the variables between calls on one context).  Nothing but A/B measurements, tooling and tests sets
// any of them: the product runs the defaults.
//   LES_HIP_MAXFLOW_...     default    clamp   set by
//   one workgroup per cell (MfKnobs):
//   CELL_KERNEL             1          -       A/B, tests: 0 sends every cell to les_maxflow.h
//   MAX_ITER                6000       >= 0    tests of the callers' host fall-back (les::kMfMaxIter)
//   ROUND_ITERS             16         >= 1    A/B (8 ... 64 measured on whole runs: flat within 3 %, tools/lab/ab_cell_kernel.sh)
//   tiled (MtKnobs):
//   TILED_K, TILED_S        8, 12      >= 1    A/B: iterations per discharge sweep, sweeps between exact relabellings (measured: K = 8 / 16 / 32 / 64 ->
//                                              4.5 / 5.2 / 6.8 / 9.7 ms on a hard layer-1 lock-step); they set K2, S2 as well
//   TILED_K2, TILED_S2      = K, S     >= 1    A/B: the same in the rounds after the first
//   MAX_ITER                2000       >= 1    tests of the callers' host fall-back: launches after which an open cell gives up (status 1)
//   HANDOVER                1          -       A/B, tests: 0 = every cell is cut by launches alone (as in round 5)
//   HANDOVER_AFTER          60         >= 1    A/B, tests: launches before a small open cell goes to the host cores
//   HANDOVER_NODES, HANDOVER_CELL_NODES
//                           40000      >= 1    A/B, tests: "small" (two spellings of one knob; the second wins)
//   HANDOVER_LATE_AFTER     220        >= 1    A/B: launches before any open cell goes
//   HANDOVER_SOLVER         1          -       A/B, tests: the host finisher, 1 = FIFO push-relabel, 0 = search trees with the push-relabel continuation
//                                              (measured slower on what is handed over: tools/residual_probe.py)
//   HANDOVER_DUMP           unset      -       tooling: a file that receives the residual graphs as handed over (tools/residual_probe.py)
namespace {
struct MfKnobs { bool cell_kernel; int max_iter, round_iters; };
struct MtKnobs {
    int K, S, K2, S2, max_launches;
    // Hand-over policy (les_maxflow_tiled.h, host/ResidualCut.h): at the progress checks -- after launch 12 and then every 16 launches, the same
    // schedule in every lock-step -- the host cores finish from its residual graph every open cell that has had `hand_after` launches and has at
    // most `hand_cell_nodes` nodes, and after `hand_late_after` launches every open cell whatever its size.  The decision looks at nothing but the
    // cell itself (its launch count, its size, its phase): the host finisher and the launches may pick different minimum cuts where float capacities
    // tie, so a rule that looked at the other cells of the lock-step -- how many are open, how large they are together, whether any finished lately
    // (round 6) -- made a cell's mask depend on its neighbours in the lock-step, and an N-rank run, whose ranks hold other bands of a set's cells,
    // differ from a single-rank run.  Cell size matters: a coarsest-layer cell (150 000 nodes) costs the host 3 ... 10 ms, more than the further
    // launches an ordinary straggler of that layer needs, so early on only small cells go (<= hand_cell_nodes: layer-1 cells of 129 x 129).
    bool hand; int hand_after; long long hand_cell_nodes; int hand_late_after;
    int finisher; const char* dump;
};
MfKnobs mf_knobs()
{
    auto num = [](const char* name, int dflt) { const char* ev = getenv(name); return ev ? atoi(ev) : dflt; };
    return {num("LES_HIP_MAXFLOW_CELL_KERNEL", 1) != 0, std::max(0, num("LES_HIP_MAXFLOW_MAX_ITER", les::kMfMaxIter)), std::max(1, num("LES_HIP_MAXFLOW_ROUND_ITERS", 16))};
}
MtKnobs mt_knobs()
{
    auto num = [](const char* name, int dflt) { const char* ev = getenv(name); return ev ? atoi(ev) : dflt; };
    auto count = [&](const char* name, int dflt) { return std::max(1, num(name, dflt)); };
    MtKnobs k;
    k.K = count("LES_HIP_MAXFLOW_TILED_K", 8); k.S = count("LES_HIP_MAXFLOW_TILED_S", 12);
    k.K2 = count("LES_HIP_MAXFLOW_TILED_K2", k.K); k.S2 = count("LES_HIP_MAXFLOW_TILED_S2", k.S);
    k.max_launches = count("LES_HIP_MAXFLOW_MAX_ITER", 2000);
    k.hand = num("LES_HIP_MAXFLOW_HANDOVER", 1) != 0;
    k.hand_after = count("LES_HIP_MAXFLOW_HANDOVER_AFTER", 60);
    k.hand_cell_nodes = 40000;
    for (const char* name : {"LES_HIP_MAXFLOW_HANDOVER_NODES", "LES_HIP_MAXFLOW_HANDOVER_CELL_NODES"})
        if (const char* ev = getenv(name)) k.hand_cell_nodes = std::max(1ll, atoll(ev));
    k.hand_late_after = count("LES_HIP_MAXFLOW_HANDOVER_LATE_AFTER", 220);
    k.finisher = num("LES_HIP_MAXFLOW_HANDOVER_SOLVER", 1);
    k.dump = getenv("LES_HIP_MAXFLOW_HANDOVER_DUMP");
    return k;
}

// One workgroup per cell either way, and the kernel is chosen for every cell on its own shape -- never on the other cells of the lock-step: the kernels
// agree only up to nodes on float ties, and a cell's cut must not depend on the cells it shares a lock-step with (an N-rank run gives each rank
// another band of a set's cells than one rank has).  A cell that fits it runs the kernel with the tiled solver's two-barrier iteration and the
// residuals in registers (les_maxflow_cell.h: 0); any other cell -- or every cell with LES_HIP_MAXFLOW_CELL_KERNEL=0 -- runs les_maxflow.h with two
// nodes per thread (1) or five (2).
int mf_cell_kind(const les_hip_rect& t, bool cell_kernel)
{
    if (t.w <= 0 || t.h <= 0) return 0;                      // (an empty cell is closed by whichever kernel gets it)
    if (cell_kernel && les::mc_fits(t.w, t.h)) return 0;
    return (long long)t.w * t.h <= 2048 ? 1 : 2;
}
// What a solve launches: up to three launches on the same stream over disjoint groups of cells, kind 0, then 1, then 2.  list[k]: the cells of group k on
// the device, in batch order -- null for a batch whose cells all go to one kernel, which is one launch over the whole batch.
struct MfPlan { int count[3]; long long max_nodes[3]; const int* list[3]; };
// ... derived from the batch's targets once per value of cell_kernel and kept with the batch
int mf_plan(const les_hip_batch* b, bool cell_kernel, MfPlan* plan)
{
    std::lock_guard<std::mutex> lk(b->mf_mu);
    const int key = cell_kernel ? 1 : 0;
    if (b->mf_list_key != key) {
        std::vector<int> list;
        list.reserve((size_t)b->n);
        int count[3] = {0, 0, 0};
        long long max_nodes[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < b->n; i++) {
                const les_hip_rect& t = b->targets[i];
                if (mf_cell_kind(t, cell_kernel) != k) continue;
                list.push_back(i); count[k]++;
                max_nodes[k] = std::max(max_nodes[k], (long long)std::max(0, t.w) * std::max(0, t.h));
            }
        if (std::max({count[0], count[1], count[2]}) < b->n) {
            if (!b->d_mf_list.p && b->d_mf_list.alloc(std::max<size_t>(1, list.size())))
                return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs: cell list allocation failed");
            if (hipMemcpy(b->d_mf_list.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
                return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs: cell list upload failed");
        }
        std::copy(count, count + 3, b->mf_count);
        std::copy(max_nodes, max_nodes + 3, b->mf_max);
        b->mf_list_key = key;
    }
    std::copy(b->mf_count, b->mf_count + 3, plan->count);
    std::copy(b->mf_max, b->mf_max + 3, plan->max_nodes);
    const bool uniform = std::max({plan->count[0], plan->count[1], plan->count[2]}) == b->n;
    const int* group = uniform ? nullptr : b->d_mf_list.p;
    for (int k = 0; k < 3; k++) { plan->list[k] = group; if (group) group += plan->count[k]; }
    return LES_HIP_OK;
}
}  // namespace

int les_hip_batch_graph_solver_kind(const les_hip_batch* b)
{
    if (!b) return -1;
    if (les_hip_batch_max_cell_nodes(b) > LES_HIP_MAXFLOW_MAX_NODES) return -1;
    const bool cell_kernel = mf_knobs().cell_kernel;
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
    const MfKnobs knobs = mf_knobs();
    MfPlan plan;
    int rc = mf_plan(b, knobs.cell_kernel, &plan);
    if (rc) return rc;
    const long long maxn = std::max({plan.max_nodes[0], plan.max_nodes[1], plan.max_nodes[2]});
    if (maxn > LES_HIP_MAXFLOW_MAX_NODES) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs: a cell of %lld nodes exceeds the limit of %d", maxn, LES_HIP_MAXFLOW_MAX_NODES);
    static_assert(LES_HIP_MAXFLOW_MAX_NODES == les::kMfMaxNodes, "header constant out of date");
    rc = ensure_dynamic_lds(c, c->maxflow_lds_ready, {{reinterpret_cast<const void*>(les::les_maxflow_kernel<2, 1024>), les::mf_lds_bytes(les::kMfMaxNodes)},
                                                      {reinterpret_cast<const void*>(les::les_maxflow_kernel<5, 512>), les::mf_lds_bytes(les::kMfMaxNodes)},
                                                      {reinterpret_cast<const void*>(les::les_maxflow_cell_kernel), les::kMcLdsBytes}}, "les_hip_batch_solve_graphs");
    if (rc) return rc;
    const les::GraphCell* cells = graph_cells(b);
    for (int k = 0; k < 3; k++) {
        if (plan.count[k] == 0) continue;
        // the LDS pitch of les_maxflow.h is the largest cell of the launch: it places the arrays, it does not change the arithmetic
        const int np = (int)((std::max<long long>(plan.max_nodes[k], 1) + 7) / 8) * 8;
        const size_t lds = les::mf_lds_bytes(np);
        if (k == 0)
            hipLaunchKernelGGL(les::les_maxflow_cell_kernel, dim3(plan.count[k]), dim3(les::kMcThreads), les::kMcLdsBytes, cur_stream(c), cells, b->d_graph_off.p, d_payload,
                               knobs.max_iter, knobs.round_iters, d_masks, d_status, d_flows, d_unsolved_total, plan.list[k]);
        else if (k == 1)
            hipLaunchKernelGGL((les::les_maxflow_kernel<2, 1024>), dim3(plan.count[k]), dim3(1024), lds, cur_stream(c), cells, b->d_graph_off.p, d_payload, np, knobs.max_iter, d_masks,
                               d_status, d_flows, d_unsolved_total, plan.list[k]);
        else
            hipLaunchKernelGGL((les::les_maxflow_kernel<5, 512>), dim3(plan.count[k]), dim3(512), lds, cur_stream(c), cells, b->d_graph_off.p, d_payload, np, knobs.max_iter, d_masks,
                               d_status, d_flows, d_unsolved_total, plan.list[k]);
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

// The steps of one tiled solve, in the order les_hip_batch_solve_graphs_tiled_stats runs them.  (A launch names no MtHost: les_hip_mem.h.)
namespace {
constexpr int kMtFirstGroup = 12, kMtGroup = 16;            // launches between two progress checks: the first check comes early, the same schedule in every lock-step
int mt_check_workspace(const les_hip_batch* b, const void* d_workspace, long long workspace_bytes)
{
    if (workspace_bytes < les_hip_batch_tiled_workspace_bytes(b))
        return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: workspace of %lld bytes, %lld needed (les_hip_batch_tiled_workspace_bytes)", workspace_bytes,
                    les_hip_batch_tiled_workspace_bytes(b));
    if (((uintptr_t)d_workspace & 255) != 0) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: the workspace must be 256-byte aligned");
    if (b->graph_nodes >= (1ll << 31) - 16) return fail(LES_HIP_ERR_ARG, "les_hip_batch_solve_graphs_tiled: %lld graph nodes exceed the 32-bit height range", b->graph_nodes);
    return LES_HIP_OK;
}
les::MtArgs mt_args(const les_hip_batch* b, const MtKnobs& k, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows, void* d_workspace, int* d_flags)
{
    les::MtArgs a;
    a.cells = graph_cells(b); a.offsets = b->d_graph_off.p; a.payload = d_payload; a.tiles = b->d_mt_tiles.p;
    a.ws = reinterpret_cast<char*>(d_workspace); a.nodes = b->graph_nodes; a.ncells = b->n;
    a.K = k.K; a.S = k.S; a.K2 = k.K2; a.S2 = k.S2; a.max_launches = k.max_launches;
    a.masks = d_masks; a.status = d_status; a.flows = d_flows; a.host_flags = d_flags;
    return a;
}
// zeroes the flag words (nothing in flight writes them: the previous user of this MtHost has synchronised) and sets up the cells' control words
int mt_init(hipStream_t st, const les_hip_batch* b, const les::MtArgs& a, volatile int* flags)
{
    for (int i = 0; i < les::kMtFlagCount; i++) flags[i] = 0;
    hipLaunchKernelGGL(les::les_maxflow_tiled_init_kernel, dim3((b->n + 255) / 256), dim3(256), 0, st, a.ws, a.nodes, a.ncells, b->d_mt_tiles_per_cell.p, a.status, a.flows, a.host_flags);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}
// n launches, then the only synchronisation of the loop: the host reads "cells done" after it.  Launches that come after the last cell finished return at once.
int launch_group(hipStream_t st, const les_hip_batch* b, const les::MtArgs& a, int n, les_hip_tiled_stats* s)
{
    for (int i = 0; i < n; i++)
        hipLaunchKernelGGL(les::les_maxflow_tiled_kernel, dim3(b->mt_ntiles), dim3(les::kMtThreads), les::kMtLdsBytes, st, a);
    s->launches += n;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return LES_HIP_OK;
}
// is a hand-over check due after `launches` launches?  (the host skips it while no cell of the batch could qualify: `smallest` is the batch's smallest cell)
bool handover_due(const MtKnobs& k, int launches, long long smallest)
{
    return k.hand && launches >= k.hand_after && (launches >= k.hand_late_after || smallest <= k.hand_cell_nodes);
}
// Parks the open cells that qualify and writes their residual graphs to the staging; *out: the kernels' arguments, which the unpack takes again.  The
// staging holds what the collect kernel selects; when it reports more than fits, it has parked nothing: grow the staging, collect again (nothing has run
// in between, the selection is the same).
int collect_handover(hipStream_t st, const les_hip_batch* b, const les::MtArgs& a, const MtKnobs& k, MtHost* hf, les::MtHandArgs* out)
{
    volatile const int* flags = hf->h_flags.p;
    les::MtHandArgs ha;
    ha.tiles = a.tiles; ha.ws = a.ws; ha.nodes = a.nodes; ha.ncells = a.ncells; ha.cells = a.cells;
    ha.hand_after = k.hand_after; ha.late_after = k.hand_late_after; ha.cell_nodes = k.hand_cell_nodes;
    ha.masks = a.masks; ha.status = a.status; ha.flows = a.flows; ha.host_flags = a.host_flags;
    if (hf->cap_nodes == 0) {
        const int rc = mt_host_stage(hf, std::min(b->graph_nodes, kMtStageFirstNodes), std::min(b->n, kMtStageFirstCells), st);
        if (rc) return rc;
    }
    for (int attempt = 0;; attempt++) {
        const MtStage d = hf->stage_at(hf->d_stage);
        ha.cap_nodes = hf->cap_nodes; ha.cap_cells = hf->cap_cells;
        ha.list = d.list; ha.rc8 = d.rc8; ha.ex = d.ex; ha.hmasks = d.masks; ha.hflows = d.flows;
        hipLaunchKernelGGL(les::les_maxflow_tiled_collect_kernel, dim3(1), dim3(64), 0, st, ha);
        hipLaunchKernelGGL(les::les_maxflow_tiled_pack_kernel, dim3(b->mt_ntiles), dim3(les::kMtThreads), 0, st, ha);      // (nothing to pack when no cell qualified)
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(st));
        const int want_cells = flags[les::kMtFlagCellsWanted], want_nodes = flags[les::kMtFlagNodesWanted];
        if (flags[les::kMtFlagCellsHanded] > 0 || want_cells == 0) break;
        if (attempt > 0) return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: hand-over staging of %lld nodes refused %d cells of %d nodes", hf->cap_nodes, want_cells, want_nodes);
        const int rc = mt_host_stage(hf, want_nodes, want_cells, st);
        if (rc) return rc;
    }
    *out = ha;
    return LES_HIP_OK;
}
// tooling: the residual graphs as handed over (tools/residual_probe.py)
void dump_handover(const char* path, const les_hip_batch* b, const MtStage& h, int cells, long long nodes)
{
    FILE* f = fopen(path, "wb");
    if (!f) return;
    fwrite(&cells, sizeof(int), 1, f); fwrite(&nodes, sizeof(long long), 1, f);
    for (int q = 0; q < cells; q++) {
        const les_hip_rect& t = b->targets[(size_t)h.list[q].cell];
        const int wh[2] = {t.w, t.h};
        fwrite(wh, sizeof(int), 2, f); fwrite(&h.list[q].hoff, sizeof(long long), 1, f);
    }
    fwrite(h.rc8, sizeof(float), (size_t)nodes * 8, f); fwrite(h.ex, sizeof(float), (size_t)nodes, f);
    fclose(f);
}
// The host cores finish the `cells` parked cells (`nodes` nodes) from the staging: one host thread per cell, at most as many as the process may keep busy (a
// persistent team owned by the calling thread); the large cells split their phases over row bands as the host cuts do.
void finish_on_host(const les_hip_batch* b, const MtKnobs& k, const MtHost& hf, int cells, long long nodes, les_hip_tiled_stats* s)
{
    const auto h0 = std::chrono::steady_clock::now();
    const MtStage h = hf.stage_at(hf.h_stage.p);
    if (k.dump) dump_handover(k.dump, b, h, cells, nodes);
    const int team = std::max(1, std::min(cells, les_host::cpuBudget()));
    std::atomic<int> next{0};
    les_host::BandPool::outer().run(team, [&](int) {
        for (int q = next.fetch_add(1); q < cells; q = next.fetch_add(1)) {
            const les_hip_rect& t = b->targets[(size_t)h.list[q].cell];
            const long long o = h.list[q].hoff;
            h.flows[q] = les_host::finishResidualCut(h.rc8 + 8 * o, h.ex + o, t.w, t.h, h.masks + o, les_host::residualBands(t.w, t.h), k.finisher);
        }
    });
    s->handed_cells += cells;
    s->handed_nodes += nodes;
    s->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
}
// copies the host's masks into place and completes the flow values and status words of the parked cells; the staging belongs to the next caller (and the
// next check) as soon as the unpack kernel has read it
int unpack_handover(hipStream_t st, const les_hip_batch* b, const les::MtHandArgs& ha)
{
    hipLaunchKernelGGL(les::les_maxflow_tiled_unpack_kernel, dim3(b->mt_ntiles), dim3(256), 0, st, ha);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return LES_HIP_OK;
}
}  // namespace

int les_hip_batch_solve_graphs_tiled_stats(les_hip_ctx* c, const les_hip_batch* b, const float* d_payload, unsigned char* d_masks, int* d_status, double* d_flows,
                                           void* d_workspace, long long workspace_bytes, les_hip_tiled_stats* stats)
{
    les_hip_tiled_stats s = {};
    struct Report {                                       // fills *stats on every exit path, with the counts so far
        les_hip_tiled_stats* out; const les_hip_tiled_stats* s;
        ~Report() { if (out) *out = *s; }
    } report{stats, &s};
    const MtKnobs k = mt_knobs();
    if (c) (void)hipSetDevice(c->p.device);                 // HIP's current device is per host thread
    if (!c || !b || !d_payload || !d_masks || !d_status || !d_workspace) return fail(LES_HIP_ERR_ARG, "null argument");
    if (b->n == 0) return LES_HIP_OK;
    int rc = mt_check_workspace(b, d_workspace, workspace_bytes);
    if (!rc) rc = mt_build_tiles(b);
    if (!rc) rc = ensure_dynamic_lds(c, c->maxflow_tiled_lds_ready, {{reinterpret_cast<const void*>(les::les_maxflow_tiled_kernel), les::kMtLdsBytes}}, "les_hip_batch_solve_graphs_tiled");
    MtHostLease lease{c, nullptr};
    if (!rc) rc = mt_host_acquire(c, &lease.m);
    if (rc) return rc;
    MtHost& hf = *lease.m;
    volatile const int* flags = hf.h_flags.p;
    const hipStream_t st = cur_stream(c);
    const les::MtArgs a = mt_args(b, k, d_payload, d_masks, d_status, d_flows, d_workspace, hf.d_flags);
    rc = mt_init(st, b, a, hf.h_flags.p);
    if (rc) return rc;
    if (b->mt_ntiles == 0) {                                // every target rect is empty: the init kernel has closed all cells
        HIPCHECK(hipStreamSynchronize(st));
        return LES_HIP_OK;
    }
    long long smallest = b->graph_nodes;
    for (const les_hip_rect& t : b->targets)
        if (t.w > 0 && t.h > 0) smallest = std::min(smallest, (long long)t.w * t.h);
    for (int group = kMtFirstGroup;; group = kMtGroup) {
        rc = launch_group(st, b, a, group, &s);
        if (rc) return rc;
        const int done = flags[les::kMtFlagCellsDone];       // (cells closed by the launches; the handed ones are closed as well)
        if (done + s.handed_cells >= b->n) break;
        if (handover_due(k, s.launches, smallest)) {
            les::MtHandArgs ha;
            rc = collect_handover(st, b, a, k, &hf, &ha);
            if (rc) return rc;
            if (flags[les::kMtFlagCellsHanded] > 0) {
                finish_on_host(b, k, hf, flags[les::kMtFlagCellsHanded], flags[les::kMtFlagNodesHanded], &s);
                rc = unpack_handover(st, b, ha);
                if (rc) return rc;
                if (done + s.handed_cells >= b->n) break;
            }
        }
        if (s.launches >= a.max_launches + group)
            return fail(LES_HIP_ERR_DEVICE, "les_hip_batch_solve_graphs_tiled: %d of %d cells still open after %d launches", b->n - done - s.handed_cells, b->n, s.launches);
    }
    s.unsolved = flags[les::kMtFlagCellsGaveUp];
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
