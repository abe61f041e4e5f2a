// les_hip.hip -- C ABI (include/localexp_hip.h) + host-side launch logic of the MI355X matching-cost path.
//
// Build (see __graft_entry__.build / localexpstereo_amd/build.py):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared les_hip.hip -o liblocalexp_hip.so
// There is no CPU fallback in this library: every entry point needs a HIP device.
// (tools/hipsim compiles this same file against a CPU fiber simulator for logic tests only.)
#include "../../include/localexp_hip.h"
#include "les_kernels.h"
#include "les_march.h"
#include "les_propose.h"
#include "les_post.h"
#include "les_pairwise.h"
#include "les_eval.h"
#include "les_maxflow.h"
#include "les_maxflow_tiled.h"
#include "les_maxflow_cell.h"
#include "les_bilateral.h"
#include "les_vdisp.h"
#include "les_dense.h"
#include "les_costvol.h"
#include "les_featvol.h"
#include "les_crossview.h"
#include "les_wtavol.h"
#include "les_confidence.h"
#include "les_sgm.h"
#include "les_planefit.h"
#include "les_pyramid.h"
#include "les_speckle.h"
#include "les_reproject.h"
#include "les_view.h"
#include "les_rectify.h"
#include "les_unrectify.h"
#include "les_fisheye.h"
#include "les_maskvol.h"

#include "../host/ResidualCut.h"      // the host cores' finisher of the tiled max-flow (plain C++: search trees / push-relabel on a residual graph)

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <mutex>
#if !defined(LES_SIM)
#include <dlfcn.h>
#endif
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// One line on stderr, once per context and reason, when work that the march kernel could have served goes to the 2.2x slower strip
// kernel (a perf cliff nobody would otherwise see; les_hip_batch_kernel_kind reports the same fact per batch).  LES_HIP_QUIET=1 silences it.
enum FallbackReason { FB_RADIUS = 0, FB_NONFINITE, FB_RANGE, FB_THRESHOLD, FB_IMAGE_SIZE, FB_GEOMETRY, FB_PATCHES, FB_GUIDE, FB_COUNT };
void note_fallback(std::atomic<unsigned>& seen, FallbackReason r, const char* fmt, ...)
{
    // (contexts are shared by concurrent host threads -- the re-entrant per-call operator, the two views: fetch_or decides who reports)
    if (seen.fetch_or(1u << r, std::memory_order_relaxed) & (1u << r)) return;
    static const bool quiet = [] { const char* e = getenv("LES_HIP_QUIET"); return e && atoi(e) != 0; }();
    if (quiet) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "localexp_hip: strip kernel instead of the march kernel: %s (LES_HIP_QUIET=1 silences this note)\n", buf);
}

#define HIPCHECK(expr)                                                                               \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(LES_HIP_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#include "les_hip_march_tables.inc"      // which kernel instantiations exist (radius -> geometry): part of what bench.py hashes as "the kernel sources"

struct ViewData {                        // (its device buffers are freed by the list in ~les_hip_ctx below: a new one needs an entry there)
    float* vol = nullptr;
    bool own_vol = false;
    float4* stats = nullptr;
    uint32_t* ipk = nullptr;
    uint32_t* ipk10 = nullptr;           // the guide pixel as signed 10-bit fields (H1 operand format of the strip kernel)
    float4* feat = nullptr;              // NaiveStereoEnergy feature image (image-based matching cost)
    // march kernel (les_march.h): guide as signed bytes, statistics in its format, cost range of the volume
    uint32_t* ipk8 = nullptr;
    float* mstats = nullptr;
    float* vol_t = nullptr;              // the volume once more, tiled [H][ceil(W/8)][D][8]: the taps of steep planes (les_march.h, role A's KIND 5); null when not built
    bool march_ok = false;               // volume finite, range condition met, tables built
    unsigned dmax_bits = 0;              // largest diagonal entry of the guide's inverse covariance (float bits): fixes the scale of a, b
    les::MarchView mv = {};
    // interpolation 2 on the march kernel: the view scaled for the widened range [lo2, th_col] (the quadratic falls below the volume's
    // minimum); calls whose raw cost leaves it are flagged and recomputed on the strip kernel
    les::MarchView mv2 = {};
    float lo2 = 0.0f;
    bool march2_ok = false;
};

}  // namespace

#include "les_hip_mem.h"                 // DevBuf / PinnedBuf: the owner of every allocation below (and what stays raw, and why)

struct MtHost;
namespace { void mt_host_free(MtHost* m); }
struct WtaVol;
namespace { void wtavol_free(WtaVol* w); }
struct SgmWork;
namespace { void sgm_free(SgmWork* w); }
struct FitTables;
namespace { void fit_tables_free(FitTables* t); }

namespace {

// Everything a fixed list of (filterRect, targetRect) calls needs for its unary costs, built once by build_unary_tables
// (les_hip_unary.inc) and immutable afterwards: the tables of every kernel that may serve the calls, since run_unary picks one at
// run time (the context's interpolation, the view's march_ok).  Two output layouts: map / slab (les_hip_batch_create's out_slabs) and
// compact (one call, row stride = target width, origin = target corner: the per-call operator's tile).  One device allocation.
struct VdispGroup { int c0, c1, slices; };
struct UnaryTables {
    int n = 0;
    DevBuf<char> mem;                            // every device table below
    const les::Job* d_jobs = nullptr; int njobs = 0;                   // strip kernel (guided filter)
    // march kernel: groups of NJ jobs cut for mentry; march_ok: every target keeps 2R distance from the filterRect borders that are
    // not image borders, so the kernel's bound on |a| holds (les_march.h)
    const les::Job* d_mjobs = nullptr; int nmgroups = 0;
    const MarchEntry* mentry = nullptr;
    bool march_ok = false;
    // raw-cost patches, one per call of its filterRect's size (interpolation 0 / 2, the image-based march kernel, bilateral / unfiltered)
    const les::RawCall* d_rawcalls = nullptr; const long long* d_raw_off = nullptr;
    long long raw_floats = 0; int raw_chunks = 1;
    // where each call's target rect is written (les_nan_spread_kernel): the rect, the float offset of its corner, the row stride
    const les::WtaJob* d_targets = nullptr; const long long* d_out_off = nullptr; int out_stride = 0;
    const les::BfJob* d_bfjobs = nullptr; int nbfjobs = 0, bf_np = 1;    // bilateral / unfiltered tiles (bf_np: most calls per tile)
    // image-based guided filter on the strip kernel: the calls' slices of the Plane::v stand-in volume (les_hip_vdisp.inc)
    std::vector<VdispGroup> vd_groups;           // calls [c0, c1) in one pass over `slices` slices
    const les::RawCall* d_vd_calls = nullptr;    // per call: its filterRect at its slice (offset slice * H * W + y * W + x)
    const float4* d_vd_stand_in = nullptr;       // per call: (0, 0, slice, 0)
    int vd_max_slices = 0, vd_chunks = 1;
};

// The device buffers a run of some UnaryTables writes, grow-only: raw-cost patches, per-call flags and masked strip jobs (interpolation 2,
// the Plane::v recompute), the Plane::v stand-in volume.  A batch's workspace is shared by the host threads that run its two views (one
// slot per view, grown under the context's lock); a scratch's is private to its caller (slot 0 for both views, no lock).
struct UnaryWorkspace {
    bool shared = false;
    struct Slot {
        DevBuf<float> raw;
        DevBuf<unsigned> flags;
        DevBuf<les::Job> rjobs;
        DevBuf<float> vol;
    } slot[2];
};

}  // namespace

struct les_hip_ctx {
    les_hip_params p;
    int filter = LES_HIP_FILTER_GF;      // aggregation (les_hip_create_filtered); the bilateral / unfiltered ones run les_hip_bilateral.inc
    int R;                               // its radius: windR / 2 (guided filter), windR (bilateral), 0 (unfiltered)
    DevBuf<float> d_bf_tab;              // bilateral / unfiltered: the weight table exp(-|dI|_1 / sig2), 766 floats
    const StripEntry* strip;
    const StripEntry* istrip[2] = {nullptr, nullptr};   // cost-volume guided filter at interpolation 0 / 2 (find_interp_strip)
    int interp = 1;                      // setInterpolationMethod (les_hip_set_interpolation): 0 nearest, 1 linear, 2 quadratic
    const MarchEntry* march = nullptr;   // null: radius not instantiated (or LES_HIP_KERNEL=strip)
    int ncu = 256;                       // compute units of the device (job cutting of the march kernel)
    std::atomic<unsigned> fallback_seen{0};   // reasons already reported by note_fallback
    hipStream_t stream;
    les::Geom geom;
    ViewData v[2];
    float naive_alpha = 0;
    float naive_th_grad = 0;             // Parameters::th_grad as given (th_grad below is scaled by alpha): what les_hip_create_half hands on
    int naive = 0;                       // 1: raw cost from the feature images (les_hip_create_naive), no volume
    float th_color = 0, th_grad = 0;
    // vertical disparity (Plane::v): the energy's MAX_VDISPARITY (les_hip_set_max_vdisparity: createRandomLabel, PROPOSE_INIT) and the
    // RandomProposer's maxVDisp (les_hip_set_random_vdisparity: PROPOSE_RANDOM); 0: no draw, the RNG streams of a context without v
    float max_vdisp = 0.0f, random_vdisp = 0.0f;
    // scratch reused by the non-prepared entry points and by batch_run
    float4* d_planes = nullptr; size_t planes_cap = 0;      // (raw: grown by ensure_planes of les_hip_march.inc)
    DevBuf<float> d_map;                            // H*W floats
    DevBuf<les::WtaJob> d_wta;
    DevBuf<float4> d_wta_planes;
    // smoothness-coefficient table of the pairwise terms, cached per (omega, epsilon)
    DevBuf<float> d_pw_tab; float pw_omega = -1.f, pw_epsilon = -1.f;
    std::mutex mu;                       // guards lazily built state (batch workspaces, scratch lists) when two host threads (the two views) share the context
    unsigned long long gen = 0;          // unique id of this context: thread-local bindings compare it, not the address (an address can be reused)
    std::vector<les_hip_scratch*> idle_scratch;  // hidden scratches whose owning thread has exited, ready for the next new thread
    bool maxflow_lds_ready = false;      // the per-device dynamic-LDS opt-in of les_maxflow_kernel has been made on this context's device
    bool maxflow_tiled_lds_ready = false;   // ... and of les_maxflow_tiled_kernel
    std::vector<les_hip_scratch*> own_scratch;   // scratch objects created behind les_hip_unary_one (one per calling thread), freed with the context
    WtaVol* wtavol = nullptr;            // les_hip_wta_labels' planes, batches, slab workspace and state, and les_hip_confidence's own state (les_hip_wtavol.inc), built on first use, freed by les_hip_destroy
    SgmWork* sgm = nullptr;              // les_hip_sgm_labels' transposed volume and path sums (les_hip_sgm.inc), built on first use, freed by les_hip_destroy
    FitTables* fit_tables = nullptr;     // les_hip_fit_planes' weight tables, one per sig seen (les_hip_planefit.inc), built on first use, freed by les_hip_destroy
    DevBuf<long long> mesh_ws[2];        // les_hip_mesh's tile offsets and counts, one per view (les_hip_reproject.inc), grown under the lock, later calls only enqueue
    std::vector<MtHost*> mt_idle; // host-mapped flag words + hand-over staging of the tiled max-flow: one per CONCURRENT caller, reused, freed with the context
    // what stays raw (les_hip_mem.h): the views' buffers and d_planes; every other table frees itself
    ~les_hip_ctx()
    {
        for (ViewData& w : v) {
            if (w.own_vol && w.vol) (void)hipFree(w.vol);    // (not own_vol: the caller's device volume)
            for (void* q : {(void*)w.stats, (void*)w.ipk, (void*)w.ipk10, (void*)w.feat, (void*)w.ipk8, (void*)w.mstats, (void*)w.vol_t})
                if (q) (void)hipFree(q);
        }
        if (d_planes) (void)hipFree(d_planes);
    }
};

// A prepared batch: the unary-cost tables of its calls (map / slab layout) and their workspace, run by run_unary (les_hip_unary.inc); the
// cell geometry of the proposers, the WTA and the cuts
struct les_hip_batch {
    int n = 0, R = 0;
    UnaryTables tab;
    mutable UnaryWorkspace ws;           // shared: two host threads may run the two views of one batch
    std::vector<les_hip_rect> targets;
    int device = 0;
    // cell geometry for the proposers / WTA
    DevBuf<les::Rect4> d_units;
    DevBuf<les::WtaJob> d_targets;
    // RANSAC proposer scratch: the owners, and the kernels' argument filled from them (les_hip_batch_set_units)
    DevBuf<float> rs_disp; DevBuf<int> rs_idx, rs_noi, rs_no; DevBuf<uint64_t> rs_state; DevBuf<float> rs_refit; DevBuf<les::RansacCell> rs_cell;
    les::RansacScratch rs = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    int wta_chunks = 1;                  // blocks per target rect in the WTA kernel
    int graph_chunks = 1;                // ... in the graph-construction kernel: about one node per thread (its loads are dependent: occupancy hides them)
    // expansion-graph payload layout (les_hip_batch_expansion_graph): node offset of every target, total node count
    std::vector<long long> graph_off;
    long long graph_nodes = 0;
    DevBuf<long long> d_graph_off;
    DevBuf<double> d_flow0;              // n * graph_chunks partial sums
    // tiled device max-flow (les_maxflow_tiled.h): the cells cut into tiles, built on first use (two host threads -- the two views -- may share a batch)
    mutable std::mutex mt_mu;
    mutable DevBuf<les::MtTile> d_mt_tiles;
    mutable DevBuf<int> d_mt_tiles_per_cell;
    mutable int mt_ntiles = -1;          // -1: not built yet
    // one-workgroup device max-flow: the plan of a solve (mf_plan, les_hip_cuts.inc) -- per kernel kind the number of cells and the largest of them, and,
    // when the cells go to more than one kernel, the cells grouped by kind on the device -- built on first use per value of LES_HIP_MAXFLOW_CELL_KERNEL
    // (mf_list_key; -1: not built yet)
    mutable std::mutex mf_mu;
    mutable DevBuf<int> d_mf_list;
    mutable int mf_list_key = -1;
    mutable int mf_count[3] = {0, 0, 0};
    mutable long long mf_max[3] = {0, 0, 0};
    // region energy of the cells (les_hip_eval.inc): partial sums, cells * region_chunks doubles per view (two host threads may run the two views of one
    // batch), built on first use (region_chunks -1: not yet)
    mutable std::mutex re_mu;
    mutable DevBuf<double> d_region_part[2];
    mutable int region_chunks = -1;
};

// Caller-owned scratch of the one-call operator (the reference's `Reusable`, LES/StereoEnergy.h:616-623): its own stream, a
// compact device tile for the target rect, pinned host staging, one workspace, and the compact-layout tables of the 16 (filterRect,
// targetRect) pairs it has used last -- a cell visit calls the operator ~10 times with the same rects (LES/FastGCStereo.h:40-49).
// Distinct scratch objects may be used concurrently from distinct host threads on one context; nothing is allocated, and the context's
// lock is not taken, once a rect pair is known and the workspace has grown to it.
struct les_hip_scratch {
    les_hip_ctx* c = nullptr;
    hipStream_t stream = nullptr;
    DevBuf<float> d_tile; PinnedBuf<float> h_tile;         // grown together
    DevBuf<float4> d_plane; PinnedBuf<float4> h_plane;
    struct Entry { les_hip_rect f, t; UnaryTables tab; unsigned long long stamp; };
    std::vector<Entry> cache;
    unsigned long long clock = 0;
    UnaryWorkspace ws;
};

namespace {

// The stream the calling thread's launches go to: the context's stream, unless this host thread has bound its own for this
// context (les_hip_set_thread_stream: two views advanced by two host threads on one context, each on its own stream).
std::atomic<unsigned long long> g_ctx_gen{0};
// live contexts by generation id (the thread-exit hook of les_hip_unary_one returns a hidden scratch to its context only if that
// very context -- not a later one at the same address -- still exists)
std::mutex g_live_mu;
std::vector<std::pair<unsigned long long, les_hip_ctx*>> g_live;
void release_hidden_scratch(unsigned long long gen, les_hip_scratch* s)
{
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (auto& e : g_live)
        if (e.first == gen) {
            std::lock_guard<std::mutex> lk2(e.second->mu);
            e.second->idle_scratch.push_back(s);         // still owned (and eventually freed) by the context
            return;
        }
    // the context is gone: it has already destroyed the scratch
}
thread_local unsigned long long tl_stream_gen = 0;       // generation id of the context the stream below is bound to (0: none)
thread_local hipStream_t tl_stream = nullptr;
inline hipStream_t cur_stream(const les_hip_ctx* c) { return (tl_stream_gen != 0 && tl_stream_gen == c->gen) ? tl_stream : c->stream; }

#include "les_hip_march.inc"             // job tables, launches and per-view set-up of the unary-cost kernels (hashed with the kernel headers by bench.py)

float naive_alpha(const les_hip_ctx* c) { return c->naive_alpha; }

#include "les_hip_vdisp.inc"             // the image-based cost with vertical disparity (Plane::v): pre-pass and strip-path recompute launches
#include "les_hip_bilateral.inc"         // the bilateral / unfiltered aggregation: per-view set-up, weight table, tiles, launches
#include "les_hip_unary.inc"             // the unary-cost tables of a list of calls, their workspace, and the one router of batches and single calls

}  // namespace

// ---- the C ABI (include/localexp_hip.h), by concern; one translation unit (the kernels are templates in headers, the context and batch structs above are
// shared by every part)
#include "les_hip_context.inc"
#include "les_hip_batch.inc"
#include "les_hip_cuts.inc"
#include "les_hip_eval.inc"
#include "les_hip_speckle.inc"
#include "les_hip_ingest_post.inc"
#include "les_hip_exchange.inc"
#include "les_hip_dense.inc"
#include "les_hip_costvol.inc"
#include "les_hip_featvol.inc"
#include "les_hip_crossview.inc"
#include "les_hip_wtavol.inc"
#include "les_hip_confidence.inc"
#include "les_hip_sgm.inc"
#include "les_hip_planefit.inc"
#include "les_hip_pyramid.inc"
#include "les_hip_reproject.inc"
#include "les_hip_view.inc"
#include "les_hip_rectify.inc"
#include "les_hip_unrectify.inc"
#include "les_hip_fisheye.inc"
#include "les_hip_maskvol.inc"
