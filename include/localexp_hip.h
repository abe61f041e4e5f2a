/*
 * localexp_hip.h -- C ABI of liblocalexp_hip.so: the MI355X (gfx950) implementation of the
 * LocalExpStereo matching-cost hot path.
 *
 * Drop-in boundary: the reference's operator interface
 *     virtual void StereoEnergy::ComputeUnaryPotential(const cv::Rect& filterRect,
 *             const cv::Rect& targetRect, const cv::Mat& costs, const Plane& plane,
 *             Reusable& reusable, int mode) const            (LES/StereoEnergy.h:625-626)
 * as implemented by CostVolumeEnergy (LES/CostVolumeEnergy.h:16-183) with the default "GF" joint
 * filter (FastGuidedImageFilter<double>, LES/GuidedFilter.h:283-327).  A maintainer binds these
 * entry points from a StereoEnergy subclass installed through
 * PMStereoBase::setStereoEnergyCPU (LES/PMStereoBase.h:58-61); see INTEGRATION.md and
 * localexpstereo_amd/host/HipCostVolumeEnergy.h.
 *
 * Plain C: pointers and sizes only, int status returns (0 = OK), no exceptions cross the boundary.
 * Every function fails (non-zero) when no HIP device is available -- there is no CPU fallback.
 */
#ifndef LOCALEXP_HIP_H
#define LOCALEXP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct les_hip_ctx les_hip_ctx;       /* one energy object (both views), cf. CostVolumeEnergy   */
typedef struct les_hip_batch les_hip_batch;   /* prepared geometry of one lock-step (a disjoint set)    */

typedef struct { int x, y, w, h; } les_hip_rect;        /* cv::Rect                                       */
typedef struct { float a, b, c, v; } les_hip_plane;     /* struct Plane, LES/Plane.h:4-9                  */

enum {
    LES_HIP_OK = 0,
    LES_HIP_ERR_ARG = 1,          /* bad argument                                                      */
    LES_HIP_ERR_DEVICE = 2,       /* no usable HIP device / HIP runtime error (see les_hip_last_error) */
    LES_HIP_ERR_UNSUPPORTED = 3   /* e.g. a guided-filter radius no kernel was instantiated for        */
};

/* Constructor arguments of CostVolumeEnergy(imL, imR, volL, volR, Parameters, MAX_DISPARITY,
 * MIN_DISPARITY) -- LES/CostVolumeEnergy.h:16; Parameters fields LES/StereoEnergy.h:13-40. */
typedef struct {
    int H, W, D;                  /* image rows, cols; volume slices (ndisp)                           */
    int windR;                    /* Parameters::windR; guided-filter radius is windR/2 (:30)          */
    double eps;                   /* Parameters::filter_param1                                         */
    float th_col;                 /* Parameters::th_col (mc_threshold, LES/main.cpp:351)               */
    float max_disparity;          /* MAX_DISPARITY (ndisp-1, LES/main.cpp:341)                         */
    float min_disparity;          /* MIN_DISPARITY                                                     */
    int device;                   /* HIP device ordinal                                                */
    int volumes_on_device;        /* != 0: volL/volR are device pointers owned by the caller (shared, not
                                     copied -- like the ref-counted cv::Mat headers, :20-21).  Their
                                     contents must not change behind the context's back: the cost range
                                     of the fixed-point kernel and the tiled copy that steep planes
                                     gather from (les_hip_tiled_volume_bytes) are taken at creation --
                                     after refilling a volume in place call les_hip_refresh_volume    */
} les_hip_params;

/* replaces: CostVolumeEnergy::CostVolumeEnergy (LES/CostVolumeEnergy.h:16-43) including the two
 * FastGuidedImageFilter<double> constructions (global guide statistics, LES/GuidedFilter.h:58-102).
 * imL/imR: H x W x 3 uint8 BGR host images; volL/volR: float [D][H][W] (host, copied to HBM once;
 * or device when volumes_on_device).  Either view may be NULL if its mode is never used. */
int les_hip_create(les_hip_ctx** out, const les_hip_params* params, const uint8_t* imL, const uint8_t* imR,
                   const float* volL, const float* volR);

/* After the caller has overwritten the cost volume of view `mode` in place (volumes_on_device; same shape): re-derives what the context
 * keeps of it -- the cost range that fixes the fixed-point scales of the march kernel, the finite-ness test, the tiled copy that steep
 * planes gather from.  The guide statistics (LES/GuidedFilter.h:58-102) depend on the images only and stay.  No reference counterpart:
 * CostVolumeEnergy shares the caller's cv::Mat and derives nothing from it (LES/CostVolumeEnergy.h:20-21).  Synchronises the stream; must
 * not run concurrently with evaluations on the same context. */
int les_hip_refresh_volume(les_hip_ctx* ctx, int mode);

/* replaces: CostVolumeEnergy::setInterpolationMethod (LES/CostVolumeEnergy.h:45-48): how a plane's disparity reads the volume --
 * 0 nearest slice (:99-119), 1 linear (:70-98, the default), 2 three-point quadratic (:120-167).  Applies to every later evaluation of the
 * context on both views (les_hip_unary_one[_scratch], les_hip_unary_batch, les_hip_batch_run, batches created before the call included) and
 * survives les_hip_refresh_volume.  The reference's (int) conversion of a double is MSVC's (NaN, +-inf and out-of-range values give INT_MIN);
 * mode 2 returns NaN raw costs at the end slices, as the reference does.  LES_HIP_ERR_ARG for values outside 0 .. 2 and for contexts of the
 * image-based energy (les_hip_create_naive*: no volume).  Like the reference's setter it is not synchronised: it must not be called while
 * another host thread evaluates on the same context (launches already queued keep the mode they were made with). */
int les_hip_set_interpolation(les_hip_ctx* ctx, int none_lin_quad);

/* replaces: NaiveStereoEnergy::NaiveStereoEnergy (LES/StereoEnergy.h:638-689) -- the image-based matching cost of the
 * MiddV2 configuration (LES/main.cpp:86-121, PMStereoBase.h:37): no cost volume; the raw cost of a plane is the truncated
 * colour + x-gradient difference between this view and the other view warped by the plane (StereoEnergy.h:702-742), then
 * the same guided-filter aggregation and validity rule.  params->D and the volume fields are ignored, th_col is
 * Parameters::th_col (10 for MiddV2), alpha / th_grad are Parameters::alpha / th_grad.  Both images are required.
 * Every other entry point (unary_one / unary_batch / batch_* / wta) works on the returned context unchanged.
 * A prepared batch of such a context owns one raw-cost patch buffer per view (the sum of its filterRect areas in floats,
 * allocated on the view's first les_hip_batch_run): runs of the same batch and view must be stream-ordered. */
int les_hip_create_naive(les_hip_ctx** out, const les_hip_params* params, const uint8_t* imL, const uint8_t* imR,
                         float alpha, float th_grad);

/* ---- choice of the cost aggregation: Parameters::filterName (LES/StereoEnergy.h:25-39; CostVolumeEnergy.h:23-42,
 * StereoEnergy.h:666-688).  les_hip_create / les_hip_create_naive always build the guided filter ("GF").
 *   LES_HIP_FILTER_GF         "GF": FastGuidedImageFilter<double>, radius windR / 2, eps = params->eps -- exactly les_hip_create(_naive).
 *   LES_HIP_FILTER_BILATERAL  "BF" (NaiveStereoEnergy) / "BL" (CostVolumeEnergy): BilateralFilter (LES/GuidedFilter.h:329-374) on the
 *                             sub-region I(filterRect): q(p) = sum over the (2 windR + 1)^2 window of p clipped to the filterRect of
 *                             exp(-|dI|_1 / sig2) raw(s), NOT normalised; I = the 8-bit BGR guide on its 0..255 scale, radius windR,
 *                             sig2 = params->eps (Parameters::filter_param1, 10 in paramsBF, LES/main.cpp:72), which must be > 0.
 *                             Supported windR: 0 .. 31 (20 is the shipped value); others give LES_HIP_ERR_UNSUPPORTED.
 *   LES_HIP_FILTER_NONE       "": no aggregation, q = raw (bit for bit); windR >= 0 (only the callers' cell geometry uses it), eps ignored.
 * Both then apply the targetRect crop and the 1e6 overwrite of invalid labels (check != 0) of the guided filter.  Every evaluation entry
 * point (les_hip_unary_one / _one_scratch / _unary_batch / les_hip_batch_run, any out_slabs, check 0 / 1) honours the context's filter;
 * the bilateral and unfiltered ones need no guided-filter kernel instantiation (csrc/les_bilateral.h), and les_hip_get_stats has no
 * statistics to return on them.  Everything else (proposals, WTA, graphs, cuts, post-processing, exchange) is independent of the filter. */
enum { LES_HIP_FILTER_GF = 0, LES_HIP_FILTER_BILATERAL = 1, LES_HIP_FILTER_NONE = 2 };
/* les_hip_create with a filter: replaces CostVolumeEnergy::CostVolumeEnergy for any filterName ("BF" and "BL" both select the bilateral
 * filter; the reference's CostVolumeEnergy only knows "BL"). */
int les_hip_create_filtered(les_hip_ctx** out, const les_hip_params* params, int filter, const uint8_t* imL, const uint8_t* imR,
                            const float* volL, const float* volR);
/* les_hip_create_naive with a filter: replaces NaiveStereoEnergy::NaiveStereoEnergy for any filterName. */
int les_hip_create_naive_filtered(les_hip_ctx** out, const les_hip_params* params, int filter, const uint8_t* imL, const uint8_t* imR,
                                  float alpha, float th_grad);
/* ---- vertical disparity (Plane::v, LES/Plane.h:4-40): labels for pairs with imperfect rectification.
 * The image-based energy (les_hip_create_naive*) samples the other view at (x - sign d(x, y), y + v) for every plane with v != 0
 * (NaiveStereoEnergy, LES/StereoEnergy.h:704-729; -0.0 counts as 0) on every evaluation entry point, view, filter and check value; the
 * cost-volume energy ignores v (LES/CostVolumeEnergy.h:64-98), as do the validity rule, the pairwise terms, disparities and post-processing.
 * The two setters below only choose draws of v: with both at 0 (the default) every generator stream is the one of a context without them.
 * replaces: the maxVDisp argument of FastGCStereo / NaiveStereoEnergy (MAX_VDISPARITY, PMStereoBase.h:37): les_hip_batch_propose(INIT)
 * draws v uniformly in [-max_vdisp, max_vdisp] after the disparity (createRandomLabel, LES/StereoEnergy.h:120-129).  Allowed on both
 * energies (only the image-based one reads v).  max_vdisp: finite, >= 0, else LES_HIP_ERR_ARG. */
int les_hip_set_max_vdisparity(les_hip_ctx* ctx, float max_vdisp);
/* replaces: RandomProposer(K, maxDisp, minDisp, maxVDisp) (LES/Proposer.h:100-148): les_hip_batch_propose(RANDOM) perturbs v within
 * max_vdisp * 0.5^(m+1) of the source label's, clamped to [-max_vdisp, max_vdisp], drawn after the disparity; 0 keeps the source's v.
 * EXPANSION keeps the source label's v; RANSAC proposes v = 0.  max_vdisp: finite, >= 0, else LES_HIP_ERR_ARG. */
int les_hip_set_random_vdisparity(les_hip_ctx* ctx, float max_vdisp);

void les_hip_destroy(les_hip_ctx* ctx);                 /* replaces: ~CostVolumeEnergy (:50-52)          */
const char* les_hip_last_error(void);                   /* thread-local description of the last failure  */

/* All launches go to this hipStream_t (NULL = the default stream).  Not in the reference. */
int les_hip_set_stream(les_hip_ctx* ctx, void* hip_stream);
/* bind != 0: from now on the launches the CALLING host thread makes on this context (and its les_hip_synchronize) go to
 * hip_stream instead; bind == 0: back to the context's stream.  For callers that advance the two views of one context from two
 * host threads (doDual: the views are independent until the post-processing, LES/FastGCStereo.h:172-185).
 * What two threads with their own streams may call concurrently on ONE context: everything that works on caller-owned or
 * batch-owned device memory -- les_hip_batch_run / _propose / _wta / _expansion_graph / _solve_graphs / _apply_masks with
 * planes_on_device != 0 and distinct batches, les_hip_unary_one[_scratch] (per-thread / per-scratch buffers), les_hip_synchronize.
 * NOT safe under per-thread streams, because they stage through one context-owned buffer: les_hip_batch_run with planes_on_device
 * == 0, les_hip_unary_batch and les_hip_wta_update -- serialise those in the caller (host/HipCostVolumeEnergy.h holds a mutex). */
int les_hip_set_thread_stream(les_hip_ctx* ctx, void* hip_stream, int bind);
int les_hip_synchronize(les_hip_ctx* ctx);

/* replaces: CostVolumeEnergy::ComputeUnaryPotential (check != 0, LES/CostVolumeEnergy.h:176-183) and
 * ::ComputeUnaryPotentialWithoutCheck (check == 0, :55-174) for ONE call.  `costs` is the HOST
 * pointer of the element (filterRect.y, filterRect.x) of a row-major float map with `row_stride`
 * floats per row, i.e. the view proposalCost(filterRect) of LES/FastGCStereo.h:49; only
 * costs(targetRect - filterRect.tl()) is written.  Synchronous. */
int les_hip_unary_one(les_hip_ctx* ctx, int mode, const les_hip_rect* filterRect, const les_hip_rect* targetRect,
                      const les_hip_plane* plane, float* costs, int row_stride, int check);

/* The re-entrant form of the same operator: `scratch` is the caller-owned per-cell scratch of the reference (struct Reusable,
 * LES/StereoEnergy.h:616-623: one per OpenMP thread / cell visit, LES/FastGCStereo.h:40).  It owns a HIP stream, a device tile
 * and pinned staging for the target rect, and the prepared job tables of the last 16 (filterRect, targetRect) pairs, so that
 * calls with distinct scratch objects may run concurrently from distinct host threads on one context (the method is `const`
 * and is called from an OpenMP team in the reference, LES/FastGCStereo.h:30-49) and nothing is allocated once a rect pair has
 * been seen.  les_hip_unary_one() itself uses one hidden scratch per calling thread, released with the context. */
typedef struct les_hip_scratch les_hip_scratch;
int les_hip_scratch_create(les_hip_ctx* ctx, les_hip_scratch** out);
void les_hip_scratch_destroy(les_hip_scratch* scratch);
int les_hip_unary_one_scratch(les_hip_ctx* ctx, les_hip_scratch* scratch, int mode, const les_hip_rect* filterRect,
                              const les_hip_rect* targetRect, const les_hip_plane* plane, float* costs, int row_stride, int check);

/* The same for n independent calls (one proposal index of one disjoint set of cells:
 * LES/FastGCStereo.h:30-49 run in lock-step) writing into one H x W map.  cost_map: HOST H*W floats;
 * only the target rects are written.  Synchronous. */
int les_hip_unary_batch(les_hip_ctx* ctx, int mode, int n, const les_hip_rect* filterRects,
                        const les_hip_rect* targetRects, const les_hip_plane* planes, float* cost_map, int check);

/* Prepared form for the hot loop: geometry is uploaded once, then reused for every proposal.
 * out_slabs == 0: outputs go into one H x W map (element (y,x) of call i at y*W+x);
 * out_slabs == k > 0: call i writes its target rect into slab i / k of a [ceil(n / k)][H][W] array.  k = 1: every call
 * its own slab (whole-image aggregation of many hypothesis planes); k = cells of a disjoint set,
 * n = k * slots: several proposal slots of the set evaluated in ONE launch, slot s into map s (the calls of a slot are
 * consecutive) -- the launch then fills the GPU where a single lock-step of a coarse layer cannot. */
int les_hip_batch_create(les_hip_ctx* ctx, int n, const les_hip_rect* filterRects, const les_hip_rect* targetRects,
                         int out_slabs, les_hip_batch** out);
void les_hip_batch_destroy(les_hip_batch* b);
int les_hip_batch_num_jobs(const les_hip_batch* b);     /* workgroups one run launches                   */
/* Diagnostic: which kernel les_hip_batch_run launches for this batch and view: 1 = the fixed-point march kernel
 * (csrc/les_march.h; needs a finite volume with th_col - min <= 8 th_col, a guided-filter radius of 2 .. 10 and every target at least 2 x radius away from
 * filterRect borders that are not image borders -- the geometry of every LayerManager cell), 0 = the fp64 strip kernel
 * (csrc/les_kernels.h; any input), -1 = bad argument.  Both implement LES/CostVolumeEnergy.h:55-183.  2 = the bilateral / unfiltered
 * kernel (csrc/les_bilateral.h): every batch of a context made with LES_HIP_FILTER_BILATERAL or LES_HIP_FILTER_NONE.
 * Under les_hip_set_interpolation 0 or 2 (guided filter, cost volume): 1 = a raw-cost pre-pass plus the march kernel serve the batch (the same
 * geometric conditions, and for 2 a volume range that leaves room below its minimum); at 2 the calls whose raw cost holds a NaN or leaves
 * that room are recomputed on the device by the strip kernel, which this value does not report.  0 = the strip kernel serves every call. */
int les_hip_batch_kernel_kind(const les_hip_ctx* ctx, const les_hip_batch* b, int mode);
/* planes: n labels, HOST (planes_on_device == 0) or DEVICE memory; out: DEVICE memory.  Asynchronous
 * on the context's stream. */
int les_hip_batch_run(les_hip_ctx* ctx, const les_hip_batch* b, int mode, const les_hip_plane* planes,
                      int planes_on_device, float* out_dev, int check);

/* ---- the unary costs of a whole label map in one dense device pass (csrc/les_dense.h)
 * replaces: the warm-start branch of FastGCStereo::initCurrentFast (LES/FastGCStereo.h:116-130): for every pixel p = (x, y) of `region`
 * (NULL: the whole image)
 *     d_cost[y * W + x] = ComputeUnaryPotential(filterRect = (p +- windR) clipped to the image, targetRect = (x, y, 1, 1), d_labels[y * W + x])
 * (check != 0; ComputeUnaryPotentialWithoutCheck for check == 0) -- what les_hip_unary_batch returns for those region.w x region.h calls, on
 * every kind of context (both energies, Plane::v, every filter, the interpolation set at call time, min_disparity, the 1e6 sentinel, NaN results
 * where the quadratic read gives NaN).  Pixels outside `region` are not written.  d_labels, d_cost: H * W elements in DEVICE memory.  One
 * launch of a kernel whose unit of work is a pixel with its own plane: a workgroup per tile of pixels, the tile's guide statistics and guide
 * in LDS, a wave per pixel.  Asynchronous on the calling thread's stream (les_hip_set_thread_stream); it stages through nothing the context
 * owns, so two host threads with their own streams may call it concurrently on one context.  LES_HIP_ERR_ARG for a view without data, a
 * region outside the image or null pointers; an empty region is a no-op. */
int les_hip_unary_labels(les_hip_ctx* ctx, int mode, const les_hip_rect* region, const les_hip_plane* d_labels, float* d_cost, int check);
/* Diagnostic: 1 = the dense kernel serves this context and view (every context this build can create: the kernel is instantiated for each
 * guided-filter radius the strip tables serve -- 1 .. 10, 12, 15 -- and takes the radius of the bilateral / unfiltered aggregation at run
 * time), 0 = one job per pixel on the strip kernel (no build does that today), -1 = bad argument. */
int les_hip_unary_labels_kind(const les_hip_ctx* ctx, int mode);

/* ---- hypothesis generation for the cells of a prepared batch (one proposal per cell per call) ----
 * replaces: IProposer::startIterations/getNextProposal as driven by LES/FastGCStereo.h:41-48, for
 * ExpansionProposer (LES/Proposer.h:62-79), RandomProposer (:120-152, `m` = outerIter + iter) and
 * RansacProposer (:163-311, MAX_SAM 500, conf 0.95, threshold 1.0), and the label part of
 * FastGCStereo::initCurrentFast (LES/FastGCStereo.h:105-109: createRandomLabel + fill of the unit region).
 * unitRects: the cells' unit regions (n rects, host).  labels_dev: H*W planes; rng_dev: n uint64
 * generator states (cv::RNG-compatible multiply-with-carry; one per cell, advanced in place);
 * planes_dev: n output labels.  Asynchronous. */
enum { LES_HIP_PROPOSE_EXPANSION = 0, LES_HIP_PROPOSE_RANDOM = 1, LES_HIP_PROPOSE_RANSAC = 2, LES_HIP_PROPOSE_INIT = 3 };
int les_hip_batch_set_units(les_hip_ctx* ctx, les_hip_batch* b, const les_hip_rect* unitRects);
int les_hip_batch_propose(les_hip_ctx* ctx, const les_hip_batch* b, int kind, int m, les_hip_plane* labels_dev,
                          uint64_t* rng_dev, les_hip_plane* planes_dev);
/* winner-take-all update over the batch's target rects with one device-resident plane per cell */
int les_hip_batch_wta(les_hip_ctx* ctx, const les_hip_batch* b, const les_hip_plane* planes_dev, float* cur_cost_dev,
                      const float* prop_cost_dev, les_hip_plane* labels_dev);

/* replaces: the winner-take-all update of the PatchMatch iterations, LES/FastGCStereo.h:56-60
 * (mask = cur > prop; cur <- prop, label <- plane under mask) for n shared regions, on DEVICE maps:
 * cur_cost/prop_cost H*W floats, labels H*W planes (row stride W).  Asynchronous. */
int les_hip_wta_update(les_hip_ctx* ctx, int n, const les_hip_rect* rects, const les_hip_plane* planes,
                       int planes_on_device, float* cur_cost_dev, const float* prop_cost_dev,
                       les_hip_plane* labels_dev);

/* ---- volume preparation on the device ("next" row N3 of the scope table) ----
 * replaces: fillOutOfView (LES/main.cpp:146-176) and convertVolumeL2R (LES/main.cpp:178-199), margin 0, on a
 * DEVICE float [D][H][W] volume (e.g. before handing it to les_hip_create with volumes_on_device).
 * mode 0 = left view, 1 = right view.  Asynchronous on hip_stream (NULL = default stream) of `device`. */
int les_hip_fill_out_of_view(float* vol_dev, int D, int H, int W, int mode, int device, void* hip_stream);
int les_hip_convert_volume_l2r(const float* src_dev, float* dst_dev, int D, int H, int W, int device, void* hip_stream);
/* valid masks in a volume: fillOutOfView with "outside the image" widened to "outside the valid image" (csrc/les_maskvol.h holds the rule and
 * the kernel; no reference counterpart beyond that).  d_vol: DEVICE float [D][H][W], slice k is disparity d = k + d0; mode 0 = left view's
 * volume (I = L, J = R), 1 = right view's (I = R, J = L); d_validI, d_validJ: H x W bytes in DEVICE memory, nonzero = valid, NULL = all valid.
 * An entry is ok iff the reference sees it (mode 0: x >= min(d, W - 1); mode 1: x < max(W - d, 1)), validI[y][x], and validJ[y][c] at its
 * partner column c = clamp(x -+ d, 0, W - 1).  An ok entry is never written; every other entry takes the 32 bits of the nearest ok entry of
 * its own row and slice (a tie goes right in mode 0, left in mode 1), and a row of a slice without one is set to `fill`.  In place and
 * idempotent.  With both masks NULL and d0 = 0 it writes exactly the bytes of les_hip_fill_out_of_view.  Enqueue only, on hip_stream.
 * LES_HIP_ERR_ARG: a null volume, a mode outside 0 / 1, a size <= 0, a fill that is not finite.  LES_HIP_ERR_UNSUPPORTED: W > 32768,
 * H > 65535, D > 65535 * 32, D H W >= 2^32.  A refused call launches nothing. */
int les_hip_fill_invalid(float* d_vol, int D, int H, int W, int mode, int d0, const uint8_t* d_validI, const uint8_t* d_validJ, float fill, int device,
                         void* hip_stream);

/* ---- matching-cost volumes from the stereo pair (csrc/les_costvol.h holds the definition) ----
 * replaces: the external MC-CNN step whose output the reference loads as im0.acrt / im1.acrt (LES/main.cpp:353-357): the classic AD-Census
 * cost instead -- cost = ta[sum_c |I_c - J_c|] + tc[popcount(census_I ^ census_J)] in [0, 1), 9 x 7 census of the integer grey value,
 * ta[s] = 0.5 (1 - exp(-(s / 3) / lambda_ad)), tc[h] = 0.5 (1 - exp(-h / lambda_census)); Mei et al. use lambda_ad = 10, lambda_census = 30.
 * Images are H x W x 3 u8 (BGR) in DEVICE memory; every index clamps to the image.  Context-free, like the volume preparation above.
 * LES_HIP_ERR_ARG for null pointers, non-positive sizes, a mode outside 0 / 1 and a lambda that is not positive and finite; nothing is
 * written on a refused call. */
/* the two tables (766 and 63 floats, HOST memory) the builder uses: double arithmetic, rounded once to float */
int les_hip_costvol_tables(float lambda_ad, float lambda_census, float* ad766_host, float* census63_host);
/* the census signatures of one image: d_sig[y * W + x], bit k = neighbour k (row-major over dy = -3..3, dx = -4..4 without the centre,
 * coordinates clamped) is darker than the centre.  Asynchronous on hip_stream. */
int les_hip_census(const uint8_t* d_bgr, unsigned long long* d_sig, int H, int W, int device, void* hip_stream);
/* the float [D][H][W] volume of one view: slice k is disparity d = k + d0 (d0: the energy's min_disparity);
 * mode 0 = left view's volume (partner column clamp(x - d)), 1 = right view's (clamp(x + d)).  Every entry is written, out-of-view
 * ones through the clamped column: les_hip_fill_out_of_view comes after it, as after a loaded volume.  The call owns its scratch (both
 * views' signatures and packed colours, the tables) and SYNCHRONISES hip_stream before it returns.  Volumes of 2^32 or more floats:
 * LES_HIP_ERR_UNSUPPORTED.  LES_HIP_COSTVOL_NT=1 / 0 selects non-temporal / plain stores (default: non-temporal; the two measure alike). */
int les_hip_build_cost_volume(const uint8_t* d_imL, const uint8_t* d_imR, float* d_vol, int D, int H, int W, int mode, int d0, float lambda_ad,
                              float lambda_census, int device, void* hip_stream);
/* diagnostics: with LES_HIP_COSTVOL_TIMING=1 in the environment les_hip_build_cost_volume brackets its launches with events; this returns the
 * device milliseconds of the calling thread's last build -- the two census launches, the volume kernel (tools/costvol_timing.py). */
int les_hip_costvol_last_times(float* census_ms, float* volume_ms);

/* ---- correlation cost volumes from feature maps (csrc/les_featvol.h holds the definitions) ----
 * replaces: the MC-CNN-fast matcher behind im0.acrt / im1.acrt (LES/main.cpp:353-368) by its last layer alone -- the correlation of two per-pixel
 * feature vectors -- so that any feature extractor, or the built-in ZNCC patch descriptor, feeds the cost-volume energy.  Feature maps are
 * float [C][H][W], contiguous, in DEVICE memory (a torch NCHW tensor with N = 1).  Context-free; both calls only enqueue on hip_stream and use
 * no scratch memory (with LES_HIP_FEATVOL_TIMING=1 they also wait for their launch).  Nothing is launched or written on a refused call. */
/* the ZNCC descriptor of one H x W x 3 u8 (BGR) device image into d_feat, float [(2 ry + 1)(2 rx + 1)][H][W]: with g the integer grey
 * (77 R + 150 G + 29 B + 128) >> 8, the N taps of the window visited row-major over (dy, dx), coordinates clamped, S = sum g, Q = sum g^2,
 * V = N Q - S^2:  channel c = (float)((double)(N g_c - S) / sqrt((double)(N V))), or 0 where V = 0 (a flat patch).  Exact integers, one IEEE
 * double sqrt and division, one rounding to float: a function of the image alone; unit norm, so the correlation of two descriptors is the
 * ZNCC of the patches.  LES_HIP_ERR_ARG: null pointers, non-positive sizes, negative radii.  LES_HIP_ERR_UNSUPPORTED: a radius above 4,
 * H > 65535. */
int les_hip_patch_features(const uint8_t* d_bgr, float* d_feat, int H, int W, int ry, int rx, int device, void* hip_stream);
/* the float [D][H][W] volume of one view from the two views' feature maps: slice k is disparity d = k + d0; mode 0 = left view's volume
 * (I = L, J = R, partner column xp = clamp(x - d, 0, W - 1)), 1 = right view's (I = R, J = L, xp = clamp(x + d, 0, W - 1));
 *   s = the f32 chain s <- fmaf(fI[c][y][x], fJ[c][y][xp], s) over c = 0 .. C - 1 from +0,      cost = fmaf(-alpha, s, beta).
 * alpha = beta = 0.5 maps unit-norm features to [0, 1]; alpha = 1, beta = 0 is the raw -dot of MC-CNN-fast.  Features are used as given
 * (normalising them is the caller's business).  Every entry is written, out-of-view ones through the clamped column:
 * les_hip_fill_out_of_view comes after it.  Computed by v_mfma_f32_32x32x2_f32 in ascending channel order: the same bytes as the chain
 * (DESIGN 3.2k), and in any case within alpha gamma_(C+1) sum_c |fI_c fJ_c| + 2^-24 |cost| of the exact value, gamma_n = n 2^-24 / (1 - n 2^-24).
 * LES_HIP_ERR_ARG: null pointers, non-positive sizes, a mode outside 0 / 1, alpha or beta not finite.  LES_HIP_ERR_UNSUPPORTED: D H W >= 2^32,
 * H > 65535, C > 512. */
int les_hip_build_feature_volume(const float* d_featL, const float* d_featR, float* d_vol, int C, int D, int H, int W, int mode, int d0, float alpha,
                                 float beta, int device, void* hip_stream);
/* diagnostics: with LES_HIP_FEATVOL_TIMING=1 in the environment the two calls above bracket their launch with events; this returns the device
 * milliseconds of the calling thread's last descriptor launch and last volume launch, -1 for one not run yet (tools/featvol_timing.py). */
int les_hip_featvol_last_times(float* features_ms, float* volume_ms);

/* replaces (on the device): the pairwise side of FastGCStereo::expansionMoveBK's graph construction
 * (LES/FastGCStereo.h:425-551) with StereoEnergy::initSmoothnessCoeff / computeSmoothnessTerm /
 * computeSmoothnessTermsExpansion (LES/StereoEnergy.h:131-163, 225-230, 398-453): for every cell i of the batch (its
 * target rect = the cell's shared region, proposal d_planes[i]) the ready-made capacities of the cell's 8-connected
 * grid graph.  d_payload: 5 floats per node {source-minus-sink terminal residual, arc capacities towards E, S, SW, SE}
 * (reverse capacities are 0), cell i at 5 * offsets[i] floats, nodes row-major over its rect; total
 * les_hip_batch_graph_nodes() nodes.  The values are bit-identical to the host construction
 * (localexpstereo_amd/host/ExpansionMove.h).  d_labels / d_cur / d_prop: current label map, current and proposal cost
 * maps (H x W, device).  flow0_host (n doubles, may be NULL): flow already routed by the t-links per cell. */
long long les_hip_batch_graph_nodes(const les_hip_batch* batch);
int les_hip_batch_graph_offsets(const les_hip_batch* batch, long long* offsets /* n */);
int les_hip_batch_expansion_graph(les_hip_ctx* ctx, const les_hip_batch* batch, int mode, const les_hip_plane* d_planes,
                                  const les_hip_plane* d_labels, const float* d_cur, const float* d_prop, float lambda, float th_smooth,
                                  float omega, float epsilon, float* d_payload, double* flow0_host);

/* replaces (on the device): the graph construction of FastGCStereo::fusionMoveBK (LES/FastGCStereo.h:241-363) with
 * StereoEnergy::computeSmoothnessTermsFusion (LES/StereoEnergy.h:331-394) -- the move that fuses the current label map d_labels with a
 * second map d_labels1 (H x W planes, device; not the same buffer), pixel by pixel, where the expansion move tries one plane per cell.  Same
 * cells, payload layout, node order and flow0 as les_hip_batch_expansion_graph, so every solver below (and les_gc_solve_prebuilt) cuts the
 * graphs unchanged; mask 255 = the pixel takes d_labels1's label.  d_cur / d_prop: the unary costs of d_labels / of d_labels1 at every pixel
 * (les_hip_unary_labels gives the latter in one dense pass).  Definition and operation order: csrc/les_pairwise.h.  Unlike the reference,
 * which drops cost11 (:255, right only for a one-plane proposal), the term of "both take" enters the graph; a pair that is not submodular
 * (c10 + c01 < c11 + c00) gets arc capacity 0, so the cut minimises an upper bound of the energy that is exact at "all keep" and "all
 * take": the move never raises the energy.  With d_labels1 constant over every cell the payload is that of the expansion graph, bit for bit.
 * d_nonsubmodular (n ints on the device, may be NULL): the truncated pairs per cell; zeroed and counted on the calling thread's stream. */
int les_hip_batch_fusion_graph(les_hip_ctx* ctx, const les_hip_batch* batch, int mode, const les_hip_plane* d_labels1,
                               const les_hip_plane* d_labels, const float* d_cur, const float* d_prop, float lambda, float th_smooth,
                               float omega, float epsilon, float* d_payload, double* flow0_host, int* d_nonsubmodular);

/* replaces (on the device, for cells of at most LES_HIP_MAXFLOW_MAX_NODES nodes): the max-flow and the segment read-out of
 * FastGCStereo::expansionMoveBK -- graph.maxflow(); graph.what_segment(i) == SOURCE (LES/FastGCStereo.h:553-559) -- on the
 * payload of les_hip_batch_expansion_graph, for all cells of the batch, one workgroup per cell with the whole graph on chip
 * (synchronous push-relabel; the cut is the canonical one of the reference's solver: SINK side = nodes that can still reach the
 * sink).  Two kernels, chosen for every cell on its own shape: a cell of at most 2048 nodes with (w + 2) * (h + 2) <= 2304 and h <= 70 -- the
 * finest layer's cells -- runs csrc/les_maxflow_cell.h (residuals in registers, two barriers per iteration), any other cell csrc/les_maxflow.h
 * (residuals in LDS); a call launches once per kernel it needs.  Same cut from both up to nodes on exact ties that float rounding moves, which
 * is why the choice never looks at the other cells.  les_hip_batch_graph_solver_kind says which kernels a call launches: the most general one of
 * its cells (0 = only les_maxflow_cell.h, 1 / 2 = les_maxflow.h with 1024 / 512 threads for some cell, -1 = a cell above the limit);
 * LES_HIP_MAXFLOW_CELL_KERNEL=0 in the environment forces les_maxflow.h.  d_masks: one byte per graph node (255 = the node takes the proposal), the input of les_hip_batch_apply_masks;
 * d_status: n ints (0 = solved, 1 = iteration limit reached: cut that cell with the host solver instead); d_flows: n doubles or
 * NULL (flow through the n-links; add flow0 of les_hip_batch_expansion_graph for the value of the cut).
 * les_hip_batch_max_cell_nodes: the largest w * h of the batch's target rects (callers check it against the limit). */
#define LES_HIP_MAXFLOW_MAX_NODES 2304
long long les_hip_batch_max_cell_nodes(const les_hip_batch* batch);
int les_hip_batch_graph_solver_kind(const les_hip_batch* batch);
int les_hip_batch_solve_graphs(les_hip_ctx* ctx, const les_hip_batch* batch, const float* d_payload, unsigned char* d_masks, int* d_status,
                               double* d_flows);
/* The same with a running count: *d_unsolved_total (a device int the caller zeroed) += 1 for every cell that hits the iteration limit.  A caller
 * that enqueues the lock-steps of a whole disjoint set without synchronising reads this ONE word at the end of the set instead of n status words
 * per lock-step (and repeats the set the slow way in the -- so far unobserved -- case that it is not zero). */
int les_hip_batch_solve_graphs_counted(les_hip_ctx* ctx, const les_hip_batch* batch, const float* d_payload, unsigned char* d_masks, int* d_status,
                                       double* d_flows, int* d_unsolved_total);

/* The same replacement (LES/FastGCStereo.h:553-559 on the graph of :411-551) for cells of ANY size -- the coarse layers, whose cells
 * (129 x 129 ... 404 x 387 nodes at the Adirondack shape) do not fit a workgroup's LDS: the graphs stay in device memory, a cell is
 * cut into tiles of <= 1920 nodes, one workgroup per tile, and the lock-step is a sequence of launches in which every cell moves
 * through exact relabelling / discharge phases on its own (region-parallel push-relabel, csrc/les_maxflow_tiled.h).  Same payload,
 * masks, status (0 = solved, non-zero = launch limit reached: cut that cell with the host solver) and flows as
 * les_hip_batch_solve_graphs; same cut (SINK side = the nodes that can still reach the sink).  Bit-reproducible from run to run (heights relabelled from a snapshot, flow
 * values summed as 64-bit integers; round 6).
 * d_workspace: caller-owned device scratch of at least les_hip_batch_tiled_workspace_bytes(batch) bytes, 256-byte aligned, not
 * shared between host threads that call concurrently (109 bytes per graph node + 64 per cell).  The call synchronises the calling
 * thread's stream (between groups of launches it looks at a host-mapped "cells done" word the kernel adds to: no copy); launches_out
 * (or NULL): launches enqueued; unsolved_out (or NULL): cells that hit the launch limit (their d_status is non-zero) -- callers that
 * only need "all solved?" read it instead of copying d_status back. */
long long les_hip_batch_tiled_workspace_bytes(const les_hip_batch* batch);
int les_hip_batch_solve_graphs_tiled(les_hip_ctx* ctx, const les_hip_batch* batch, const float* d_payload, unsigned char* d_masks, int* d_status,
                                     double* d_flows, void* d_workspace, long long workspace_bytes, int* launches_out, int* unsolved_out);
/* Hand-over (round 6): a lock-step lasts as long as its slowest cell, and the launches are at their worst on the tail of a hard cell (a few
 * hundred small excesses, one cell's tiles on a 256-CU chip).  At the progress checks (after launch 12, then every 16 launches) every open cell
 * that has had 60 launches and has at most 40 000 nodes -- and after 220 launches every open cell -- goes to the host cores: its residual graph
 * (8 residual capacities + the excess per node, 36 bytes) is written to host-mapped memory and finished with FIFO push-relabel from the remaining
 * excess nodes (host/ResidualCut.h; one thread per cell).  The residual graph of a feasible preflow has the minimum cuts of the graph it came
 * from, so masks, status and flows mean what they mean without it.  LES_HIP_MAXFLOW_HANDOVER=0 switches it off (the other LES_HIP_MAXFLOW_* variables
 * -- A/B measurements, tooling, tests -- are listed in one table, above MfKnobs / MtKnobs in csrc/les_hip_cuts.inc).
 * The _stats form reports what happened (the plain form = the _stats form without the report).
 * Both device max-flows keep one property that multi-rank runs (N ranks == 1 rank, bit for bit) and repeatable runs rest on: a cell's cut -- mask,
 * status, flow value -- is a function of its graph and the solver parameters (environment knobs included), not of the other cells of the call, their
 * order or their number; the hand-over decision looks at the cell alone.  tests/parity_cases.py: case_cut_is_a_function_of_the_cell holds it. */
typedef struct les_hip_tiled_stats {
    int launches;            /* launches of les_maxflow_tiled_kernel enqueued */
    int unsolved;            /* cells that hit the launch limit (d_status non-zero) */
    int handed_cells;        /* cells finished by the host cores from their residual graphs */
    long long handed_nodes;  /* ... and their graph nodes (36 bytes each crossed PCIe, 1 byte came back) */
    double host_ms;          /* wall-clock of the host cores' part */
} les_hip_tiled_stats;
int les_hip_batch_solve_graphs_tiled_stats(les_hip_ctx* ctx, const les_hip_batch* batch, const float* d_payload, unsigned char* d_masks, int* d_status,
                                           double* d_flows, void* d_workspace, long long workspace_bytes, les_hip_tiled_stats* stats);

/* replaces: the mask updates after a graph cut -- subProposalCost.copyTo(subCurrentCost, updateMask);
 * subCurrentLabeling.setTo(label, updateMask) (LES/FastGCStereo.h:61-62) -- for all cells of the batch.  d_masks: one
 * byte per graph node in the payload order of les_hip_batch_expansion_graph (non-zero = the node takes the proposal). */
int les_hip_batch_apply_masks(les_hip_ctx* ctx, const les_hip_batch* batch, const les_hip_plane* d_planes, const unsigned char* d_masks,
                              float* d_cur, const float* d_prop, les_hip_plane* d_labels);

/* replaces: the same mask updates after a fusion move (LES/FastGCStereo.h:61-62 with the label map of fusionMoveBK, :253, in the place of
 * the one plane): where the mask is non-zero, d_cur <- d_prop and d_labels <- d_labels1 (H x W planes, device; not the same buffer). */
int les_hip_batch_apply_masks_labels(les_hip_ctx* ctx, const les_hip_batch* batch, const les_hip_plane* d_labels1, const unsigned char* d_masks,
                                     float* d_cur, const float* d_prop, les_hip_plane* d_labels);

/* ---- evaluation of the device-resident solution on the device (csrc/les_eval.h) ----
 * replaces: Evaluator::evaluate's numbers (LES/Evaluator.h:113-187; its PNG dumps and windows are not part of this) with
 * PMStereoBase::computeCurrentEnergy (LES/PMStereoBase.h:263-270) = cv::sum(currentCost) + StereoEnergy::computeSmoothnessCost
 * (LES/StereoEnergy.h:165-203), Evaluator::quantize (:106-111) and the bad-pixel counts (:133-140), in one pass over the device label
 * and cost maps of a view, without copying either to the host.
 * An evaluator holds the ground truth and the non-occlusion mask (H x W floats / bytes on the host, uploaded once; both may be NULL: the
 * four counts are then 0; a NULL mask with ground truth counts every pixel as non-occluded), the error threshold, the precision the
 * disparities are quantised to (<= 0: none) and a device-resident log of max_rows rows.  One host thread at a time uses an evaluator;
 * two views take two evaluators. */
typedef struct les_hip_evaluator les_hip_evaluator;
typedef struct les_hip_eval_row {
    int index, mode;                     /* as given to les_hip_evaluate */
    double data, smooth;                 /* sum of the cost map; sum of the forward pair terms inside the image */
    long long good_valid, good_nonocc;   /* pixels with |d - gt| <= threshold among the valid (gt > 0 and finite) / the non-occluded ones */
    long long n_valid, n_nonocc;
} les_hip_eval_row;
int les_hip_evaluator_create(les_hip_ctx* ctx, const float* gt_host, const unsigned char* nonocc_host, float error_threshold, float precision,
                             int max_rows, les_hip_evaluator** out);
void les_hip_evaluator_destroy(les_hip_evaluator* ev);
/* Appends one row for the maps d_labels / d_cost of view `mode`.  ENQUEUE ONLY, on the calling thread's stream of the context
 * (les_hip_set_thread_stream is honoured): no synchronisation and no allocation (the first call, and a call with another omega or epsilon
 * than the context's last pairwise call, build the 766-entry coefficient table and synchronise once).  The row describes the maps as they
 * are at this point of the stream.  Every f32 term is added in fp64 in an order that depends on (H, W) only: the same maps give the same
 * bits on any stream, beside any other work.  A NaN term makes its sum NaN, as on the host.  A full log is an error, returned before
 * anything is enqueued. */
int les_hip_evaluate(les_hip_ctx* ctx, les_hip_evaluator* ev, int mode, const les_hip_plane* d_labels, const float* d_cost, float lambda,
                     float th_smooth, float omega, float epsilon, int index);
/* Synchronises the calling thread's stream and copies the rows written so far (*n of them; capacity = room in rows_host). */
int les_hip_evaluator_rows(les_hip_ctx* ctx, les_hip_evaluator* ev, les_hip_eval_row* rows_host, int capacity, int* n);
/* replaces (on the device): the energy side of the reference's flow == energy self-check (LES/FastGCStereo.h:561-594) -- for every cell i of
 * the batch (its target rect = the shared region) the energy of the CURRENT maps that the move can change: the cost of every pixel of the
 * region plus every forward pair term with at least one endpoint in the region and both in the image.  Called after
 * les_hip_batch_apply_masks it is the energy of the fused labelling, which the cut's value (flow0 + flow) equals.  d_energy: n doubles on
 * the device.  Enqueue only on the calling thread's stream, except that the first call per (batch, view) allocates the partial-sum slots (hipMalloc:
 * an implicit synchronisation) and the first call, or one with another omega or epsilon than the context's last pairwise call, builds the coefficient
 * table and synchronises once.  A cell's value is a function of its rect and the maps, not of the other cells of the call. */
int les_hip_batch_region_energy(les_hip_ctx* ctx, const les_hip_batch* batch, int mode, const les_hip_plane* d_labels, const float* d_cost,
                                float lambda, float th_smooth, float omega, float epsilon, double* d_energy);

/* replaces: PMStereoBase::doConsistencyCheck (LES/PMStereoBase.h:111-144) -- left-right check of the disparities of two
 * device label maps (H x W planes each): fail = 255 where |d_other(x -/+ d) - d| > threshold, 128 where the pixel maps
 * outside the other view, 0 otherwise.  d_failL / d_failR: H x W bytes on the device. */
int les_hip_consistency_check(les_hip_ctx* ctx, const les_hip_plane* d_labelsL, const les_hip_plane* d_labelsR, float threshold,
                              unsigned char* d_failL, unsigned char* d_failR);

/* ---- cross-view fusion: a label map of one view expressed in the other view's coordinates (csrc/les_crossview.h holds the definition) ----
 * No reference counterpart: the reference's two views meet only in the post-processing (LES/FastGCStereo.h:172-203); this is PatchMatch Stereo's
 * "view propagation".  d_src: the H x W planes of view src_mode (0 left, 1 right); every source pixel (xs, y) with disparity d lands on column
 * floor(xs -/+ d + 0.5) of row y of the other view, its plane rewritten for that view: (a, b, c) / (1 -/+ a), v negated.  The largest d wins a
 * target pixel (then the largest xs); planes with 1 -/+ a < 0.125, non-finite components or a landing column outside the image are not
 * proposed.  d_out: target pixels with a winner get its plane, the others d_fallback's plane bit for bit; d_hit (H x W bytes, may be NULL):
 * 1 / 0.  The result is a function of the inputs only.  d_out may be d_fallback (each target pixel is read and written by one thread), NOT
 * d_src (LES_HIP_ERR_ARG).  The output is a second labelling for les_hip_batch_fusion_graph.
 * Enqueue only, on the calling thread's stream (les_hip_set_thread_stream is honoured): no allocation, no synchronisation; one launch, one
 * workgroup per row.  Rows wider than 8192 pixels: LES_HIP_ERR_UNSUPPORTED, nothing is launched. */
int les_hip_warp_labels(les_hip_ctx* ctx, int src_mode, const les_hip_plane* d_src, const les_hip_plane* d_fallback, les_hip_plane* d_out,
                        unsigned char* d_hit /* may be NULL */);

/* ---- winner-take-all labels of the aggregated cost volume (csrc/les_wtavol.h holds the definition) ----
 * No reference counterpart: the reference starts every run from one random plane per finest-layer cell (initCurrentFast,
 * LES/FastGCStereo.h:94-115) and never reads a whole aggregated volume.  This is cost-volume filtering's read-out of the H1 workload (the slabs
 * of K fronto-parallel planes, les_hip_batch_create with out_slabs = 1): per pixel the slab k* of least cost -- the comparison is c < best from
 * best = +inf, so NaN and +inf never win and of equal costs the lowest disparity wins -- refined by the parabola through the costs of slabs
 * k* - 1, k*, k* + 1 (off = 0.5 (cm - cp) / ((cm - c0) + (cp - c0)) when 0 < k* < K - 1, cm and cp are finite and the denominator is positive,
 * else 0; |off| <= 0.5).  Label (0, 0, (k* + off) + min_disparity, 0), cost c0; a pixel without a winner gets (0, 0, min_disparity, 0) and +inf.
 *
 * The reduction streams: les_hip_slab_argmin consumes one chunk of n slabs ([n][H][W] floats on the device; slab i is slab k_first + i of the
 * volume) and updates d_state (les_hip_slab_argmin_state_bytes(H, W) bytes on the device, 16-byte aligned, opaque; k_first == 0 initialises it, so
 * it needs no clearing); the chunks of one volume are fed in order, each slab once.  les_hip_slab_argmin_finish turns the state after K slabs
 * into d_labels (H x W planes) and d_cost (H x W floats); subpixel == 0: off = 0 everywhere.  How the K slabs are cut into chunks changes no bit
 * of the outputs.  Both are enqueue only, on the calling thread's stream (les_hip_set_thread_stream is honoured): no allocation, no
 * synchronisation; calls on distinct states may come from distinct host threads. */
size_t les_hip_slab_argmin_state_bytes(int H, int W);
int les_hip_slab_argmin(les_hip_ctx* ctx, const float* d_slabs, int n, int k_first, void* d_state);
int les_hip_slab_argmin_finish(les_hip_ctx* ctx, const void* d_state, int K, int subpixel, les_hip_plane* d_labels, float* d_cost);
/* The whole operation for view `mode`: K = int(max_disparity - min_disparity) + 1 planes (0, 0, min_disparity + k, 0) with filterRect =
 * targetRect = the image and check = 0 run through the batch path (the kernel les_hip_batch_kernel_kind reports for such a batch: any context,
 * any filter, the interpolation that is set), `chunk` planes per launch (chunk <= 0: 32; clamped to K) into a slab workspace the context owns;
 * each chunk is reduced as it lands, then the state is finished into d_labels / d_cost.  Every label is a valid one (its disparity lies in
 * [min_disparity, min_disparity + K - 1]).  A view that was not supplied at creation, or a null output: LES_HIP_ERR_ARG.
 * Asynchronous on the calling thread's stream, except that the first call on a context -- and one with a larger chunk, or after the disparity
 * range changed -- allocates (planes, one prepared batch per chunk length, chunk x H x W floats of slabs, the state: hipMalloc and table uploads
 * synchronise).  The workspace is one per context: ONE host thread at a time may call this on a context (the two views one after the other);
 * other entry points may run beside it on other threads. */
int les_hip_wta_labels(les_hip_ctx* ctx, int mode, int chunk, int subpixel, les_hip_plane* d_labels, float* d_cost);

/* ---- the confidence of a label map under the aggregated cost volume (csrc/les_confidence.h holds the definition) ----
 * No reference counterpart: the reference hands back disparities without saying which to trust.  The cost-margin measure on the filtered volume,
 * a second reduction over the slabs les_hip_wta_labels reduces: a pixel with label (a, b, c, v) has its own disparity d = (a x + b y) + c
 * (un-fused) and u = d - min_disparity; slab k is in band iff fabsf((float)k - u) <= band.  own = the least cost of the slabs in band, rival =
 * the least cost of the others and k_r its slab (comparisons c < best from +inf: NaN and +inf never win, of equal costs the lowest k wins).
 * conf = 0 when no in-band slab won (a label outside the volume's range, a NaN label, costs all NaN / +inf), else 1 when no rival won, else
 * (rival - own) / scale clamped to [0, 1] (NaN: 0).  All in f32.
 *
 * The reduction streams: les_hip_slab_confidence consumes one chunk of n slabs ([n][H][W] floats on the device; slab i is slab k_first + i of
 * the volume) and updates d_state (les_hip_slab_confidence_state_bytes(H, W) bytes on the device, 16-byte aligned, opaque).  k_first == 0
 * initialises the state from d_labels (H x W planes), which is read only then (it may be NULL for k_first > 0); `band` is the same in every call
 * of one volume; the chunks are fed in order, each slab once.  les_hip_slab_confidence_finish turns the state into d_conf (H x W floats in
 * [0, 1]) and, where not NULL, d_own, d_rival (H x W floats: +inf where nothing won) and d_krival (H x W ints: -1 where no rival won).  How the
 * slabs are cut into chunks changes no bit of the outputs.  Both are enqueue only, on the calling thread's stream (les_hip_set_thread_stream is
 * honoured): no allocation, no synchronisation; calls on distinct states may come from distinct host threads.
 * A null pointer, n or k_first negative, a state that is not 16-byte aligned, band negative or NaN, scale not positive or not finite:
 * LES_HIP_ERR_ARG, nothing is launched or written. */
size_t les_hip_slab_confidence_state_bytes(int H, int W);
int les_hip_slab_confidence(les_hip_ctx* ctx, const les_hip_plane* d_labels, const float* d_slabs, int n, int k_first, float band, void* d_state);
int les_hip_slab_confidence_finish(les_hip_ctx* ctx, const void* d_state, float scale, float* d_conf, float* d_own /* may be NULL */,
                                   float* d_rival /* may be NULL */, int* d_krival /* may be NULL */);
/* The whole operation for the device label map d_labels of view `mode`: the K planes of les_hip_wta_labels run through the batch path `chunk`
 * at a time (chunk <= 0: 32; clamped to K) and each chunk is reduced as it lands.  It shares les_hip_wta_labels' planes, prepared batches and
 * slab workspace on the context; the confidence state is a buffer of its own (freed with the context), so a call changes nothing a later
 * les_hip_wta_labels returns, and the converse.  d_labels is only read.  A sensible `scale` is the largest value a raw matching cost of the
 * context can take: th_col for the cost-volume energy, (1 - alpha) th_col + alpha th_grad for the image-based one.
 * A null context, d_labels or d_conf, a view that was not supplied at creation, band negative or NaN, scale not positive or not finite, a
 * disparity range les_hip_wta_labels refuses: LES_HIP_ERR_ARG, nothing is launched or written.
 * Threading and streams as for les_hip_wta_labels: asynchronous on the calling thread's stream, except that a call that has to allocate (the
 * first on a context, a larger chunk, a changed disparity range) synchronises; the workspace is one per context, so ONE host thread at a time may
 * call this or les_hip_wta_labels on a context, and calls on different streams must be ordered by the caller; other entry points may run beside it. */
int les_hip_confidence(les_hip_ctx* ctx, int mode, const les_hip_plane* d_labels, int chunk, float band, float scale, float* d_conf,
                       float* d_own /* may be NULL */, float* d_rival /* may be NULL */, int* d_krival /* may be NULL */);

/* ---- semi-global matching over a view's matching-cost volume (csrc/les_sgm.h holds the definition) ----
 * No reference counterpart (as above).  The classic step between local aggregation and a global graph cut: scan-line dynamic programming over the
 * RAW volume of view `mode` (float [D][H][W], slice k = disparity min_disparity + k; K = int(max_disparity - min_disparity) + 1 slices are
 * used, K <= D) along the first `paths` (2, 4 or 8) of the directions (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1).  Costs are
 * truncated first: C' = C where C is finite and below th_col, else th_col.  Along direction r, with q = p - r: L(p,k) = C'(p,k) where q lies
 * outside the image, else C'(p,k) + (min(L(q,k), min(L(q,k-1), L(q,k+1)) + p1, m + p2) - m) with m = min_j L(q,j) and only the neighbours that
 * exist.  S = ((L_0 + L_1) + L_2) + ... in direction order, all in f32, a function of the inputs only (no atomics; the directions are successive
 * launches).  The read-out over S(p, 0..K-1) is les_hip_wta_labels' rule: the first minimum wins, the parabola offset when subpixel != 0;
 * label (0, 0, (k* + off) + min_disparity, 0) into d_labels (H x W planes), S(p,k*) into d_sum (H x W floats; may be NULL).
 * A view that was not supplied at creation, a null d_labels, paths outside {2, 4, 8}, a negative or non-finite penalty, p2 < p1, a non-finite
 * th_col, K > D: LES_HIP_ERR_ARG.  A context of the image-based energy (it holds no volume), K > 512, H > 65535: LES_HIP_ERR_UNSUPPORTED.
 * Nothing is launched and nothing written in either case.
 * The workspace -- the transposed volume and S, 2 H W Kp floats with Kp = K rounded up to 64, 128, 256 or 512: les_hip_sgm_workspace_bytes for the
 * current disparity range, 0 where les_hip_sgm_labels would refuse the context -- belongs to the context: built by the first call, regrown when the
 * disparity range grows (hipMalloc: an implicit synchronisation), freed by les_hip_destroy.  Otherwise enqueue only, on the calling thread's stream
 * (les_hip_set_thread_stream is honoured).  ONE host thread and ONE stream at a time may use this on a context (the two views one after the other):
 * the calls share the workspace and nothing orders them across streams, so a call on another stream than the context's last SGM call must follow a
 * synchronisation of that one.  Other entry points may run beside it on other threads.
 * LES_HIP_SGM_TIMING=1 (read per call): the call brackets its kernels with events and waits for the last; les_hip_sgm_last_times then gives the
 * calling thread the device milliseconds of its last call: *n = paths + 2 values (transpose, one per direction, read-out), the first min(*n, cap)
 * of them into ms.  LES_HIP_ERR_ARG when the thread has made no such call. */
size_t les_hip_sgm_workspace_bytes(const les_hip_ctx* ctx);
int les_hip_sgm_labels(les_hip_ctx* ctx, int mode, int paths, float p1, float p2, int subpixel, les_hip_plane* d_labels, float* d_sum /* may be NULL */);
int les_hip_sgm_last_times(float* ms, int cap, int* n);

/* ---- slanted planes fitted to a disparity map (csrc/les_planefit.h holds the definition) ----
 * No reference counterpart: the reference's only start is one random plane per finest-layer cell (initCurrentFast, LES/FastGCStereo.h:94-115).
 * Per pixel p of view `mode` an edge-aware weighted least-squares plane through the disparities of its (2 radius + 1)^2 window: the input is
 * EITHER d_labels (H x W planes; d = (a x + b y) + c, the output keeps the centre label's v) OR d_disp (H x W floats; v = 0), the other one
 * NULL.  A tap s is taken iff its disparity is finite and |d(s) - d(p)| <= gate0 + gate_slope max(|dx|, |dy|); its weight is
 * exp(-|I(p) - I(s)|_1 / sig) of the view's 8-bit guide colours (sig == 0: 1).  The nine sums are taken in fp64 in a fixed tap order and the
 * 3 x 3 normal equations solved by cofactors, so the result is a function of the inputs only.  The fit (a, b, c, v) is accepted -- d_kind 2 --
 * iff it has at least min_support taps, its support is not collinear (det > 1e-3 S^3), it passes within gate0 of d(p), |a|, |b| <= max_slope
 * and the plane is a valid label at p (IsValiLabel).  Otherwise the pixel gets (0, 0, d(p), v) -- d_kind 1 -- when d(p) lies in the energy's
 * disparity range, else -- d_kind 0, also when d(p) is not finite -- d_fallback's label bit for bit ((0, 0, min_disparity, 0) when
 * d_fallback is NULL).  d_kind may be NULL.  d_out may be d_fallback; it may not be the input map.
 * radius 1 .. 15 (above: LES_HIP_ERR_UNSUPPORTED); sig >= 0, gate0 > 0, gate_slope >= 0, max_slope > 0, all finite; min_support >= 3;
 * anything else, both or neither input map, a null d_out, a view without an image: LES_HIP_ERR_ARG, nothing launched.
 * Enqueue only, on the calling thread's stream (les_hip_set_thread_stream is honoured), except that the first call with a value of sig
 * uploads its 766-entry weight table and waits for that stream; the context keeps the tables of the last 8 values. */
int les_hip_fit_planes(les_hip_ctx* ctx, int mode, const les_hip_plane* d_labels /* or NULL */, const float* d_disp /* or NULL */,
                       const les_hip_plane* d_fallback /* may be NULL */, les_hip_plane* d_out, unsigned char* d_kind /* may be NULL */, int radius,
                       float sig, float gate0, float gate_slope, float max_slope, int min_support);

/* ---- a half-resolution solve as a start: pooled images and volumes, upsampled planes (csrc/les_pyramid.h holds the definitions) ----
 * No reference counterpart: the reference solves at one resolution (LES/FastGCStereo.h:133-227).  Sizes: Hh = (H + 1) / 2, Wh = (W + 1) / 2,
 * Dh = (D + 1) / 2; every source index clamps to its range.  All three operations are exact (integers, or f32 in a fixed order with
 * power-of-two multipliers only): the same inputs give the same bytes on every build.
 * les_hip_pool_image: u8 [H][W][3] -> [Hh][Wh][3] in DEVICE memory, per channel (p00 + p01 + p10 + p11 + 2) >> 2.
 * les_hip_pool_volume: f32 [D][H][W] -> [Dh][Hh][Wh] in DEVICE memory; half slice k is full slice 2k: per pixel of the 2 x 2 block
 * t = (0.25 C[2k - 1] + 0.5 C[2k]) + 0.25 C[2k + 1], result (((t00 + t01) + t10) + t11) 0.25; NaN and +-inf propagate.  Reads the volume once.
 * LES_HIP_PYRAMID_NT=1 / 0 selects non-temporal / plain loads (default: non-temporal).
 * Both are context-free and enqueue only on hip_stream of `device`.  LES_HIP_ERR_ARG for null pointers and non-positive sizes;
 * LES_HIP_ERR_UNSUPPORTED for volumes of 2^32 or more floats; nothing is written on a refused call. */
int les_hip_pool_image(const uint8_t* d_src, uint8_t* d_dst, int H, int W, int device, void* hip_stream);
int les_hip_pool_volume(const float* d_src, float* d_dst, int D, int H, int W, int device, void* hip_stream);
/* A new, independent context of the same kind as src (cost-volume or image-based energy), filter and interpolation at half resolution, built
 * from src's own device images and volumes: the images pooled, every volume pooled into memory the new context owns, guide statistics, march
 * tables and the tiled copy exactly as les_hip_create* would build them from the same pooled inputs.  Its parameters: H, W, D -> Hh, Wh, Dh;
 * max_disparity, min_disparity and the two vertical-disparity settings halved; windR -> max(1, (windR + 1) / 2); everything else (eps,
 * th_col, alpha, th_grad, device, the context's stream) unchanged.  src may be destroyed before it.  A min_disparity that is not an even integer:
 * LES_HIP_ERR_UNSUPPORTED (half slice k would not sit on an integer disparity); null arguments: LES_HIP_ERR_ARG; a halved radius no kernel
 * serves: what les_hip_create* returns for it.  Synchronises the calling thread's stream of src. */
int les_hip_create_half(les_hip_ctx** out, const les_hip_ctx* src);
/* The H x W x 3 u8 BGR image of view `mode` as the context holds it, into HOST memory (for a context of les_hip_create_half: the pooled
 * image, so that a caller need not pool it again).  A view without an image, null pointers: LES_HIP_ERR_ARG.  Synchronous. */
int les_hip_get_image(les_hip_ctx* ctx, int mode, uint8_t* out_host);
/* The way up: d_src, the Hh x Wh planes of view `mode` found on ctx_half, re-expressed at full resolution into d_out (H x W planes; not d_src),
 * guided by the two contexts' images of that view.  Full pixel (X, Y) takes, of the half pixels (X >> 1, Y >> 1), its horizontal neighbour on
 * the side of X's parity, the vertical one likewise and the diagonal one (coordinates clamped), the one whose pooled colour is nearest to the
 * pixel's own in L1 (the first wins ties); its plane (a, b, c, v) becomes (a, b, (2c - a / 2) - b / 2, 2v), i.e. d_full(X, Y) =
 * 2 d_half((X - 1/2) / 2, (Y - 1/2) / 2).  Kept -- d_kind 0 -- iff it is a valid label of ctx_full at (X, Y) (IsValiLabel); otherwise
 * (0, 0, its disparity at (X, Y) clamped to ctx_full's range, 0) -- d_kind 1 -- or, when that disparity is not finite, (0, 0, min_disparity, 0)
 * -- d_kind 2.  d_kind: H x W bytes or NULL.  ctx_half must have the half size of ctx_full and its device; a view without an image, null
 * pointers: LES_HIP_ERR_ARG.  Enqueue only, on the calling thread's stream of ctx_full (les_hip_set_thread_stream is honoured). */
int les_hip_upsample_labels(les_hip_ctx* ctx_full, const les_hip_ctx* ctx_half, int mode, const les_hip_plane* d_src, les_hip_plane* d_out,
                            unsigned char* d_kind /* may be NULL */);

/* replaces: PMStereoBase::postProcess (LES/PMStereoBase.h:146-256), called by FastGCStereo::run for two-view runs
 * (LES/FastGCStereo.h:199-203, threshold 1.5): consistency check, horizontal fill of the failed pixels from the nearest
 * consistent neighbours (smaller disparity wins), then the colour-weighted median of the labels over the
 * (2 windR + 1)^2 window with weights exp(-|dI|_1 / omega) (StereoEnergy::computePatchWeight, LES/StereoEnergy.h:251-257).
 * Both device label maps are updated in place.  Needs both views' images in the context; windR <= 31. */
int les_hip_post_process(les_hip_ctx* ctx, les_hip_plane* d_labelsL, les_hip_plane* d_labelsR, float threshold, float omega);

/* ---- speckle filter (csrc/les_speckle.h holds the definition; no reference counterpart, the convention is OpenCV's filterSpeckles) ----
 * The connected components of the disparity map of a device label map (H x W planes; d = (a x + b y) + c in float, un-fused, whatever the
 * view): two 4-neighbours are connected iff both disparities are finite and fabsf(d(p) - d(q)) <= max_diff; a pixel with a non-finite
 * disparity is a component of its own.  A pixel is a speckle iff its component has at most max_size pixels (max_size 0: none is).
 * d_mask: H x W bytes, 255 speckle / 0; d_root (H x W ints or NULL): per pixel the smallest linear index y W + x of its component; d_size
 * (H x W ints or NULL): per pixel its component's pixel count.  Exact integers, a function of the inputs alone.  Runs on the calling
 * thread's stream and synchronises it before it returns.  max_size < 0, max_diff negative or NaN, null labels or mask: LES_HIP_ERR_ARG;
 * H W >= 2^31: LES_HIP_ERR_UNSUPPORTED.  Scratch: 12 bytes per pixel for the call's duration. */
int les_hip_speckle_mask(les_hip_ctx* ctx, const les_hip_plane* d_labels, int max_size, float max_diff, unsigned char* d_mask /* 255 / 0 */,
                         int* d_root /* or NULL */, int* d_size /* or NULL */);
/* The tile one workgroup of the component labelling owns (rows, columns): the compiled-in geometry, for tests and diagnostics. */
int les_hip_speckle_tile(int* th, int* tw);
/* les_hip_post_process with the failure mask widened: per view, fail = (left-right check failed) OR (speckle of that view's map); both
 * masks come from the labels before any label is modified; the dilation, the fill and the weighted median then run as in
 * les_hip_post_process.  One of the two label pointers may be NULL -- the one-view form: the mask is the speckle mask alone, only that
 * view's image is needed, `threshold` is ignored.  max_size 0: with both views exactly les_hip_post_process, with one view the labels stay
 * untouched.  Both pointers NULL, max_size < 0, max_diff negative or NaN: LES_HIP_ERR_ARG; windR > 31: LES_HIP_ERR_UNSUPPORTED. */
int les_hip_post_process_speckle(les_hip_ctx* ctx, les_hip_plane* d_labelsL /* or NULL */, les_hip_plane* d_labelsR /* or NULL */,
                                 float threshold, float omega, int max_size, float max_diff);
/* les_hip_post_process_speckle with the caller's own failure masks: d_failL / d_failR are H x W bytes on the device, nonzero = failed (a
 * thresholded les_hip_confidence map, say); either may be NULL.  Per view, fail = (left-right check failed) OR (speckle) OR (the caller's
 * mask); all masks are taken before any label is modified.  With both masks NULL it is les_hip_post_process_speckle, byte for byte; the
 * one-view form (one label pointer NULL; that view's mask is ignored) and the refusals are those of les_hip_post_process_speckle. */
int les_hip_post_process_masked(les_hip_ctx* ctx, les_hip_plane* d_labelsL /* or NULL */, les_hip_plane* d_labelsR /* or NULL */, float threshold,
                                float omega, int max_size, float max_diff, const unsigned char* d_failL /* or NULL */,
                                const unsigned char* d_failR /* or NULL */);

/* ---- 3D reconstruction: points, normals and a mesh from a label map (csrc/les_reproject.h holds the definition; the reference only paints
 * the normals as a picture, computeNormalMap, LES/StereoEnergy.h:274-289) ----
 * The calibration of a rectified pinhole pair, Middlebury v3's calib.txt: f = cam0[0][0], cx = cam0[0][2], cy = cam0[1][2] (pixels), doffs
 * (pixels) and baseline (any length unit: the points come out in it).  View m has cx_m = cx + (m ? doffs : 0); each view's points are in
 * that view's own camera frame, X right, Y down, Z forward, so X_left = X_right + baseline. */
typedef struct les_hip_calib {
    float f, cx, cy, doffs, baseline;
} les_hip_calib;
/* Per pixel (x, y) of the device label map of view `mode`, d = (a x + b y) + c in float, un-fused; then in double, rounded to float once:
 * D = d + doffs, Z = (f baseline) / D, X = ((x - cx_m) Z) / f, Y = ((y - cy) Z) / f, and the unit normal -n / |n| of the label's plane,
 * n = (a f, b f, ((a cx_m + b cy) + c) + doffs) -- the plane is exactly n . P = f baseline, and the normal faces the camera.  A pixel is valid
 * iff d is finite, D > 0, d_drop_mask (H x W bytes or NULL) is zero there, and Z <= z_max when z_max > 0.  d_points / d_normals: H x W x 3
 * floats each (either may be NULL), NaN at invalid pixels; d_valid: H x W bytes, 255 / 0.  Enqueue only (the calling thread's stream).
 * A null context, label map, calibration or valid map, a view not supplied at creation, f or baseline not finite or <= 0: LES_HIP_ERR_ARG;
 * H W >= 2^31: LES_HIP_ERR_UNSUPPORTED. */
int les_hip_reproject(les_hip_ctx* ctx, int mode, const les_hip_plane* d_labels, const unsigned char* d_drop_mask /* or NULL */,
                      const les_hip_calib* calib, float z_max, float* d_points /* or NULL */, float* d_normals /* or NULL */,
                      unsigned char* d_valid);
/* The triangle mesh over the pixel grid.  Pixels p, q are connected iff d_valid is nonzero at both and
 * |l_p(p) - l_q(p)| + |l_p(q) - l_q(q)| <= max_jump in float (the un-truncated pairwise term, LES/StereoEnergy.h:238-241; +inf connects every
 * valid neighbour).  Quad (x, y) with corners p00, p10, p01, p11 (first index: the x offset) yields T0 = (p00, p01, p10) and
 * T1 = (p10, p01, p11) -- the order whose geometric normal faces the camera -- each emitted iff its three edges are connected.  Vertex k is
 * the k-th valid pixel in row-major order; triangles are in row-major quad order, T0 before T1: a function of the inputs alone.
 * d_vertex_index: H x W ints, the pixel's vertex number or -1; d_vertex_pixel: room for H W ints, entry k = the linear pixel index of vertex
 * k; d_triangles: room for 2 (H - 1) (W - 1) x 3 ints (at least 1), vertex numbers; d_counts: two long longs on the device, the vertex and
 * the triangle count.  Four launches (count, scan, two emits), no atomics, no workgroup waits on another.  The tile workspace is kept on the
 * context per view: once it exists a call only enqueues on the calling thread's stream.  A null argument, a view not supplied at creation,
 * max_jump negative or NaN: LES_HIP_ERR_ARG; H W >= 2^31: LES_HIP_ERR_UNSUPPORTED. */
int les_hip_mesh(les_hip_ctx* ctx, int mode, const les_hip_plane* d_labels, const unsigned char* d_valid, float max_jump, int* d_vertex_index,
                 int* d_vertex_pixel, int* d_triangles, long long* d_counts);
/* The flat run of pixels one workgroup of the mesh kernels owns and the tiles the scan takes per turn of its loop: the compiled-in geometry,
 * for tests and diagnostics. */
int les_hip_mesh_tile(int* pixels, int* scan_width);

/* ---- view synthesis and the photometric check: a label map turned back into an image (csrc/les_view.h holds the definitions) ----
 * No reference counterpart.  All maps are device pointers: an image is H x W x 3 bytes (b, g, r), disp H x W floats, hit / src / vis H x W
 * bytes.  Every operation is f32, rounded, in the order of csrc/les_view.h: the outputs are a function of the inputs alone.  Each call is one
 * launch, one workgroup per row, enqueued on the calling thread's stream (les_hip_set_thread_stream is honoured): no allocation, no
 * synchronisation.  Rows wider than 8192 pixels: LES_HIP_ERR_UNSUPPORTED, nothing is launched.
 *
 * les_hip_render_view: the view of a camera at fraction t in [0, 1] of the baseline, counted from view src_mode (0 left, 1 right) towards the
 * other view, from that view's label map and image (d_image NULL: the context's image of src_mode).  Every source pixel (xs, y) with disparity
 * d = a xs + b y + c lands on column floor(xs -/+ d t + 0.5) of row y; of the pixels that land on one column the largest d wins (then the
 * largest xs): d_out_hit 1, d_out_disp its d (in view src_mode's full-baseline units).  A single column without a winner between two winners
 * whose d differ by at most 1 is a crack of a stretched surface: d_out_hit 2, d_out_disp their mean.  The colour of every hit column is the
 * source image sampled linearly at rx +/- disp t, clamped to the row, and rounded to nearest.  A hole: d_out_hit 0, colour 0, disp NaN.  t = 0
 * returns the source image wherever d is finite.  A null pointer (d_image aside), t outside [0, 1] or NaN, d_out_bgr == d_image: LES_HIP_ERR_ARG. */
int les_hip_render_view(les_hip_ctx* ctx, int src_mode, const les_hip_plane* d_labels, const unsigned char* d_image /* may be NULL */, float t,
                        unsigned char* d_out_bgr, float* d_out_disp, unsigned char* d_out_hit);
/* les_hip_blend_views: two renders of one camera -- (d_bgrL, d_dispL, d_hitL) view 0 rendered at t, (d_bgrR, d_dispR, d_hitR) view 1 rendered at
 * 1 - t; either triple may be NULL as a whole -- as one image.  Per pixel: both hit and |dL - dR| <= tol: colour (1 - t) cL + t cR rounded to
 * nearest, disp (1 - t) dL + t dR, d_out_src 3; both hit otherwise: the one of larger disp (a tie: the left one), d_out_src 1 (left) or 2
 * (right); one hit: that one; none: a hole, d_out_src 0, colour 0, disp NaN.  fill != 0: a hole takes colour and disp of the nearest pixel to
 * its left or to its right on the row that was not a hole, the one of smaller disp (the background; a tie: the left one), and d_out_src 4; a
 * row without any pixel stays a hole.  tol negative or NaN, t outside [0, 1], a partly given triple, both triples NULL, an output that is one
 * of the renders: LES_HIP_ERR_ARG. */
int les_hip_blend_views(les_hip_ctx* ctx, float t, float tol, int fill, const unsigned char* d_bgrL, const float* d_dispL, const unsigned char* d_hitL,
                        const unsigned char* d_bgrR, const float* d_dispR, const unsigned char* d_hitR, unsigned char* d_out_bgr, float* d_out_disp,
                        unsigned char* d_out_src);
/* les_hip_photo_error: the photometric consistency of the label map of view `mode` with the context's two images, without ground truth.  Per
 * pixel (xs, y): d_vis 0 where its landing column in the other view, floor(xs -/+ d + 0.5), does not exist; 2 where another pixel of the row
 * wins that column (larger d: the label map itself says the pixel is occluded); 0 where xo = xs -/+ d lies outside [0, W - 1]; else 1, and
 * d_err = (|db| + |dg| + |dr|) / 3 between the other image sampled linearly at xo and the pixel's own colour.  d_err is NaN wherever d_vis != 1.
 * A context created with one image, a null pointer: LES_HIP_ERR_ARG. */
int les_hip_photo_error(les_hip_ctx* ctx, int mode, const les_hip_plane* d_labels, float* d_err, unsigned char* d_vis);

/* ---- rectification: a calibrated raw stereo pair turned into the rectified pair every other entry assumes (csrc/les_rectify.h holds the
 * definitions; no reference counterpart, the reference reads rectified pairs only) ----
 * Camera model: a point (X, Y, Z) of a raw camera's frame (X right, Y down, Z forward) is seen at pixel (u, v), pixel centres at integer
 * coordinates, with dist = (k1, k2, p1, p2, k3, k4, k5, k6):  x' = X / Z, y' = Y / Z, r2 = x'^2 + y'^2,
 * rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),  x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2),
 * y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y',  u = fx x'' + cx, v = fy y'' + cy.  The two cameras of a rig are related by
 * X1 = R X0 + T (X0, X1: one point in the left and the right raw frame); the rectified pair has doffs = cx1 - cx0 and baseline = |T|
 * (io.stereo_rectify of the Python package makes the rectifying rotations and the les_hip_calib from K0, dist0, K1, dist1, R, T). */
typedef struct les_hip_camera {
    double fx, fy, cx, cy, dist[8];
} les_hip_camera;
/* d_map[y][x] = (u, v): where in the raw image rectified pixel (x, y) comes from.  M (row-major 3 x 3, host memory) takes a ray of the
 * rectified frame into the raw camera's frame -- the transpose of the view's rectifying rotation; f, cx, cy are the rectified view's
 * intrinsics.  The ray ((x - cx) / f, (y - cy) / f, 1) goes through M and the camera model above in fp64, in the one order of operations
 * csrc/les_rectify.h states, not contracted, and (u, v) is rounded to f32 once: the map is a function of the arguments alone, bit for bit.
 * A ray with Z <= 0 behind M, or a denominator of rad that is 0 or not finite, gives (NaN, NaN).  One work-item per pixel; the 25 doubles
 * travel as kernel arguments.  d_map: H x W x 2 floats on the device, 8-byte aligned.
 * les_hip_remap: d_dst[y][x][k] = d_src (Hs x Ws x channels bytes, channels 1 or 3) sampled at d_map[y][x]; interp 0 nearest (the tap
 * floor(u + 0.5)), 1 linear (four taps), 2 cubic (4 x 4 Catmull-Rom, a = -0.5); tap indices clamp to the image, the weights come from the
 * exact fp64 fractions of the f32 coordinates, the taps are summed in fp64 in one stated order and the result is floor(s + 0.5) clamped to
 * 0 .. 255: bit for bit a function of the inputs.  A pixel is valid iff its map entry is finite, 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1;
 * an invalid one gets 0 in every channel and reads nothing from d_src (NaN, +-inf and coordinates beyond the int range never form an index).
 * d_valid (H x W bytes or NULL): 1 valid / 0.  d_dst may not be d_src.
 * Both are context-free and enqueue only on hip_stream of `device`.  LES_HIP_ERR_ARG for null pointers, non-positive sizes, a map that is not
 * 8-byte aligned, f, fx or fy not finite or <= 0, channels or interp out of range; LES_HIP_ERR_UNSUPPORTED for Hs Ws channels >= 2^31 and
 * for H > 65535 (the launch grid); a refused call launches nothing. */
int les_hip_rectify_map(const les_hip_camera* raw, const double M[9], double f, double cx, double cy, float* d_map /* [H][W][2] */, int H, int W,
                        int device, void* hip_stream);
int les_hip_remap(const uint8_t* d_src, int Hs, int Ws, int channels /* 1 or 3 */, const float* d_map, uint8_t* d_dst,
                  unsigned char* d_valid /* may be NULL */, int H, int W, int interp /* 0 nearest, 1 linear, 2 cubic */, int device, void* hip_stream);

/* ---- the way back: results of the rectified pair registered to the pixels of the raw camera (csrc/les_unrectify.h holds the definitions; no
 * reference counterpart) ----
 * les_hip_unrectify_map: d_map[v][u] = (xs, ys), where in the rectified frame raw pixel (u, v) of one view lies -- the inverse of
 * les_hip_rectify_map's map, in its layout (Hs x Ws x 2 floats on the device, 8-byte aligned), so that les_hip_remap resamples any rectified-grid
 * byte image onto the raw grid through it.  R (row-major 3 x 3, host memory) is the view's rectifying rotation, a ray of the raw camera's frame
 * into the rectified frame (the transpose of les_hip_rectify_map's M); f, cx, cy are the rectified view's intrinsics.  The distortion of the
 * camera model above is inverted by `steps` (1 .. 64) rounds of the additive fixed point x <- x - (distort(x) - xd), which needs no division
 * beyond the model's own and converges where the distortion is a contraction; the forward model is then evaluated once more and the pixel is
 * kept only if its residual is at most `tol` (> 0) RAW pixels in u and in v.  A pixel that has not converged, a denominator of rad that is 0 or
 * not finite in any evaluation, and a ray with Z <= 0 in the rectified frame give (NaN, NaN): a position that fails the residual test is never
 * stored.  fp64 in the one order of operations csrc/les_unrectify.h states, not contracted, rounded to f32 once: bit for bit a function of
 * the arguments.
 * les_hip_unrectify_labels: the H x W label map of one view (d_labels, 16-byte aligned; d_drop: H x W bytes or NULL, nonzero = dropped) as geometry
 * on that view's raw grid through its inverse map d_invmap (Hs x Ws x 2).  A raw pixel whose (xs, ys) lies in [0, W - 1] x [0, H - 1] takes the label
 * of the nearest rectified pixel (floor(xs + 0.5), floor(ys + 0.5)) and evaluates that plane at its own position: d = a xs + b ys + c -- exact
 * on a surface, nothing mixed across a depth edge.  With D = d + doffs, Zr = f baseline / D: valid iff inside, d finite, D > 0, not dropped
 * and, when z_max > 0, Zr <= z_max.  d_points: M ((xs - cx) Zr / f, (ys - cy) Zr / f, Zr), the point in the RAW camera's frame (X right, Y down,
 * Z forward, the baseline's unit; the third component is the raw depth); d_normals: the unit normal of the label's plane in that frame, facing
 * the camera; d_disparity: d; each Hs x Ws (x 3) floats or NULL.  d_valid: Hs x Ws bytes, 255 / 0.  An invalid pixel holds NaN (0x7fc00000) in
 * every float output; a pixel outside the frame reads no label.  M (row-major 3 x 3, host memory) = R^T takes the rectified frame into the raw
 * camera's; f, cx, cy, doffs, baseline: the rectified calibration with cx the VIEW'S OWN principal point.  fp64 in one stated order, rounded once.
 * Both are context-free and enqueue only on hip_stream of `device`, one work-item per raw pixel.  LES_HIP_ERR_ARG for null pointers (the three
 * optional outputs and d_drop aside), non-positive sizes, a map that is not 8-byte or labels that are not 16-byte aligned, f, fx, fy or baseline
 * not finite or <= 0, steps outside 1 .. 64, tol not > 0; LES_HIP_ERR_UNSUPPORTED for Hs > 65535 (the launch grid) and H W >= 2^31; a refused
 * call launches nothing. */
int les_hip_unrectify_map(const les_hip_camera* raw, const double R[9], double f, double cx, double cy, int steps, double tol,
                          float* d_map /* [Hs][Ws][2] */, int Hs, int Ws, int device, void* hip_stream);
int les_hip_unrectify_labels(const les_hip_plane* d_labels, int H, int W, const unsigned char* d_drop /* may be NULL */, const float* d_invmap, int Hs, int Ws,
                             const double M[9], double f, double cx, double cy, double doffs, double baseline, float z_max, float* d_points /* may be NULL */,
                             float* d_normals /* may be NULL */, float* d_disparity /* may be NULL */, unsigned char* d_valid, int device, void* hip_stream);

/* ---- a fisheye raw camera: the two maps above for the equidistant (Kannala-Brandt) model (csrc/les_fisheye.h holds the camera model and the
 * definitions; no reference counterpart) ----
 * Camera model: a point (X, Y, Z) of the raw camera's frame is seen at (u, v), pixel centres at integer coordinates, zero skew, with
 * k = (k1, k2, k3, k4):  a = X / Z, b = Y / Z, r = sqrt(a^2 + b^2), theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6
 * + k4 theta^8), u = fx (theta_d / r) a + cx, v = fy (theta_d / r) b + cy (r = 0: the principal point).  theta_max in (0, pi] is the largest
 * theta the lens is calibrated for: a ray beyond it has no pixel (the guard against the polynomial folding back; io.fisheye_theta_max of the
 * Python package finds the fold).  Rays with Z <= 0 have no pixel either.
 * les_hip_rectify_map_fisheye is les_hip_rectify_map and les_hip_unrectify_map_fisheye is les_hip_unrectify_map for such a camera: the same
 * arguments, the same map layout (so les_hip_remap and les_hip_unrectify_labels take the maps unchanged), (NaN, NaN) where a pixel has no
 * position.  atan, sin and cos are stated in csrc/les_fisheye.h in plain fp64 operations in a fixed order (within 2.3e-16 of the C library's),
 * so both maps are, like the pinhole ones, a function of their arguments alone, bit for bit.  The inverse solves theta P(theta) = theta_d by
 * `steps` (1 .. 64) Newton steps -- it converges wherever d theta_d / d theta > 0, the whole field of a lens of 180 degrees and more -- and
 * keeps a pixel only where the forward model's residual is at most `tol` (> 0) RAW pixels: a position that fails the test is never stored.
 * Both are context-free and enqueue only on hip_stream of `device`.  The refusals and codes of the pinhole entries, and LES_HIP_ERR_ARG for a
 * k that is not finite and for a theta_max that is NaN or outside (0, pi]; a refused call launches nothing. */
typedef struct les_hip_fisheye {
    double fx, fy, cx, cy, k[4], theta_max;
} les_hip_fisheye;
int les_hip_rectify_map_fisheye(const les_hip_fisheye* raw, const double M[9], double f, double cx, double cy, float* d_map /* [H][W][2] */, int H, int W,
                                int device, void* hip_stream);
int les_hip_unrectify_map_fisheye(const les_hip_fisheye* raw, const double R[9], double f, double cx, double cy, int steps, double tol,
                                  float* d_map /* [Hs][Ws][2] */, int Hs, int Ws, int device, void* hip_stream);

/* ---- multi-GPU: publishing the tiles a rank updated (not in the reference, which is single-process; SURVEY 8(e): the cells of a
 * disjoint set -- LES/LayerManager.h:168-172 -- are split over the ranks, replicas of the label / cost maps are kept coherent by one
 * all-gather per set of the label (16 B/px) and cost (4 B/px) tiles of the shared regions, LES/FastGCStereo.h:22-72).
 * An exchange object is the plan for one (layer, set): rects = the target rects of ALL ranks' cells in rank order, first[r] .. first[r+1]
 * those of rank r (first has world + 1 entries).  Slot of a rank in the gathered buffer = les_hip_exchange_slot_floats floats:
 * [float4 labels x lmax][float costs x lmax] in rect order, row-major inside a rect.
 *   les_hip_exchange_pack    this rank's tiles (device maps) -> its slot (device buffer of slot_floats floats)
 *   les_hip_exchange_unpack  the gathered world x slot_floats buffer -> the other ranks' tiles into this rank's device maps
 *   les_hip_exchange_tiles   pack -> ncclAllGather on the ncclComm_t the HOST created (RCCL, resolved at run time with dlopen:
 *                            single-GPU users need no librccl) -> unpack, all enqueued on the calling thread's stream of the
 *                            context, no host synchronisation.  world == 1 with a null communicator is a no-op.
 * pack / unpack are exposed so that a host with another transport (torch.distributed in the tests) can move the slot itself. */
typedef struct les_hip_exchange les_hip_exchange;
int les_hip_exchange_create(les_hip_ctx* ctx, int rank, int world, int n_rects, const les_hip_rect* rects, const int* first, les_hip_exchange** out);
void les_hip_exchange_destroy(les_hip_exchange* x);
long long les_hip_exchange_slot_floats(const les_hip_exchange* x);
int les_hip_exchange_pack(les_hip_ctx* ctx, const les_hip_exchange* x, const les_hip_plane* d_labels, const float* d_cost, float* d_slot);
int les_hip_exchange_unpack(les_hip_ctx* ctx, const les_hip_exchange* x, const float* d_gathered, les_hip_plane* d_labels, float* d_cost);
int les_hip_exchange_tiles(les_hip_ctx* ctx, les_hip_exchange* x, void* nccl_comm, les_hip_plane* d_labels, float* d_cost);

/* diagnostics: dword-per-lane streaming copy of n floats (device pointers), the known-byte-count pattern used to
 * calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters for this library's access width (profiles/). */
int les_hip_calib_copy(const float* d_src, float* d_dst, size_t n, int device, void* stream);
/* the same with 16 bytes per lane (n a multiple of 4, 16-byte aligned pointers): the streaming-copy ceiling that bench.py measures
 * in its own run and reports as roofline.peak_achievable. */
int les_hip_calib_copy_wide(const float* d_src, float* d_dst, size_t n, int device, void* stream);

/* Device memory helpers for callers without a HIP toolchain (host C++ adapter, ctypes). */
int les_hip_malloc(les_hip_ctx* ctx, void** dev_ptr, size_t bytes);
int les_hip_free(les_hip_ctx* ctx, void* dev_ptr);
int les_hip_memcpy_h2d(les_hip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int les_hip_memcpy_d2h(les_hip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int les_hip_memset(les_hip_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* Test/diagnostic: guide statistics of view `mode` as the kernels consume them:
 * out[(y*W+x)*12 + k*4 + {0,1,2,3}] = {mean_I_k - 1/2, inv[k][0], inv[k][1], inv[k][2]} (float32). */
int les_hip_get_stats(les_hip_ctx* ctx, int mode, float* out_host);
/* Strip geometry the build was compiled with for radius R (0 if unsupported): output columns per
 * workgroup. */
int les_hip_strip_width(int R);
/* Bytes of the TILED copy of view `mode`'s cost volume ([H][ceil(W/8)][D][8] floats: 8 columns x all slices contiguous), which the
 * march kernel's gather reads for planes that are steep along x (their two taps per pixel then lie within a few contiguous 32-byte
 * pieces instead of one 128-byte line per slice of [D][H][W]).  0 when the context holds none: LES_HIP_TILED=0, the image-based energy,
 * a view on the strip kernel, a copy of 2^30 floats or more, or an allocation that failed -- every plane then gathers from [D][H][W]
 * (identical costs).  A second resident copy of the volume is the price: this many bytes per view.
 * (no reference counterpart; LES/CostVolumeEnergy.h:73-96 reads its cv::Mat volume in place) */
size_t les_hip_tiled_volume_bytes(les_hip_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif
