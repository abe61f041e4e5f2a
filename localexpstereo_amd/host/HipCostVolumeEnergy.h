// HipCostVolumeEnergy.h -- drop-in replacement of class CostVolumeEnergy (LES/CostVolumeEnergy.h:6-184)
// whose ComputeUnaryPotential runs on an MI355X through the C ABI of include/localexp_hip.h.
//
// Same constructor shape (imL, imR, volL, volR, Parameters, MAX_DISPARITY, MIN_DISPARITY), same operator
// semantics, same threading contract: the operator is const and may be called concurrently from OpenMP
// threads, one cell per thread, each writing a disjoint rect of one shared map (LES/FastGCStereo.h:30-49).
// Error behaviour: like the reference the operator returns void and never throws; a device failure is
// reported on stderr and leaves COST_FOR_INVALID in the target rect (the reference's only failure
// signal is that sentinel, LES/CostVolumeEnergy.h:87-90).  The constructor throws std::runtime_error when
// no HIP device / library is available -- there is no CPU fallback.
#pragma once

#include <algorithm>
#include <cstdio>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "DeviceArray.h"
#include "StereoEnergy.h"
#include "localexp_hip.h"

namespace les_host {

class HipCostVolumeEnergy : public StereoEnergy {
public:
    // Parameters::filterName -> the aggregation of les_hip_create_filtered (LES/StereoEnergy.h:25): "GF" the guided filter, "BF" and
    // "BL" the joint bilateral filter (NaiveStereoEnergy calls it "BF", CostVolumeEnergy "BL" -- and dereferences a null filter given
    // "BF"; both names mean it for both energies here), "" no aggregation.  "GFfloat" is not implemented.
    static int filter_kind(const std::string& name)
    {
        if (name == "GF") return LES_HIP_FILTER_GF;
        if (name == "BF" || name == "BL") return LES_HIP_FILTER_BILATERAL;
        if (name.empty()) return LES_HIP_FILTER_NONE;
        throw std::runtime_error("HipCostVolumeEnergy: unsupported filterName \"" + name + "\" (GF, BF / BL or \"\")");
    }

    // imL/imR: H x W x 3 uint8 BGR (cv::imread layout); volL/volR: float [D][H][W] (shared with the caller in
    // the reference, copied to HBM once here).
    HipCostVolumeEnergy(const uint8_t* imL, const uint8_t* imR, int width, int height, const float* volL, const float* volR,
                        int ndisp, Parameters p, float MAX_DISPARITY, float MIN_DISPARITY = 0, int device = 0)
        : StereoEnergy(width, height, std::move(p), MAX_DISPARITY, MIN_DISPARITY), ctx_(nullptr)
    {
        const int filter = filter_kind(params.filterName);
        les_hip_params hp;
        hp.H = height; hp.W = width; hp.D = ndisp;
        hp.windR = params.windR; hp.eps = params.filter_param1; hp.th_col = params.th_col;
        hp.max_disparity = MAX_DISPARITY; hp.min_disparity = MIN_DISPARITY;
        hp.device = device; hp.volumes_on_device = 0;
        if (les_hip_create_filtered(&ctx_, &hp, filter, imL, imR, volL, volR) != LES_HIP_OK)
            throw std::runtime_error(std::string("les_hip_create_filtered: ") + les_hip_last_error());
        setImages(imL, imR);           // pairwise weights for the host graph cut
    }
    ~HipCostVolumeEnergy() override { les_hip_destroy(ctx_); }

protected:
    // image-based matching cost (HipNaiveStereoEnergy below)
    struct NaiveTag {};
    HipCostVolumeEnergy(NaiveTag, const uint8_t* imL, const uint8_t* imR, int width, int height, Parameters p, float MAX_DISPARITY,
                        float MIN_DISPARITY, float MAX_VDISPARITY, int device)
        : StereoEnergy(width, height, std::move(p), MAX_DISPARITY, MIN_DISPARITY, MAX_VDISPARITY), ctx_(nullptr), naive_(true)
    {
        const int filter = filter_kind(params.filterName);
        les_hip_params hp;
        hp.H = height; hp.W = width; hp.D = 1;
        hp.windR = params.windR; hp.eps = params.filter_param1; hp.th_col = params.th_col;
        hp.max_disparity = MAX_DISPARITY; hp.min_disparity = MIN_DISPARITY;
        hp.device = device; hp.volumes_on_device = 0;
        if (les_hip_create_naive_filtered(&ctx_, &hp, filter, imL, imR, params.alpha, params.th_grad) != LES_HIP_OK)
            throw std::runtime_error(std::string("les_hip_create_naive_filtered: ") + les_hip_last_error());
        if (les_hip_set_max_vdisparity(ctx_, MAX_VDISPARITY) != LES_HIP_OK) {
            const std::string e = les_hip_last_error();
            les_hip_destroy(ctx_);
            throw std::invalid_argument("les_hip_set_max_vdisparity: " + e);
        }
        setImages(imL, imR);
    }

    // the half-resolution twin of `src` (half() below): adopts the context les_hip_create_half built
    struct HalfTag {};
    HipCostVolumeEnergy(HalfTag, const HipCostVolumeEnergy& src, les_hip_ctx* ctx, Parameters p)
        : StereoEnergy((src.width + 1) / 2, (src.height + 1) / 2, std::move(p), 0.5f * src.MAX_DISPARITY, 0.5f * src.MIN_DISPARITY, 0.5f * src.MAX_VDISPARITY), ctx_(ctx), naive_(src.naive_)
    {
        std::vector<uint8_t> im[2];
        for (int m = 0; m < 2; m++) {
            im[m].resize((size_t)width * height * 3);
            if (les_hip_get_image(ctx_, m, im[m].data()) != LES_HIP_OK) im[m].clear();      // (a view the source was built without)
        }
        setImages(im[0].empty() ? nullptr : im[0].data(), im[1].empty() ? nullptr : im[1].data());
    }

public:
    HipCostVolumeEnergy(const HipCostVolumeEnergy&) = delete;
    HipCostVolumeEnergy& operator=(const HipCostVolumeEnergy&) = delete;

    void ComputeUnaryPotentialWithoutCheck(const Rect& filterRect, const Rect& targetRect, float* costs, int row_stride,
                                           const Plane& plane, Reusable& reusable, int mode = 0) const override
    {
        call(filterRect, targetRect, costs, row_stride, plane, reusable, mode, 0);
    }
    void ComputeUnaryPotential(const Rect& filterRect, const Rect& targetRect, float* costs, int row_stride, const Plane& plane,
                               Reusable& reusable, int mode = 0) const override
    {
        call(filterRect, targetRect, costs, row_stride, plane, reusable, mode, 1);
    }

    // Batched form (one proposal index of one disjoint set): n calls into one H x W host map.
    void ComputeUnaryPotentialBatch(const std::vector<Rect>& filterRects, const std::vector<Rect>& targetRects,
                                    const std::vector<Plane>& planes, float* cost_map, int mode = 0, bool check = true) const
    {
        static_assert(sizeof(Rect) == sizeof(les_hip_rect) && sizeof(Plane) == sizeof(les_hip_plane), "ABI layout");
        std::lock_guard<std::mutex> lk(mu_);               // the batched form uses the context's own stream and scratch map
        if (les_hip_unary_batch(ctx_, mode, (int)filterRects.size(), reinterpret_cast<const les_hip_rect*>(filterRects.data()),
                                reinterpret_cast<const les_hip_rect*>(targetRects.data()),
                                reinterpret_cast<const les_hip_plane*>(planes.data()), cost_map, check ? 1 : 0) != LES_HIP_OK)
            fprintf(stderr, "HipCostVolumeEnergy: %s\n", les_hip_last_error());
    }

    // The unary cost of every pixel's own label (the warm-start branch of FastGCStereo::initCurrentFast, LES/FastGCStereo.h:116-130): for
    // every pixel p of `region` (the whole image by default), cost_map(p) = ComputeUnaryPotential((p +- windR) & image, (p, 1 x 1), labels(p)),
    // in one dense device pass (les_hip_unary_labels).  labels, cost_map: width * height elements in HOST memory; pixels outside the region
    // keep what cost_map held.  Returns false (and reports on stderr) when the library refuses the call.
    bool ComputeUnaryPotentialOfLabels(const Plane* labels, float* cost_map, int mode = 0, bool check = true, const Rect* region = nullptr) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<float> d_cost(ctx_, st, cost_map, P);
        les_hip_rect r{0, 0, width, height};
        if (region) r = les_hip_rect{region->x, region->y, region->width, region->height};
        if (st.ok()) st(les_hip_unary_labels(ctx_, mode, &r, abi(d_lab), d_cost.get(), check ? 1 : 0));
        return d_cost.download(cost_map, P);
    }

    // Cross-view fusion's warp (les_hip_warp_labels, csrc/les_crossview.h; no reference counterpart): the label map `src` of view src_mode (0 left,
    // 1 right) expressed in the other view's coordinates into `out`; target pixels no source pixel lands on keep `fallback`'s plane.  hit (may be
    // null): 1 where a source pixel landed.  All maps: width * height elements in HOST memory; out may be fallback.  Returns false (and reports
    // on stderr) when the library refuses the call (rows wider than 8192 pixels).
    bool warpLabels(int src_mode, const Plane* src, const Plane* fallback, Plane* out, unsigned char* hit = nullptr) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_src(ctx_, st, src, P), d_out(ctx_, st, fallback, P);
        DeviceArray<unsigned char> d_hit(ctx_, st, hit ? P : 0);
        if (st.ok() && st(les_hip_warp_labels(ctx_, src_mode, abi(d_src), abi(d_out), abi(d_out), d_hit.get()))) st(les_hip_synchronize(ctx_));
        return d_out.download(out, P) && d_hit.download(hit, P);
    }

    // Winner-take-all labels of the aggregated cost volume (les_hip_wta_labels, csrc/les_wtavol.h; no reference counterpart): per pixel of view
    // `mode` the fronto-parallel plane (0, 0, d, 0) of least aggregated cost among the disparities min ... max of the energy, refined to sub-pixel
    // by the parabola through its neighbours' costs when `subpixel`; cost (may be null): that least cost.  A start for run() (its `labeling`
    // argument) or a second labelling for a fusion move.  labels, cost: width * height elements in HOST memory; chunk: planes per launch (0: the
    // library's choice).  Returns false (and reports on stderr) when the library refuses the call (a view without data).
    bool wtaLabels(Plane* labels, float* cost = nullptr, int mode = 0, bool subpixel = true, int chunk = 0) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, P);
        DeviceArray<float> d_cost(ctx_, st, P);
        if (st.ok() && st(les_hip_wta_labels(ctx_, mode, chunk, subpixel ? 1 : 0, abi(d_lab), d_cost.get()))) st(les_hip_synchronize(ctx_));
        return d_lab.download(labels, P) && d_cost.download(cost, P);
    }

    // The largest value a raw matching cost of this energy can take: th_col for the volume energy (its costs are truncated there),
    // (1 - alpha) th_col + alpha th_grad for the image-based one.  The default scale of confidence().
    float rawCostMax() const { return naive_ ? (1.0f - params.alpha) * params.th_col + params.alpha * params.th_grad : params.th_col; }

    // The confidence of a label map under view `mode`'s aggregated cost volume (les_hip_confidence, csrc/les_confidence.h; no reference
    // counterpart): conf in [0, 1] per pixel -- how much cheaper the aggregated cost is within `band` slabs of the pixel's own disparity than
    // anywhere else on its cost curve, (rival - own) / scale clamped; 0 for a label outside the disparity range or not finite, 1 where the band
    // covers every finite cost.  own / rival / krival (may be null): the in-band and the rival minimum (+inf where none) and the rival's slab
    // (-1 where none).  scale <= 0: rawCostMax(); chunk: planes per launch (0: the library's choice).  All maps: width * height elements in HOST
    // memory.  Returns false (and reports on stderr) when the library refuses the call.
    bool confidence(const Plane* labels, float* conf, float* own = nullptr, float* rival = nullptr, int* krival = nullptr, int mode = 0, float band = 1.f,
                    float scale = 0.f, int chunk = 0) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<float> d_conf(ctx_, st, P), d_own(ctx_, st, own ? P : 0), d_rival(ctx_, st, rival ? P : 0);
        DeviceArray<int> d_kr(ctx_, st, krival ? P : 0);
        if (st.ok() && st(les_hip_confidence(ctx_, mode, abi(d_lab), chunk, band, scale > 0.f ? scale : rawCostMax(), d_conf.get(), d_own.get(), d_rival.get(), d_kr.get()))) st(les_hip_synchronize(ctx_));
        return d_conf.download(conf, P) && d_own.download(own, P) && d_rival.download(rival, P) && d_kr.download(krival, P);
    }

    // Slanted planes fitted to a disparity map (les_hip_fit_planes, csrc/les_planefit.h; no reference counterpart): per pixel of view `mode` an
    // edge-aware weighted least-squares plane through the disparities of its (2 radius + 1)^2 window, guided by that view's image.  Exactly one of
    // labels (planes whose own disparities are fitted; the result keeps their v) and disp (a disparity map) is given, the other one null; fallback
    // (may be null: (0, 0, MIN_DISPARITY, 0)) supplies the pixels that get neither a fit nor their own disparity; kind (may be null): 2 slanted fit,
    // 1 fronto-parallel at the pixel's own disparity, 0 fallback.  All maps: width * height elements in HOST memory; out may be fallback.  A start
    // for run() or a second labelling for a fusion move.  Returns false (and reports on stderr) when the library refuses the call.
    bool fitPlanes(const Plane* labels, const float* disp, const Plane* fallback, Plane* out, unsigned char* kind = nullptr, int mode = 0, int radius = 5,
                   float sig = 10.f, float gate0 = 1.f, float gate_slope = 0.5f, float max_slope = 2.f, int min_support = 6) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P), d_fb(ctx_, st, fallback, P), d_out(ctx_, st, P);
        DeviceArray<float> d_disp(ctx_, st, disp, P);
        DeviceArray<unsigned char> d_kind(ctx_, st, kind ? P : 0);
        if (st.ok() && st(les_hip_fit_planes(ctx_, mode, abi(d_lab), d_disp.get(), abi(d_fb), abi(d_out), d_kind.get(), radius, sig, gate0, gate_slope, max_slope, min_support))) st(les_hip_synchronize(ctx_));
        return d_out.download(out, P) && d_kind.download(kind, P);
    }

    // The half-resolution twin of this energy (les_hip_create_half, csrc/les_pyramid.h; no reference counterpart): a new, independent energy of the
    // same kind, filter and interpolation over this one's images and volumes pooled by two on the device -- width, height and slices (n + 1) / 2,
    // the disparity ranges halved, windR -> max(1, (windR + 1) / 2).  Its Parameters are this one's with that windR and, because disparity
    // differences halve, lambda x 2 and th_smooth / 2 (a reasoned default, not tuned).  A solution found on it is a start for this one through
    // upsampleLabels.  Throws std::runtime_error when the library refuses (a MIN_DISPARITY that is not an even integer).
    std::unique_ptr<HipCostVolumeEnergy> half() const
    {
        les_hip_ctx* h = nullptr;
        if (les_hip_create_half(&h, ctx_) != LES_HIP_OK) throw std::runtime_error(std::string("les_hip_create_half: ") + les_hip_last_error());
        Parameters p = params;
        p.windR = std::max(1, (params.windR + 1) / 2);
        p.lambda = params.lambda * 2;
        p.th_smooth = params.th_smooth / 2;
        try {
            return std::unique_ptr<HipCostVolumeEnergy>(new HipCostVolumeEnergy(HalfTag{}, *this, h, std::move(p)));
        } catch (...) {
            les_hip_destroy(h);
            throw;
        }
    }

    // The way up (les_hip_upsample_labels): `src`, the label map of view `mode` found on `half` (this energy's half()), re-expressed at this
    // energy's resolution, edge-aware, into `out`; kind (may be null): 0 the upsampled plane was kept, 1 it was not a valid label here and the
    // pixel got the fronto-parallel plane at its clamped disparity, 2 its disparity was not finite.  src: half.width * half.height planes, out and
    // kind: width * height elements, all in HOST memory.  Returns false (and reports on stderr) when the library refuses the call.
    bool upsampleLabels(const HipCostVolumeEnergy& half, const Plane* src, Plane* out, unsigned char* kind = nullptr, int mode = 0) const
    {
        const size_t P = (size_t)width * height, Ph = (size_t)half.width * half.height;
        Status st(kWho);
        DeviceArray<Plane> d_src(ctx_, st, src, Ph), d_out(ctx_, st, P);
        DeviceArray<unsigned char> d_kind(ctx_, st, kind ? P : 0);
        if (st.ok() && st(les_hip_upsample_labels(ctx_, half.ctx_, mode, abi(d_src), abi(d_out), d_kind.get()))) st(les_hip_synchronize(ctx_));
        return d_out.download(out, P) && d_kind.download(kind, P);
    }

    // The speckle mask of a label map (les_hip_speckle_mask, csrc/les_speckle.h; no reference counterpart, OpenCV's filterSpeckles convention):
    // mask 255 where the pixel's connected component of the disparity map -- 4-neighbours whose finite disparities differ by at most max_diff --
    // has at most max_size pixels, else 0; root / size (may be null): per pixel the smallest linear index of its component and the component's
    // pixel count.  All maps: width * height elements in HOST memory.  Returns false (and reports on stderr) when the library refuses the call.
    bool speckleMask(const Plane* labels, int max_size, float max_diff, unsigned char* mask, int* root = nullptr, int* size = nullptr) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<unsigned char> d_mask(ctx_, st, P);
        DeviceArray<int> d_root(ctx_, st, root ? P : 0), d_size(ctx_, st, size ? P : 0);
        if (st.ok()) st(les_hip_speckle_mask(ctx_, abi(d_lab), max_size, max_diff, d_mask.get(), d_root.get(), d_size.get()));      // (waits itself)
        return d_mask.download(mask, P) && d_root.download(root, P) && d_size.download(size, P);
    }

    // 3D geometry of a label map of view `mode` (les_hip_reproject, csrc/les_reproject.h; the reference only paints computeNormalMap): per pixel
    // the point of its disparity and the exact unit normal of its label's plane in the view's own camera frame (X right, Y down, Z forward;
    // the normal faces the camera), width * height * 3 floats each (either may be null), NaN where invalid; valid: width * height bytes, 255 / 0.
    // drop (may be null): width * height bytes, nonzero = invalid; z_max <= 0: no depth limit.  All maps in HOST memory.  Returns false (and
    // reports on stderr) when the library refuses the call.
    bool reproject(const Plane* labels, const les_hip_calib& calib, float* points, float* normals, unsigned char* valid, int mode = 0,
                   const unsigned char* drop = nullptr, float z_max = 0.f) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<unsigned char> d_drop(ctx_, st, drop, P), d_valid(ctx_, st, P);
        DeviceArray<float> d_points(ctx_, st, points ? 3 * P : 0), d_normals(ctx_, st, normals ? 3 * P : 0);
        if (st.ok() && st(les_hip_reproject(ctx_, mode, abi(d_lab), d_drop.get(), &calib, z_max, d_points.get(), d_normals.get(), d_valid.get()))) st(les_hip_synchronize(ctx_));
        return d_valid.download(valid, P) && d_points.download(points, 3 * P) && d_normals.download(normals, 3 * P);
    }

    // The triangle mesh over the pixel grid (les_hip_mesh): vertex k is the k-th valid pixel in row-major order; neighbours are joined iff both are
    // valid and the un-truncated pairwise term of their labels is <= max_jump (the energy's th_smooth is the natural choice); quad (x, y) yields
    // (p00, p01, p10) and (p10, p01, p11), each iff its three edges are joined, in row-major quad order.  vertex_index: width * height ints (-1
    // where invalid); vertex_pixel: the linear pixel index per vertex; triangles: 3 vertex numbers each.  HOST memory; the vectors are resized
    // to the counts.  Returns false (and reports on stderr) when the library refuses the call.
    bool mesh(const Plane* labels, const unsigned char* valid, float max_jump, std::vector<int>& vertex_index, std::vector<int>& vertex_pixel,
              std::vector<int>& triangles, int mode = 0) const
    {
        const size_t P = (size_t)width * height, T = std::max<size_t>(1, 2 * (size_t)(width - 1) * (size_t)(height - 1));
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<unsigned char> d_valid(ctx_, st, valid, P);
        DeviceArray<int> d_vi(ctx_, st, P), d_vp(ctx_, st, P), d_tri(ctx_, st, 3 * T);
        DeviceArray<long long> d_counts(ctx_, st, 2);
        long long counts[2] = {0, 0};
        if (st.ok() && st(les_hip_mesh(ctx_, mode, abi(d_lab), d_valid.get(), max_jump, d_vi.get(), d_vp.get(), d_tri.get(), d_counts.get()))) st(les_hip_synchronize(ctx_));
        if (!d_counts.download(counts, 2)) return false;
        vertex_index.resize(P);
        vertex_pixel.resize((size_t)counts[0]);
        triangles.resize(3 * (size_t)counts[1]);
        return d_vi.download(vertex_index.data(), P) && d_vp.download(vertex_pixel.data(), vertex_pixel.size()) && d_tri.download(triangles.data(), triangles.size());
    }

    // The view of a camera at fraction t in [0, 1] of the baseline, counted from view src_mode towards the other view, rendered from that view's
    // label map and image (les_hip_render_view, csrc/les_view.h; no reference counterpart).  image (may be null: the energy's own image of
    // src_mode): width * height * 3 bytes b, g, r.  bgr: width * height * 3 bytes; disp: width * height floats, the disparity of what is seen
    // (NaN in holes); hit: width * height bytes, 1 a source pixel landed, 2 a one-column crack closed, 0 a hole.  All maps in HOST memory.
    // Returns false (and reports on stderr) when the library refuses the call (t outside [0, 1], rows wider than 8192 pixels).
    bool renderView(int src_mode, const Plane* labels, const unsigned char* image, float t, unsigned char* bgr, float* disp, unsigned char* hit) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<unsigned char> d_img(ctx_, st, image, 3 * P), d_bgr(ctx_, st, 3 * P), d_hit(ctx_, st, P);
        DeviceArray<float> d_disp(ctx_, st, P);
        if (st.ok() && st(les_hip_render_view(ctx_, src_mode, abi(d_lab), d_img.get(), t, d_bgr.get(), d_disp.get(), d_hit.get()))) st(les_hip_synchronize(ctx_));
        return d_bgr.download(bgr, 3 * P) && d_disp.download(disp, P) && d_hit.download(hit, P);
    }

    // Two renders of the camera at fraction t of the baseline (from the left view) as one image (les_hip_blend_views): (bgrL, dispL, hitL) is view
    // 0 rendered at t, (bgrR, dispR, hitR) view 1 rendered at 1 - t; either triple may be null as a whole.  Colours are mixed (1 - t) : t where both
    // see the pixel and their disparities agree within tol, the nearer one is taken where they do not; with fill a hole takes the farther of its
    // nearest neighbours on the row.  src: 0 hole, 1 left, 2 right, 3 both, 4 filled.  All maps in HOST memory.  Returns false (and reports on
    // stderr) when the library refuses the call.
    bool blendViews(float t, float tol, bool fill, const unsigned char* bgrL, const float* dispL, const unsigned char* hitL, const unsigned char* bgrR,
                    const float* dispR, const unsigned char* hitR, unsigned char* bgr, float* disp, unsigned char* src) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<unsigned char> d_bl(ctx_, st, bgrL, 3 * P), d_hl(ctx_, st, hitL, P), d_br(ctx_, st, bgrR, 3 * P), d_hr(ctx_, st, hitR, P);
        DeviceArray<float> d_dl(ctx_, st, dispL, P), d_dr(ctx_, st, dispR, P), d_disp(ctx_, st, P);
        DeviceArray<unsigned char> d_bgr(ctx_, st, 3 * P), d_src(ctx_, st, P);
        if (st.ok() && st(les_hip_blend_views(ctx_, t, tol, fill ? 1 : 0, d_bl.get(), d_dl.get(), d_hl.get(), d_br.get(), d_dr.get(), d_hr.get(), d_bgr.get(),
                                              d_disp.get(), d_src.get())))
            st(les_hip_synchronize(ctx_));
        return d_bgr.download(bgr, 3 * P) && d_disp.download(disp, P) && d_src.download(src, P);
    }

    // The photometric consistency of a label map of view `mode` with the energy's two images, no ground truth needed (les_hip_photo_error): vis 1
    // where the pixel is seen in the other view, 2 where the label map itself says it is occluded, 0 where it leaves the image; err: the mean
    // absolute difference over b, g, r between the other image sampled where the label says the pixel is and the pixel's own colour, NaN where
    // vis != 1.  width * height elements each in HOST memory.  Returns false (and reports on stderr) when the library refuses the call.
    bool photoError(const Plane* labels, float* err, unsigned char* vis, int mode = 0) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_lab(ctx_, st, labels, P);
        DeviceArray<float> d_err(ctx_, st, P);
        DeviceArray<unsigned char> d_vis(ctx_, st, P);
        if (st.ok() && st(les_hip_photo_error(ctx_, mode, abi(d_lab), d_err.get(), d_vis.get()))) st(les_hip_synchronize(ctx_));
        return d_err.download(err, P) && d_vis.download(vis, P);
    }

    // PMStereoBase::postProcess with the failure mask widened by the speckle mask (les_hip_post_process_speckle), in place on HOST label maps of
    // width * height planes.  One of labelsL / labelsR may be null: the one-view form, whose mask is the speckle mask alone (threshold is ignored).
    // max_size 0: with both views PMStereoBase::postProcess itself, with one view nothing changes.  Returns false (and reports on stderr) when the
    // library refuses the call.
    bool postProcessSpeckle(Plane* labelsL, Plane* labelsR, float threshold, float omega, int max_size, float max_diff) const
    {
        const size_t P = (size_t)width * height;
        Status st(kWho);
        DeviceArray<Plane> d_l(ctx_, st, labelsL, P), d_r(ctx_, st, labelsR, P);
        if (st.ok()) st(les_hip_post_process_speckle(ctx_, abi(d_l), abi(d_r), threshold, omega, max_size, max_diff));      // (waits itself)
        return d_l.download(labelsL, P) && d_r.download(labelsR, P);
    }

    // CostVolumeEnergy::setInterpolationMethod (LES/CostVolumeEnergy.h:45-48): 0 nearest slice, 1 linear (the default), 2 quadratic.  Like the
    // reference's setter it is not synchronised with evaluations running on other threads.
    virtual void setInterpolationMethod(int none_lin_quad)
    {
        if (les_hip_set_interpolation(ctx_, none_lin_quad) != LES_HIP_OK)
            throw std::invalid_argument(std::string("setInterpolationMethod: ") + les_hip_last_error());
    }

    les_hip_ctx* handle() const { return ctx_; }

private:
    void call(const Rect& fr, const Rect& tr, float* costs, int row_stride, const Plane& plane, Reusable&, int mode, int check) const
    {
        const les_hip_rect f{fr.x, fr.y, fr.width, fr.height}, t{tr.x, tr.y, tr.width, tr.height};
        const les_hip_plane p{plane.a, plane.b, plane.c, plane.v};
        // re-entrant: the library keeps one scratch (stream, device tile, pinned staging, job tables of the recent rect pairs) per
        // calling thread, so the OpenMP threads of the reference loop (LES/FastGCStereo.h:30-49) run their cells concurrently
        const int rc = les_hip_unary_one(ctx_, mode, &f, &t, &p, costs, row_stride, check);
        if (rc != LES_HIP_OK) {
            fprintf(stderr, "HipCostVolumeEnergy: %s\n", les_hip_last_error());
            for (int y = 0; y < tr.height; y++)
                for (int x = 0; x < tr.width; x++)
                    costs[(size_t)(tr.y - fr.y + y) * row_stride + (tr.x - fr.x + x)] = (float)COST_FOR_INVALID;
        }
    }

    // the staged wrappers above: what their Status reports as, and a staged label map as the ABI's type
    static constexpr const char* kWho = "HipCostVolumeEnergy";
    static les_hip_plane* abi(const DeviceArray<Plane>& a)
    {
        static_assert(sizeof(Plane) == sizeof(les_hip_plane), "ABI layout");
        return reinterpret_cast<les_hip_plane*>(a.get());
    }

    les_hip_ctx* ctx_;
    bool naive_ = false;                 // the image-based energy (HipNaiveStereoEnergy): what rawCostMax() tells apart
    mutable std::mutex mu_;
};

// Drop-in for NaiveStereoEnergy (LES/StereoEnergy.h:629-764), the energy of the MiddV2 configuration
// (LES/PMStereoBase.h:37, parameters LES/main.cpp:86-121): same operator, raw cost from the two images.
class HipNaiveStereoEnergy : public HipCostVolumeEnergy {
public:
    // MAX_VDISPARITY: the range of Plane::v of the initial labels (NaiveStereoEnergy's MAX_VDISPARITY, LES/StereoEnergy.h:120-129); the
    // cost samples row y + v for every plane (csrc/les_vdisp.h)
    HipNaiveStereoEnergy(const uint8_t* imL, const uint8_t* imR, int width, int height, Parameters p, float MAX_DISPARITY,
                         float MIN_DISPARITY = 0, int device = 0, float MAX_VDISPARITY = 0)
        : HipCostVolumeEnergy(NaiveTag{}, imL, imR, width, height, std::move(p), MAX_DISPARITY, MIN_DISPARITY, MAX_VDISPARITY, device) {}

    // NaiveStereoEnergy has no volume and no interpolation setting
    void setInterpolationMethod(int) override
    {
        throw std::invalid_argument("setInterpolationMethod: the image-based energy has no cost volume");
    }
};

}  // namespace les_host
