"""Python driver of the whole local expansion loop around the GPU path (mirror of FastGCStereo / PMStereoBase,
LES/FastGCStereo.h:88-227, LES/PMStereoBase.h) and of the two data-set front ends MidV2 / MidV3 (LES/main.cpp:270-420).

What runs where: proposals, unary costs, winner-take-all updates, graph construction, the graph cuts of the main iterations and of the
fusion moves, post-processing -> MI355X through the C ABI (liblocalexp_hip.so); the host cores (liblocalexp_host.so) cut only what device_cuts
leaves to them ("fine" / "none", the simulator build) or the device solvers hand over, and serve check_flow_energy=True; file formats and the
Evaluator -> numpy (io.py), or the device evaluator (evaluate_on_device).  One process per GPU: pass rank/world to shard the cells of every
disjoint set.
"""
import contextlib
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import api, gc, io, pm

PARAMS_GF = dict(lambda_=1.0, windR=20, eps=1e-4, alpha=0.9, omega=10.0, th_grad=2.0, th_col=10.0, th_smooth=1.0, epsilon=0.01, filter="GF")   # paramsGF, LES/main.cpp:73
# paramsBF, LES/main.cpp:72 -- Parameters(20, 20, "BF", 10), the default of Parameters: joint bilateral filter of radius windR, sig2 = eps
# (filter_param1); lambda 20 is scaled to its un-normalised window sums
PARAMS_BF = dict(PARAMS_GF, lambda_=20.0, windR=20, eps=10.0, filter="BF")


class FastGCStereo:
    def __init__(self, energy, imL, imR, params, device="cuda", rank=0, world=1, seed=1, host_threads=0, device_cuts=None, random_vdisp=None,
                 evaluate_on_device=False, inner_loop_log=False, check_flow_energy=False, recost_after_post=False, cross_view=0, coarse_params=None,
                 speckle=None, confidence=False, min_confidence=None, confidence_band=1.0, max_photo_error=None, valid=None):
        self.e, self.imL, self.imR, self.p = energy, imL, imR, dict(PARAMS_GF, **params)
        # Opt-in, no reference counterpart: valid={view: H x W mask, nonzero = valid} (a rectification's validL / validR, the caller's own masks)
        # adds each view's own invalid pixels to its failure mask of the post-processing, so that they are filled like a failed left-right
        # check.  It composes with speckle, min_confidence and max_photo_error, and like them gives a one-view call a post-processing (with that
        # mask alone); raw_labelings stay raw.  The volumes are another matter (io.build_volumes(valid=), csrc/les_maskvol.h).  Single rank.
        # None (the default) changes nothing.
        self.valid = None
        if valid is not None:
            H, W = (int(n) for n in np.asarray(imL).shape[:2])
            self.valid = {}
            for m, v in dict(valid).items():
                v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
                if int(m) not in (0, 1) or v.shape != (H, W):
                    raise ValueError(f"valid: {{view 0 / 1: an {H} x {W} mask}} expected, got view {m!r} with shape {v.shape}")
                self.valid[int(m)] = np.ascontiguousarray(v != 0)
        # Opt-in, no reference counterpart (csrc/les_confidence.h): confidence=True -- run(), wta() and sgm() set self.confidences = {view: H x W
        # float32 in [0, 1]}, the confidence of each view's RAW labelling (before the post-processing) under that view's aggregated cost volume
        # (les_hip_confidence: how much cheaper the cost is within confidence_band slabs of the pixel's own disparity than anywhere else on its cost
        # curve), taken on the device; the returned labellings are unchanged.  min_confidence=t, 0 < t <= 1, implies it and adds conf < t to each
        # view's failure mask of the post-processing (les_hip_post_process_masked), and a one-view call is then post-processed with that mask (and
        # the speckle mask, when set) alone.  Single rank.  The defaults change nothing.
        self.min_confidence = None if min_confidence is None else float(min_confidence)
        if self.min_confidence is not None and not 0.0 < self.min_confidence <= 1.0:
            raise ValueError(f"min_confidence {min_confidence}: None or a threshold in (0, 1]")
        self.confidence_band = float(confidence_band)
        if not self.confidence_band >= 0.0:
            raise ValueError(f"confidence_band {confidence_band}: a half-width in slabs, >= 0")
        self.with_confidence = bool(confidence) or self.min_confidence is not None
        # Opt-in, no reference counterpart (csrc/les_view.h): max_photo_error=tau >= 0 adds to each view's failure mask of the post-processing every
        # pixel of that view's RAW labelling that is seen in the other view (les_hip_photo_error: vis == 1) with a photometric error above tau grey
        # levels -- a wrong match the cost curve may be sure of.  It composes with speckle and min_confidence, and like them gives a one-view call a
        # post-processing (with that mask alone).  Single rank.  None (the default) changes nothing.
        self.max_photo_error = None if max_photo_error is None else float(max_photo_error)
        if self.max_photo_error is not None and not self.max_photo_error >= 0.0:
            raise ValueError(f"max_photo_error {max_photo_error}: None or a threshold in grey levels, >= 0")
        self.confidences = {}                     # run(), wta(), sgm() with confidence=True: view -> the H x W confidence map of its raw labelling
        # Opt-in, no reference counterpart: (max_size, max_diff) -- the post-processing step of run(), wta() and sgm() also treats as failed every
        # pixel whose connected component of the view's disparity map (4-neighbours within max_diff) has at most max_size pixels
        # (les_hip_post_process_speckle, csrc/les_speckle.h), and a one-view call, which has no left-right check, is post-processed with that mask
        # alone.  None (the default): nothing changes -- two views get the left-right check, one view returns its raw map.
        self.speckle = None if speckle is None else (int(speckle[0]), float(speckle[1]))
        if self.speckle is not None and (self.speckle[0] < 0 or not self.speckle[1] >= 0):
            raise ValueError(f"speckle {speckle}: None or (max_size >= 0, max_diff >= 0)")
        # Opt-in, no reference counterpart (the reference's views meet only in the post-processing): n > 0 -- in a two-view run, after every n-th
        # graph-cut iteration and after the last one, each view fuses the other view's solution, warped into its own coordinates on the device
        # (les_hip_warp_labels, csrc/les_crossview.h), into its own by fusion moves (pm.PMRunner.fuse).  0 (the default): nothing changes.
        self.cross_view = int(cross_view)
        if self.cross_view < 0:
            raise ValueError(f"cross_view {cross_view}: 0 (off) or the number of graph-cut iterations between two cross-view steps")
        self.cross_stats = {}                     # cross_fuse(): view -> the runner's fuse report + hit_pixels, energy_before, energy_after
        self.cross_view_stats = []                # run(): one dict(iteration=, views={view: report + hit_pixels}) per cross-view step
        # Opt-in: after postProcess (two-view runs) every view's cost map is re-evaluated from its final labels (pm.PMRunner.recost: one dense
        # pass), so the last row's `data` belongs to the labels it is logged with.  Off (the default, the reference's behaviour,
        # LES/FastGCStereo.h:205-206): that row reports the data term of the labels before the left-right check, fill and weighted median.
        self.recost_after_post = bool(recost_after_post)
        # what every plane fit of this driver uses (fit_planes, run(labeling="wta+planes" / a disparity map), wta(slanted=True)): keywords of
        # api.HipCostVolumeEnergy.fit_planes (radius, sig, gate0, gate_slope, max_slope, min_support); {}: its defaults
        self.fit_params = {}
        # what the "sgm" / "sgm+planes" starts of run() use: keywords of api.HipCostVolumeEnergy.sgm_labels (paths, p1, p2, subpixel); {}: its defaults
        self.sgm_params = {}
        # what the "half" start of run() solves at half resolution first (_half_starts): graph-cut and PatchMatch iterations and the start of that
        # nested run (None, "wta", "sgm", "half": the next level down), over the same viewModes; an optional key coarse_params gives the next
        # level its own settings (without it a "half" below runs these defaults)
        self.coarse_params = dict(COARSE_DEFAULTS, **(coarse_params or {}))
        self.coarse_seconds, self.coarse_stats = 0.0, {}    # run(labeling="half"): wall-clock of the way down, the nested run and the way up; what the nested run reports
        self._coarse = False                      # set on the nested driver of a "half" start: no post-processing, the views' maps stay on the device (self._device_maps)
        self.slant_stats = {}                     # run(labeling="wta+planes") / wta(slanted=True): view -> the runner's fuse report + kind_pixels [fallback, fronto, slanted]
        self.raw_labelings = {}                   # run(): view -> its H x W x 4 labelling before the post-processing (what a later run resumes from)
        self.random_vdisp = random_vdisp          # maxVDisp of the RANDOM proposals (pm.PMRunner); None: the energy's setting (0 by default)
        # Parameters::filterName: the energy aggregates with the filter it was built with; a params dict that names another one is a mistake
        if "filter" in params and api.filter_kind(params["filter"]) != getattr(energy, "filter", api.FILTER_GF):
            raise ValueError(f"params name filter {params['filter']!r}, the energy was built with filter kind {energy.filter}")
        self.device, self.rank, self.world, self.seed = device, rank, world, seed
        self.units, self.table = [], []
        self.evaluator = None
        self._dev_eval, self._inner = None, {}      # set by run() / fuse(), open while they work: the device evaluators of the log rows / per view of the inner-loop log
        self.log = []
        # the reference's flow == energy self-check (LES/FastGCStereo.h:561-594).  True: the iteration moves to the host route (host maps, host graph
        # construction, host cuts: what the reference does).  "device": it stays on the device path -- device graphs, device cuts, the region energies of
        # les_hip_batch_region_energy before and after every lock-step (pm.PMRunner._checked_moves); gc_max_gap is the largest relative
        # |flow - energy|, gc_moves_raised the number of cells whose move raised the energy.  A diagnostic mode (it synchronises every lock-step).
        self.check_flow_energy = check_flow_energy
        self.gc_moves_raised = 0
        # Opt-in: every row of the log from les_hip_evaluate (csrc/les_eval.h) instead of the host route (copy the disparities down, copy labels
        # and costs into the host graph-cut context, sum there): no copy of a map, no host sum, and `smooth` is a number in every row
        # (the host route has no context before the graph-cut iterations and logs NaN there).
        self.evaluate_on_device = bool(evaluate_on_device)
        # Opt-in, the reference's doInnerLoopLog (LES/FastGCStereo.h:20,65): one row per view after every disjoint set of every layer, in
        # PatchMatch and graph-cut iterations, enqueued without a synchronisation and read once at the end of run() into self.inner_log
        # (iteration, layer, set, mode, data, smooth, energy, all, nonocc; no time: nothing synchronised).  Implies device evaluation.
        self.inner_loop_log = bool(inner_loop_log)
        self.inner_log = []
        # two-view runs: graph-cut iterations of the two views in parallel host threads.  Pays when the host cuts dominate
        # (1436 x 992: 14.2 -> 11.3 s); on small images the shared stream's synchronisations cost more (cones: 2.3 -> 3.1 s)
        # (never with several ranks: the per-set all-gathers of the two views would be issued from two threads in an order
        # that differs between ranks).  joint_views: the alternative -- both views advance in lock-step and ONE host team cuts
        # the cells of both (pm.PMRunner.gc_iteration_joint); measured 12.4 s at 1436 x 992 because the right view's cuts are the
        # slow ones (7-8 s of the 10 s of cuts) and then sit on the critical path of every lock-step, so it is not the default.
        self.concurrent_views = world == 1 and int(np.asarray(imL).shape[0]) * int(np.asarray(imL).shape[1]) >= 500_000
        self.joint_views = False
        self._swap_view_threads = False                 # tooling: start the right view's thread first
        if os.environ.get("LES_VIEWS"):                 # tooling: "joint" | "concurrent" | "serial" | "concurrent-swapped"
            v = os.environ["LES_VIEWS"]
            self.joint_views = v == "joint"
            self.concurrent_views = v.startswith("concurrent")
            self._swap_view_threads = v == "concurrent-swapped"
        self.host_threads = host_threads         # threads of the host max-flows (0: library default = at most 16)
        # which cells are CUT on the GPU: None / "all" = every layer when there is a GPU (cells that fit a workgroup's LDS by les_maxflow_kernel, larger
        # ones by the tiled solver, csrc/les_maxflow_tiled.h), "fine" = only the cells that fit the LDS (rounds 2-4), "none" / False = all cuts on the host
        self.device_cuts = device_cuts
        self._view_groups = None                 # two-view runs on several ranks: one process group per view, created once, destroyed by close()
        self.bytes_exchanged, self.all_gathers = 0, 0       # of the last run(): payload received by this rank in the per-set tile all-gathers, and their number

    def close(self):
        """Releases the per-view process groups of multi-rank two-view runs (the energy context belongs to the caller)."""
        if self._view_groups is not None:
            import torch.distributed as dist
            for gr in self._view_groups:
                try:
                    dist.destroy_process_group(gr)
                except Exception:
                    pass
            self._view_groups = None

    def addLayer(self, unit_region_size, proposers):
        """proposers: list of (kind, K) with kind in api.PROPOSE_EXPANSION / _RANDOM / _RANSAC (LES/FastGCStereo.h:88-92)."""
        self.units.append(int(unit_region_size))
        self.table.append(list(proposers))

    def setEvaluator(self, evaluator, precision=-1.0):
        self.evaluator, self.precision = evaluator, precision

    def _pairwise(self):
        return dict(lambda_=float(self.p["lambda_"]), th_smooth=float(self.p["th_smooth"]), omega=float(self.p["omega"]), epsilon=float(self.p["epsilon"]))

    # -- what every entry point makes: each registers with the caller's contextlib.ExitStack, which closes it also when the call raises
    def _runner(self, stack, m, **ranks):
        """View m's runner.  The views' seeds are 7919 apart; every runner gets random_vdisp (pm.PMRunner sets the energy's setting from it).
        ranks: rank, world, group of the ranks that share this view's cells."""
        return stack.enter_context(contextlib.closing(pm.PMRunner(self.e, self.units, self.table, seed=self.seed + 7919 * m, device=self.device, mode=m,
                                                                  random_vdisp=self.random_vdisp, device_cuts=self.device_cuts, **ranks)))

    def _graph_cut(self, stack):
        return stack.enter_context(contextlib.closing(gc.GraphCut(self.imL, self.imR, **self._pairwise())))

    def _eval_args(self):
        """The evaluator as keywords of api.DeviceEvaluator ({}: no ground truth, the rows carry the energy only)."""
        return {} if self.evaluator is None else dict(dispGT=self.evaluator.gt, nonocc=self.evaluator.nonocc, error_threshold=self.evaluator.threshold, precision=self.precision)

    def _device_evaluator(self, stack, max_rows, rates=True):
        return stack.enter_context(contextlib.closing(api.DeviceEvaluator(self.e, max_rows=max_rows, **(self._eval_args() if rates else {}))))

    def _start(self, runner, start):
        """The first half of ready to cut.  None: the reference's random start; else the warm start (LES/FastGCStereo.h:116-130) from a host or device map."""
        if start is None:
            runner.init_labels()
        else:
            runner.init_from_labels(start)

    def _ready_to_cut(self, runner, start, g):
        """Both halves: the runner starts from `start` and begins its cuts on g.  (run() has its PatchMatch iterations between the two.)"""
        self._start(runner, start)
        runner.begin_gc(g)
        return runner

    def _row(self, labels, cost, mode, index, t0, g=None, ev=None, rates=True):
        """Evaluator::evaluate (LES/Evaluator.h:113-187) of a view's device maps -> the row of the log.  ev: the api.DeviceEvaluator of the device
        route; None: the host route, whose sums are those of the host graph-cut context g (None, before the first cut: no pairwise sum, smooth is
        NaN).  rates: the row carries all / nonocc (the ground truth is the left view's)."""
        row = dict(index=index, time=time.perf_counter() - t0 - self.eval_seconds)
        if ev is not None:
            ev.evaluate(labels.data_ptr(), cost.data_ptr(), mode=mode, index=index, **self._pairwise())
            r = ev.rows()[-1]
            row.update(energy=r["data"] + r["smooth"], data=r["data"], smooth=r["smooth"])
            if rates:
                row["all"], row["nonocc"] = r["all"], r["nonocc"]
            return row
        d = pm.disparities(labels).cpu().numpy() if rates else None
        if g is not None:
            g.labels[mode][...], g.costs[mode][...] = labels.cpu().numpy(), cost.cpu().numpy()
            dc, sc = g.data_cost(mode), g.smoothness_cost(mode)
        else:
            dc, sc = float(cost.sum(dtype=torch.float64)), float("nan")
        row.update(energy=dc + (0.0 if sc != sc else sc), data=dc, smooth=sc)
        if rates:
            if self.precision > 0:                                         # Evaluator::quantize, LES/Evaluator.h:106-111
                d = (np.rint(d / np.float32(self.precision)) * np.float32(self.precision)).astype(np.float32)
            row["all"], row["nonocc"] = self.evaluator.evaluate(d)
        return row

    def _evaluate_body(self, index, mode, runner, g, t0):
        ev = self._dev_eval[mode] if self._dev_eval is not None else None
        self.log.append(self._row(runner.labels, runner.cur, mode, index, t0, g if runner.gc is g else None, ev, rates=self.evaluator is not None))

    def _evaluate(self, index, mode, runner, g, t0):
        """A row of the runner's view.  Like the reference's evaluator, it stops the run's clock while it works (stop() / start() around the body,
        LES/Evaluator.h:115-116,183-184): `time` excludes evaluation."""
        runner._sync()
        te = time.perf_counter()
        try:
            self._evaluate_body(index, mode, runner, g, t0)
        finally:
            self.eval_seconds += time.perf_counter() - te

    def run(self, maxIteration, viewModes=(0,), pmInit=0, labeling=None):
        """FastGCStereo::run (LES/FastGCStereo.h:133-227).  Returns (labeling, rawlabeling) of the left view as
        H x W x 4 float arrays (the raw one is the labelling before the post-processing: of two-view runs, and with FastGCStereo(speckle=)
        of one-view runs too, whose mask is then the speckle mask alone).  `labeling`: optional
        start labelling (the reference's `labeling` argument; every view starts from it, as in the reference), or a dict {view: H x W x 4
        map} that gives each view of a two-view run its own (self.raw_labelings of an earlier run resumes it), or the string "wta": each view starts
        from the winner-take-all map of its own filtered cost volume (les_hip_wta_labels, csrc/les_wtavol.h; the map stays on the device; single
        rank).  A map that is H x W (alone or in the dict) is a disparity map: the view starts from the planes fitted to it (fit_planes:
        les_hip_fit_planes, csrc/les_planefit.h; self.fit_params).  "wta+planes": the "wta" start, and right after begin_gc, before the first
        graph-cut iteration, each view fuses the planes fitted to its WTA map (the WTA map is the fit's fallback) into its solution by fusion
        moves (pm.PMRunner.fuse; the report goes to self.slant_stats; no map visits the host; with maxIteration == 0 the start is the WTA map
        alone; single rank).  "sgm" / "sgm+planes": the same two starts from the semi-global matching map of each view's own raw cost volume
        (les_hip_sgm_labels, csrc/les_sgm.h; self.sgm_params; not for the image-based energy: ValueError).  "half": coarse to fine -- the energy's
        half-resolution twin (api.HipCostVolumeEnergy.half: images and volumes pooled on the device, csrc/les_pyramid.h) is solved first by a nested
        driver with self.coarse_params, and each view starts from its coarse planes re-expressed at full resolution on the device
        (les_hip_upsample_labels); see _half_starts for the nested run's layers and pairwise parameters (a reasoned default, not tuned);
        self.coarse_seconds and self.coarse_stats report it; single rank.  The costs of a start labelling come from one dense device pass per view (pm.PMRunner.init_from_labels)."""
        with contextlib.ExitStack() as stack:        # closes the runners, the graph-cut context and the device evaluators of the run, also when it raises
            return self._run(stack, maxIteration, tuple(viewModes), pmInit, labeling)

    def fuse(self, labeling, others, viewMode=0, layers=None):
        """Fusion moves (FastGCStereo::fusionMoveBK, LES/FastGCStereo.h:241-410, which no mode of the reference reaches): starts from `labeling`
        (H x W x 4) by the route of run(..., labeling=) -- the costs of its labels from one dense device pass -- and fuses each map of `others` into it in
        turn, over every disjoint set of the layers added by addLayer (layers: their indices, None = all), by graph cuts on the device
        (pm.PMRunner.fuse).  A pixel of the result carries its label of `labeling` or of one of `others`; no map raises the energy.  With an evaluator
        set, self.log gets one row for the start and one after each map (device evaluation when evaluate_on_device); self.fuse_stats: the runner's
        report per map.  Single rank.  -> the fused labelling, H x W x 4."""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.fuse is single-rank: multi-rank fusion is not implemented")
        t0 = time.perf_counter()
        self.eval_seconds, self.log, self.fuse_stats = 0.0, [], []
        m = int(viewMode)
        with contextlib.ExitStack() as stack:
            runner, g = self._runner(stack, m), self._graph_cut(stack)
            self._dev_eval = {m: self._device_evaluator(stack, len(others) + 1)} if self.evaluate_on_device else None
            self._ready_to_cut(runner, labeling, g)
            if self.evaluator is not None:
                self._evaluate(0, m, runner, g, t0)
            for k, other in enumerate(others):
                self.fuse_stats.append(runner.fuse(other, layers=layers, nthreads=self.host_threads))
                if self.evaluator is not None:
                    self._evaluate(k + 1, m, runner, g, t0)
            runner._sync()
            return runner.labels.cpu().numpy().copy()

    def fit_planes(self, disp_or_labeling, viewMode=0, **params):
        """Slanted planes from a disparity map (no reference counterpart; csrc/les_planefit.h): per pixel of view viewMode an edge-aware weighted
        least-squares plane through the disparities of its window, guided by that view's image (api.HipCostVolumeEnergy.fit_planes).
        disp_or_labeling: an H x W disparity map (a PFM file, another matcher, the previous frame) or an H x W x 4 label map, whose own
        disparities are fitted.  Pixels without an accepted fit keep their own disparity as a fronto-parallel plane; non-finite or out-of-range
        ones get (0, 0, min_disp, 0).  params: over self.fit_params (radius, sig, gate0, gate_slope, max_slope, min_support).
        -> the H x W x 4 map, a start for run(labeling=) or a second labelling for fuse()."""
        out = self.e.fit_planes(disp_or_labeling, mode=int(viewMode), device=self.device, **dict(self.fit_params, **params))
        self.e.synchronize()
        return out.cpu().numpy().copy()

    def _fuse_fitted(self, runner, wta_map):
        """A runner that is ready to cut (begin_gc) fuses the planes fitted to `wta_map` (a device map, also the fit's fallback) into its solution.
        -> the runner's fuse report + kind_pixels: how many pixels of the fitted map are [fallback, fronto-parallel, slanted]"""
        fitted, kind = self.e.fit_planes(wta_map, mode=runner.mode, fallback=wta_map, with_kind=True, device=self.device, **self.fit_params)
        report = runner.fuse(fitted, nthreads=self.host_threads)
        report["kind_pixels"] = torch.bincount(kind.flatten().to(torch.int64), minlength=3).tolist()
        return report

    def _cross_view_step(self, runners, layers=None):
        """One cross-view step on two runners that are ready to cut (begin_gc): both label maps are snapshotted on the device, then each view fuses
        the OTHER view's snapshot, warped into its coordinates with its own snapshot as the fallback, into its solution.  Both warps read the
        snapshots, so the order of the views does not matter.  The labels make no host round trip.  -> {view: fuse report + hit_pixels}"""
        snap = {m: runners[m].labels.clone() for m in (0, 1)}
        out = {}
        for m in (0, 1):
            warped = torch.empty_like(snap[m])
            hit = torch.empty((self.e.H, self.e.W), dtype=torch.uint8, device=warped.device)
            self.e.warp_labels(1 - m, snap[1 - m].data_ptr(), snap[m].data_ptr(), warped.data_ptr(), hit.data_ptr())
            out[m] = runners[m].fuse(warped, layers=layers, nthreads=self.host_threads)
            out[m]["hit_pixels"] = int(hit.sum())
        return out

    def cross_fuse(self, labelings, layers=None):
        """Cross-view fusion of two finished views (no reference counterpart; csrc/les_crossview.h): labelings = {0: L, 1: R}, both H x W x 4.
        Each view starts from its map by the route of fuse() and fuses the other view's map, warped into its coordinates, into it:
            L' = fuse(L, [warp(R -> view 0, fallback L)])        R' = fuse(R, [warp(L -> view 1, fallback R)])
        over every disjoint set of the layers added by addLayer (layers: their indices, None = all).  Both warps are taken from the input maps.  A
        pixel of L' carries its label of L or of the warped map; no view's energy rises.  self.cross_stats: per view the runner's fuse report plus
        hit_pixels (target pixels some source pixel landed on) and energy_before / energy_after.  Single rank.  -> {0: L', 1: R'}"""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.cross_fuse is single-rank: multi-rank cross-view fusion is not implemented")
        if sorted(labelings) != [0, 1]:
            raise ValueError(f"cross_fuse takes the maps of both views, {{0: L, 1: R}} (views given: {sorted(labelings)})")
        with contextlib.ExitStack() as stack:
            runners = {m: self._runner(stack, m) for m in (0, 1)}
            g = self._graph_cut(stack)
            before = {}
            for m in (0, 1):
                self._ready_to_cut(runners[m], labelings[m], g)
                before[m] = sum(runners[m].energy(self._pairwise()))
            self.cross_stats = self._cross_view_step(runners, layers)
            for m in (0, 1):
                self.cross_stats[m].update(energy_before=before[m], energy_after=sum(runners[m].energy(self._pairwise())))
            return {m: runners[m].labels.cpu().numpy().copy() for m in (0, 1)}

    def confidence(self, labeling, viewMode=0, **kw):
        """The confidence of any H x W x 4 label map of view viewMode under that view's aggregated cost volume (no reference counterpart;
        csrc/les_confidence.h; api.HipCostVolumeEnergy.confidence, whose keywords -- band (default: confidence_band), scale, chunk, parts -- kw
        passes on).  -> the H x W float32 map in [0, 1]; parts=True: (conf, own, rival, k_rival).  Single rank."""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.confidence is single-rank: the multi-rank form is not implemented")
        out = self.e.confidence(labeling, mode=int(viewMode), device=self.device, **dict(dict(band=self.confidence_band), **kw))
        self.e.synchronize()
        return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()

    def reconstruct(self, labeling, calib, viewMode=0, conf=None, min_confidence=None, speckle=None, max_jump=None, z_max=None):
        """The 3D reconstruction of any H x W x 4 label map of view viewMode (no reference counterpart; csrc/les_reproject.h;
        api.HipCostVolumeEnergy.reproject and .mesh): every label is a surface element, so the points AND the normals are exact, and the surface
        is torn where the energy's own smoothness term says two pixels lie on different surfaces.  calib: io.calib3d's Calib, read_calib's dict or
        a plain dict(f, cx, cy, doffs, baseline); the points are in the view's own camera frame (X right, Y down, Z forward) in the baseline's
        unit.  A pixel is dropped where conf (an H x W map, FastGCStereo.confidence's) < min_confidence, or where the speckle mask of
        speckle=(max_size, max_diff) is set (api.speckle_mask), when either is given; or where Z > z_max.  max_jump: two neighbouring pixels
        are joined iff the un-truncated pairwise term of their labels is <= max_jump (None: this energy's th_smooth, where the term saturates).
        -> dict(points, normals: H x W x 3 float32, NaN where invalid; valid: H x W bool; vertices, vertex_normals: N x 3 float32 and colors:
        N x 3 uint8 RGB from the context's image, per vertex in row-major pixel order; vertex_pixel: N int32 linear pixel indices; triangles:
        M x 3 int32 vertex numbers whose winding faces the camera), host arrays ready for io.write_ply.  It changes no estimate.  Single rank."""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.reconstruct is single-rank: the multi-rank form is not implemented")
        if (conf is None) != (min_confidence is None):
            raise ValueError("reconstruct: give conf and min_confidence together, or neither")
        from . import io as lio
        m, dev = int(viewMode), torch.device(self.device)
        lab = labeling if torch.is_tensor(labeling) else torch.from_numpy(np.array(labeling, dtype=np.float32, order="C"))
        lab = lab.to(device=dev, dtype=torch.float32).contiguous()
        drop = None
        if speckle is not None:
            drop = self.e.speckle_mask(lab, int(speckle[0]), float(speckle[1]), device=dev)        # (synchronises)
        if conf is not None:
            c = conf if torch.is_tensor(conf) else torch.from_numpy(np.array(conf, dtype=np.float32, order="C"))
            low = (c.to(device=dev, dtype=torch.float32) < float(min_confidence)).to(torch.uint8) * 255
            drop = low if drop is None else torch.maximum(drop, low)
        jump = float(self.p["th_smooth"]) if max_jump is None else float(max_jump)
        points, normals, valid = self.e.reproject(lab, lio.calib3d(calib), mode=m, drop=drop, z_max=z_max, device=dev)
        self.e.synchronize()
        vindex, vpixel, tri = self.e.mesh(lab, valid, jump, mode=m, device=dev)
        # per-vertex gathers: plumbing, torch indexing by vertex_pixel
        idx = vpixel.long()
        rgb = torch.from_numpy(np.ascontiguousarray(self.e.image(m)[..., ::-1])).to(dev)
        out = dict(points=points, normals=normals, valid=valid != 0, vertices=points.reshape(-1, 3)[idx], vertex_normals=normals.reshape(-1, 3)[idx],
                   colors=rgb.reshape(-1, 3)[idx], vertex_pixel=vpixel, triangles=tri)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def synthesize(self, labelings, t=0.5, tol=1.0, fill=True, viewMode=0):
        """The image a camera at fraction t in [0, 1] of the baseline, counted from the LEFT view, would see (no reference counterpart;
        csrc/les_view.h; api.HipCostVolumeEnergy.render_view and .blend_views).  labelings: {0: L, 1: R}, H x W x 4 maps of both views -- each view is
        rendered from its own image (view 0 at t, view 1 at 1 - t) and the two renders are blended: mixed (1 - t) : t where their disparities agree
        within tol, the nearer one where they do not -- or one H x W x 4 map of view viewMode, rendered alone.  fill: a hole takes the farther of
        its nearest neighbours on the row.  -> (image H x W x 3 uint8 b, g, r; disparity H x W float32, NaN in holes; source H x W uint8: 0 hole,
        1 left view, 2 right view, 3 both, 4 filled), host arrays.  It changes no estimate.  Single rank."""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.synthesize is single-rank: the multi-rank form is not implemented")
        maps = labelings if isinstance(labelings, dict) else {int(viewMode): labelings}
        if not maps or any(m not in (0, 1) for m in maps):
            raise ValueError(f"synthesize takes one label map or {{0: L, 1: R}} (views given: {sorted(maps)})")
        t = float(t)
        sides = {m: self.e.render_view(maps[m], src_mode=m, t=t if m == 0 else 1.0 - t, device=self.device) for m in sorted(maps)}
        out = self.e.blend_views(t, left=sides.get(0), right=sides.get(1), tol=tol, fill=fill, device=self.device)
        self.e.synchronize()
        return tuple(o.cpu().numpy() for o in out)

    def photo_error(self, labeling, viewMode=0):
        """The photometric error of any H x W x 4 label map of view viewMode against the two images, no ground truth needed (no reference
        counterpart; csrc/les_view.h; api.HipCostVolumeEnergy.photo_error).  -> (err H x W float32, vis H x W uint8): vis 1 seen in the other
        view, 2 occluded by the label map's own account, 0 outside; err the mean absolute colour difference, NaN where vis != 1.  io.photometric
        sums them up.  Single rank."""
        if self.world > 1:
            raise NotImplementedError("FastGCStereo.photo_error is single-rank: the multi-rank form is not implemented")
        err, vis = self.e.photo_error(labeling, mode=int(viewMode), device=self.device)
        self.e.synchronize()
        return err.cpu().numpy(), vis.cpu().numpy()

    def _confidences(self, maps):
        """With confidence=True: self.confidences of the device label maps {view: map} as they are (raw), -> {view: the device confidence map};
        otherwise {} (and self.confidences is emptied)."""
        self.confidences = {}
        if not self.with_confidence:
            return {}
        conf = {m: self.e.confidence(lab, mode=m, band=self.confidence_band, device=self.device) for m, lab in maps.items()}
        self.e.synchronize()
        self.confidences = {m: c.cpu().numpy() for m, c in conf.items()}
        return conf

    def wta(self, viewModes=(0,), post_process=True, subpixel=True, slanted=False):
        """Cost-volume filtering without a graph cut (no reference counterpart; csrc/les_wtavol.h): every view of viewModes gets the winner-take-all
        map of its filtered cost volume -- per pixel the fronto-parallel plane of least aggregated cost, refined to sub-pixel when `subpixel`
        (les_hip_wta_labels: the H1 workload and a streaming arg-min over its slabs, a few milliseconds).  With an evaluator set, self.log gets one
        row per view (index = mode = the view; energy, data, smooth; all / nonocc for the left view, whose ground truth the evaluator holds), made
        from the maps before any post-processing, through the device evaluator when evaluate_on_device (the host route has no pairwise sum without
        a graph-cut context: smooth is NaN there, as in run() before the first cut).  With two views and post_process, the left-right check, fill
        and weighted median of run() follow (threshold 1.5, the run's omega); with FastGCStereo(speckle=) the mask is widened by the speckle mask and one
        view is post-processed too (with that mask alone).  Sets self.raw_labelings.  Single rank.
        slanted (opt-in; needs the layers of addLayer, it raises without): before the rows and the post-processing each view fuses the planes
        fitted to its WTA map (les_hip_fit_planes, csrc/les_planefit.h; self.fit_params) into that map by fusion moves over every disjoint set of
        the layers (pm.PMRunner.fuse); a pixel ends with its WTA label or its fitted one, and the costs of the rows are the dense re-scoring's.
        The reports go to self.slant_stats.
        -> (labeling, rawlabeling) of the left view as run() does (None without the left view)."""
        return self._volume_maps("wta", viewModes, post_process, slanted, subpixel=subpixel)

    def sgm(self, viewModes=(0,), paths=8, p1=None, p2=None, post_process=True, subpixel=True, slanted=False):
        """Semi-global matching without a graph cut (no reference counterpart; csrc/les_sgm.h), the twin of wta(): every view of viewModes gets the
        SGM map of its own RAW cost volume -- the costs truncated at th_col, scan-line dynamic programming along `paths` (2, 4 or 8) directions
        with the penalties p1 <= p2 (None: 0.16 th_col and 1.28 th_col), summed, read out per pixel as wta() does (les_hip_sgm_labels).  The rows of
        self.log, the two-view post-processing, `slanted`, self.raw_labelings, self.slant_stats and the return value are wta()'s; the costs of the
        rows are the dense re-scoring of the labels (the summed path cost is not the energy's unary cost).  Not for the image-based energy
        (api.LesHipError, error 3: it holds no volume).  Single rank."""
        return self._volume_maps("sgm", viewModes, post_process, slanted, paths=paths, p1=p1, p2=p2, subpixel=subpixel)

    def _volume_map(self, source, m, **params):
        """View m's "wta" / "sgm" map -> (labels, the read-out's costs), both on the device: what wta(), sgm() and run(labeling=<name>) start from."""
        return (self.e.sgm_labels if source == "sgm" else self.e.wta_labels)(mode=m, device=self.device, **params)

    def _volume_maps(self, source, viewModes, post_process, slanted, **params):
        """The body wta() and sgm() share: each view's _volume_map, the optional fusion of the fitted planes, the rows, the two-view post-processing."""
        if self.world > 1:
            raise NotImplementedError(f"FastGCStereo.{source} is single-rank: the multi-rank form is not implemented")
        views = tuple(int(m) for m in viewModes)
        t0 = time.perf_counter()
        self.eval_seconds, self.log = 0.0, []
        if slanted and not self.units:
            raise ValueError(f"{source}(slanted=True) fuses over the cells of the layers: add layers (addLayer) first")
        maps = {}
        for m in views:
            maps[m] = lab, cost = self._volume_map(source, m, **params)
            if source == "sgm":          # the summed path cost is not the energy's unary cost: the costs of the labels from one dense device pass
                self.e.unary_labels(lab.data_ptr(), cost.data_ptr(), mode=m, check=True)
        if slanted:
            self.slant_stats = {}
            with contextlib.ExitStack() as stack:
                g = self._graph_cut(stack)
                for m in views:
                    with contextlib.ExitStack() as view_stack:
                        runner = self._ready_to_cut(self._runner(view_stack, m), maps[m][0], g)
                        self.slant_stats[m] = self._fuse_fitted(runner, maps[m][0])
                        runner._sync()
                        maps[m] = (runner.labels.clone(), runner.cur.clone())
        self.e.synchronize()
        self.raw_labelings = {m: maps[m][0].cpu().numpy().copy() for m in views}
        if self.evaluator is not None:
            for m in views:
                te = time.perf_counter()
                with contextlib.ExitStack() as stack:          # (the ground truth is the left view's: the other view's row carries no rates)
                    ev = self._device_evaluator(stack, 1, rates=m == 0) if self.evaluate_on_device else None
                    self.log.append(dict(index=m, mode=m) | self._row(maps[m][0], maps[m][1], m, m, t0, ev=ev, rates=m == 0))
                self.eval_seconds += time.perf_counter() - te
        conf = self._confidences({m: maps[m][0] for m in views})
        if post_process and self._post_processes(views):
            self._post_process({m: maps[m][0] for m in views}, conf)
            self.e.synchronize()
        lab = maps[0][0].cpu().numpy().copy() if 0 in maps else None
        self.seconds = time.perf_counter() - t0 - self.eval_seconds
        return lab, self.raw_labelings.get(0)

    def _post_processes(self, views):
        """Whether a call over `views` ends with the post-processing: two views always, one view when a speckle filter, min_confidence,
        max_photo_error or valid masks are set."""
        return len(views) == 2 or self.speckle is not None or self.min_confidence is not None or self.max_photo_error is not None or self.valid is not None

    def _post_process(self, maps, conf=None):
        """The post-processing step of run(), wta() and sgm() in place on the device label maps {view: map}: threshold 1.5, the run's omega
        (LES/FastGCStereo.h:202), (left, right) whatever the order of the views; with self.speckle the widened mask, and the one-view form; with
        self.min_confidence each view's mask widened by conf[view] < min_confidence (conf: what _confidences returned for the same maps); with
        self.max_photo_error by vis == 1 and err > max_photo_error of the view's map as it comes in (les_hip_photo_error); with self.valid by
        the view's own invalid pixels."""
        ptr = {m: maps[m].data_ptr() if m in maps else None for m in (0, 1)}
        if self.min_confidence is not None or self.max_photo_error is not None or self.valid is not None:
            low = {m: torch.zeros(maps[m].shape[:2], dtype=torch.bool, device=maps[m].device) for m in maps}
            if self.valid is not None:
                low = {m: low[m] | ~torch.from_numpy(self.valid[m]).to(maps[m].device) if m in self.valid else low[m] for m in maps}
            if self.min_confidence is not None:
                low = {m: low[m] | (conf[m] < self.min_confidence) for m in maps}
            if self.max_photo_error is not None:
                photo = {m: self.e.photo_error(maps[m], mode=m, device=self.device) for m in maps}
                self.e.synchronize()
                low = {m: low[m] | ((photo[m][1] == 1) & (photo[m][0] > self.max_photo_error)) for m in maps}
            low = {m: low[m].to(torch.uint8).contiguous() for m in maps}
            if any(t.is_cuda for t in low.values()):     # (torch made the masks on its stream; the library reads them on the context's)
                torch.cuda.current_stream().synchronize()
            self.e.post_process(ptr[0], ptr[1], 1.5, self.p["omega"], speckle=self.speckle, fail=tuple(low[m].data_ptr() if m in low else None for m in (0, 1)))
            self.e.synchronize()                 # (the masks live until the launches that read them are done)
        elif self.speckle is None:
            self.e.post_process(ptr[0], ptr[1], 1.5, self.p["omega"])
        else:
            self.e.post_process(ptr[0], ptr[1], 1.5, self.p["omega"], speckle=self.speckle)

    # -- run(), stage by stage
    def _check_run(self, maxIteration, viewModes, labeling):
        """What run() refuses.  -> (with_planes: each view fuses the planes fitted to its start map in before the first cut; the graph-cut
        iterations, counted from 1, that end with a cross-view step: every cross_view-th one and the last one)"""
        with_planes = False
        if isinstance(labeling, str):
            source, with_planes = _parse_start(labeling)
            if source == "sgm" and self.e.sgm_workspace_bytes() == 0:
                raise ValueError(f"labeling=\"{labeling}\": semi-global matching runs over a cost volume of at most 512 disparities; this energy (the image-based "
                                 "one holds no volume) has none it can use")
            if self.world > 1:
                raise NotImplementedError(f"labeling=\"{labeling}\" is single-rank: the multi-rank start is not implemented")
        if self.with_confidence and self.world > 1:
            raise NotImplementedError("confidence / min_confidence are single-rank: the multi-rank form is not implemented")
        if self.max_photo_error is not None and self.world > 1:
            raise NotImplementedError("max_photo_error is single-rank: the multi-rank form is not implemented")
        if self.valid is not None and self.world > 1:
            raise NotImplementedError("valid is single-rank: the multi-rank form is not implemented")
        if self.inner_loop_log and self.world > 1:
            raise ValueError("inner_loop_log is a single-rank log: with several ranks a rank holds only its band of a set's cells until the exchange")
        if self.cross_view > 0:
            if self.world > 1:
                raise NotImplementedError("cross_view is single-rank: multi-rank cross-view fusion is not implemented")
            if sorted(viewModes) != [0, 1]:
                raise ValueError("cross_view needs a two-view run (viewModes (0, 1)): there is no other view to fuse with")
        cross_after = {it + 1 for it in range(maxIteration) if (it + 1) % self.cross_view == 0 or it + 1 == maxIteration} if self.cross_view > 0 else set()
        return with_planes and maxIteration > 0, cross_after

    def _split_views(self, all_views):
        """Several ranks and two views: the views are independent until the post-processing (LES/FastGCStereo.h:172-185), so the ranks are
        split into one group per view -- the first ceil(world / 2) ranks advance the left view, the others the right one -- and each
        group shards the cells of ITS view.  A coarse layer has only 4-6 cells per disjoint set (SURVEY 8 geometry table): spread
        over world / 2 ranks instead of world, and the two views no longer take turns.  The groups meet once, before the
        post-processing (_gather).  -> (this rank's group, its rank and world within it, {view: its group's first rank}, this rank's views)"""
        if self.world == 1 or len(all_views) != 2:
            return None, self.rank, self.world, {}, all_views
        import torch.distributed as dist
        n0 = (self.world + 1) // 2
        if self._view_groups is None:                      # (every rank creates both groups; once per object, not per run)
            self._view_groups = [dist.new_group(list(range(0, n0))), dist.new_group(list(range(n0, self.world)))]
        mine = 0 if self.rank < n0 else 1
        return (self._view_groups[mine], self.rank - (0 if mine == 0 else n0), (n0 if mine == 0 else self.world - n0),
                {all_views[0]: 0, all_views[1]: n0}, (all_views[mine],))

    def _open_evaluators(self, stack, runners, log_rows, inner_rows_per_set):
        """Device evaluation: one evaluator for the rows of the log (the left view's, as the host route's), one per view for the inner-loop log
        (the ground truth is the left view's: the right view's rows carry the energy only)."""
        self._dev_eval = {0: self._device_evaluator(stack, log_rows)} if self.evaluate_on_device or self.inner_loop_log else None
        self._inner, self.inner_log = {}, []
        if self.inner_loop_log:
            for m, r in runners.items():
                ev = self._device_evaluator(stack, max(1, len(r.sets) * inner_rows_per_set), rates=m == 0)
                self._inner[m] = r.inner_log = SimpleNamespace(evaluator=ev, params=self._pairwise(), meta=[])

    def _half_starts(self, views):
        """The "half" start: the energy's half-resolution twin solved by a nested driver, each view's coarse map upsampled on the device.
        The nested driver has the same seed, device, host threads and cut settings, no evaluator and no post-processing; its layers are those of
        addLayer with unit sizes max(3, (s + 1) // 2), duplicates dropped; its rows (the energy only) come from the device evaluator; its pairwise parameters are lambda_ x 2 and th_smooth / 2, because
        disparity differences halve with the resolution (a reasoned default, not tuned); iterations, pmInit and labeling come from
        self.coarse_params.  The labels make no host round trip.  -> {view: H x W x 4 device map}"""
        t0 = time.perf_counter()
        cp = dict(COARSE_DEFAULTS, **self.coarse_params)
        below = cp.pop("coarse_params", None)
        if set(cp) != set(COARSE_DEFAULTS):
            raise TypeError(f"coarse_params: unknown keys {sorted(set(cp) - set(COARSE_DEFAULTS))}")
        if not self.units:
            raise ValueError("labeling=\"half\" solves over the layers halved: add layers (addLayer) first")
        with contextlib.ExitStack() as stack:
            half = stack.enter_context(contextlib.closing(self.e.half()))
            params = {k: v for k, v in self.p.items() if k != "filter"}
            params.update(lambda_=2.0 * float(self.p["lambda_"]), th_smooth=0.5 * float(self.p["th_smooth"]), windR=half.params.windR)
            st = FastGCStereo(half, half.imL, half.imR, params, device=self.device, seed=self.seed, host_threads=self.host_threads, device_cuts=self.device_cuts,
                              random_vdisp=None if self.random_vdisp is None else 0.5 * self.random_vdisp, evaluate_on_device=True)
            st._coarse = True
            st.fit_params, st.sgm_params = dict(self.fit_params), dict(self.sgm_params)
            if below is not None:
                st.coarse_params = dict(below)
            for s, table in zip(self.units, self.table):
                u = max(3, (s + 1) // 2)
                if u not in st.units:
                    st.addLayer(u, table)
            st.run(int(cp["iterations"]), views, int(cp["pmInit"]), labeling=cp["labeling"])
            starts, kinds = {}, {}
            for m in views:
                starts[m], kind = self.e.upsample_labels(half, st._device_maps[m], mode=m, with_kind=True, device=self.device)
                kinds[m] = torch.bincount(kind.flatten().to(torch.int64), minlength=3).tolist()       # (synchronises: the half context may close)
            self.coarse_stats = dict(shape=(half.H, half.W, half.D), windR=half.params.windR, units=list(st.units), iterations=int(cp["iterations"]), pmInit=int(cp["pmInit"]),
                                     labeling=cp["labeling"], lambda_=params["lambda_"], th_smooth=params["th_smooth"], seconds=st.seconds, log=st.log,
                                     gc_seconds=dict(st.gc_seconds), kind_pixels=kinds, coarse_seconds=st.coarse_seconds, coarse_stats=st.coarse_stats)
        self.coarse_seconds = time.perf_counter() - t0
        return starts

    def _start_map(self, labeling, m, named=None):
        """What view m starts from, of run()'s `labeling`: None (the random start), a name (the view's _volume_map, on the device; "half": its map
        of `named`, what _half_starts returned), an H x W x 4 map, an H x W disparity map (the planes fitted to it, made on the device) or a dict
        {view: one of the two}."""
        if labeling is None:
            return None
        if isinstance(labeling, str):
            source = _parse_start(labeling)[0]
            if source == "half":
                return named[m]
            return self._volume_map(source, m, **(self.sgm_params if source == "sgm" else {}))[0]
        if isinstance(labeling, dict) and m not in labeling:
            raise ValueError(f"labeling has no map for view {m} (views given: {sorted(labeling)})")
        start = labeling[m] if isinstance(labeling, dict) else labeling
        if not hasattr(start, "shape"):
            start = np.asarray(start, np.float32)
        if len(start.shape) == 2:
            start = self.e.fit_planes(start, mode=m, device=self.device, **self.fit_params)
        return start

    def _cut_view(self, runner, it, main_device, nthreads):
        """Graph-cut iteration `it` of one view, on the calling thread (the current device is per host thread)."""
        dev = torch.device(self.device)
        if dev.type == "cuda":
            torch.cuda.set_device(dev.index if dev.index is not None else main_device)
        runner.gc_iteration(it, check=self.check_flow_energy, nthreads=nthreads)

    def _cut_view_in_thread(self, runner, it, main_device, nthreads, errors):
        """The thread body of the concurrent schedule.  On the GPU each view advances on its own stream: its synchronisations (one per lock-step)
        then wait for its own kernels only, and the two views' kernels overlap.  An error goes to `errors` (re-raised on the caller's thread)."""
        try:
            dev = torch.device(self.device)
            if dev.type != "cuda":
                return self._cut_view(runner, it, main_device, nthreads)
            torch.cuda.set_device(dev.index if dev.index is not None else main_device)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.default_stream())
            with torch.cuda.stream(side):
                self.e.set_thread_stream(side.cuda_stream)
                try:
                    self._cut_view(runner, it, main_device, nthreads)
                    side.synchronize()
                finally:
                    self.e.set_thread_stream(0, bind=False)
        except BaseException as ex:
            errors.append(ex)

    def _gc_iteration(self, runners, it, main_device):
        """Graph-cut iteration `it` of this rank's views under the chosen schedule (the two views are independent until the post-processing,
        LES/FastGCStereo.h:172-185): joint, concurrent or one view after the other."""
        views = list(runners)
        if len(views) == 2 and self.joint_views and self.world == 1 and not self.check_flow_energy:
            pm.PMRunner.gc_iteration_joint([runners[m] for m in views], it, nthreads=self.host_threads)
        elif len(views) == 2 and self.concurrent_views:
            # two host threads (the C calls release the GIL).  Two teams cut at the same time: 16 threads each measured best on the 2 x 64-core host
            # (1436 x 992, two views: 12 threads 10.3 s, 16 threads 10.2 s, 24 threads 10.8 s, 32 threads 11.1 s, 64 threads 11.7 s)
            import threading
            errors, per_view = [], self.host_threads if self.host_threads > 0 else 16
            ths = [threading.Thread(target=self._cut_view_in_thread, args=(runners[m], it, main_device, per_view, errors))
                   for m in (reversed(views) if self._swap_view_threads else views)]
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            if errors:
                raise errors[0]
        else:
            for m in views:
                self._cut_view(runners[m], it, main_device, self.host_threads)

    def _graph_cuts(self, runners, g, maxIteration, pmInit, fit_from, cross_after, t0):
        """The graph-cut iterations of this rank's views (fit_from: view -> the start map whose fitted planes it fuses in before the first one); then
        what their runners counted, summed over the views."""
        for m, r in runners.items():
            r.begin_gc(g)
            if m in fit_from:
                self.slant_stats[m] = self._fuse_fitted(r, fit_from[m])
        main_device = torch.cuda.current_device() if torch.device(self.device).type == "cuda" else 0
        for it in range(maxIteration):
            for r in runners.values():
                r.inner_iteration = it + 1 + pmInit
            self._gc_iteration(runners, it, main_device)
            if it + 1 in cross_after:
                # whichever schedule cut the iteration: both views are at rest here, on the driver's thread and stream (the fusion's sets
                # add their rows to the inner-loop log under this iteration, after the rows of its cuts)
                self.cross_view_stats.append(dict(iteration=it + 1, views=self._cross_view_step(runners)))
            if 0 in runners:
                self._evaluate(it + 1 + pmInit, 0, runners[0], g, t0)
        for r in runners.values():
            self.gc_max_gap = max(self.gc_max_gap, r.gc_max_gap)
            self.gc_moves_raised += int(r.gc_seconds.get("moves_raised", 0))
            for k, v in r.gc_seconds.items():      # sums over the views; a worst gap is the worst of the views
                self.gc_seconds[k] = max(self.gc_seconds.get(k, 0.0), v) if k.startswith("own_max_gap_") else self.gc_seconds.get(k, 0.0) + v

    def _gather(self, runners, all_views, view_root):
        """-> {view: its final label map on the device}.  Where the ranks were split into view groups, the groups meet here: every rank receives
        both maps (16 B/px each) from the first rank of each group."""
        if not view_root:
            return {m: runners[m].labels for m in all_views}
        import torch.distributed as dist
        final = {m: (runners[m].labels if m in runners else torch.zeros((self.e.H, self.e.W, 4), dtype=torch.float32, device=torch.device(self.device)))
                 for m in all_views}
        for m in all_views:
            if final[m].is_cuda and dist.get_backend() == "gloo":          # (one-GPU functional tests of the multi-rank path: gloo moves host memory)
                h = final[m].cpu()
                dist.broadcast(h, src=view_root[m])
                final[m].copy_(h)
            else:
                dist.broadcast(final[m], src=view_root[m])
        return final

    def _collect_stats(self, runners):
        """What the runners counted, before they close: the exchanges, the tiled solver's lock-steps, the inner-loop log."""
        self.bytes_exchanged = sum(r.bytes_exchanged for r in runners.values())
        self.all_gathers = sum(r.exchanges for r in runners.values())
        self.exchange_seconds = sum(r.exchange_seconds() for r in runners.values())     # device time inside pack -> all-gather -> unpack on this rank
        # per view and layer: how long the lock-steps cut by the tiled solver took (p50 / p90 / max ms, launches)
        self.tiled_lockstep_stats = {}
        for m, r in runners.items():
            for li, rows in r.tiled_lockstep_ms.items():
                a = np.array(rows, np.float64)
                self.tiled_lockstep_stats[f"view{m}_layer{li}"] = dict(locksteps=len(a), ms_p50=round(float(np.percentile(a[:, 0], 50)), 2), ms_p90=round(float(np.percentile(a[:, 0], 90)), 2),
                                                                       ms_max=round(float(a[:, 0].max()), 2), ms_sum=round(float(a[:, 0].sum()), 1), launches_p50=int(np.percentile(a[:, 1], 50)),
                                                                       launches_max=int(a[:, 1].max()))
        # the inner-loop log: read once, here (each view's rows were enqueued on the stream that ran its sets)
        for m, lg in self._inner.items():
            for (iteration, li, k), r in zip(lg.meta, lg.evaluator.rows()):
                self.inner_log.append(dict(iteration=iteration, layer=li, set=k, mode=m, data=r["data"], smooth=r["smooth"], energy=r["data"] + r["smooth"],
                                           all=r.get("all"), nonocc=r.get("nonocc")))

    def _run(self, stack, maxIteration, all_views, pmInit, labeling):
        with_planes, cross_after = self._check_run(maxIteration, all_views, labeling)
        self.slant_stats, self.cross_view_stats = {}, []
        t0 = time.perf_counter()
        self.eval_seconds = 0.0
        view_group, view_rank, view_world, view_root, views = self._split_views(all_views)
        runners = {m: self._runner(stack, m, rank=view_rank, world=view_world, group=view_group) for m in views}
        self._open_evaluators(stack, runners, maxIteration + pmInit + 3, maxIteration + pmInit + len(cross_after) + int(with_planes))
        g = self._graph_cut(stack) if maxIteration > 0 else None
        starts = {}
        self.coarse_seconds, self.coarse_stats = 0.0, {}
        named = self._half_starts(views) if isinstance(labeling, str) and _parse_start(labeling)[0] == "half" else None
        for m, r in runners.items():       # per view: its start map, its costs, its first row
            starts[m] = self._start_map(labeling, m, named)
            self._start(r, starts[m])
            if m == 0:                     # (the rows of run() are the left view's)
                self._evaluate(0, 0, r, None, t0)
        # the reference starts its clock HERE -- START_TIMER after initCurrentFast and the first evaluation (LES/FastGCStereo.h:135-141),
        # with the layers (addLayer, LES/main.cpp:395-397) and the energy built before run() -- `seconds` below keeps counting from the top
        # of this function; `seconds_reference_clock` is the same run on the reference's clock
        self.init_seconds = time.perf_counter() - t0 - self.eval_seconds
        for it in range(pmInit):
            for m, r in runners.items():
                r.inner_iteration = it + 1
                r.iteration(it)
                if m == 0:
                    self._evaluate(it + 1, 0, r, None, t0)
        self.gc_max_gap, self.gc_seconds, self.gc_moves_raised = 0.0, {}, 0
        if maxIteration > 0:
            self._graph_cuts(runners, g, maxIteration, pmInit, starts if with_planes else {}, cross_after, t0)
        final = self._gather(runners, all_views, view_root)
        if self._coarse:                   # the nested run of a "half" start: its maps stay on the device, raw (the views meet at full resolution)
            self._device_maps = {m: final[m].clone() for m in all_views}
            self.raw_labelings = {}
            self.seconds = time.perf_counter() - t0 - self.eval_seconds
            self.seconds_reference_clock = self.seconds - self.init_seconds
            self._collect_stats(runners)
            return None, None
        self.raw_labelings = {m: final[m].cpu().numpy().copy() for m in all_views}
        conf = self._confidences(final)
        if self._post_processes(all_views):
            self._post_process(final, conf)
            if self.recost_after_post:
                for r in runners.values():
                    r.recost()
            if 0 in runners:               # (the rows of the log belong to the ranks of the left view's group)
                self._evaluate(maxIteration + 1 + pmInit, 0, runners[0], None, t0)
        lab = final[0].cpu().numpy().copy() if 0 in final else None
        self.seconds = time.perf_counter() - t0 - self.eval_seconds          # evaluation excluded (as in the reference), set-up and initialisation included (unlike it)
        self.seconds_reference_clock = self.seconds - self.init_seconds
        self._collect_stats(runners)
        return lab, self.raw_labelings.get(0)


COARSE_DEFAULTS = dict(iterations=5, pmInit=2, labeling=None)      # FastGCStereo.coarse_params: the nested run of the "half" start


def _parse_start(name):
    """A start's name -> (source "wta" / "sgm" / "half", with_planes)"""
    if name not in ("wta", "wta+planes", "sgm", "sgm+planes", "half"):
        raise ValueError(f"labeling {name!r}: a label map, a disparity map, a dict of them, \"wta\", \"wta+planes\", \"sgm\", \"sgm+planes\" or \"half\"")
    source, _, planes = name.partition("+")
    return source, bool(planes)


def disparities(labeling):
    H, W = labeling.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    return labeling[..., 0] * xs + labeling[..., 1] * ys + labeling[..., 2]


def vertical_disparities(labeling):
    """The v map of a labeling (H x W x 4 planes a, b, c, v): the vertical offset each pixel's label samples the other view at."""
    return np.asarray(labeling)[..., 3].copy()


def _layers(st, sizes):
    e, r, p = api.PROPOSE_EXPANSION, api.PROPOSE_RANSAC, api.PROPOSE_RANDOM
    st.addLayer(sizes[0], [(e, 1), (r, 1), (p, 7)])                    # LES/main.cpp:300-306 / :391-397
    st.addLayer(sizes[1], [(e, 2), (r, 1)])
    st.addLayer(sizes[2], [(e, 2), (r, 1)])


def _front_end(e, data, params, evaluator, precision, layer_sizes, iterations, pmIterations, doDual, init, **kw):
    """The tail MidV2 and MidV3 share: the driver on energy `e` with the evaluator and the three layers runs, and driver and energy close, also
    when it raises.  -> (the driver, labeling, rawlabeling)"""
    try:
        st = FastGCStereo(e, data["imL"], data["imR"], params, **kw)
        try:
            st.setEvaluator(evaluator, precision=precision)
            _layers(st, layer_sizes)
            lab, raw = st.run(iterations, (0, 1) if doDual else (0,), pmIterations, labeling=init)
        finally:
            st.close()
    finally:
        e.close()
    return st, lab, raw


def MidV2(data, iterations=5, pmIterations=2, doDual=False, smooth_weight=None, filterRadious=20, device="cuda", seed=1, lib=None, params=None,
          vdisp=0.0, random_vdisp=0.0, init=None, valid=None, **kw):
    """MidV2 (LES/main.cpp:270-328) on a data dict of io.load_data: image-based matching cost, layers 5/15/25, error
    threshold 0.5, disparities quantised to the ground-truth precision before evaluation.  params: PARAMS_GF (the reference's choice,
    default) or PARAMS_BF (or a dict with their keys): filter, eps, alpha, th_col, th_grad; smooth_weight (default: params' lambda_)
    and filterRadious override lambda_ and windR as the reference's options do (:284-286).
    vdisp: the vertical-disparity range of the energy (MAX_VDISPARITY, :281): initial labels draw v in [-vdisp, vdisp].  As in main.cpp
    the random proposer keeps range 0 (RandomProposer(7, maxdisp)); random_vdisp (opt-in, not in main.cpp) gives it its own maxVDisp.
    init: the start labelling of run() -- None (the default): the reference's random start; "wta": every view starts from the winner-take-all
    map of its filtered cost volume (FastGCStereo.run's labeling="wta"); "wta+planes": that start, and the slanted planes fitted to it are fused
    in before the first graph-cut iteration (labeling="wta+planes").  "sgm" / "sgm+planes" (MidV3's semi-global matching starts) raise ValueError
    here: MidV2 uses the image-based energy, which holds no cost volume to run them over.  "half": coarse to fine -- the half-resolution problem
    (both images pooled) is solved first and its planes, upsampled, are the start (FastGCStereo.run's labeling="half"; coarse_params=dict(...)
    among the further keywords sets the nested run's iterations, pmInit and labeling).
    valid (MidV3's valid masks) raises ValueError here: the masks go into cost volumes, and the image-based energy holds none.
    Further keywords go to FastGCStereo (cross_view=n with doDual: cross-view fusion after every n-th graph-cut iteration)."""
    if isinstance(init, str) and _parse_start(init)[0] == "sgm":
        raise ValueError(f"MidV2(init={init!r}): MidV2 uses the image-based energy, which holds no cost volume; semi-global matching runs over one (MidV3)")
    if valid is not None and valid is not False:
        raise ValueError("MidV2(valid=...): MidV2 uses the image-based energy, which holds no cost volume for the masks to go into (MidV3)")
    p = dict(PARAMS_GF if params is None else params)
    lam = p["lambda_"] if smooth_weight is None else smooth_weight
    maxdisp = float(data["ndisp"] - 1)
    e = api.HipCostVolumeEnergy.naive(data["imL"], data["imR"], windR=filterRadious, eps=p["eps"], alpha=p["alpha"],
                                      th_col=p["th_col"], th_grad=p["th_grad"], max_disp=maxdisp,
                                      device=torch.device(device).index or 0, lib=lib, filter=p["filter"], max_vdisp=vdisp)
    return _front_end(e, data, dict(p, lambda_=lam, windR=filterRadious), io.Evaluator(data["dispGT"], data["nonocc"], 0.5), data.get("gt_prec", -1.0), (5, 15, 25),
                      iterations, pmIterations, doDual, init, device=device, seed=seed, random_vdisp=random_vdisp, **kw)


def MidV3(data, volL=None, volR=None, iterations=5, pmIterations=2, doDual=False, smooth_weight=0.5, mc_threshold=0.5, filterRadious=20,
          error_threshold=1.0, device="cuda", seed=1, lib=None, params=None, interpolate=1, lambda_ad=10.0, lambda_census=30.0, init=None,
          cost="adcensus", patch=(2, 2), features=None, valid=None, **kw):
    """MidV3 (LES/main.cpp:330-420): cost-volume energy (volumes ingested on the device), layers 1 % / 3 % / 9 % of the
    image width.  volL / volR: host arrays / memmaps [ndisp][H][W] (volR None: synthesised from the left one).  params: PARAMS_GF
    (default) or PARAMS_BF: filter and eps; smooth_weight, mc_threshold and filterRadious override lambda_, th_col and windR (:351-353).
    interpolate: the energy's setInterpolationMethod (LES/CostVolumeEnergy.h:45-48) -- 0 nearest, 1 linear (default), 2 quadratic.
    volL None: no volume files -- both views' AD-Census volumes (io.build_volumes; lambda_ad, lambda_census) are built on the device from
    data["imL"], data["imR"] and data["ndisp"]; cost="zncc" builds the ZNCC volumes of (2 ry + 1) x (2 rx + 1) grey patches instead, patch = (ry, rx), and
    features= (a pair of float32 [C][H][W] device tensors, or a callable image -> such a tensor) the correlation volumes of those feature maps, used as given
    (io.build_volumes; csrc/les_featvol.h).  cost / patch / features together with explicit volumes: ValueError.  init: as for MidV2 (None: the random start; "wta": the winner-take-all start; "wta+planes": with its fitted planes fused in), and "sgm" / "sgm+planes": every view starts from the semi-global matching map of its own raw volume (FastGCStereo.run's labeling="sgm" / "sgm+planes"; csrc/les_sgm.h); "half": the coarse-to-fine start over the pooled volumes (labeling="half"; csrc/les_pyramid.h).  Further keywords go to FastGCStereo (cross_view=n with doDual: cross-view fusion after every
    n-th graph-cut iteration).
    valid (opt-in): a pair (validL, validR) of H x W masks, nonzero = valid, or True for data["validL"] / data["validR"] (Rectifier.data(valid=True)):
    the volumes' fills become the nearest-valid row fill (io.build_volumes / io.ingest_volumes(valid=); csrc/les_maskvol.h), and each view's
    invalid pixels join its failure mask of the post-processing (FastGCStereo(valid=))."""
    p = dict(PARAMS_GF if params is None else params)
    maxdisp = float(data["ndisp"] - 1)
    if valid is False:
        valid = None
    if valid is True:
        valid = (data["validL"], data["validR"])
    if valid is not None:
        valid = tuple(valid)
        if len(valid) != 2:
            raise ValueError("MidV3(valid=...): a pair (validL, validR) of H x W masks, or True for data['validL'] / data['validR']")
        kw = dict(kw, valid={0: valid[0], 1: valid[1]})
    if volL is None:
        if volR is not None:
            raise ValueError("volR without volL")
        tl, tr = io.build_volumes(data["imL"], data["imR"], data["ndisp"], device=device, lib=lib, lambda_ad=lambda_ad, lambda_census=lambda_census,
                                  cost=cost, patch=patch, features=features, valid=valid)
    else:
        if cost != "adcensus" or features is not None or tuple(patch) != (2, 2):
            raise ValueError("cost / patch / features build the volumes from the pair: not together with explicit volumes")
        tl, tr = io.ingest_volumes(volL, volR, device=device, lib=lib, valid=valid)
    D, H, W = tl.shape
    e = api.HipCostVolumeEnergy(data["imL"], data["imR"], tl.data_ptr(), tr.data_ptr(), windR=filterRadious, eps=p["eps"],
                                th_col=mc_threshold, max_disp=maxdisp, device=torch.device(device).index or 0, volumes_on_device=True,
                                shape=(D, H, W), lib=lib, filter=p["filter"], interpolate=interpolate)
    # (tl, tr: the energy reads the volumes in place; they live until the run has returned)
    return _front_end(e, data, dict(p, lambda_=smooth_weight, windR=filterRadious, th_col=mc_threshold), io.Evaluator(data["dispGT"], data["nonocc"], error_threshold), -1.0,
                      (int(W * 0.01), int(W * 0.03), int(W * 0.09)), iterations, pmIterations, doDual, init, device=device, seed=seed, **kw)


class Rectifier:
    """The front end of a calibrated rig (no reference counterpart; csrc/les_rectify.h): two raw, distorted frames -> the rectified pair every
    other entry of the package assumes, on the device, and the calibration with which reconstruct gives metric points.
    K0, dist0, K1, dist1, R, T, f, principal: io.stereo_rectify's (X1 = R X0 + T; dist up to (k1, k2, p1, p2, k3, k4, k5, k6); pixel centres at
    integer coordinates).  raw_size = (Hs, Ws) of the raw frames; size = (H, W) of the rectified ones (default: raw_size; neither crops nor
    rescales to the valid region).  interp: "nearest", "linear" or "cubic".  Both maps are built on the device once, here
    (api.rectify_map); a frame then costs one api.remap launch per image, enqueued on torch's current stream of the device.
    .transform: io.stereo_rectify's dict; .calib: its api.Calib (doffs = cx1 - cx0, baseline = |T|); .maps: the two H x W x 2 float32 device
    tensors of raw positions, (NaN, NaN) where a rectified pixel has none.
    The way back (csrc/les_unrectify.h): .inverse_maps, the two Hs x Ws x 2 device tensors of rectified positions of the raw pixels, built on
    first use with `steps` fixed-point steps and a residual bound of `tol` raw pixels (api.unrectify_map); .unrectify puts a label map's
    geometry and .to_raw a rectified-grid image onto the raw grid; .valid_rect and .crop give a rectified pair without invalid borders.
    model="fisheye": the raw cameras are equidistant fisheye cameras (csrc/les_fisheye.h): dist0, dist1 are (k1, k2, k3, k4), fov the lenses' full
    field of view in degrees (io.stereo_rectify's); both maps come from api.rectify_map_fisheye / api.unrectify_map_fisheye, `steps` counts
    Newton steps (default api.FISHEYE_STEPS), and everything that works on the maps is unchanged.  Frame a wide lens with f=, principal=, size=
    and crop(): a pinhole frame cannot hold rays near 90 degrees off its axis."""

    def __init__(self, K0, dist0, K1, dist1, R, T, raw_size, size=None, f=None, principal=None, interp="linear", device="cuda", lib=None,
                 steps=None, tol=api.UNRECTIFY_TOL, model="pinhole", fov=None):
        if interp not in api.INTERP_NAMES:
            raise ValueError(f"unknown interp {interp!r}: one of {sorted(api.INTERP_NAMES)}")
        self.transform = tr = io.stereo_rectify(K0, dist0, K1, dist1, R, T, f=f, principal=principal, model=model, fov=fov)
        self.model = model
        self.steps, self.tol = int((api.FISHEYE_STEPS if model == "fisheye" else api.UNRECTIFY_STEPS) if steps is None else steps), float(tol)
        self._inverse_maps = self._valid_rect = None
        self.calib = tr["calib"]
        self.raw_size = tuple(int(n) for n in raw_size)
        self.size = self.raw_size if size is None else tuple(int(n) for n in size)
        self.interp, self.lib = interp, lib
        self.device = torch.device(device)
        self.index = self.device.index or 0 if self.device.type == "cuda" else 0
        H, W = self.size
        self.maps = []
        for m in (0, 1):
            t = torch.empty((H, W, 2), dtype=torch.float32, device=self.device)
            if model == "fisheye":
                api.rectify_map_fisheye(self._fisheye(m), tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], t.data_ptr(), H, W, device=self.index,
                                        stream=self._stream(), lib=lib)
            else:
                api.rectify_map(api.camera(tr[f"K{m}"], tr[f"dist{m}"]), tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], t.data_ptr(), H, W, device=self.index,
                                stream=self._stream(), lib=lib)
            self.maps.append(t)

    def _fisheye(self, m):
        tr = self.transform
        return api.fisheye(tr[f"K{m}"], tr[f"dist{m}"], tr[f"theta_max{m}"])

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0

    def rectify(self, rawL, rawR):
        """rawL, rawR: the raw frames, Hs x Ws x 3 uint8 BGR, numpy arrays or tensors on the device.  -> dict(imL, imR: H x W x 3 uint8, validL,
        validR: H x W bool -- False where the rectified pixel has no raw position or one outside the frame; such a pixel is black --, calib);
        host arrays for host frames, device tensors for device frames."""
        Hs, Ws = self.raw_size
        H, W = self.size
        out, on_device = {}, torch.is_tensor(rawL) and torch.is_tensor(rawR)
        for name, raw, mp in (("L", rawL, self.maps[0]), ("R", rawR, self.maps[1])):
            src = raw if torch.is_tensor(raw) else torch.from_numpy(np.array(raw, order="C"))
            if src.dtype != torch.uint8 or tuple(src.shape) != (Hs, Ws, 3):
                raise ValueError(f"rectify: a {Hs} x {Ws} x 3 uint8 frame expected, got {tuple(src.shape)} {src.dtype}")
            src = src.to(self.device).contiguous()
            dst = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            valid = torch.empty((H, W), dtype=torch.uint8, device=self.device)
            api.remap(src.data_ptr(), Hs, Ws, 3, mp.data_ptr(), dst.data_ptr(), valid.data_ptr(), H, W, interp=self.interp, device=self.index,
                      stream=self._stream(), lib=self.lib)
            out["im" + name], out["valid" + name] = dst, valid != 0
        if not on_device:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        out["calib"] = self.calib
        return out

    def data(self, rawL, rawR, ndisp, valid=False):
        """The data dict of io.load_data for the rectified pair, so that MidV2(data) / MidV3(data) run on it unchanged: imL, imR (host arrays),
        ndisp, nonocc = validL, dispGT zeros (no ground truth), gt_prec -1.  valid=True adds validL, validR (H x W bool host arrays), what
        MidV3(data, valid=True) feeds into its volumes."""
        r = self.rectify(rawL, rawR)
        host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
        imL, imR, validL = host(r["imL"]), host(r["imR"]), host(r["validL"])
        out = dict(imL=imL, imR=imR, dispGT=np.zeros(imL.shape[:2], np.float32), nonocc=validL, ndisp=int(ndisp), gt_prec=-1.0)
        if valid:
            out.update(validL=validL, validR=host(r["validR"]))
        return out

    # -- the way back to the raw camera (csrc/les_unrectify.h) ------------------------------------------------------------------------------
    @property
    def inverse_maps(self):
        """The two Hs x Ws x 2 float32 device tensors (xs, ys): where in the rectified frame of this Rectifier every raw pixel of a view lies;
        (NaN, NaN) where the inversion has not converged or the pixel has no rectified position.  Built on first use."""
        if self._inverse_maps is None:
            tr, (Hs, Ws) = self.transform, self.raw_size
            maps = []
            for m in (0, 1):
                t = torch.empty((Hs, Ws, 2), dtype=torch.float32, device=self.device)
                if self.model == "fisheye":
                    api.unrectify_map_fisheye(self._fisheye(m), tr[f"R{m}"], tr["f"], tr[f"cx{m}"], tr["cy"], t.data_ptr(), Hs, Ws, steps=self.steps,
                                              tol=self.tol, device=self.index, stream=self._stream(), lib=self.lib)
                else:
                    api.unrectify_map(api.camera(tr[f"K{m}"], tr[f"dist{m}"]), tr[f"R{m}"], tr["f"], tr[f"cx{m}"], tr["cy"], t.data_ptr(), Hs, Ws, steps=self.steps,
                                      tol=self.tol, device=self.index, stream=self._stream(), lib=self.lib)
                maps.append(t)
            self._inverse_maps = maps
        return self._inverse_maps

    def unrectify(self, labeling, viewMode=0, drop=None, z_max=None):
        """The H x W x 4 label map of rectified view viewMode as geometry registered to the pixels of that view's RAW image: every raw pixel takes the
        plane of the nearest rectified pixel and evaluates it at its own sub-pixel rectified position.  drop: an H x W map, nonzero = dropped;
        z_max: a limit on the rectified depth.  -> dict(points, normals: Hs x Ws x 3 float32 in the raw camera's frame (X right, Y down, Z
        forward, the baseline's unit); disparity: Hs x Ws float32, the rectified disparity at the raw pixel; depth: points[..., 2]; valid:
        Hs x Ws bool), NaN where invalid; host arrays for a host labeling, device tensors for a device one."""
        m, tr, (Hs, Ws), (H, W) = int(viewMode), self.transform, self.raw_size, self.size
        if m not in (0, 1):
            raise ValueError(f"unrectify: viewMode {viewMode!r} (0 or 1)")
        on_device = torch.is_tensor(labeling)
        lab = labeling if on_device else torch.from_numpy(np.array(labeling, dtype=np.float32, order="C"))
        if tuple(lab.shape) != (H, W, 4):
            raise ValueError(f"unrectify: a {H} x {W} x 4 label map expected, got {tuple(lab.shape)}")
        lab = lab.to(device=self.device, dtype=torch.float32).contiguous()
        mask = None
        if drop is not None:
            mask = drop if torch.is_tensor(drop) else torch.from_numpy(np.array(drop, order="C"))
            if tuple(mask.shape) != (H, W):
                raise ValueError(f"unrectify: an {H} x {W} drop map expected, got {tuple(mask.shape)}")
            mask = (mask.to(self.device) != 0).to(torch.uint8).contiguous()
        points, normals = (torch.empty((Hs, Ws, 3), dtype=torch.float32, device=self.device) for _ in range(2))
        disparity = torch.empty((Hs, Ws), dtype=torch.float32, device=self.device)
        valid = torch.empty((Hs, Ws), dtype=torch.uint8, device=self.device)
        api.unrectify_labels(lab.data_ptr(), H, W, mask.data_ptr() if mask is not None else None, self.inverse_maps[m].data_ptr(), Hs, Ws, tr[f"R{m}"].T,
                             tr["f"], tr[f"cx{m}"], tr["cy"], tr["doffs"], tr["baseline"], valid.data_ptr(), points.data_ptr(), normals.data_ptr(),
                             disparity.data_ptr(), z_max=z_max, device=self.index, stream=self._stream(), lib=self.lib)
        out = dict(points=points, normals=normals, disparity=disparity, depth=points[..., 2], valid=valid != 0)
        return out if on_device else {k: v.cpu().numpy() for k, v in out.items()}

    def to_raw(self, image, viewMode=0, interp="nearest"):
        """A rectified-grid H x W or H x W x 3 uint8 image of view viewMode (a mask, a rendered view, the rectified image itself) resampled onto
        that view's raw grid through the inverse map (api.remap).  -> (image_raw Hs x Ws[ x 3] uint8, valid Hs x Ws bool); a raw pixel without
        a rectified position inside the frame is 0 and invalid.  Host arrays for a host image, device tensors for a device one."""
        m, (Hs, Ws), (H, W) = int(viewMode), self.raw_size, self.size
        if m not in (0, 1) or interp not in api.INTERP_NAMES:
            raise ValueError(f"to_raw: viewMode {viewMode!r} (0 or 1), interp {interp!r} (one of {sorted(api.INTERP_NAMES)})")
        on_device = torch.is_tensor(image)
        src = image if on_device else torch.from_numpy(np.array(image, order="C"))
        if src.dtype != torch.uint8 or tuple(src.shape) not in ((H, W), (H, W, 3)):
            raise ValueError(f"to_raw: an {H} x {W}[ x 3] uint8 image expected, got {tuple(src.shape)} {src.dtype}")
        src = src.to(self.device).contiguous()
        dst = torch.empty((Hs, Ws) + tuple(src.shape[2:]), dtype=torch.uint8, device=self.device)
        valid = torch.empty((Hs, Ws), dtype=torch.uint8, device=self.device)
        api.remap(src.data_ptr(), H, W, 3 if src.dim() == 3 else 1, self.inverse_maps[m].data_ptr(), dst.data_ptr(), valid.data_ptr(), Hs, Ws, interp=interp,
                  device=self.index, stream=self._stream(), lib=self.lib)
        valid = valid != 0
        return (dst, valid) if on_device else (dst.cpu().numpy(), valid.cpu().numpy())

    def valid_rect(self):
        """(y0, x0, h, w): the largest axis-aligned rectangle of the rectified frame whose pixels are valid in BOTH views, by the sampler's rule on
        .maps (0 <= u <= Ws - 1 and 0 <= v <= Hs - 1).  Ties: the largest area, then the smallest y0, then the smallest x0, then the larger h.
        (0, 0, 0, 0) when no pixel is.  Host numpy, computed once."""
        if self._valid_rect is None:
            Hs, Ws = self.raw_size
            both = np.ones(self.size, bool)
            for mp in self.maps:
                uv = mp.cpu().numpy().astype(np.float64)
                with np.errstate(invalid="ignore"):
                    both &= (uv[..., 0] >= 0.0) & (uv[..., 0] <= Ws - 1.0) & (uv[..., 1] >= 0.0) & (uv[..., 1] <= Hs - 1.0)
            self._valid_rect = largest_rect(both)
        return self._valid_rect

    def crop(self, rect=None):
        """A Rectifier on the same calibration whose rectified frame is the rectangle rect = (y0, x0, h, w) of this one's (None: valid_rect()).
        Its maps are the slices of this one's, so its rectify returns exactly the crop of this one's output; size, transform (cx0, cx1, cy) and
        calib (cx, cy) are shifted by (x0, y0), doffs, f and baseline are unchanged; its inverse maps are built from the shifted intrinsics."""
        import copy
        y0, x0, h, w = (int(v) for v in (self.valid_rect() if rect is None else rect))
        H, W = self.size
        if not (0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= H and x0 + w <= W):
            raise ValueError(f"crop: the rectangle (y0, x0, h, w) = {(y0, x0, h, w)} is empty or leaves the {H} x {W} frame")
        c = copy.copy(self)
        c.size = (h, w)
        c.maps = [mp[y0:y0 + h, x0:x0 + w].contiguous() for mp in self.maps]
        c.transform = tr = dict(self.transform)
        tr["cx0"], tr["cx1"], tr["cy"] = tr["cx0"] - x0, tr["cx1"] - x0, tr["cy"] - y0
        c.calib = tr["calib"] = io.calib3d(dict(f=tr["f"], cx=tr["cx0"], cy=tr["cy"], doffs=tr["doffs"], baseline=tr["baseline"]))
        c._inverse_maps = c._valid_rect = None
        return c


def largest_rect(mask):
    """(y0, x0, h, w) of the largest all-True axis-aligned rectangle of a 2D bool array; ties: the largest area, then the smallest y0, then the
    smallest x0, then the larger h; (0, 0, 0, 0) when nothing is True.  Every rectangle of the largest area cannot grow, so it is, for the row
    it ends on, the widest run of columns at least as tall as itself: the histogram scan below meets each such run once per row."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    best_key, best = None, (0, 0, 0, 0)
    height = np.zeros(W + 1, np.int64)                       # (a sentinel column of height 0 closes every run)
    for y in range(H):
        height[:W] = np.where(mask[y], height[:W] + 1, 0)
        hs, stack = height.tolist(), []                      # stack: (first column of the run, height), heights increasing
        for x, hx in enumerate(hs):
            start = x
            while stack and stack[-1][1] >= hx:
                start, h = stack.pop()
                if h > 0:
                    key = (-h * (x - start), y - h + 1, start, -h)
                    if best_key is None or key < best_key:
                        best_key, best = key, (y - h + 1, start, h, x - start)
            stack.append((start, hx))
    return best
