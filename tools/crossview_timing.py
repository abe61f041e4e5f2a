#!/usr/bin/env python
"""Timings of the cross-view fusion (csrc/les_crossview.h) on the MI355X -> profiles/crossview_timing.json (summarised in DESIGN 3.4c).

  python tools/crossview_timing.py [--out profiles/crossview_timing.json]

Recorded:
  * warp_kernel: les_warp_labels_kernel at 1436 x 992 and 1500 x 1000 (planes of a piecewise-slanted scene, both source views), next to
    les_hip_calib_copy of the same number of bytes the warp moves (49 B per pixel: two label maps read, one written, the hit byte) -- each a
    group of one of tools/timing.py (which states the protocol) after 3 warm-up calls, one launch per timing;
  * cross_fuse: the whole stereo.FastGCStereo.cross_fuse pass per view on the two views' solutions of the "objects" scene of
    tools/e2e_bench.py at 1436 x 992 x 256 (MidV3 energy and layers);
  * runs: that scene, two views, 2 PatchMatch + 5 graph-cut iterations at cross_view 0 / 1 / 5: seconds, each view's final energy (its labelling
    before the post-processing with its own dense costs), the pixels that fail the left-right check before the post-processing
    (les_hip_consistency_check at 1.5: 255 = inconsistent, 128 = maps outside the other view, per view) and bad-1.0 of the final left labelling.
Nothing here is a gate: the quality figures are recorded, not asserted."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import timing  # noqa: E402

H, W, D = 992, 1436, 256


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def slanted_labels(h, w, seed, cell=40, maxd=200.0, slant=0.3):
    """Random slanted planes, one per cell x cell block, through their drawn disparity at the block's centre."""
    rng = np.random.default_rng(seed)
    hb, wb = -(-h // cell), -(-w // cell)
    pl = np.stack([rng.uniform(-slant, slant, (hb, wb)), rng.uniform(-slant, slant, (hb, wb)), rng.uniform(0, maxd, (hb, wb)), np.zeros((hb, wb))], -1)
    lab = np.repeat(np.repeat(pl, cell, 0), cell, 1)[:h, :w].astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    cx, cy = (xs // cell) * cell + cell // 2, (ys // cell) * cell + cell // 2
    lab[..., 2] = (lab[..., 2] - lab[..., 0] * cx - lab[..., 1] * cy).astype(np.float32)
    return np.ascontiguousarray(lab)


def time_kernel(torch, api, h, w, timings):
    im = np.zeros((h, w, 3), np.uint8)
    e = api.HipCostVolumeEnergy.naive(im, im, windR=0, max_disp=255.0, filter="")
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    src, fb = (torch.from_numpy(slanted_labels(h, w, s)).cuda() for s in (1, 2))
    out, hit = torch.empty_like(src), torch.empty((h, w), dtype=torch.uint8, device="cuda")
    clock = timing.Clock(torch, "cuda")
    one = lambda f: timing.spread(1e3 * np.asarray(timing.time_one(clock, f, timings, warm=3)), 3)
    rec = dict(shape=[w, h], bytes_moved=49 * h * w)
    for mode in (0, 1):
        rec[f"warp_us_src_view{mode}"] = one(lambda: e.warp_labels(mode, src.data_ptr(), fb.data_ptr(), out.data_ptr(), hit.data_ptr()))
        rec[f"hit_share_src_view{mode}"] = round(float(hit.float().mean()), 4)
    rec["copy_us"] = one(timing.copy_call(api, rec["bytes_moved"], torch.cuda.current_stream().cuda_stream))
    _note("kernel", rec["shape"], rec["warp_us_src_view0"], rec["warp_us_src_view1"], rec["copy_us"])
    rec["warp_over_copy"] = round(max(rec["warp_us_src_view0"]["median"], rec["warp_us_src_view1"]["median"]) / rec["copy_us"]["median"], 3)
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true", help="the kernel timings only")
    a = ap.parse_args()
    torch = timing.require_gpu("crossview_timing.py")
    import e2e_bench
    from localexpstereo_amd import api, io as lio, pm, stereo
    rec = dict(timings=a.timings, warp_kernel=[time_kernel(torch, api, h, w, a.timings) for h, w in ((992, 1436), (1000, 1500))])
    if not a.skip_runs:
        imL, imR, gt, volL = e2e_bench.scene_inputs("objects", H, W, D, "cuda")
        p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
        tl, tr = lio.ingest_volumes(volL, None, device="cuda")
        e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(D - 1), volumes_on_device=True,
                                    shape=(D, H, W), filter=p["filter"])

        def driver(cross_view):
            st = stereo.FastGCStereo(e, imL, imR, p, device="cuda", seed=1, cross_view=cross_view)
            st.setEvaluator(lio.Evaluator(gt, np.ones((H, W), bool), 1.0), precision=-1.0)
            stereo._layers(st, (int(W * 0.01), int(W * 0.03), int(W * 0.09)))
            return st

        def energy_of(st, labels, mode):
            r = pm.PMRunner(e, st.units, st.table, seed=1, device="cuda", mode=mode)
            try:
                r.init_from_labels(labels)
                return float(sum(r.energy(st._pairwise())))
            finally:
                r.close()

        def lr_failures(maps):
            lab = [torch.from_numpy(np.ascontiguousarray(maps[m], np.float32)).cuda() for m in (0, 1)]
            fail = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in (0, 1)]
            e.consistency_check(lab[0].data_ptr(), lab[1].data_ptr(), fail[0].data_ptr(), fail[1].data_ptr(), 1.5)
            return {f"view{m}": dict(inconsistent_255=int((fail[m] == 255).sum()), outside_128=int((fail[m] == 128).sum())) for m in (0, 1)}

        runs, maps0 = {}, None
        for cv in (0, 1, 5):
            st = driver(cv)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.run(5, (0, 1), 2)
            wall = time.perf_counter() - t0
            maps = dict(st.raw_labelings)
            if cv == 0:
                maps0 = maps
            steps = [dict(iteration=s["iteration"], **{f"view{m}": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s["views"][m].items()} for m in (0, 1)})
                     for s in st.cross_view_stats]
            _note("run cross_view", cv, round(st.seconds, 3), "s")
            runs[f"cross_view_{cv}"] = dict(seconds=round(st.seconds, 3), wall_seconds=round(wall, 3), final_energy={f"view{m}": energy_of(st, maps[m], m) for m in (0, 1)},
                                            lr_check_before_post=lr_failures(maps), bad1_all_final=st.log[-1]["all"], bad1_all_before_post=st.log[-2]["all"],
                                            cross_view_steps=steps)
        passes = []
        for _ in range(3):                                  # (the first one warms the launches up)
            st = driver(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.cross_fuse(maps0)
            wall = time.perf_counter() - t0
            _note("cross_fuse pass", round(wall, 3), "s")
            passes.append(dict(driver_seconds_with_warm_starts=round(wall, 4), **{f"view{m}": {k: (round(v, 4) if isinstance(v, float) else v)
                                                                                           for k, v in st.cross_stats[m].items()} for m in (0, 1)}))
        rec.update(shape=[W, H, D], scene="objects", maps="both views' solutions of seed 1 before the post-processing (2 PatchMatch + 5 graph-cut iterations)",
                   cross_fuse=dict(passes=passes, **{f"fuse_seconds_view{m}": timing.spread([q[f"view{m}"]["seconds"] for q in passes[1:]], 3) for m in (0, 1)}), runs=runs)
        e.close()
    timing.write_record(a.out, rec)


if __name__ == "__main__":
    main()
