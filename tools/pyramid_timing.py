#!/usr/bin/env python
"""Timings of the half-resolution solve (csrc/les_pyramid.h) on the MI355X -> profiles/pyramid_timing.json (summarised in DESIGN 3.2j).

  python tools/pyramid_timing.py [--out profiles/pyramid_timing.json] [--reps 20] [--skip-runs] [--skip-kernels] [--scenes objects,three_surfaces,cones]

Every group of measurements runs in a child process of its own under its own time limit; the first child that fails ends the run.
  * kernels, at 1436 x 992 x 256 (each a group of one of tools/timing.py, which states the protocol: `reps` timings after two warm-up calls):
    les_pool_volume_kernel with non-temporal and with plain loads, and on the dword path (the same shape one column wider); les_pool_image_kernel;
    les_upsample_labels_kernel; the whole HipCostVolumeEnergy.half() call (wall clock: pools, guide statistics, march tables, tiled copy of both views); each next to
    les_hip_calib_copy of the bytes the kernel moves (read + written) / 8 floats -- a copy of n floats moves 8 n bytes;
  * runs: the two synthetic scenes of tools/e2e_bench.py at 1436 x 992 x 256 and the cones crop of tests/golden (64 disparities, AD-Census
    volumes), two views, MidV3 energy and layers: the Evaluator log of the default run (2 PatchMatch + 5 graph-cut iterations) and of the "half"
    start (coarse_params at their defaults: 2 + 5 at half resolution) followed by 1, 2 and 5 full-resolution graph-cut iterations -- energy of the
    start row and after the last iteration, bad-1.0 after the post-processing, seconds (coarse part apart).
Nothing here is a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import timing  # noqa: E402

W, H, D = 1436, 992, 256
CHILD_SECONDS = {"kernels": 240, "objects": 420, "three_surfaces": 420, "cones": 240}


def child_kernels(torch, reps):
    from localexpstereo_amd import api
    hs = api.half_size
    rec = dict(shape=[W, H, D])
    clock = timing.Clock(torch, "cuda")
    timed = lambda f: timing.time_one(clock, f, reps, warm=2)

    def entry(ms, nbytes):
        c = timing.spread(timed(timing.copy_call(api, nbytes, None)), 4)
        return dict(ms=timing.spread(ms, 4), bytes=int(nbytes), GBps=round(nbytes / float(np.median(ms)) / 1e6, 1), calib_copy_same_bytes_ms=c,
                    over_copy=round(float(np.median(ms)) / c["median"], 3))

    for name, w in (("pool_volume", W), ("pool_volume_dword_path_W_plus_1", W + 1)):
        vol = torch.rand((D, H, w), device="cuda")
        out = torch.empty((hs(D), hs(H), hs(w)), device="cuda")
        nbytes = 4 * (vol.numel() + out.numel())
        for nt in (("nontemporal", "plain") if w == W else ("plain",)):
            os.environ["LES_HIP_PYRAMID_NT"] = "1" if nt == "nontemporal" else "0"
            ms = timed(lambda: api.pool_volume(vol.data_ptr(), out.data_ptr(), D, H, w))
            rec[name if w != W else f"{name}_{nt}"] = entry(ms, nbytes)
        os.environ.pop("LES_HIP_PYRAMID_NT", None)
        del vol, out
    im = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    imh = torch.empty((hs(H), hs(W), 3), dtype=torch.uint8, device="cuda")
    rec["pool_image"] = entry(timed(lambda: api.pool_image(im.data_ptr(), imh.data_ptr(), H, W)), im.numel() + imh.numel())
    # the upsample and the whole half() call on a context of that shape
    rng = np.random.default_rng(1)
    imL = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    vl = torch.rand((D, H, W), device="cuda") * 0.6
    e = api.HipCostVolumeEnergy(imL, imL, vl.data_ptr(), vl.data_ptr(), windR=20, th_col=0.5, max_disp=float(D - 1), volumes_on_device=True, shape=(D, H, W))
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        half = e.half()
        walls.append(1e3 * (time.perf_counter() - t0))
        if len(walls) < 3:
            half.close()
    rec["half_call_wall_ms"] = timing.spread(walls, 4)
    src = torch.zeros((half.H, half.W, 4), device="cuda")
    src[..., 2] = torch.rand((half.H, half.W), device="cuda") * 100 + 5
    up = lambda: e.upsample_labels(half, src, with_kind=True)
    # per full pixel: its guide word, a plane written, a kind byte; per half pixel (through the cache): a guide word and a plane
    rec["upsample_labels"] = entry(timed(up), H * W * (4 + 16 + 1) + half.H * half.W * (4 + 16))
    half.close()
    e.close()
    return rec


def _drive(torch, stereo, lio, e, imL, imR, gt, nonocc, p, w):
    def driver():
        st = stereo.FastGCStereo(e, imL, imR, p, device="cuda", seed=1, evaluate_on_device=True)
        st.setEvaluator(lio.Evaluator(gt, nonocc, 1.0), precision=-1.0)
        stereo._layers(st, (max(1, int(w * 0.01)), int(w * 0.03), int(w * 0.09)))
        return st

    rec = {}
    driver().run(1, (0, 1), 0, labeling="half")                    # (warms the process up: libraries, allocator, the host cut's threads)
    for name, gc_it, pm_it, labeling in (("default", 5, 2, None), ("half+1", 1, 0, "half"), ("half+2", 2, 0, "half"), ("half+5", 5, 0, "half")):
        st = driver()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run(gc_it, (0, 1), pm_it, labeling=labeling)
        wall = time.perf_counter() - t0
        by_index = {r["index"]: r for r in st.log}
        rec[name] = dict(wall_seconds=round(wall, 3), seconds=round(st.seconds, 3), coarse_seconds=round(st.coarse_seconds, 3), pm_iterations=pm_it, gc_iterations=gc_it,
                         start=dict(energy=round(st.log[0]["energy"], 1), bad1_all=round(st.log[0]["all"], 3), bad1_nonocc=round(st.log[0]["nonocc"], 3)),
                         energy_after_last_iteration=round(by_index[pm_it + gc_it]["energy"], 1),
                         bad1_all_after_post=round(st.log[-1]["all"], 3), bad1_nonocc_after_post=round(st.log[-1]["nonocc"], 3))
        if labeling:
            cs = st.coarse_stats
            rec[name]["coarse"] = dict(shape=list(cs["shape"]), units=cs["units"], seconds=round(cs["seconds"], 3), kind_pixels=cs["kind_pixels"],
                                       energy_rows=[round(r["energy"], 1) for r in cs["log"]])
        sys.stderr.write(f"{name}: {json.dumps(rec[name])}\n")
    return rec


def child_scene(scene):
    import torch
    import e2e_bench
    from localexpstereo_amd import api, io as lio, stereo
    imL, imR, gt, volL = e2e_bench.scene_inputs(scene, H, W, D, "cuda")
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.ingest_volumes(volL, None, device="cuda")
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(D - 1), volumes_on_device=True,
                                shape=(D, H, W), filter=p["filter"])
    try:
        return dict(scene=scene, shape=[W, H, D], **_drive(torch, stereo, lio, e, imL, imR, gt, np.ones((H, W), bool), p, W))
    finally:
        e.close()


def child_cones():
    import torch
    from localexpstereo_amd import api, io as lio, stereo
    z = np.load(os.path.join(ROOT, "tests", "golden", "cones_crop.npz"))
    imL = np.ascontiguousarray(z["imL"])
    h, w = imL.shape[:2]
    imR, gt = np.ascontiguousarray(z["imR_wide"][:, 64:64 + w]), z["gt"].astype(np.float32)
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.build_volumes(imL, imR, 64, device="cuda")
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=63.0, volumes_on_device=True, shape=(64, h, w),
                                filter=p["filter"])
    try:
        return dict(scene="cones crop", shape=[w, h, 64], **_drive(torch, stereo, lio, e, imL, imR, np.where(gt > 0, gt, np.inf).astype(np.float32), gt > 0, p, w))
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true", help="the kernel timings only")
    ap.add_argument("--skip-kernels", action="store_true", help="the end-to-end runs only")
    ap.add_argument("--scenes", default="objects,three_surfaces,cones", help="the end-to-end runs to make (an --out file that exists keeps its other groups)")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        torch = timing.require_gpu("pyramid_timing.py")
        rec = child_kernels(torch, a.reps) if a.child == "kernels" else child_cones() if a.child == "cones" else child_scene(a.child)
        print("RESULT " + json.dumps(rec))
        return
    out = dict(note="one MI355X, one run; kernel numbers are medians of device-event timings after two warm-up calls", reps=a.reps)
    if a.out and os.path.exists(a.out):
        out = json.load(open(a.out))
    scenes = [s for s in a.scenes.split(",") if s]
    if any(s not in CHILD_SECONDS or s == "kernels" for s in scenes):
        raise SystemExit(f"--scenes: of objects, three_surfaces, cones (got {a.scenes})")
    groups = ([] if a.skip_kernels else ["kernels"]) + ([] if a.skip_runs else scenes)
    for what in groups:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", what], capture_output=True, text=True, timeout=CHILD_SECONDS[what])
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"pyramid_timing.py: the {what} measurements failed (exit {p.returncode}); nothing further was run")
        rec = json.loads(lines[-1][len("RESULT "):])
        if what == "kernels":
            out["kernels"] = rec
        else:
            out["runs"] = [r for r in out.get("runs", []) if r["scene"] != rec["scene"]] + [rec]
        print(json.dumps(rec, indent=1), flush=True)
        if a.out:                                                   # (written after every group: a later group's failure keeps the earlier ones)
            timing.write_json(a.out, out)


if __name__ == "__main__":
    main()
