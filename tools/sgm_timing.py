#!/usr/bin/env python
"""Timings of semi-global matching over a cost volume (csrc/les_sgm.h) on the MI355X -> profiles/sgm_timing.json (summarised in DESIGN 3.2i).

  python tools/sgm_timing.py [--out profiles/sgm_timing.json] [--skip-runs] [--skip-kernels]

Recorded:
  * sizes: les_hip_sgm_labels over a resident 256-slice U[0,1) volume at 1436 x 992 and 1500 x 1000, 4 and 8 paths -- the whole call (device events
    around it, LES_HIP_SGM_TIMING off) and every kernel of it (transpose, each direction, read-out: the library's own event brackets,
    LES_HIP_SGM_TIMING=1), the whole call a group of one of tools/timing.py (which states the protocol) after 3 warm-up calls; next to them the
    bytes each kernel has to move, computed from the shapes (byte_model below), and les_hip_calib_copy_wide moving the same number of bytes in the same
    run (whole copies of the volume, 2 V bytes each);
  * runs (unless --skip-runs): the two synthetic scenes of tools/e2e_bench.py at 1436 x 992 x 256, two views, MidV3 energy and layers: the
    Evaluator log of the default run (2 PatchMatch + 5 graph-cut iterations) and of the "wta", "wta+planes", "sgm" and "sgm+planes" starts at
    0 + 5 iterations -- energy after 1 / 3 / 5 iterations, bad-1.0 after the post-processing, seconds -- and FastGCStereo.sgm((0, 1)) alone.
Nothing here is a gate."""
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

D = 256
SIZES = ((992, 1436), (1000, 1500))
PATHS = (4, 8)


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def byte_model(h, w, k, paths):
    """The bytes each kernel has to move, with V = H W K 4: the transpose reads and writes the volume once (2 V), the first direction reads Ct and
    writes S (2 V), each later one reads Ct, reads and writes S (3 V), the read-out reads S (1 V).  (The padding of K to 64 / 128 / 256 / 512 and
    the 20 bytes per pixel of output are not counted.)"""
    v = h * w * k * 4
    per = [2 * v, 2 * v] + [3 * v] * (paths - 1) + [v]
    return dict(V=v, per_kernel=per, total=sum(per))


def time_size(torch, api, synth, h, w, timings):
    P = h * w
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    vol = torch.rand((D, h, w), device="cuda", dtype=torch.float32, generator=gen)
    e = api.HipCostVolumeEnergy(synth.make_guide(h, w, 1234), None, vol.data_ptr(), None, windR=20, eps=1e-4, th_col=0.5, max_disp=D - 1,
                                volumes_on_device=True, shape=(D, h, w))
    stream = torch.cuda.current_stream()
    e.set_stream(stream.cuda_stream)
    labels, cost = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w), device="cuda")
    rec = dict(shape=[w, h, D], workspace_bytes=e.sgm_workspace_bytes(), penalties=[float(x) for x in e.sgm_penalties()])
    clock = timing.Clock(torch, "cuda")
    one = lambda f: timing.spread(timing.time_one(clock, f, timings, warm=3), 4)
    copy = timing.copy_call(api, 2 * 4 * D * P, stream.cuda_stream, wide=True)          # one whole copy of the volume: 2 V bytes
    for paths in PATHS:
        bm = byte_model(h, w, D, paths)
        r = dict(byte_model=bm)
        call = lambda: e.sgm_labels(0, paths, None, None, True, labels.data_ptr(), cost.data_ptr())
        os.environ.pop("LES_HIP_SGM_TIMING", None)
        r["whole_call_ms"] = one(call)
        copies = bm["total"] // (2 * bm["V"])                  # whole copies of the volume that move the call's bytes
        assert copies * 2 * bm["V"] == bm["total"]
        r["copy_wide_same_bytes_ms"] = one(lambda: [copy() for _ in range(copies)])
        r["copy_wide_copies"] = copies
        r["whole_call_over_copy"] = round(r["whole_call_ms"]["median"] / r["copy_wide_same_bytes_ms"]["median"], 3)
        r["whole_call_GBps"] = round(bm["total"] / r["whole_call_ms"]["median"] / 1e6, 1)
        os.environ["LES_HIP_SGM_TIMING"] = "1"
        per = []
        for _ in range(timings):
            call()
            per.append(e.sgm_last_times())
        os.environ.pop("LES_HIP_SGM_TIMING", None)
        per = np.asarray(per)
        names = ["transpose"] + [f"direction_{i}" for i in range(paths)] + ["readout"]
        r["kernels"] = {nm: dict(ms=timing.spread(per[:, i], 4), bytes=bm["per_kernel"][i], GBps=round(bm["per_kernel"][i] / float(np.median(per[:, i])) / 1e6, 1))
                        for i, nm in enumerate(names)}
        r["kernels_sum_ms"] = round(float(np.median(per.sum(1))), 4)
        rec[f"paths{paths}"] = r
        _note(rec["shape"], paths, "paths:", r["whole_call_ms"], "copy", r["copy_wide_same_bytes_ms"], "ratio", r["whole_call_over_copy"],
              {k: v["ms"]["median"] for k, v in r["kernels"].items()})
    e.close()
    return rec


def time_runs(torch, api, stereo, lio, e2e_bench, scene):
    h, w = SIZES[0]
    imL, imR, gt, volL = e2e_bench.scene_inputs(scene, h, w, D, "cuda")
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.ingest_volumes(volL, None, device="cuda")
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(D - 1), volumes_on_device=True,
                                shape=(D, h, w), filter=p["filter"])

    def driver():
        st = stereo.FastGCStereo(e, imL, imR, p, device="cuda", seed=1, evaluate_on_device=True)
        st.setEvaluator(lio.Evaluator(gt, np.ones((h, w), bool), 1.0), precision=-1.0)
        stereo._layers(st, (int(w * 0.01), int(w * 0.03), int(w * 0.09)))
        return st

    rec = dict(scene=scene, shape=[w, h, D])
    for name, fn in (("sgm_only", lambda st: st.sgm((0, 1))), ("wta_only", lambda st: st.wta((0, 1)))):
        fn(driver())                                            # (warms the context's workspace up)
        st = driver()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lab, _ = fn(st)
        wall = time.perf_counter() - t0
        bad = float((np.abs(stereo.disparities(lab) - gt) > 1.0).mean() * 100)
        rec[name] = dict(wall_seconds=round(wall, 4), seconds=round(st.seconds, 4), bad1_all_after_post=round(bad, 3),
                         rows=[dict(mode=r["mode"], energy=round(r["energy"], 1), bad1_all=round(r["all"], 3) if "all" in r else None) for r in st.log])
        _note(scene, name, rec[name])
    for name, pm_it, labeling in (("default", 2, None), ("wta", 0, "wta"), ("wta+planes", 0, "wta+planes"), ("sgm", 0, "sgm"), ("sgm+planes", 0, "sgm+planes")):
        st = driver()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run(5, (0, 1), pm_it, labeling=labeling)
        by_index = {r["index"]: r for r in st.log}
        rec[name] = dict(wall_seconds=round(time.perf_counter() - t0, 3), seconds=round(st.seconds, 3), pm_iterations=pm_it, gc_iterations=5,
                         start=dict(energy=round(st.log[0]["energy"], 1), bad1_all=round(st.log[0]["all"], 3)),
                         energy_after={i: round(by_index[pm_it + i]["energy"], 1) for i in (1, 3, 5)},
                         bad1_all_after_post=round(st.log[-1]["all"], 3))
        _note(scene, name, rec[name])
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true", help="the kernel and whole-call timings only")
    ap.add_argument("--skip-kernels", action="store_true", help="the end-to-end runs only")
    a = ap.parse_args()
    torch = timing.require_gpu("sgm_timing.py")
    import e2e_bench
    from localexpstereo_amd import api, io as lio, stereo, synth
    rec = dict(timings=a.timings)
    if not a.skip_kernels:
        rec["sizes"] = [time_size(torch, api, synth, h, w, a.timings) for h, w in SIZES]
    if not a.skip_runs:
        rec["runs"] = [time_runs(torch, api, stereo, lio, e2e_bench, scene) for scene in ("objects", "three_surfaces")]
    timing.write_record(a.out, rec)


if __name__ == "__main__":
    main()
