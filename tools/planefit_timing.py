#!/usr/bin/env python
"""Timings of the plane fit (csrc/les_planefit.h) on the MI355X -> profiles/planefit_timing.json (summarised in DESIGN 3.2h).

  python tools/planefit_timing.py [--out profiles/planefit_timing.json] [--skip-runs] [--skip-kernels]

Recorded:
  * kernel: les_plane_fit_kernel at 1436 x 992 and 1500 x 1000 for radius 5, 10 and 15, from a label map and from a disparity map (slanted planes in
    cells of 48 pixels, 2 % isolated outliers, 1 % non-finite; the default parameters; fallback and kind map given), next to the kernel's issue floor
    -- LANE_OPS_PER_TAP x (2 r + 1)^2 x pixels / 3.93e13 lane-operations/s, counted from the compiled tap loop -- and to les_hip_calib_copy_wide of
    the bytes the call reads and writes; each a group of one of tools/timing.py (which states the protocol) after 3 warm-up calls;
  * runs (unless --skip-runs): the two synthetic scenes of tools/e2e_bench.py at 1436 x 992 x 256, two views, MidV3 energy and layers, no PatchMatch
    iteration and 5 graph-cut iterations from labeling="wta" and from labeling="wta+planes": the Evaluator log, the fusion's report, wall clock.
Nothing here is a gate."""
import argparse
import json
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
RADII = (5, 10, 15)
LANE_OPS_PER_TAP = 29.5        # VALU instructions of one taken tap of the compiled loop (DESIGN 3.2h lists them)
LANE_OPS_PER_SECOND = 3.93e13


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def test_map(h, w, seed):
    rng = np.random.default_rng(seed)
    cell = 48
    hb, wb = -(-h // cell), -(-w // cell)
    pl = np.stack([rng.uniform(-0.3, 0.3, (hb, wb)), rng.uniform(-0.3, 0.3, (hb, wb)), rng.uniform(20, 200, (hb, wb)), np.zeros((hb, wb))], -1)
    lab = np.repeat(np.repeat(pl, cell, 0), cell, 1)[:h, :w].astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    lab[..., 2] -= (lab[..., 0] * ((xs // cell) * cell + cell // 2) + lab[..., 1] * ((ys // cell) * cell + cell // 2)).astype(np.float32)
    u = rng.uniform(0, 1, (h, w))
    lab[u < 0.02] = 0
    lab[..., 2][u < 0.02] = rng.uniform(0, 255, int((u < 0.02).sum())).astype(np.float32)
    lab[..., 2][(u >= 0.02) & (u < 0.03)] = np.nan
    return np.ascontiguousarray(lab)


def time_size(torch, api, synth, h, w, timings):
    P = h * w
    guide = synth.make_guide(h, w, 1234)
    e = api.HipCostVolumeEnergy.naive(guide, guide, windR=0, max_disp=float(D - 1), filter="")
    stream = torch.cuda.current_stream()
    e.set_stream(stream.cuda_stream)
    lab = torch.from_numpy(test_map(h, w, 7)).cuda()
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    disp = ((lab[..., 0] * xs + lab[..., 1] * ys) + lab[..., 2]).contiguous()
    fb = lab.clone()
    out, kind = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w), device="cuda", dtype=torch.uint8)
    rec = dict(shape=[w, h], kernels=[])
    clock = timing.Clock(torch, "cuda")
    one = lambda f: timing.spread(timing.time_one(clock, f, timings, warm=3), 4)
    for form in ("labels", "disparities"):
        bytes_moved = P * ((16 if form == "labels" else 4) + 4 + 16 + 16 + 1)            # the input map, the guide, the fallback; the labels and the kind map
        copy = one(timing.copy_call(api, bytes_moved, stream.cuda_stream, wide=True, random=False))
        for r in RADII:
            args = (0, lab.data_ptr() if form == "labels" else None, None if form == "labels" else disp.data_ptr(), fb.data_ptr(), out.data_ptr(), kind.data_ptr())
            ms = one(lambda: e.fit_planes_ptr(*args, radius=r))
            floor = LANE_OPS_PER_TAP * (2 * r + 1) ** 2 * P / LANE_OPS_PER_SECOND * 1e3
            k = torch.bincount(kind.flatten().to(torch.int64), minlength=3).tolist()
            row = dict(form=form, radius=r, ms=ms, issue_floor_ms=round(floor, 4), over_issue_floor=round(ms["median"] / floor, 3), bytes_moved=bytes_moved,
                       copy_wide_ms=copy, over_copy=round(ms["median"] / copy["median"], 3), kind_pixels=k)
            rec["kernels"].append(row)
            _note(rec["shape"], row)
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

    def rows(st):
        return [dict(index=r["index"], seconds=round(r["time"], 3), energy=round(r["energy"], 1), bad1_all=round(r["all"], 3)) for r in st.log]
    rec = dict(scene=scene, shape=[w, h, D])
    driver().wta((0, 1))                                        # (warms the context's workspace up)
    for name, labeling in (("wta_start", "wta"), ("wta_planes_start", "wta+planes")):
        st = driver()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run(5, (0, 1), 0, labeling=labeling)
        rec[name] = dict(wall_seconds=round(time.perf_counter() - t0, 3), seconds=round(st.seconds, 3), pm_iterations=0, gc_iterations=5, log=rows(st))
        if st.slant_stats:
            rec[name]["fusion"] = {f"view{m}": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items()} for m, s in st.slant_stats.items()}
        _note(scene, name, rec[name]["seconds"], "s, energies", [r["energy"] for r in rec[name]["log"]], "bad1", rec[name]["log"][-1]["bad1_all"], rec[name].get("fusion"))
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true", help="the kernel timings only")
    ap.add_argument("--skip-kernels", action="store_true", help="the end-to-end runs only")
    a = ap.parse_args()
    torch = timing.require_gpu("planefit_timing.py")
    import e2e_bench
    from localexpstereo_amd import api, io as lio, stereo, synth
    rec = dict(timings=a.timings, lane_ops_per_tap=LANE_OPS_PER_TAP)
    if a.out and os.path.exists(a.out):                        # (the two halves may be taken in two runs)
        rec.update({k: v for k, v in json.load(open(a.out)).items() if k in ("sizes", "runs")})
    if not a.skip_kernels:
        rec["sizes"] = [time_size(torch, api, synth, h, w, a.timings) for h, w in SIZES]
    if not a.skip_runs:
        rec["runs"] = [time_runs(torch, api, stereo, lio, e2e_bench, scene) for scene in ("objects", "three_surfaces")]
    timing.write_record(a.out, rec)


if __name__ == "__main__":
    main()
