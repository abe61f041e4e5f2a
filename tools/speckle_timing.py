#!/usr/bin/env python
"""Timings and quality figures of the speckle filter (csrc/les_speckle.h) on the MI355X -> profiles/speckle.md (summarised in DESIGN 3.4d).

  python tools/speckle_timing.py --out profiles/speckle.md [--json profiles/speckle.json] [--skip-quality] [--skip-timing]
  python tools/speckle_timing.py --calls gc|wta --maps DIR        # only the calls, for a profiler run of their kernels (see below)
  python tools/speckle_timing.py --kernel-stats gc=CSV wta=CSV --json profiles/speckle.json --out profiles/speckle.md   # merge the profiler's figures

Recorded:
  * timing at 1436 x 992 ("objects" scene of tools/e2e_bench.py, MidV3 energy, one view): les_hip_speckle_mask (100, 1.0) on a finished graph-cut map
    (2 PatchMatch + 5 graph-cut iterations: few large components) and on the raw winner-take-all map (very many small ones): the whole call (host
    clock around it: it synchronises, and allocates and frees its 12 B/px of scratch) -- each a group of one of tools/timing.py (which states the
    protocol) after 3 warm-up calls -- next to
    les_hip_calib_copy of the bytes it cannot avoid (16 B/px of labels read, 1 B/px written) and to the one-view les_hip_post_process_speckle
    (mask + dilation + fill + weighted median, windR 20) on the same map.  The two maps are saved under --maps (default: the temporary directory);
  * per kernel: the profiler's job.  `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/speckle_timing.py --calls gc --maps ...` (and
    wta) in runs of their own make 10 calls each of les_hip_speckle_mask and of the one-view post-processing; --kernel-stats reads the
    *_kernel_stats.csv they leave and adds the kernels' average times;
  * quality (unless --skip-quality): bad-1.0 (all / nonocc) of the left view on the cones crop of the tests and the two synthetic 1436 x 992 x 256
    scenes, for one-view wta, sgm and run and two-view run, without the filter and with each (max_size, max_diff) of PAIRS applied to the SAME raw
    maps (HipCostVolumeEnergy.post_process(speckle=): what FastGCStereo(speckle=) returns, tests/test_speckle.py holds the two to each other).
Nothing here is a gate."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import timing  # noqa: E402

H, W, D = 992, 1436, 256
PAIRS = ((100, 1.0), (400, 1.0), (100, 2.0))      # at most three; the first is where the issue starts
TIMED = (100, 1.0)
KERNELS = ("les_disparity_kernel", "les_speckle_tile_kernel", "les_speckle_merge_kernel", "les_speckle_flatten_kernel", "les_speckle_mask_kernel",
           "les_fail_dilate_kernel", "les_nn_fill_kernel", "les_weighted_median_kernel")


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def synthetic(api, lio, stereo, e2e_bench, scene, device, lib, h=H, w=W, d=D):
    imL, imR, gt, volL = e2e_bench.scene_inputs(scene, h, w, d, device)
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.ingest_volumes(volL, None, device=device)
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(d - 1), volumes_on_device=True,
                                shape=(d, h, w), filter=p["filter"], lib=lib)
    st = stereo.FastGCStereo(e, imL, imR, p, device=device, seed=1, evaluate_on_device=True)
    ev = lio.Evaluator(gt, np.ones((h, w), bool), 1.0)
    st.setEvaluator(ev, precision=-1.0)
    stereo._layers(st, (int(w * 0.01), int(w * 0.03), int(w * 0.09)))
    return st, e, ev, (tl, tr)


def cones(api, lio, stereo, device, lib):
    """The cones crop of the tests with the cost-volume energy of its AD-Census volumes (64 disparities, th_col 0.5, windR 6, two layers)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "cones_crop.npz"))
    imL = np.ascontiguousarray(z["imL"])
    h, w = imL.shape[:2]
    imR, gt = np.ascontiguousarray(z["imR_wide"][:, 64:64 + w]), z["gt"].astype(np.float32)
    tl, tr = lio.build_volumes(imL, imR, 64, device=device, lib=lib)
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=6, th_col=0.5, max_disp=63.0, volumes_on_device=True, shape=(64, h, w), lib=lib)
    st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=0.5, windR=6, th_col=0.5), device=device, seed=3, evaluate_on_device=True)
    ev = lio.Evaluator(np.where(gt > 0, gt, np.inf).astype(np.float32), gt > 0, 1.0)
    st.setEvaluator(ev, precision=-1.0)
    e_, r_ = api.PROPOSE_EXPANSION, api.PROPOSE_RANSAC
    st.addLayer(16, [(e_, 1), (r_, 1)])
    st.addLayer(60, [(e_, 1)])
    return st, e, ev, (tl, tr)


def quality(stereo, st, e, ev, name, pm, it):
    """Per method the rates of the unfiltered result and of every pair of PAIRS applied to the same raw maps."""
    rows = []
    methods = (("wta, one view", (0,), lambda v: st.wta(v)), ("sgm, one view", (0,), lambda v: st.sgm(v)),
               (f"run {pm}+{it}, one view", (0,), lambda v: st.run(it, v, pm)), (f"run {pm}+{it}, two views", (0, 1), lambda v: st.run(it, v, pm)))
    for method, views, call in methods:
        st.log = []
        t0 = time.perf_counter()
        lab, raw = call(views)
        sec = time.perf_counter() - t0
        rawR = st.raw_labelings.get(1)
        row = dict(scene=name, method=method, seconds=round(sec, 3), off=[round(x, 3) for x in ev.evaluate(stereo.disparities(lab))])
        for pair in PAIRS:
            t1 = time.perf_counter()
            out = e.post_process_host(raw, rawR, 1.5, st.p["omega"], speckle=pair)[0]
            ms = (time.perf_counter() - t1) * 1e3
            changed = int((out.view(np.uint32) != raw.view(np.uint32)).any(-1).sum())
            row[f"{pair[0]},{pair[1]}"] = dict(rates=[round(x, 3) for x in ev.evaluate(stereo.disparities(out))], changed_vs_raw=changed, host_form_ms=round(ms, 1))
        rows.append(row)
        _note(row)
    return rows


def measure(torch, api, stereo, st, e, maps_dir, n, lib):
    clock = timing.Clock(torch, "cpu", sync=torch.cuda.synchronize)         # the host clock: the calls synchronise themselves
    timed = lambda f, n: timing.spread(timing.time_one(clock, f, n, warm=3), 4)
    P = H * W
    st.log = []
    gc, _ = st.run(5, (0,), 2)
    wta, _ = st.wta((0,))
    os.makedirs(maps_dir, exist_ok=True)
    np.save(os.path.join(maps_dir, "gc.npy"), gc)
    np.save(os.path.join(maps_dir, "wta.npy"), wta)
    np.save(os.path.join(maps_dir, "imL.npy"), np.asarray(st.imL))
    copy = timed(timing.copy_call(api, 17 * P, None, lib=lib, random=False), n)             # (on the default stream)
    rec = dict(shape=[W, H], pair=list(TIMED), calib_copy_17_bytes_per_pixel_ms=copy, maps={})
    for name, lab in (("gc", gc), ("wta", wta)):
        t = torch.from_numpy(np.ascontiguousarray(lab)).cuda()
        mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        root = torch.empty((H, W), dtype=torch.int32, device="cuda")
        size = torch.empty((H, W), dtype=torch.int32, device="cuda")
        call = timed(lambda: e.speckle_mask_ptr(t.data_ptr(), *TIMED, mask.data_ptr()), n)
        e.speckle_mask_ptr(t.data_ptr(), *TIMED, mask.data_ptr(), root.data_ptr(), size.data_ptr())
        work = t.clone()

        def post():
            work.copy_(t)
            e.post_process(work.data_ptr(), None, 1.5, st.p["omega"], speckle=TIMED)
        post_ms = timed(post, max(3, n // 4))
        rec["maps"][name] = dict(components=int(torch.unique(root).numel()), largest=int(size.max()), speckle_pixels=int((mask > 0).sum()),
                                 speckle_mask_call_ms=call, one_view_post_process_call_ms=post_ms)
        _note(name, rec["maps"][name])
    return rec


def calls_only(torch, api, which, maps_dir, n=10):
    """The calls a profiler run watches: n x les_hip_speckle_mask and n x the one-view post-processing on the saved map."""
    lab = np.load(os.path.join(maps_dir, which + ".npy"))
    im = np.load(os.path.join(maps_dir, "imL.npy"))
    e = api.HipCostVolumeEnergy.naive(im, im, windR=20, max_disp=float(D - 1))
    t = torch.from_numpy(np.ascontiguousarray(lab)).cuda()
    mask = torch.empty(lab.shape[:2], dtype=torch.uint8, device="cuda")
    work = t.clone()
    for _ in range(n):
        e.speckle_mask_ptr(t.data_ptr(), *TIMED, mask.data_ptr())
    for _ in range(n):
        work.copy_(t)
        e.post_process(work.data_ptr(), None, 1.5, 10.0, speckle=TIMED)
    e.close()


def read_stats(path):
    """{kernel: (calls, average microseconds)} of a rocprofv3 *_kernel_stats.csv for the kernels of KERNELS."""
    out = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name", "")
        for k in KERNELS:
            if k in name:
                calls, avg = int(r["Calls"]), float(r["AverageNs"]) / 1e3
                c0, a0 = out.get(k, (0, 0.0))
                out[k] = (c0 + calls, (a0 * c0 + avg * calls) / (c0 + calls))
    return {k: dict(calls=c, average_us=round(a, 2)) for k, v in out.items() for c, a in [v]}


def markdown(rec):
    L = ["# Speckle filter: timings and quality on the MI355X", "",
         "Written by `tools/speckle_timing.py`; nothing here is a gate.  Times: host clock around calls that end in a stream synchronise, medians; kernel",
         "times: `rocprofv3 --kernel-trace --stats` in runs of their own.", ""]
    t = rec.get("timing")
    if t:
        L += [f"## `les_hip_speckle_mask` at {t['shape'][0]} x {t['shape'][1]}, (max_size, max_diff) = {tuple(t['pair'])}", "",
              "| map | components | largest | speckle pixels | whole call, ms | one-view post-processing call, ms |", "|---|---|---|---|---|---|"]
        for name, m in t["maps"].items():
            L.append(f"| {name} | {m['components']} | {m['largest']} | {m['speckle_pixels']} | {m['speckle_mask_call_ms']['median']} "
                     f"({m['speckle_mask_call_ms']['min']} .. {m['speckle_mask_call_ms']['max']}) | {m['one_view_post_process_call_ms']['median']} |")
        c = t["calib_copy_17_bytes_per_pixel_ms"]
        L += ["", f"`les_hip_calib_copy` of 17 B/px (16 read, 1 written; enqueue + synchronise): {c['median']} ms ({c['min']} .. {c['max']}).", ""]
    ks = rec.get("kernel_stats")
    if ks:
        L += ["## Kernels (average per launch, microseconds)", "", "| kernel | " + " | ".join(ks) + " |", "|---|" + "---|" * len(ks)]
        for k in KERNELS:
            L.append(f"| `{k}` | " + " | ".join(str(ks[m].get(k, {}).get("average_us", "-")) for m in ks) + " |")
        L.append("")
    q = rec.get("quality")
    if q:
        pairs = [f"{a},{b}" for a, b in PAIRS]
        L += ["## bad-1.0 of the left view, all / nonocc (%), without the filter and with (max_size, max_diff)", "",
              "| scene | method | off | " + " | ".join(f"({p})" for p in pairs) + " |", "|---|---|---|" + "---|" * len(pairs)]
        for r in q:
            L.append(f"| {r['scene']} | {r['method']} | {r['off'][0]:.2f} / {r['off'][1]:.2f} | " +
                     " | ".join(f"{r[p]['rates'][0]:.2f} / {r[p]['rates'][1]:.2f}" for p in pairs) + " |")
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--json")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--maps", default=os.path.join(tempfile.gettempdir(), "speckle_maps"))
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--calls", choices=("gc", "wta"))
    ap.add_argument("--kernel-stats", nargs="*", metavar="MAP=CSV")
    ap.add_argument("--lib", help="a dry run of the script's logic on the simulator build (with --device cpu --small): its figures mean nothing")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--small", action="store_true", help="the cones crop only, no timing")
    a = ap.parse_args()
    rec = json.load(open(a.json)) if a.json and os.path.exists(a.json) else {}
    if a.kernel_stats is not None:
        rec["kernel_stats"] = {kv.split("=", 1)[0]: read_stats(kv.split("=", 1)[1]) for kv in a.kernel_stats}
    else:
        import torch
        import e2e_bench
        from localexpstereo_amd import api, io as lio, stereo
        if a.device == "cuda":
            timing.require_gpu("speckle_timing.py")
        if a.calls:
            calls_only(torch, api, a.calls, a.maps)
            return
        if not a.skip_timing and not a.small:
            st, e, ev, keep = synthetic(api, lio, stereo, e2e_bench, "objects", a.device, a.lib)
            rec["timing"] = measure(torch, api, stereo, st, e, a.maps, a.timings, a.lib)
            e.close()
            del keep
        if not a.skip_quality:
            rows = []
            st, e, ev, keep = cones(api, lio, stereo, a.device, a.lib)
            rows += quality(stereo, st, e, ev, "cones crop", 0 if a.small else 2, 0 if a.small else 5)
            e.close()
            del keep
            for scene in () if a.small else ("objects", "three_surfaces"):
                st, e, ev, keep = synthetic(api, lio, stereo, e2e_bench, scene, a.device, a.lib)
                rows += quality(stereo, st, e, ev, scene, 2, 5)
                e.close()
                del keep
            rec["quality"] = rows
    if a.json:
        timing.write_json(a.json, rec)
    md = markdown(rec)
    print(md)
    if a.out:
        timing.write_text(a.out, md + "\n")


if __name__ == "__main__":
    main()
