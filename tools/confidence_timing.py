#!/usr/bin/env python
"""Timings and quality figures of the confidence map (csrc/les_confidence.h) on the MI355X -> profiles/confidence.md (summarised in DESIGN 3.4e).

  python tools/confidence_timing.py --out profiles/confidence.md [--json profiles/confidence.json] [--skip-quality] [--skip-timing]
  python tools/confidence_timing.py --calls           # only the calls, for a profiler run of their kernels (see below)
  python tools/confidence_timing.py --kernel-stats run1=CSV run2=CSV --json profiles/confidence.json --out profiles/confidence.md

Recorded:
  * timing at 1436 x 992 x 256 ("objects" scene of tools/e2e_bench.py, MidV3 energy, left view), chunk 32: the whole les_hip_confidence call (on the
    view's own WTA map) next to the whole les_hip_wta_labels call -- host clock around enqueue + synchronise, each a group of one of
    tools/timing.py (which states the protocol) after 3 warm-up calls;
  * per kernel: the profiler's job.  `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/confidence_timing.py --calls` makes 10
    calls each of les_hip_wta_labels and les_hip_confidence on one context (the same slabs: both reduce the chunks the batch path writes for the
    same planes); --kernel-stats reads the *_kernel_stats.csv (or *_results.db) of two such runs (the run-to-run spread of the arg-min kernel, the parent's code,
    is the yardstick) and adds the kernels' average times and the step kernels' achieved bytes per second;
  * quality (unless --skip-quality): on the cones crop of the tests and the two synthetic 1436 x 992 x 256 scenes, for one-view wta, sgm and run
    2 + 5 and the two-view run: the sparsification figures of the left view's confidence map (io.sparsification) and bad-1.0 without a mask, with
    speckle=(100, 1.0), with min_confidence at each tau of TAUS, and with both, all applied to the SAME raw maps and confidence maps
    (HipCostVolumeEnergy.post_process_host(fail=): what FastGCStereo(min_confidence=) returns, tests/test_confidence.py holds the two to each other).
Nothing here is a gate."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import speckle_timing as spk      # noqa: E402  (the scenes)
import timing                     # noqa: E402

H, W, D, CHUNK = spk.H, spk.W, spk.D, 32
TAUS = (0.02, 0.05, 0.1)
SPECKLE = (100, 1.0)
KERNELS = ("les_slab_argmin_kernel", "les_slab_confidence_kernel", "les_slab_argmin_finish_kernel", "les_slab_confidence_finish_kernel")
_note = spk._note


def measure(torch, st, e, n):
    clock = timing.Clock(torch, "cpu", sync=torch.cuda.synchronize)         # the host clock around enqueue + synchronise
    timed = lambda f: timing.spread(timing.time_one(clock, f, n, warm=3), 4)
    lab, cost = e.wta_labels(0, chunk=CHUNK)
    conf = torch.empty((H, W), dtype=torch.float32, device="cuda")
    scale = float(e.raw_cost_max())
    wta = timed(lambda: e.wta_labels(0, CHUNK, True, lab.data_ptr(), cost.data_ptr()))
    cf = timed(lambda: e.confidence_ptr(0, lab.data_ptr(), CHUNK, 1.0, scale, conf.data_ptr()))
    rec = dict(shape=[W, H, D], chunk=CHUNK, wta_labels_call_ms=wta, confidence_call_ms=cf)
    _note(rec)
    return rec


def calls_only(torch, e, n=10):
    """The calls a profiler run watches: n x les_hip_wta_labels and n x les_hip_confidence on one context, chunk 32."""
    lab, cost = e.wta_labels(0, chunk=CHUNK)
    conf = torch.empty((H, W), dtype=torch.float32, device="cuda")
    scale = float(e.raw_cost_max())
    for _ in range(n):
        e.wta_labels(0, CHUNK, True, lab.data_ptr(), cost.data_ptr())
    for _ in range(n):
        e.confidence_ptr(0, lab.data_ptr(), CHUNK, 1.0, scale, conf.data_ptr())
    torch.cuda.synchronize()


def read_stats(path):
    """{kernel: calls, average microseconds} of a rocprofv3 run for the kernels of KERNELS (the two instantiations of a step kernel are one entry):
    a *_kernel_stats.csv, or the *_results.db (a rocpd SQLite database, its `kernels` view) that newer rocprofv3 writes by default."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = [dict(Name=n, Calls=c, AverageNs=a) for n, c, a in db.execute('select name, count(*), avg("end" - start) from kernels group by name')]
    else:
        rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r.get("Name", "")
        for k in sorted(KERNELS, key=len, reverse=True):          # (the finish kernels' names contain the step kernels')
            if k in name:
                calls, avg = int(r["Calls"]), float(r["AverageNs"]) / 1e3
                c0, a0 = out.get(k, (0, 0.0))
                out[k] = (c0 + calls, (a0 * c0 + avg * calls) / (c0 + calls))
                break
    return {k: dict(calls=c, average_us=round(a, 2)) for k, (c, a) in out.items()}


def quality(lio, stereo, st, e, ev, gt, name, pm, it):
    rows = []
    st.with_confidence = True
    methods = (("wta, one view", (0,), lambda v: st.wta(v, post_process=False)), ("sgm, one view", (0,), lambda v: st.sgm(v, post_process=False)),
               (f"run {pm}+{it}, one view", (0,), lambda v: st.run(it, v, pm)), (f"run {pm}+{it}, two views", (0, 1), lambda v: st.run(it, v, pm)))
    rate = lambda lab: round(ev.evaluate(stereo.disparities(lab))[0], 3)
    for method, views, call in methods:
        st.log = []
        lab, raw = call(views)
        rawR, conf = st.raw_labelings.get(1), st.confidences
        post = lambda **kw: e.post_process_host(raw, rawR, 1.5, st.p["omega"], **kw)[0]
        sp = lio.sparsification(stereo.disparities(raw), gt, conf[0], threshold=1.0)
        row = dict(scene=name, method=method, sparsification={k: round(v, 5) for k, v in sp.items()}, raw=rate(raw), off=rate(lab if len(views) == 2 else raw),
                   speckle=rate(post(speckle=SPECKLE)), tau={})
        for tau in TAUS:
            low = tuple(conf[m] < np.float32(tau) if m in conf else None for m in (0, 1))
            row["tau"][str(tau)] = dict(alone=rate(post(fail=low)), with_speckle=rate(post(fail=low, speckle=SPECKLE)), masked_percent=round(100.0 * float(low[0].mean()), 2))
        rows.append(row)
        _note(row)
    return rows


def markdown(rec):
    L = ["# Confidence map: timings and quality on the MI355X", "",
         "Written by `tools/confidence_timing.py`; nothing here is a gate.  Call times: host clock around enqueue + stream synchronise, medians; kernel",
         "times: `rocprofv3 --kernel-trace --stats` in runs of their own.", ""]
    t = rec.get("timing")
    if t:
        w, c = t["wta_labels_call_ms"], t["confidence_call_ms"]
        L += [f"## Whole calls at {t['shape'][0]} x {t['shape'][1]} x {t['shape'][2]}, chunk {t['chunk']}, left view", "",
              "| call | ms, median (min .. max) |", "|---|---|",
              f"| `les_hip_wta_labels` | {w['median']} ({w['min']} .. {w['max']}) |", f"| `les_hip_confidence` | {c['median']} ({c['min']} .. {c['max']}) |", ""]
    ks = rec.get("kernel_stats")
    if ks:
        P = H * W
        step_bytes = {"les_slab_argmin_kernel": CHUNK * P * 4 + 2 * 20 * P, "les_slab_confidence_kernel": CHUNK * P * 4 + 2 * 16 * P}
        L += [f"## Kernels (average per launch, microseconds; the step kernels consume {CHUNK} slabs of {W} x {H} per launch)", "",
              "| kernel | " + " | ".join(ks) + " |", "|---|" + "---|" * len(ks)]
        for k in KERNELS:
            L.append(f"| `{k}` | " + " | ".join(str(ks[m].get(k, {}).get("average_us", "-")) for m in ks) + " |")
        L += ["", "Achieved TB/s of the step kernels (slab bytes + state in and out, the first chunk's skipped state read counted as read):", "",
              "| kernel | " + " | ".join(ks) + " |", "|---|" + "---|" * len(ks)]
        for k, b in step_bytes.items():
            L.append(f"| `{k}` | " + " | ".join(f"{b / (ks[m][k]['average_us'] * 1e-6) / 1e12:.2f}" if k in ks[m] else "-" for m in ks) + " |")
        L += ["", "(Each chunk of slabs was written by the batch kernel just before its reduction: part of it is served from the last-level cache.)"]
        both = [m for m in ks if all(k in ks[m] for k in step_bytes)]
        if both:
            L += ["", "Step kernel of the confidence / arg-min step kernel, same run: " + ", ".join(
                f"{m}: {ks[m]['les_slab_confidence_kernel']['average_us'] / ks[m]['les_slab_argmin_kernel']['average_us']:.3f}" for m in both) + "."]
        L.append("")
    q = rec.get("quality")
    if q:
        L += ["## Sparsification of the left view's raw map by its confidence (bad-1.0 as a fraction)", "", "| scene | method | bad | auc | auc_optimal | auc / bad |",
              "|---|---|---|---|---|---|"]
        for r in q:
            s = r["sparsification"]
            L.append(f"| {r['scene']} | {r['method']} | {s['bad']:.4f} | {s['auc']:.4f} | {s['auc_optimal']:.4f} | {s['auc'] / s['bad'] if s['bad'] else float('nan'):.3f} |")
        taus = [str(t_) for t_ in TAUS]
        L += ["", f"## bad-1.0 of the left view, all (%): no mask, speckle {SPECKLE}, `min_confidence` alone / with that speckle filter (masked % of the pixels)", "",
              "| scene | method | raw | off | speckle | " + " | ".join(f"tau {t_}" for t_ in taus) + " |", "|---|---|---|---|---|" + "---|" * len(taus)]
        for r in q:
            L.append(f"| {r['scene']} | {r['method']} | {r['raw']:.2f} | {r['off']:.2f} | {r['speckle']:.2f} | " +
                     " | ".join(f"{r['tau'][t_]['alone']:.2f} / {r['tau'][t_]['with_speckle']:.2f} ({r['tau'][t_]['masked_percent']:.1f})" for t_ in taus) + " |")
        L += ["", "raw: the map before any post-processing; off: what the call returns without the keywords (one view: the raw map; two views: the left-right check)."]
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--json")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--kernel-stats", nargs="*", metavar="RUN=CSV_OR_DB")
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
            timing.require_gpu("confidence_timing.py")
        if a.calls or (not a.skip_timing and not a.small):
            st, e, ev, keep = spk.synthetic(api, lio, stereo, e2e_bench, "objects", a.device, a.lib)
            if a.calls:
                calls_only(torch, e)
                e.close()
                return
            rec["timing"] = measure(torch, st, e, a.timings)
            e.close()
            del keep
        if not a.skip_quality:
            rows = []
            st, e, ev, keep = spk.cones(api, lio, stereo, a.device, a.lib)
            rows += quality(lio, stereo, st, e, ev, ev.gt, "cones crop", 0 if a.small else 2, 0 if a.small else 5)
            e.close()
            del keep
            for scene in () if a.small else ("objects", "three_surfaces"):
                st, e, ev, keep = spk.synthetic(api, lio, stereo, e2e_bench, scene, a.device, a.lib)
                rows += quality(lio, stereo, st, e, ev, ev.gt, scene, 2, 5)
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
