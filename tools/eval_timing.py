#!/usr/bin/env python
"""Timings of the device-side Evaluator (csrc/les_eval.h) on the MI355X -> profiles/eval_timing.json (summarised in DESIGN 3.6).

  python tools/eval_timing.py routes   [--out f.json]   one evaluation by the device route and by the default host route (synchronise, two D2H
                                                        copies, host sums), alternating, host clock around a synchronise, at 1500 x 1000 and
                                                        1436 x 992; and the device time per evaluation from events around 200 enqueued ones
  python tools/eval_timing.py inner    [--out f.json]   "objects", one view, 2 + 5 iterations, inner_loop_log on against off, alternating: seconds,
                                                        rows logged, and the count of synchronising calls the driver made
  python tools/eval_timing.py kernels                   the workload for `rocprofv3 --kernel-trace --stats -- python tools/eval_timing.py kernels`
                                                        (a run of its own): 100 evaluations per shape, region energies of a lock-step per layer
  python tools/eval_timing.py stats <kernel_stats.csv> [--out f.json]    the eval / region kernels' rows of that run, per-call averages

tools/timing.py states the protocol; routes: the two routes are one group (one warm-up call each), the back-to-back device route a group of one
without a warm-up, both on the host clock, and the enqueued evaluations 5 bursts of 200.
The traffic floor of one evaluation is 29 B per pixel (16 label + 4 cost + 4 guide + 4 ground truth + 1 mask) over the peak HBM rate."""
import argparse
import csv
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import timing  # noqa: E402

SHAPES = ((1000, 1500), (992, 1436))
PW = dict(lambda_=0.5, th_smooth=1.0, omega=10.0, epsilon=0.01)
PEAK_HBM = 8.0e12


def _scene(H, W, seed=1):
    import torch
    from localexpstereo_amd import api
    rng = np.random.default_rng(seed)
    imL = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    e = api.HipCostVolumeEnergy.naive(imL, imL, windR=0, max_disp=255.0, filter="")
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    lab = np.zeros((H, W, 4), np.float32)
    lab[..., :2] = rng.uniform(-0.3, 0.3, (H, W, 2))
    lab[..., 2] = rng.uniform(0, 200, (H, W))
    cost = rng.uniform(0, 0.5, (H, W)).astype(np.float32)
    gt = rng.uniform(1, 200, (H, W)).astype(np.float32)
    return e, imL, torch.from_numpy(lab).cuda(), torch.from_numpy(cost).cuda(), gt


def spread(v):
    return timing.spread(v, samples=True)


def routes(repeats=15):
    import torch
    from localexpstereo_amd import api, gc as lgc, io as lio
    out = {}
    for H, W in SHAPES:
        e, imL, lab, cost, gt = _scene(H, W)
        ev = api.DeviceEvaluator(e, dispGT=gt, nonocc=np.ones((H, W), bool), error_threshold=1.0, max_rows=4096)
        g = lgc.GraphCut(imL, None, **PW)
        ref = lio.Evaluator(gt, np.ones((H, W), bool), 1.0)
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")

        def device_route():
            ev.evaluate(lab.data_ptr(), cost.data_ptr(), mode=0, index=0, **PW)
            return ev.rows()[-1]

        def host_route():            # stereo.FastGCStereo._evaluate_body with a host context (a graph-cut row)
            disp = (lab[..., 0] * xs + lab[..., 1] * ys + lab[..., 2]).cpu().numpy()
            e.synchronize()
            g.labels[0][...] = lab.cpu().numpy()
            g.costs[0][...] = cost.cpu().numpy()
            return g.data_cost(0), g.smoothness_cost(0), ref.evaluate(disp)

        host = timing.Clock(torch, "cpu", sync=torch.cuda.synchronize)
        t, _ = timing.time_calls(host, dict(device=device_route, host=host_route), repeats, warm=1)
        tb = timing.time_one(host, device_route, repeats, warm=0)        # the device route alone, back to back (no idle GPU in between)
        # device time of an enqueued evaluation: events around 200 of them (two kernels each, back to back on one stream)
        k = itertools.count()
        enqueue = lambda: ev.evaluate(lab.data_ptr(), cost.data_ptr(), mode=0, index=next(k) % 200, **PW)
        per = 1e3 * np.asarray(timing.time_calls(timing.Clock(torch, "cuda"), dict(enqueue=enqueue), 0, warm=0, burst=200, burst_rounds=5)[1]["enqueue"])
        floor_us = 29.0 * H * W / PEAK_HBM * 1e6
        out[f"{W}x{H}"] = dict(device_route_ms=spread(t["device"]), host_route_ms=spread(t["host"]), device_route_back_to_back_ms=spread(tb), enqueued_evaluation_us=spread(per), traffic_floor_us=floor_us,
                               enqueued_over_floor=float(np.median(per)) / floor_us)
        ev.close(); g.close(); e.close()
    return out


class _SyncCounter:
    """Counts the calls through which the Python driver waits for the GPU: les_hip_synchronize, the evaluator's read-out, Tensor.item / .cpu of
    a device tensor, torch.cuda.synchronize, Stream.synchronize."""

    def __enter__(self):
        import torch
        from localexpstereo_amd import api
        self.n, self.saved = 0, []

        def wrap(owner, name, only_cuda=False):
            orig = getattr(owner, name)

            def f(*a, **k):
                if not only_cuda or a[0].is_cuda:
                    self.n += 1
                return orig(*a, **k)
            self.saved.append((owner, name, orig))
            setattr(owner, name, f)
        wrap(api.HipCostVolumeEnergy, "synchronize")
        wrap(api.DeviceEvaluator, "rows")
        wrap(api.Batch, "solve_graphs_tiled")
        wrap(torch.Tensor, "item", True)
        wrap(torch.Tensor, "cpu", True)
        wrap(torch.cuda, "synchronize")
        wrap(torch.cuda.Stream, "synchronize")
        return self

    def __exit__(self, *exc):
        for owner, name, orig in self.saved:
            setattr(owner, name, orig)


def inner(repeats=3):
    import e2e_bench
    from localexpstereo_amd import stereo
    H, W, D = 992, 1436, 256
    imL, imR, gt, volL = e2e_bench.scene_inputs("objects", H, W, D, "cuda")
    data = dict(imL=imL, imR=imR, dispGT=gt, nonocc=np.ones((H, W), bool), ndisp=D, gt_prec=-1.0)

    def run(**opts):
        with _SyncCounter() as sc:
            st, lab, raw = stereo.MidV3(data, volL, None, iterations=5, pmIterations=2, doDual=False, smooth_weight=0.5, mc_threshold=0.5, error_threshold=1.0,
                                        device="cuda", **opts)
        return st, sc.n, lab
    run()
    rec = dict(off=[], on=[], device_rows=[])
    syncs, rows, same = {}, 0, True
    for _ in range(repeats):
        for name, opts in (("off", {}), ("device_rows", dict(evaluate_on_device=True)), ("on", dict(inner_loop_log=True))):
            st, n, lab = run(**opts)
            rec[name].append(st.seconds)
            syncs[name] = n
            if name == "off":
                ref = lab
            else:
                same = same and ref.tobytes() == lab.tobytes()
            if name == "on":
                rows = len(st.inner_log)
    return dict(shape=f"{W}x{H}", iterations="2 + 5", seconds_log_off=spread(rec["off"]), seconds_rows_on_device=spread(rec["device_rows"]),
                seconds_inner_log_on=spread(rec["on"]), inner_rows=rows, synchronising_calls=syncs, labels_identical=same)


def kernels():
    import torch
    from localexpstereo_amd import api, pm
    for H, W in SHAPES:
        e, imL, lab, cost, gt = _scene(H, W)
        ev = api.DeviceEvaluator(e, dispGT=gt, nonocc=np.ones((H, W), bool), error_threshold=1.0, max_rows=128)
        for k in range(100):
            ev.evaluate(lab.data_ptr(), cost.data_ptr(), mode=0, index=k, **PW)
        ev.rows()
        if (H, W) == SHAPES[1]:          # the region energies of one lock-step of a set of each MidV3 layer
            for unit in (int(W * 0.01), int(W * 0.03), int(W * 0.09)):
                units, shared, filt, sets = pm.layer_geometry(W, H, 0, unit)
                b = api.Batch(e, filt[sets[0]], shared[sets[0]])
                out = torch.zeros(len(sets[0]), dtype=torch.float64, device="cuda")
                for _ in range(10):
                    b.region_energy(lab.data_ptr(), cost.data_ptr(), out.data_ptr(), mode=0, **PW)
                torch.cuda.synchronize()
                b.destroy()
        ev.close(); e.close()


def stats(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "les_eval" in name or "les_region_energy" in name:
            rows[name.split("(")[0]] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("routes", "inner", "kernels", "stats"))
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels()
        return
    rec = {a.what: routes() if a.what == "routes" else inner() if a.what == "inner" else stats(a.csv)}
    print(json.dumps(rec, indent=1))
    if a.out:                                                       # (the file keeps the groups of earlier runs)
        timing.write_json(a.out, dict(json.load(open(a.out)) if os.path.exists(a.out) else {}, **rec))


if __name__ == "__main__":
    main()
