#!/usr/bin/env python3
"""Times the warm start (the unary cost of every pixel's own label) two ways on one GPU, alternating, in one command:

  old   PMRunner.init_from_labels of an EARLIER commit of this repository, exported with `git archive <commit> | tar -x -C <dir>` and built there
        (one job per pixel on the strip / march kernels, job tables built on the host per band of 64 rows);
  new   this tree's dense pass (les_hip_unary_labels, csrc/les_dense.h).

Two cases: the Adirondack-H shape 1436 x 992 x 256 (synthetic volume generated on the device, windR 20, guided filter, linear interpolation) and
the image-based energy on cones (450 x 375, windR 20).  Same seeded label map (a distinct plane per pixel, slants up to 0.3) on both sides.
Each side lives in its own child process (the two trees hold a package of the same name); the parent process tells them in turn to run one
timed call: warm-up call first, device-synchronised wall clock, median of --reps.  --band: time both on the band of 128 rows through the
middle plus the top 32 rows instead of the whole map (for an old side that needs more than a minute per map).

  python tools/dense_unary_bench.py --old-root <dir> [--reps 5] [--band] [--out profiles/dense_unary.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("adirondack", "cones")


def label_map(H, W, D, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W, 4), np.float32)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    lab[..., 0] = rng.uniform(-0.3, 0.3, (H, W))
    lab[..., 1] = rng.uniform(-0.3, 0.3, (H, W))
    lab[..., 2] = rng.uniform(1, D - 2, (H, W)).astype(np.float32) - lab[..., 0] * xs - lab[..., 1] * ys
    return lab


def bands(H, band):
    return [(0, 32), (H // 2 - 64, H // 2 + 64)] if band else [(0, H)]


def worker(root, side, band):
    """Child process: builds both cases from the tree at `root`, then serves 'run <case>' lines with one timed call each."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from localexpstereo_amd import api, io as lio, pm, synth
    dev = torch.device("cuda")
    ctx = {}
    H, W, D = 992, 1436, 256
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    vol = torch.rand((D, H, W), device="cuda", dtype=torch.float32, generator=gen)
    e = api.HipCostVolumeEnergy(synth.make_guide(H, W, 1234), None, vol.data_ptr(), None, volumes_on_device=True, shape=(D, H, W), max_disp=D - 1)
    ctx["adirondack"] = (e, pm.PMRunner(e, (1000,), [[(api.PROPOSE_EXPANSION, 1)]], seed=1, device="cuda"), label_map(H, W, D, 11), D)
    g = os.path.join(ROOT, "tests", "golden", "cones")
    imL, imR = lio._imread_bgr(os.path.join(g, "imL.png")), lio._imread_bgr(os.path.join(g, "imR.png"))
    e2 = api.HipCostVolumeEnergy.naive(imL, imR, max_disp=63.0)
    ctx["cones"] = (e2, pm.PMRunner(e2, (400,), [[(api.PROPOSE_EXPANSION, 1)]], seed=1, device="cuda"), label_map(imL.shape[0], imL.shape[1], 64, 12), 64)

    def jobs_route(r, ya0, ya1, rows_per_launch=64):
        # the old side's loop (PMRunner.init_from_labels) restricted to rows [ya0, ya1)
        R, W_, H_ = r.e.params.windR, r.W, r.H
        xs = np.arange(W_, dtype=np.int32)
        x0, x1 = np.maximum(xs - R, 0), np.minimum(xs + R + 1, W_)
        for ya in range(ya0, ya1, rows_per_launch):
            yb = min(ya1, ya + rows_per_launch)
            ys = np.arange(ya, yb, dtype=np.int32)
            y0, y1 = np.maximum(ys - R, 0), np.minimum(ys + R + 1, H_)
            fr = np.stack([np.broadcast_to(x0, (yb - ya, W_)), np.broadcast_to(y0[:, None], (yb - ya, W_)),
                           np.broadcast_to(x1 - x0, (yb - ya, W_)), np.broadcast_to((y1 - y0)[:, None], (yb - ya, W_))], -1).reshape(-1, 4)
            tr = np.stack([np.broadcast_to(xs, (yb - ya, W_)), np.broadcast_to(ys[:, None], (yb - ya, W_)),
                           np.ones((yb - ya, W_), np.int32), np.ones((yb - ya, W_), np.int32)], -1).reshape(-1, 4)
            b = api.Batch(r.e, np.ascontiguousarray(fr, np.int32), np.ascontiguousarray(tr, np.int32))
            b.run(r.labels[ya:yb].data_ptr(), r.cur.data_ptr(), mode=r.mode, check=True, planes_on_device=True)
            r._sync()
            b.destroy()

    def one(case):
        e_, r, lab, _ = ctx[case]
        torch.cuda.synchronize()
        t = time.perf_counter()
        if not band:
            r.init_from_labels(lab)
        else:
            r.labels.copy_(torch.as_tensor(lab).to(dev))
            for y0, y1 in bands(r.H, True):
                if side == "old":
                    jobs_route(r, y0, y1)
                else:
                    e_.unary_labels(r.labels.data_ptr(), r.cur.data_ptr(), mode=0, region=(0, y0, r.W, y1 - y0), check=True)
            r._sync()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "run":
            print(json.dumps(dict(seconds=one(cmd[1]))), flush=True)
        elif cmd[0] == "dump":          # the cost map of the last call (rows of the bands), for the cross-check of the two sides
            _, r, _, _ = ctx[cmd[1]]
            rows = np.concatenate([np.arange(a, b) for a, b in bands(r.H, band)])
            np.save(cmd[2], r.cur.cpu().numpy()[rows])
            print(json.dumps(dict(saved=cmd[2])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-root")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a.root, a.worker, a.band)
        return
    if not a.old_root:
        ap.error("--old-root: the tree of the earlier commit (git archive <commit> | tar -x -C <dir>, then build it there)")
    import numpy as np
    import tempfile
    procs = {}
    for side, root in (("old", os.path.abspath(a.old_root)), ("new", ROOT)):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--root", root] + (["--band"] if a.band else [])
        procs[side] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        assert procs[side].stdout.readline().strip() == "ready", f"the {side} side did not start"

    def ask(side, line):
        procs[side].stdin.write(line + "\n")
        procs[side].stdin.flush()
        return json.loads(procs[side].stdout.readline())
    result = dict(band=a.band, reps=a.reps, cases={})
    tmp = tempfile.mkdtemp()
    try:
        for case in CASES:
            times = {"old": [], "new": []}
            for side in ("old", "new"):
                ask(side, f"run {case}")                        # warm-up
            for _ in range(a.reps):
                for side in ("old", "new"):                     # alternating
                    times[side].append(ask(side, f"run {case}")["seconds"])
            maps = {}
            for side in ("old", "new"):
                f = os.path.join(tmp, f"{case}_{side}.npy")
                ask(side, f"dump {case} {f}")
                maps[side] = np.load(f)
            same = maps["old"] == np.float32(1e6)
            assert np.array_equal(same, maps["new"] == np.float32(1e6)), "the two sides disagree on invalid labels"
            diff = float(np.abs(maps["old"][~same].astype(np.float64) - maps["new"][~same]).max())
            row = {}
            for side in ("old", "new"):
                t = sorted(times[side])
                row[side] = dict(median_s=statistics.median(t), min_s=t[0], max_s=t[-1])
            row["speedup"] = row["old"]["median_s"] / row["new"]["median_s"]
            row["max_abs_diff"] = diff
            row["pixels"] = int(maps["new"].size)
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
