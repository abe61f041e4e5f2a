#!/usr/bin/env python
"""Timings of the 3D reconstruction (csrc/les_reproject.h) on the MI355X -> profiles/reproject_timing.json (summarised in DESIGN 3.4f).

  python tools/reproject_timing.py --out profiles/reproject_timing.json
  python tools/reproject_timing.py --calls                 # only the calls, for a profiler run of their kernels (see below)
  python tools/reproject_timing.py --kernel-trace CSV --out profiles/reproject_timing.json     # merge the profiler's per-kernel figures

Recorded, at 1436 x 992 and 1500 x 1000, for slanted planes in 48-pixel cells and for the same map with 10 % of the pixels invalid (NaN):
  * les_hip_reproject (one kernel) and les_hip_mesh (four launches together): each a group of one of tools/timing.py (which states the protocol),
    20 timings after 3 warm-up calls, the events recorded on the stream the context launches on, each next to les_hip_calib_copy_wide over
    the bytes the call reads and writes (counted from the shapes and the mesh's own counts: bytes_moved below);
  * the whole FastGCStereo.reconstruct call (host clock: it ends with the results on the host);
  * each of the four mesh launches: the profiler's job.  `rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python
    tools/reproject_timing.py --calls` in a run of its own makes 20 calls per shape and input; --kernel-trace reads the *_kernel_trace.csv it
    leaves and adds the medians per kernel and shape (the dispatches are told apart by their grid).
--lib PATH --device cpu rehearses the script on the simulator build with the host clock; such a record says so and is no measurement.
Nothing here is a gate."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import timing  # noqa: E402

SHAPES = ((992, 1436), (1000, 1500))
CELL = 48
CALIB = dict(f=3997.684, cx=700.0, cy=500.0, doffs=131.111, baseline=193.001)
KERNELS = ("les_reproject_kernel", "les_mesh_count_kernel", "les_mesh_scan_kernel", "les_mesh_vertices_kernel", "les_mesh_triangles_kernel")
N = 20


def make_labels(H, W, invalid, seed=5):
    """Slanted planes, one per CELL x CELL cell, disparities 20 .. 200 at the cell; invalid: that share of the pixels gets a NaN offset."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W, 4), np.float32)
    for y0 in range(0, H, CELL):
        for x0 in range(0, W, CELL):
            a, b = rng.uniform(-0.3, 0.3, 2)
            lab[y0:y0 + CELL, x0:x0 + CELL, :3] = (a, b, rng.uniform(20, 200) - a * x0 - b * y0)
    if invalid > 0:
        lab[rng.random((H, W)) < invalid, 2] = np.nan
    return lab


def bytes_moved(P, nv, nt):
    """The bytes each call cannot avoid: labels 16 B/px, masks 1 B/px, points and normals 12 B/px each, 4 B per index."""
    return dict(reproject=P * (16 + 12 + 12 + 1),
                mesh_count=P * (16 + 1), mesh_vertices=P * (1 + 4) + nv * 4, mesh_triangles=P * (16 + 1 + 4) + nt * 12,
                mesh=P * (16 + 1) + P * (1 + 4) + nv * 4 + P * (16 + 1 + 4) + nt * 12)


def context(api, H, W, lib):
    im = np.full((H, W, 3), 90, np.uint8)
    im[::7, ::5] = (10, 200, 90)
    vol = np.zeros((2, H, W), np.float32)
    return api.HipCostVolumeEnergy(im, im, vol, vol, windR=2, eps=1.0, th_col=0.5, lib=lib, filter=""), im


def buffers(torch, e, lab, device):
    H, W = lab.shape[:2]
    t = torch.from_numpy(lab).to(device)
    o = dict(lab=t, points=torch.empty((H, W, 3), dtype=torch.float32, device=device), normals=torch.empty((H, W, 3), dtype=torch.float32, device=device),
             valid=torch.empty((H, W), dtype=torch.uint8, device=device), vi=torch.empty((H, W), dtype=torch.int32, device=device),
             vpix=torch.empty((H * W,), dtype=torch.int32, device=device), tri=torch.empty((2 * (H - 1) * (W - 1), 3), dtype=torch.int32, device=device),
             counts=torch.zeros((2,), dtype=torch.int64, device=device))
    if device != "cpu":
        torch.cuda.synchronize()
    return o


def calls(api, e, b, calib, jump):
    rp = lambda: e.reproject_ptr(0, b["lab"].data_ptr(), None, calib, None, b["points"].data_ptr(), b["normals"].data_ptr(), b["valid"].data_ptr())
    ms = lambda: e.mesh_ptr(0, b["lab"].data_ptr(), b["valid"].data_ptr(), jump, b["vi"].data_ptr(), b["vpix"].data_ptr(), b["tri"].data_ptr(), b["counts"].data_ptr())
    return rp, ms


def measure(torch, api, lio, stereo, shapes, lib, device):
    rec = dict(device="MI355X" if device != "cpu" else "CPU simulator build: a rehearsal of the script, NOT a measurement", cell=CELL, calls=N, shapes={})
    for H, W in shapes:
        P = H * W
        e, im = context(api, H, W, lib)
        try:
            stream = None
            if device != "cpu":                                 # (the events go on the stream the context launches on)
                stream = torch.cuda.Stream()
                e.set_stream(stream.cuda_stream)
            clock = timing.Clock(torch, device, stream=stream, sync=e.synchronize)
            timed = lambda f: timing.spread(timing.time_one(clock, f, N, warm=3), 4)
            st = stereo.FastGCStereo(e, im, im, dict(lambda_=0.5, windR=2, th_col=0.5), device=device, seed=1)
            calib, jump = lio.calib3d(CALIB), float(st.p["th_smooth"])
            row = {}
            for name, invalid in (("cells", 0.0), ("cells_10pct_invalid", 0.1)):
                lab = make_labels(H, W, invalid)
                b = buffers(torch, e, lab, device)
                rp, ms = calls(api, e, b, calib, jump)
                rp(); ms(); e.synchronize()
                nv, nt = (int(v) for v in b["counts"].cpu())
                by = bytes_moved(P, nv, nt)
                r = dict(vertices=nv, triangles=nt, bytes=by, reproject_ms=timed(rp), mesh_four_launches_ms=timed(ms))
                for k in ("reproject", "mesh", "mesh_count", "mesh_vertices", "mesh_triangles"):
                    r[f"copy_wide_{k}_bytes_ms"] = timed(timing.copy_call(api, by[k], stream.cuda_stream if stream else None, wide=True,
                                                                          device="cpu" if device == "cpu" else 0, lib=lib, random=False))
                r["reproject_over_copy"] = round(r["reproject_ms"]["median"] / r["copy_wide_reproject_bytes_ms"]["median"], 2)
                r["mesh_over_copy"] = round(r["mesh_four_launches_ms"]["median"] / r["copy_wide_mesh_bytes_ms"]["median"], 2)
                out = {}                                        # (host clock, no synchronise: the call ends with the results on the host)
                whole = timing.time_one(timing.Clock(torch, "cpu"), lambda: out.update(st.reconstruct(lab, calib)), N, warm=3)
                assert len(out["vertices"]) == nv and len(out["triangles"]) == nt
                r["reconstruct_whole_call_host_ms"] = timing.spread(whole, 4)
                row[name] = r
                print(f"{W} x {H} {name}:", json.dumps({k: v for k, v in r.items() if k != "bytes"}), file=sys.stderr, flush=True)
            rec["shapes"][f"{W}x{H}"] = row
        finally:
            e.close()
    return rec


def calls_only(torch, api, lio, shapes, lib, device):
    """What a profiler run watches: per shape and input 3 + N calls of les_hip_reproject and of les_hip_mesh."""
    for H, W in shapes:
        e, _ = context(api, H, W, lib)
        try:
            for invalid in (0.0, 0.1):
                b = buffers(torch, e, make_labels(H, W, invalid), device)
                rp, ms = calls(api, e, b, lio.calib3d(CALIB), 1.0)
                for _ in range(3 + N):
                    rp()
                    ms()
                e.synchronize()
        finally:
            e.close()


def read_trace(path, shapes):
    """Medians per kernel and shape from a rocprofv3 *_kernel_trace.csv: the dispatches of a shape are told apart by their grid (work-items)."""
    rows = list(csv.DictReader(open(path)))
    out = {}
    for H, W in shapes:
        P = H * W
        grids = {"les_reproject_kernel": (P + 255) // 256 * 256, "les_mesh_scan_kernel": 256}
        tiles = (P + 1023) // 1024 * 256
        per = {}
        for k in KERNELS:
            want = grids.get(k, tiles)
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"] and int(r.get("Grid_Size_X", r.get("Grid_Size", want))) == want]
            if us:
                per[k] = dict(median_us=round(float(np.median(us)), 2), min_us=round(min(us), 2), max_us=round(max(us), 2), dispatches=len(us))
        out[f"{W}x{H}"] = per
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--shapes", default=None, help="HxW,HxW (default: 992x1436,1000x1500)")
    args = ap.parse_args()
    shapes = tuple(tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")) if args.shapes else SHAPES
    rec = json.load(open(args.out)) if args.out and os.path.exists(args.out) and args.kernel_trace else {}
    if args.kernel_trace:
        rec["kernels_rocprofv3_kernel_trace"] = read_trace(args.kernel_trace, shapes)
        rec["kernels_note"] = ("medians over the dispatches of one profiler run of its own (--calls: both inputs, 3 + 20 calls each; the scan kernel's figure "
                               "covers both shapes: its grid is one workgroup)")
    else:
        import torch
        from localexpstereo_amd import api, io as lio, stereo
        if args.device != "cpu" and not torch.cuda.is_available():
            raise SystemExit("no GPU: this is a measurement and has no fallback (--lib PATH --device cpu rehearses the script)")
        if args.calls:
            calls_only(torch, api, lio, shapes, args.lib, args.device)
            return
        rec = measure(torch, api, lio, stereo, shapes, args.lib, args.device)
    timing.write_record(args.out, rec)


if __name__ == "__main__":
    main()
