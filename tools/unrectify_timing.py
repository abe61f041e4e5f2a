#!/usr/bin/env python
"""Timings of the kernels of the way back to the raw camera (csrc/les_unrectify.h) on the MI355X -> profiles/unrectify.md and .json (summarised
in DESIGN 3.2m).

  python tools/unrectify_timing.py [--out profiles/unrectify]

Recorded at 1436 x 992, raw and rectified frames of the same size (the rig of tools/rectify_timing.py: 2 degree rotations, all eight distortion
coefficients; slanted random labels), all in one run:
  * les_unrectify_map_kernel at the default 20 steps (8 B per raw pixel written);
  * les_unrectify_labels_kernel with every output (per raw pixel: 8 B of map and a 16 B label gathered = 24 B read, 12 + 12 + 4 + 1 = 29 B written);
  * les_hip_calib_copy of each kernel's own byte count.
One group of tools/timing.py (which states the protocol): `--timings` rounds after 3 warm-up calls, and bursts of 20 launches.  Nothing here is a gate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rectify_timing as rt  # noqa: E402  (the rig is that tool's)
import timing  # noqa: E402

H, W = rt.H, rt.W
BYTES = dict(unrectify_map=8, unrectify_labels=8 + 16 + 29)      # per raw pixel, read and written once
BURST = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    torch = timing.require_gpu("unrectify_timing.py")
    from localexpstereo_amd import api, stereo
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(12)
    rect = rt.rig(stereo)
    tr = rect.transform
    inv = rect.inverse_maps[0]
    lab = np.zeros((H, W, 4), np.float32)
    lab[..., 0], lab[..., 1], lab[..., 2] = rng.uniform(-0.01, 0.01, (H, W)), rng.uniform(-0.01, 0.01, (H, W)), rng.uniform(20.0, 200.0, (H, W))
    lab = torch.from_numpy(lab).cuda()
    mp = torch.empty_like(inv)
    points, normals = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")
    disparity, valid = torch.empty((H, W), device="cuda"), torch.empty((H, W), dtype=torch.uint8, device="cuda")
    cam = api.camera(tr["K0"], tr["dist0"])
    calls = {"unrectify_map": lambda: api.unrectify_map(cam, tr["R0"], tr["f"], tr["cx0"], tr["cy"], mp.data_ptr(), H, W, stream=stream),
             "unrectify_labels": lambda: api.unrectify_labels(lab.data_ptr(), H, W, None, inv.data_ptr(), H, W, tr["R0"].T, tr["f"], tr["cx0"], tr["cy"], tr["doffs"],
                                                              tr["baseline"], valid.data_ptr(), points.data_ptr(), normals.data_ptr(), disparity.data_ptr(),
                                                              stream=stream)}
    for k in BYTES:
        calls[f"copy_{BYTES[k]}B_per_pixel"] = timing.copy_call(api, BYTES[k] * H * W, stream)
    single, burst = timing.time_calls(timing.Clock(torch, "cuda"), calls, a.timings, warm=3, burst=BURST)
    us = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in single.items()}
    bus = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in burst.items()}
    ratios = {}
    for k in BYTES:
        own = f"copy_{BYTES[k]}B_per_pixel"
        ratios[k] = dict(single_over_own_copy=round(us[k]["median"] / us[own]["median"], 3), burst_over_own_copy=round(bus[k]["median"] / bus[own]["median"], 3))
    stored = float((~torch.isnan(inv[..., 0])).float().mean())
    rec = dict(device=timing.device_label(torch), shape=[W, H], timings=a.timings,
               burst_launches=BURST, steps=rect.steps, tol=rect.tol, bytes_per_pixel=BYTES, converged_share=round(stored, 4),
               valid_share=round(float((valid != 0).float().mean()), 4), single_launch_us=us, burst_us_per_launch=bus, ratios=ratios)
    md = (f"# The way back to the raw camera: kernel timings\n\n`python tools/unrectify_timing.py --out profiles/unrectify` on {rec['device']}, raw and "
          f"rectified frames of {W} x {H}, {rect.steps} fixed-point steps, tol {rect.tol} px; medians of {a.timings} device-event timings of one launch "
          f"each (rounds over all calls, after a warm-up); burst: per launch of {BURST} launches between one pair of events.  "
          f"{100 * rec['converged_share']:.1f} % of the raw pixels have a rectified position, {100 * rec['valid_share']:.1f} % are valid in the "
          f"labels kernel.  The numbers are in `unrectify.json`.\n\n"
          "| call | one launch, us (min .. max) | burst, us per launch |\n|---|---|---|\n")
    for k in calls:
        md += f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {bus[k]['median']} |\n"
    md += ("\nAgainst `les_hip_calib_copy` of the kernel's own bytes (map: 8 B per raw pixel written; labels: 8 B of map + a 16 B label read, "
           "12 + 12 + 4 + 1 = 29 B written = 53 B):\n\n| kernel | one launch / copy | burst / copy |\n|---|---|---|\n")
    for k, r in ratios.items():
        md += f"| {k} | {r['single_over_own_copy']} | {r['burst_over_own_copy']} |\n"
    md += ("\nWhere the time goes, from the code, not from a profile.  The map is arithmetic: 21 evaluations of the distortion, each with an fp64 "
           "division and some thirty fp64 multiplies and adds, for 8 bytes stored; it runs once per calibration.  The labels kernel moves 53 bytes per "
           "raw pixel, the label through a 16-byte gather whose addresses follow the inverse map (neighbouring raw pixels read neighbouring or "
           "the same labels), and stores the two 12-byte triples with a stride of 12 bytes per work-item, not through LDS; on top come three fp64 "
           "divisions, a square root and three more divisions for the normal.  Not measured: `rocprofv3` kernel times, other sizes.\n")
    timing.write_record(a.out, rec, md)


if __name__ == "__main__":
    main()
