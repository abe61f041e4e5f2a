#!/usr/bin/env python
"""Timings of the rectification kernels (csrc/les_rectify.h) on the MI355X -> profiles/rectify.md and .json (summarised in DESIGN 3.2l).

  python tools/rectify_timing.py [--out profiles/rectify]

Recorded at 1436 x 992 from a source of the same size (a rig of 2 degree rotations with all eight distortion coefficients, a random 3-channel
image), all in one run:
  * les_rectify_map_kernel (8 B per pixel written) and les_remap_kernel at the three interpolations (per pixel: 8 B of map and 3 B of source
    read, 3 B of image and 1 B of valid written = 15 B);
  * les_hip_calib_copy of each kernel's own byte count.
One group of tools/timing.py (which states the protocol): `--timings` rounds after 3 warm-up calls, and bursts of 20 launches.  Nothing here is a gate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import timing  # noqa: E402

H, W = 992, 1436
BYTES = dict(map=8, remap=15)                # per pixel, read and written once
BURST = 20
DIST0 = (-0.12, 0.05, 0.001, -0.0008, 0.01, 0.02, -0.01, 0.004)
DIST1 = (-0.10, 0.04, -0.0009, 0.0007, 0.008, 0.015, 0.01, -0.003)


def _rot(rx, ry, rz):
    a, b, c = np.radians([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rig(stereo, h=H, w=W):
    """The rig of the rectify, unrectify and maskvol timings: 2 degree rotations, all eight distortion coefficients, raw frames of h x w."""
    K0 = np.array([[1500.0, 0, 0.5 * (w - 1) + 3.0], [0, 1495.0, 0.5 * (h - 1) - 2.0], [0, 0, 1]])
    K1 = np.array([[1490.0, 0, 0.5 * (w - 1) - 4.0], [0, 1502.0, 0.5 * (h - 1) + 1.5], [0, 0, 1]])
    return stereo.Rectifier(K0, DIST0, K1, DIST1, _rot(2.0, -2.0, 2.0), (-0.2, 0.004, -0.003), raw_size=(h, w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    torch = timing.require_gpu("rectify_timing.py")
    from localexpstereo_amd import api, stereo
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    rect = rig(stereo)
    tr = rect.transform
    src = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    mp, dst, valid = torch.empty_like(rect.maps[0]), torch.empty_like(src), torch.empty((H, W), dtype=torch.uint8, device="cuda")
    cam = api.camera(tr["K0"], tr["dist0"])
    calls = {"rectify_map": lambda: api.rectify_map(cam, tr["R0"].T, tr["f"], tr["cx0"], tr["cy"], mp.data_ptr(), H, W, stream=stream)}
    for name, interp in api.INTERP_NAMES.items():
        calls[f"remap_{name}"] = (lambda interp=interp: api.remap(src.data_ptr(), H, W, 3, rect.maps[0].data_ptr(), dst.data_ptr(), valid.data_ptr(), H, W,
                                                                  interp=interp, stream=stream))
    for k in BYTES:
        calls[f"copy_{BYTES[k]}B_per_pixel"] = timing.copy_call(api, BYTES[k] * H * W, stream)
    single, burst = timing.time_calls(timing.Clock(torch, "cuda"), calls, a.timings, warm=3, burst=BURST)
    us = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in single.items()}
    bus = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in burst.items()}
    ratios = {}
    for k in calls:
        if k.startswith("copy_"):
            continue
        own = f"copy_{BYTES['map' if k == 'rectify_map' else 'remap']}B_per_pixel"
        ratios[k] = dict(single_over_own_copy=round(us[k]["median"] / us[own]["median"], 3), burst_over_own_copy=round(bus[k]["median"] / bus[own]["median"], 3))
    rec = dict(device=timing.device_label(torch), shape=[W, H], timings=a.timings, burst_launches=BURST, bytes_per_pixel=BYTES,
               valid_share=round(float(valid.float().mean()), 4), single_launch_us=us, burst_us_per_launch=bus, ratios=ratios)
    md = (f"# Rectification: kernel timings\n\n`python tools/rectify_timing.py --out profiles/rectify` on {rec['device']}, {W} x {H} from a source of "
          f"the same size, medians of {a.timings} device-event timings of one launch each (rounds over all calls, after a warm-up); burst: per "
          f"launch of {BURST} launches between one pair of events.  {100 * rec['valid_share']:.1f} % of the rectified pixels are valid.  The "
          f"numbers are in `rectify.json`.\n\n"
          "| call | one launch, us (min .. max) | burst, us per launch |\n|---|---|---|\n")
    for k in calls:
        md += f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {bus[k]['median']} |\n"
    md += ("\nAgainst `les_hip_calib_copy` of the kernel's own bytes (map 8 B per pixel; remap 8 B of map + 3 B of source + 3 B of image + 1 B of "
           "valid = 15 B):\n\n| kernel | one launch / copy | burst / copy |\n|---|---|---|\n")
    for k, r in ratios.items():
        md += f"| {k} | {r['single_over_own_copy']} | {r['burst_over_own_copy']} |\n"
    timing.write_record(a.out, rec, md)


if __name__ == "__main__":
    main()
