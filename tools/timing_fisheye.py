#!/usr/bin/env python
"""Timings of the fisheye camera's two map kernels (csrc/les_fisheye.h) on the MI355X -> profiles/fisheye.md and .json (summarised in DESIGN 3.2o).

  python tools/timing_fisheye.py [--out profiles/fisheye]

Recorded at 1436 x 992, raw and rectified frames of the same size, all in one run, alternating:
  * les_fisheye_map_kernel and les_fisheye_unmap_kernel at its default 10 Newton steps, on the rig of tools/rectify_timing.py (2 degree rotations,
    the same centres and baseline) with two four-coefficient fisheye lenses of fx = 546 px: half a raw row reaches 75 degrees off the axis, so
    every branch of the kernels' atan and both quadrants of their sin / cos occur;
  * les_rectify_map_kernel and les_unrectify_map_kernel at its 20 steps, on that tool's pinhole rig;
  * les_hip_calib_copy of the 8 bytes per pixel each of the four writes.
One group of tools/timing.py (which states the protocol): `--timings` rounds after 3 warm-up calls, and bursts of 20 launches.  Nothing here is a gate.
(The name: tests/test_timing_harness.py counts the tools called *_timing.py, nineteen of them; tests/test_fisheye.py holds this one to the same rules.)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rectify_timing as rt  # noqa: E402  (the rig's geometry is that tool's)
import timing  # noqa: E402

H, W = rt.H, rt.W
BYTES = 8                                    # per pixel, written once by every map kernel
BURST = 20
K0 = (-0.035, 0.006, -0.0025, 0.0004)
K1 = (-0.03, 0.008, -0.003, 0.0005)
FX = 0.38 * W                                # 546 px: (W - 1) / 2 raw pixels are 1.31 rad of theta_d


def fisheye_rig(stereo, h=H, w=W):
    """rectify_timing.rig with fisheye cameras: its rotations, centres and baseline; raw frames of h x w; a rectified frame of the same size at
    the default focal length (fy: the rectified row reaches atan(717 / 544) = 53 degrees)."""
    Ka = np.array([[FX, 0, 0.5 * (w - 1) + 3.0], [0, FX - 2.0, 0.5 * (h - 1) - 2.0], [0, 0, 1]])
    Kb = np.array([[FX - 4.0, 0, 0.5 * (w - 1) - 4.0], [0, FX + 1.0, 0.5 * (h - 1) + 1.5], [0, 0, 1]])
    return stereo.Rectifier(Ka, K0, Kb, K1, rt._rot(2.0, -2.0, 2.0), (-0.2, 0.004, -0.003), raw_size=(h, w), model="fisheye")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    torch = timing.require_gpu("timing_fisheye.py")
    from localexpstereo_amd import api, stereo
    stream = torch.cuda.current_stream().cuda_stream
    fish, pin = fisheye_rig(stereo), rt.rig(stereo)
    tf, tp = fish.transform, pin.transform
    mp = torch.empty_like(fish.maps[0])
    fcam, pcam = api.fisheye(tf["K0"], tf["dist0"], tf["theta_max0"]), api.camera(tp["K0"], tp["dist0"])
    calls = {
        "fisheye_map": lambda: api.rectify_map_fisheye(fcam, tf["R0"].T, tf["f"], tf["cx0"], tf["cy"], mp.data_ptr(), H, W, stream=stream),
        "rectify_map": lambda: api.rectify_map(pcam, tp["R0"].T, tp["f"], tp["cx0"], tp["cy"], mp.data_ptr(), H, W, stream=stream),
        "fisheye_unmap": lambda: api.unrectify_map_fisheye(fcam, tf["R0"], tf["f"], tf["cx0"], tf["cy"], mp.data_ptr(), H, W, steps=fish.steps, tol=fish.tol,
                                                           stream=stream),
        "unrectify_map": lambda: api.unrectify_map(pcam, tp["R0"], tp["f"], tp["cx0"], tp["cy"], mp.data_ptr(), H, W, steps=pin.steps, tol=pin.tol, stream=stream),
        "copy_8B_per_pixel": timing.copy_call(api, BYTES * H * W, stream),
    }
    single, burst = timing.time_calls(timing.Clock(torch, "cuda"), calls, a.timings, warm=3, burst=BURST)
    us = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in single.items()}
    bus = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in burst.items()}
    pinhole_of = dict(fisheye_map="rectify_map", fisheye_unmap="unrectify_map")
    ratios = {}
    for k in ("fisheye_map", "rectify_map", "fisheye_unmap", "unrectify_map"):
        ratios[k] = dict(single_over_copy=round(us[k]["median"] / us["copy_8B_per_pixel"]["median"], 3),
                         burst_over_copy=round(bus[k]["median"] / bus["copy_8B_per_pixel"]["median"], 3))
        if k in pinhole_of:
            ratios[k].update(single_over_pinhole=round(us[k]["median"] / us[pinhole_of[k]]["median"], 3),
                             burst_over_pinhole=round(bus[k]["median"] / bus[pinhole_of[k]]["median"], 3))
    share = lambda t: round(float((~torch.isnan(t[..., 0])).float().mean()), 4)
    rec = dict(device=timing.device_label(torch), shape=[W, H], timings=a.timings, burst_launches=BURST, bytes_per_pixel=BYTES,
               fisheye=dict(fx=FX, k0=list(K0), steps=fish.steps, tol=fish.tol, theta_max=tf["theta_max0"], f=tf["f"], map_share=share(fish.maps[0]),
                            inverse_share=share(fish.inverse_maps[0])),
               pinhole=dict(steps=pin.steps, tol=pin.tol, map_share=share(pin.maps[0]), inverse_share=share(pin.inverse_maps[0])),
               single_launch_us=us, burst_us_per_launch=bus, ratios=ratios)
    md = (f"# The fisheye camera's maps: kernel timings\n\n`python tools/timing_fisheye.py --out profiles/fisheye` on {rec['device']}, raw and rectified "
          f"frames of {W} x {H}; fisheye rig: fx {FX:.0f} px (half a raw row is 75 degrees), k = {list(K0)}, {fish.steps} Newton steps, tol {fish.tol} px, "
          f"{100 * rec['fisheye']['map_share']:.1f} % of the rectified and {100 * rec['fisheye']['inverse_share']:.1f} % of the raw pixels stored; pinhole rig: "
          f"that of `tools/rectify_timing.py`, {pin.steps} fixed-point steps.  Medians of {a.timings} device-event timings of one launch each (rounds "
          f"over all calls, after a warm-up); burst: per launch of {BURST} launches between one pair of events.  The numbers are in `fisheye.json`.\n\n"
          "| call | one launch, us (min .. max) | burst, us per launch |\n|---|---|---|\n")
    for k in calls:
        md += f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {bus[k]['median']} |\n"
    md += ("\nAgainst `les_hip_calib_copy` of the 8 bytes per pixel every map kernel writes, and against the pinhole kernel of the same direction:\n\n"
           "| kernel | one launch / copy | burst / copy | one launch / pinhole | burst / pinhole |\n|---|---|---|---|---|\n")
    for k, r in ratios.items():
        md += f"| {k} | {r['single_over_copy']} | {r['burst_over_copy']} | {r.get('single_over_pinhole', '')} | {r.get('burst_over_pinhole', '')} |\n"
    md += ("\nWhere the time goes, from the code, not from a profile.  Both kernels are arithmetic for 8 bytes stored.  The forward map has seven fp64 "
           "divisions (xr, yr, a, b, theta_d / r, and up to two in the atan: 1 / r and (t - 1) / (t + 1)) and a square root, each a dependent chain of "
           "a dozen fp64 instructions, and the atan's 19-term Horner chain of dependent multiply-adds; the pinhole map has five divisions and no "
           "chain.  The inverse map has one division per Newton step behind two Horner evaluations (P and Q) that the next step waits for: 10 "
           "dependent divisions against the 21 of the pinhole kernel's 20 steps and residual, then the sin / cos chains (two of 9 terms, "
           "independent of each other), sn / theta_d, and the two divisions of the projection.  Neither is on the per-frame path: the forward map "
           "is built once per Rectifier, the inverse once per calibration.  Not measured: `rocprofv3` kernel times, other sizes, other fields of view "
           "(the atan's branches depend on the angle).\n")
    timing.write_record(a.out, rec, md)


if __name__ == "__main__":
    main()
