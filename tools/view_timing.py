#!/usr/bin/env python
"""Timings of view synthesis and of the photometric check (csrc/les_view.h) on the MI355X -> profiles/view_synthesis.md and .json (summarised
in DESIGN 3.4g).

  python tools/view_timing.py [--out profiles/view_synthesis]

Recorded at 1436 x 992 (planes of a piecewise-slanted scene with disparities up to 200, random images), all in one run:
  * les_render_view_kernel (both source views, t = 0.5 and t = 1, the context's image), les_blend_views_kernel (the two renders of t = 0.5, with
    and without the hole fill) and les_photo_error_kernel (both views);
  * les_warp_labels_kernel on the same labels, and les_hip_calib_copy of each kernel's own byte count (what it must read and write once: render
    28 B per pixel, blend 24, photo error 29, label warp 49);
One group of tools/timing.py (which states the protocol): `--timings` rounds after 3 warm-up calls, and bursts of 20 launches.  Nothing here is a gate."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import timing  # noqa: E402

H, W = 992, 1436
BYTES = dict(render=28, blend=24, photo=29, warp=49)          # per pixel, read and written once
BURST = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    torch = timing.require_gpu("view_timing.py")
    from crossview_timing import slanted_labels
    from localexpstereo_amd import api
    rng = np.random.default_rng(11)
    imL, imR = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=0, max_disp=255.0, filter="")
    stream = torch.cuda.current_stream().cuda_stream
    e.set_stream(stream)
    lab = [torch.from_numpy(slanted_labels(H, W, s)).cuda() for s in (1, 2)]
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    side = [(new((H, W, 3), torch.uint8), new((H, W), torch.float32), new((H, W), torch.uint8)) for _ in range(2)]
    out = (new((H, W, 3), torch.uint8), new((H, W), torch.float32), new((H, W), torch.uint8))
    wout, whit = torch.empty_like(lab[0]), new((H, W), torch.uint8)
    ptrs = lambda ts: tuple(t.data_ptr() for t in ts)
    calls = {}
    for m in (0, 1):
        for t in (0.5, 1.0):
            calls[f"render_view{m}_t{t}"] = (lambda m=m, t=t: e.render_view_ptr(m, lab[m].data_ptr(), None, t, *ptrs(out)))
        calls[f"photo_error_view{m}"] = (lambda m=m: e.photo_error_ptr(m, lab[m].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
        calls[f"warp_labels_view{m}"] = (lambda m=m: e.warp_labels(m, lab[m].data_ptr(), lab[1 - m].data_ptr(), wout.data_ptr(), whit.data_ptr()))
    for fill in (1, 0):
        calls[f"blend_views_fill{fill}"] = (lambda fill=fill: e.blend_views_ptr(0.5, 1.0, fill, ptrs(side[0]), ptrs(side[1]), *ptrs(out)))
    for k in BYTES:
        calls[f"copy_{BYTES[k]}B_per_pixel"] = timing.copy_call(api, BYTES[k] * H * W, stream)
    # the blend's inputs: the two renders of t = 0.5
    for m in (0, 1):
        e.render_view_ptr(m, lab[m].data_ptr(), None, 0.5, *ptrs(side[m]))
    torch.cuda.synchronize()
    shares = dict(hit_share_view0=round(float((side[0][2] != 0).float().mean()), 4), hit_share_view1=round(float((side[1][2] != 0).float().mean()), 4))
    single, burst = timing.time_calls(timing.Clock(torch, "cuda"), calls, a.timings, warm=3, burst=BURST)
    e.blend_views_ptr(0.5, 1.0, 1, ptrs(side[0]), ptrs(side[1]), *ptrs(out))
    torch.cuda.synchronize()
    shares["blend_src_counts_0_to_4"] = torch.bincount(out[2].flatten().long(), minlength=5).tolist()
    us = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in single.items()}
    bus = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in burst.items()}
    med = lambda prefix, table: max(v["median"] for k, v in table.items() if k.startswith(prefix))
    ratios = {}
    for table, tag in ((us, "single"), (bus, "burst")):
        warp = med("warp_labels", table)
        for name, key in (("render_view", "render"), ("blend_views", "blend"), ("photo_error", "photo")):
            own = table[f"copy_{BYTES[key]}B_per_pixel"]["median"]
            ratios[f"{name}_{tag}"] = dict(us=med(name, table), over_own_copy=round(med(name, table) / own, 3), over_label_warp=round(med(name, table) / warp, 3),
                                           over_2x_larger_yardstick=round(med(name, table) / (2 * max(warp, table[f"copy_{BYTES['warp']}B_per_pixel"]["median"])), 3))
    rec = dict(device=timing.device_label(torch), shape=[W, H], timings=a.timings, burst_launches=BURST, bytes_per_pixel=BYTES, scene=shares,
               single_launch_us=us, burst_us_per_launch=bus, ratios_of_slowest_variant=ratios)
    e.close()
    md = (f"# View synthesis and photometric check: kernel timings\n\n`python tools/view_timing.py --out profiles/view_synthesis` on {rec['device']}, "
          f"{W} x {H}, medians of {a.timings} device-event timings of one launch each (rounds over all kernels, after a warm-up); burst: per launch "
          f"of {BURST} launches between one pair of events.  The numbers are in `view_synthesis.json`.\n\n"
          "| call | one launch, us (min .. max) | burst, us per launch |\n|---|---|---|\n")
    for k in calls:
        md += f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {bus[k]['median']} |\n"
    md += ("\nSlowest variant of each kernel against the yardsticks (its own byte count copied by les_hip_calib_copy; les_warp_labels_kernel; "
           "2 x the larger of the label warp and the copy of its 49 B per pixel):\n\n| kernel | us | / own copy | / label warp | / 2 x larger yardstick |\n|---|---|---|---|---|\n")
    for k, r in ratios.items():
        md += f"| {k} | {r['us']} | {r['over_own_copy']} | {r['over_label_warp']} | {r['over_2x_larger_yardstick']} |\n"
    md += f"\nScene: {json.dumps(shares)}\n"
    timing.write_record(a.out, rec, md)


if __name__ == "__main__":
    main()
