#!/usr/bin/env python
"""Timings of view synthesis and of the photometric check (csrc/les_view.h) on the MI355X -> profiles/view_synthesis.md and .json (summarised
in DESIGN 3.4g).

  python tools/view_timing.py [--out profiles/view_synthesis]

Recorded at 1436 x 992 (planes of a piecewise-slanted scene with disparities up to 200, random images), all in one run:
  * les_render_view_kernel (both source views, t = 0.5 and t = 1, the context's image), les_blend_views_kernel (the two renders of t = 0.5, with
    and without the hole fill) and les_photo_error_kernel (both views);
  * les_warp_labels_kernel on the same labels, and les_hip_calib_copy of each kernel's own byte count (what it must read and write once: render
    28 B per pixel, blend 24, photo error 29, label warp 49);
Every figure is the median of `--timings` device-event timings of ONE launch each, taken in rounds (each round times every kernel once, so a
drift of the machine hits them alike) after a warm-up of every kernel; `burst` is the time per launch of 20 launches between one pair of
events, which leaves the launch gap out.  Nothing here is a gate."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W = 992, 1436
BYTES = dict(render=28, blend=24, photo=29, warp=49)          # per pixel, read and written once
BURST = 20


def _spread(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), n=int(len(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    import torch
    from crossview_timing import slanted_labels
    from localexpstereo_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("view_timing.py measures on the GPU: no HIP device")
    rng = np.random.default_rng(11)
    imL, imR = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=0, max_disp=255.0, filter="")
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lab = [torch.from_numpy(slanted_labels(H, W, s)).cuda() for s in (1, 2)]
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    side = [(new((H, W, 3), torch.uint8), new((H, W), torch.float32), new((H, W), torch.uint8)) for _ in range(2)]
    out = (new((H, W, 3), torch.uint8), new((H, W), torch.float32), new((H, W), torch.uint8))
    wout, whit = torch.empty_like(lab[0]), new((H, W), torch.uint8)
    ptrs = lambda ts: tuple(t.data_ptr() for t in ts)
    copies = {}
    for k, b in BYTES.items():
        n = (b * H * W + 7) // 8                             # floats a copy reads AND writes for the same traffic: 8 n bytes
        copies[k] = (torch.rand(n, device="cuda"), torch.empty(n, device="cuda"), n)

    def copy(k):
        s, d, n = copies[k]
        return lambda: e._chk(e.L.les_hip_calib_copy(C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), C.c_size_t(n), 0, stream))

    calls = {}
    for m in (0, 1):
        for t in (0.5, 1.0):
            calls[f"render_view{m}_t{t}"] = (lambda m=m, t=t: e.render_view_ptr(m, lab[m].data_ptr(), None, t, *ptrs(out)))
        calls[f"photo_error_view{m}"] = (lambda m=m: e.photo_error_ptr(m, lab[m].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
        calls[f"warp_labels_view{m}"] = (lambda m=m: e.warp_labels(m, lab[m].data_ptr(), lab[1 - m].data_ptr(), wout.data_ptr(), whit.data_ptr()))
    for fill in (1, 0):
        calls[f"blend_views_fill{fill}"] = (lambda fill=fill: e.blend_views_ptr(0.5, 1.0, fill, ptrs(side[0]), ptrs(side[1]), *ptrs(out)))
    for k in BYTES:
        calls[f"copy_{BYTES[k]}B_per_pixel"] = copy(k)
    # the blend's inputs: the two renders of t = 0.5
    for m in (0, 1):
        e.render_view_ptr(m, lab[m].data_ptr(), None, 0.5, *ptrs(side[m]))
    torch.cuda.synchronize()
    shares = dict(hit_share_view0=round(float((side[0][2] != 0).float().mean()), 4), hit_share_view1=round(float((side[1][2] != 0).float().mean()), 4))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    single, burst = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(a.timings):
        for k, f in calls.items():
            ev0.record(); f(); ev1.record()
            torch.cuda.synchronize()
            single[k].append(1e3 * ev0.elapsed_time(ev1))
    for _ in range(5):
        for k, f in calls.items():
            ev0.record()
            for _ in range(BURST):
                f()
            ev1.record()
            torch.cuda.synchronize()
            burst[k].append(1e3 * ev0.elapsed_time(ev1) / BURST)
    e.blend_views_ptr(0.5, 1.0, 1, ptrs(side[0]), ptrs(side[1]), *ptrs(out))
    torch.cuda.synchronize()
    shares["blend_src_counts_0_to_4"] = torch.bincount(out[2].flatten().long(), minlength=5).tolist()
    us = {k: _spread(v) for k, v in single.items()}
    bus = {k: _spread(v) for k, v in burst.items()}
    med = lambda prefix, table: max(v["median"] for k, v in table.items() if k.startswith(prefix))
    ratios = {}
    for table, tag in ((us, "single"), (bus, "burst")):
        warp = med("warp_labels", table)
        for name, key in (("render_view", "render"), ("blend_views", "blend"), ("photo_error", "photo")):
            own = table[f"copy_{BYTES[key]}B_per_pixel"]["median"]
            ratios[f"{name}_{tag}"] = dict(us=med(name, table), over_own_copy=round(med(name, table) / own, 3), over_label_warp=round(med(name, table) / warp, 3),
                                           over_2x_larger_yardstick=round(med(name, table) / (2 * max(warp, table[f"copy_{BYTES['warp']}B_per_pixel"]["median"])), 3))
    rec = dict(device=f"{torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})", shape=[W, H], timings=a.timings, burst_launches=BURST, bytes_per_pixel=BYTES, scene=shares,
               single_launch_us=us, burst_us_per_launch=bus, ratios_of_slowest_variant=ratios)
    e.close()
    print(json.dumps(rec, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rec, open(a.out + ".json", "w"), indent=1)
        with open(a.out + ".md", "w") as f:
            f.write(f"# View synthesis and photometric check: kernel timings\n\n`python tools/view_timing.py --out profiles/view_synthesis` on {rec['device']}, "
                    f"{W} x {H}, medians of {a.timings} device-event timings of one launch each (rounds over all kernels, after a warm-up); burst: per launch "
                    f"of {BURST} launches between one pair of events.  The numbers are in `view_synthesis.json`.\n\n")
            f.write("| call | one launch, us (min .. max) | burst, us per launch |\n|---|---|---|\n")
            for k in calls:
                f.write(f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {bus[k]['median']} |\n")
            f.write("\nSlowest variant of each kernel against the yardsticks (its own byte count copied by les_hip_calib_copy; les_warp_labels_kernel; "
                    "2 x the larger of the label warp and the copy of its 49 B per pixel):\n\n| kernel | us | / own copy | / label warp | / 2 x larger yardstick |\n|---|---|---|---|---|\n")
            for k, r in ratios.items():
                f.write(f"| {k} | {r['us']} | {r['over_own_copy']} | {r['over_label_warp']} | {r['over_2x_larger_yardstick']} |\n")
            f.write(f"\nScene: {json.dumps(shares)}\n")


if __name__ == "__main__":
    main()
