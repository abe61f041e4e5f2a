#!/usr/bin/env python
"""Timings of the nearest-valid row fill of a cost volume (csrc/les_maskvol.h) on the MI355X -> profiles/maskvol.md and .json (summarised in
DESIGN 3.2n).

  python tools/maskvol_timing.py [--out profiles/maskvol]

Recorded on a 256 x 992 x 1436 float volume, both views' volumes (mode 0 and mode 1), all in one process:
  (a) les_hip_fill_invalid with both masks null against les_hip_fill_out_of_view on the same volume: both write the same bytes (the test suite
      holds them to each other), and both are idempotent, so every launch does the same work;
  (b) les_hip_fill_invalid with the valid masks of the rig of tools/unrectify_timing.py (2 degree rotations, all eight distortion
      coefficients), on a volume of its own;
  *   les_hip_calib_copy of the bytes each rewrites (it reads and writes that many).
One group of tools/timing.py (which states the protocol): `--timings` rounds after 3 warm-up calls, no bursts.  Nothing here is a gate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rectify_timing as rt  # noqa: E402  (the rig is that tool's)
import timing  # noqa: E402

H, W, D = rt.H, rt.W, 256


def rewritten(vI, vJ, mode):
    """entries of a [D][H][W] volume that are not ok (what the pass rewrites), counted with torch on the device"""
    import torch
    xs = torch.arange(W, device="cuda")
    n = 0
    for d in range(D):
        seen, c = (xs >= min(d, W - 1), (xs - d).clamp(0, W - 1)) if mode == 0 else (xs < max(W - d, 1), (xs + d).clamp(0, W - 1))
        n += H * W - int((vI & vJ[:, c] & seen[None, :]).sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="path without extension: <out>.md and <out>.json are written")
    ap.add_argument("--timings", type=int, default=30)
    a = ap.parse_args()
    torch = timing.require_gpu("maskvol_timing.py")
    from localexpstereo_amd import api, stereo
    stream = torch.cuda.current_stream().cuda_stream
    rect = rt.rig(stereo)
    black = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    r = rect.rectify(black, black)
    valid = [r["validL"].to(torch.uint8).contiguous(), r["validR"].to(torch.uint8).contiguous()]
    ones = torch.ones((H, W), dtype=torch.bool, device="cuda")
    vol_a, vol_b = torch.rand((D, H, W), device="cuda"), torch.rand((D, H, W), device="cuda")
    calls, entries = {}, {}
    for mode in (0, 1):
        calls[f"a_fill_out_of_view_mode{mode}"] = lambda mode=mode: api.fill_out_of_view(vol_a.data_ptr(), D, H, W, mode, stream=stream)
        calls[f"a_fill_invalid_null_mode{mode}"] = lambda mode=mode: api.fill_invalid(vol_a.data_ptr(), D, H, W, mode, stream=stream)
        calls[f"b_fill_invalid_masks_mode{mode}"] = lambda mode=mode: api.fill_invalid(vol_b.data_ptr(), D, H, W, mode, validI=valid[mode].data_ptr(),
                                                                                      validJ=valid[1 - mode].data_ptr(), stream=stream)
        entries[f"a_mode{mode}"] = rewritten(ones, ones, mode)
        entries[f"b_mode{mode}"] = rewritten(valid[mode] != 0, valid[1 - mode] != 0, mode)
    for k, n in entries.items():
        calls[f"copy_{k}"] = timing.copy_call(api, 8 * n, stream)           # as many floats as the pass rewrites, read and written
    # the two entries write the same bytes: checked here once more, on this volume
    check = vol_a[:8].clone()
    ref = check.clone()
    api.fill_out_of_view(ref.data_ptr(), 8, H, W, 0, stream=stream)
    api.fill_invalid(check.data_ptr(), 8, H, W, 0, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int32), check.view(torch.int32))
    single, _ = timing.time_calls(timing.Clock(torch, "cuda"), calls, a.timings, warm=3)
    us = {k: timing.spread(1e3 * np.asarray(v), 3) for k, v in single.items()}
    ratios = {}
    for mode in (0, 1):
        old, new, masked = (us[f"{k}_mode{mode}"] for k in ("a_fill_out_of_view", "a_fill_invalid_null", "b_fill_invalid_masks"))
        ratios[f"mode{mode}"] = dict(null_over_fill_out_of_view=round(new["median"] / old["median"], 3),
                                     null_over_own_copy=round(new["median"] / us[f"copy_a_mode{mode}"]["median"], 3),
                                     fill_out_of_view_over_own_copy=round(old["median"] / us[f"copy_a_mode{mode}"]["median"], 3),
                                     masks_over_own_copy=round(masked["median"] / us[f"copy_b_mode{mode}"]["median"], 3))
    rec = dict(device=timing.device_label(torch), shape=[D, H, W], timings=a.timings,
               valid_share=[round(float((v != 0).float().mean()), 4) for v in valid], valid_both_share=round(float(((valid[0] != 0) & (valid[1] != 0)).float().mean()), 4),
               rewritten_entries=entries, rewritten_MB={k: round(4e-6 * n, 1) for k, n in entries.items()}, single_launch_us=us, ratios=ratios)
    md = (f"# Nearest-valid row fill of a cost volume: kernel timings\n\n`python tools/maskvol_timing.py --out profiles/maskvol` on {rec['device']}, a float volume of "
          f"{D} x {H} x {W}; medians of {a.timings} device-event timings of one launch each (rounds over all calls, after a warm-up).  (a): both masks null, "
          f"against `les_hip_fill_out_of_view` on the same volume (the same bytes).  (b): the valid masks of a rig with 2 degree rotations "
          f"({100 * rec['valid_share'][0]:.1f} % / {100 * rec['valid_share'][1]:.1f} % of the pixels valid, {100 * rec['valid_both_share']:.1f} % in both).  "
          f"copy: `les_hip_calib_copy` of as many floats as the pass rewrites (it reads and writes them).  The numbers are in `maskvol.json`.\n\n"
          "| call | one launch, us (min .. max) | entries rewritten, MB |\n|---|---|---|\n")
    for k in calls:
        key = k.split("_")[0] + "_" + k.split("_")[-1] if not k.startswith("copy_") else k[5:]
        md += f"| {k} | {us[k]['median']} ({us[k]['min']} .. {us[k]['max']}) | {rec['rewritten_MB'][key]} |\n"
    md += "\n| view | null masks / fill_out_of_view | fill_out_of_view / copy | null masks / copy | masks / copy |\n|---|---|---|---|---|\n"
    for m, r_ in ratios.items():
        md += f"| {m} | {r_['null_over_fill_out_of_view']} | {r_['fill_out_of_view_over_own_copy']} | {r_['null_over_own_copy']} | {r_['masks_over_own_copy']} |\n"
    md += ("\nWhat was measured is above; nothing was fixed in advance.  From the code, not from a profile: `les_fill_out_of_view_kernel` launches a "
           "work-item per entry of the volume, most of which return at once; `les_fill_invalid_kernel` launches 256 work-items per row and 32 slices, "
           "makes the ok flags of a row as words from the staged mask bits, and touches the volume only where a word has a hole.  "
           "Not measured: `rocprofv3` kernel times, other sizes.\n")
    timing.write_record(a.out, rec, md)


if __name__ == "__main__":
    main()
