#!/usr/bin/env python
"""Timings of the AD-Census cost-volume builder (csrc/les_costvol.h) on the MI355X -> profiles/costvol_timing.json (summarised in DESIGN 3.2f).

  python tools/costvol_timing.py [--out profiles/costvol_timing.json] [--reps 20]

Shapes 1436 x 992 x 256 (Adirondack-H) and 1500 x 1000 x 256, both modes, random 8-bit images.  Every group of measurements runs in a child
process of its own under its own time limit; the first child that fails ends the run.  Each number is a group of one of tools/timing.py
(which states the protocol): `reps` timings after two warm-up calls.  Recorded per shape:
  * builder: les_costvol_kernel alone and the two census launches (the library's own events, LES_HIP_COSTVOL_TIMING=1), and the whole
    les_hip_build_cost_volume call (events around it: allocation and release of its scratch included), with plain and with non-temporal stores;
    the dword store path on the same shape one column wider (W % 4 != 0);
  * synth.ad_volume on the same shape: the torch.roll loop that was the only way to make a volume before;
  * les_hip_calib_copy of D H W floats.  A copy moves twice the bytes the builder writes: half its time is the write floor.
Nothing here is a gate."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import timing  # noqa: E402

SHAPES = [(1436, 992, 256), (1500, 1000, 256)]
CHILD_SECONDS = 240


def child_builder(torch, W, H, D, reps):
    import ctypes as C
    from localexpstereo_amd import api
    os.environ["LES_HIP_COSTVOL_TIMING"] = "1"
    L = api.load()
    rng = np.random.default_rng(1)
    rec = {}
    for name, w in (("vector_stores", W), ("dword_stores_W_plus_1", W + 1)):
        imL, imR = (torch.from_numpy(rng.integers(0, 256, (H, w, 3), dtype=np.uint8)).cuda() for _ in range(2))
        vol = torch.empty((D, H, w), dtype=torch.float32, device="cuda")
        for mode in ((0, 1) if w == W else (0,)):
            for nt in (("plain", "nontemporal") if w == W else ("plain",)):
                os.environ["LES_HIP_COSTVOL_NT"] = "1" if nt == "nontemporal" else "0"
                kern, cen = [], []

                def call():
                    api.build_cost_volume(imL.data_ptr(), imR.data_ptr(), vol.data_ptr(), D, H, w, mode)
                    a, b = C.c_float(), C.c_float()
                    assert L.les_hip_costvol_last_times(C.byref(a), C.byref(b)) == 0
                    cen.append(a.value)
                    kern.append(b.value)

                whole = timing.time_one(timing.Clock(torch, "cuda"), call, reps, warm=2)
                rec.setdefault(name, {}).setdefault(f"mode{mode}", {})[nt] = {k: timing.spread(v, 4) for k, v in (
                    ("volume_kernel_ms", kern[-reps:]), ("census_two_images_ms", cen[-reps:]), ("whole_call_ms", whole))}
        del imL, imR, vol
    return rec


def child_baselines(torch, W, H, D, reps):
    from localexpstereo_amd import api, synth
    rng = np.random.default_rng(1)
    imL, imR = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    clock = timing.Clock(torch, "cuda")
    one = lambda f: timing.spread(timing.time_one(clock, f, reps, warm=2), 4)
    ad = one(lambda: synth.ad_volume(imL, imR, D, "cuda"))
    nbytes = 2 * 4 * D * H * W                                 # a copy of D H W floats
    return dict(synth_ad_volume_ms=ad, calib_copy_ms=one(timing.copy_call(api, nbytes, None)), calib_copy_wide_ms=one(timing.copy_call(api, nbytes, None, wide=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", nargs=4, metavar=("WHAT", "W", "H", "D"))
    a = ap.parse_args()
    if a.child:
        what, (W, H, D) = a.child[0], (int(v) for v in a.child[1:])
        torch = timing.require_gpu("costvol_timing.py")
        print("RESULT " + json.dumps((child_builder if what == "builder" else child_baselines)(torch, W, H, D, a.reps)))
        return
    shapes = {}
    for W, H, D in SHAPES:
        rec = dict(floats=W * H * D, bytes_written=4 * W * H * D)
        for what in ("builder", "baselines"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", what, str(W), str(H), str(D)], capture_output=True, text=True,
                               timeout=CHILD_SECONDS)
            lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"costvol_timing.py: the {what} measurements at {W} x {H} x {D} failed (exit {p.returncode}); nothing further was run")
            rec.update(json.loads(lines[-1][len("RESULT "):]))
        floor = rec["calib_copy_ms"]["median"] / 2.0
        rec["write_floor_ms"] = round(floor, 4)
        rec["write_floor_wide_copy_ms"] = round(rec["calib_copy_wide_ms"]["median"] / 2.0, 4)
        for mode, by_store in rec["vector_stores"].items():
            k = {nt: v["volume_kernel_ms"]["median"] for nt, v in by_store.items()}
            best = min(k.values())
            rec.setdefault("summary", {})[mode] = dict(plain_ms=k["plain"], nontemporal_ms=k["nontemporal"], nontemporal_over_plain=round(k["nontemporal"] / k["plain"], 4),
                                                      write_GBps=round(4e-6 * W * H * D / best, 1), kernel_over_write_floor=round(best / floor, 3),
                                                      ad_volume_over_builder_call=round(rec["synth_ad_volume_ms"]["median"] / min(v["whole_call_ms"]["median"] for v in by_store.values()), 2))
        shapes[f"{W}x{H}x{D}"] = rec
    out = dict(note="one MI355X, one run; medians of device-event timings after two warm-up calls", reps=a.reps, shapes=shapes)
    timing.write_record(a.out, out)


if __name__ == "__main__":
    main()
