#!/usr/bin/env python
"""Timings of the correlation cost-volume kernel and the patch descriptor (csrc/les_featvol.h) on the MI355X -> profiles/featvol_timing.json and
the table profiles/featvol.md (summarised in DESIGN 3.2k).

  python tools/featvol_timing.py [--out profiles/featvol_timing.json] [--md profiles/featvol.md] [--reps 20]

Shape 1436 x 992 x 256 (Adirondack-H), both modes, C = 25 (the ZNCC 5 x 5 descriptors of two random 8-bit images) and C = 64 (unit-normalised
Gaussian features).  Every group of measurements runs in a child process of its own under its own time limit; the first child that fails ends the
run.  Each number is the median of `reps` timings by the library's own events (LES_HIP_FEATVOL_TIMING=1) after two warm-up calls; the copy is a
group of one of tools/timing.py, which states the protocol.
Three yardsticks from the same run:
  (a) les_hip_calib_copy of D H W floats (a copy moves twice the bytes the kernel writes);
  (b) les_costvol_kernel at the same shape (LES_HIP_COSTVOL_TIMING=1): the store-bound builder of the AD-Census volume;
  (c) the MFMA issue floor of the tiles les_featvol_kernel issues -- workgroups x 4 waves x kFvTiles tiles x ceil(C / 2) instructions of
      64 cycles each on 256 CUs x 4 SIMDs at 2.4 GHz -- of which kFvChunk / (32 kFvTiles) = 2 / 3 land in the band.
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

SHAPE = (1436, 992, 256)
CHANNELS = (25, 64)
CHILD_SECONDS = 240
SEG, CHUNK, TILES = 128, 64, 3                      # kFvSeg, kFvChunk, kFvTiles of csrc/les_featvol.h
SIMDS, HZ, MFMA_CYCLES = 256 * 4, 2.4e9, 64         # MI355X: 256 CUs x 4 SIMDs, 2.4 GHz; v_mfma_f32_32x32x2_f32 issues every 64 cycles per SIMD


def mfma_floor_ms(W, H, D, Cn):
    n = -(-W // SEG) * H * -(-D // CHUNK) * 4 * TILES * -(-Cn // 2)
    return 1e3 * n * MFMA_CYCLES / SIMDS / HZ


def child_volume(torch, W, H, D, Cn, reps):
    import ctypes as C
    from localexpstereo_amd import api
    os.environ["LES_HIP_FEATVOL_TIMING"] = "1"
    L = api.load()
    rng = np.random.default_rng(1)
    a, b = C.c_float(), C.c_float()
    rec = {}
    if Cn == 25:
        feats, desc = [], []
        for _ in range(2):
            im = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
            f = torch.empty((Cn, H, W), dtype=torch.float32, device="cuda")
            for _ in range(2 + reps):
                api.patch_features(im.data_ptr(), f.data_ptr(), H, W, 2, 2)
                assert L.les_hip_featvol_last_times(C.byref(a), C.byref(b)) == 0
                desc.append(a.value)
            feats.append(f)
        rec["patch_features_5x5_one_image_ms"] = timing.spread(desc[2:2 + reps] + desc[4 + reps:], 4)
    else:
        feats = [torch.nn.functional.normalize(torch.randn((Cn, H, W), device="cuda"), dim=0).contiguous() for _ in range(2)]
    vol = torch.empty((D, H, W), dtype=torch.float32, device="cuda")
    for mode in (0, 1):
        ms = []
        for _ in range(2 + reps):
            api.build_feature_volume(feats[0].data_ptr(), feats[1].data_ptr(), vol.data_ptr(), Cn, D, H, W, mode)
            assert L.les_hip_featvol_last_times(C.byref(a), C.byref(b)) == 0
            ms.append(b.value)
        rec[f"mode{mode}"] = dict(volume_kernel_ms=timing.spread(ms[2:], 4))
    return rec


def child_baselines(torch, W, H, D, Cn, reps):
    import ctypes as C
    from localexpstereo_amd import api
    os.environ["LES_HIP_COSTVOL_TIMING"] = "1"
    L = api.load()
    rng = np.random.default_rng(1)
    copy = timing.copy_call(api, 2 * 4 * D * H * W, None)                       # a copy of D H W floats
    rec = dict(calib_copy_ms=timing.spread(timing.time_one(timing.Clock(torch, "cuda"), copy, reps, warm=2), 4))
    dst = copy.buffers[1]                                                       # (the builder writes where the copy wrote)
    imL, imR = (torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(2))
    a, b = C.c_float(), C.c_float()
    for mode in (0, 1):
        ms = []
        for _ in range(2 + reps):
            api.build_cost_volume(imL.data_ptr(), imR.data_ptr(), dst.data_ptr(), D, H, W, mode)
            assert L.les_hip_costvol_last_times(C.byref(a), C.byref(b)) == 0
            ms.append(b.value)
        rec[f"costvol_kernel_mode{mode}_ms"] = timing.spread(ms[2:], 4)
    return rec


def markdown(out):
    W, H, D = SHAPE
    base = out["baselines"]
    lines = [f"# les_featvol_kernel at {W} x {H} x {D}", "",
             f"{out['note']}; written by tools/featvol_timing.py, {out['reps']} repetitions.", "",
             f"Yardsticks of the same run: (a) les_hip_calib_copy of the volume's {4 * W * H * D / 1e9:.2f} GB {base['calib_copy_ms']['median']:.3f} ms; "
             f"(b) les_costvol_kernel {base['costvol_kernel_mode0_ms']['median']:.3f} ms (mode 0) / {base['costvol_kernel_mode1_ms']['median']:.3f} ms (mode 1); "
             f"(c) the MFMA issue floor of the issued tiles, below per C.  Band efficiency {CHUNK}/{32 * TILES} = {CHUNK / (32 * TILES):.3f}.", "",
             "| C | mode | kernel median (min .. max) ms | (c) MFMA issue floor ms | kernel / max(a, c) | in-band TFLOP/s |", "|---|---|---|---|---|---|"]
    for Cn in CHANNELS:
        rec = out[f"C{Cn}"]
        for mode in (0, 1):
            k = rec[f"mode{mode}"]["volume_kernel_ms"]
            lines.append(f"| {Cn} | {mode} | {k['median']:.3f} ({k['min']:.3f} .. {k['max']:.3f}) | {rec['mfma_issue_floor_ms']:.3f} | "
                         f"{k['median'] / max(base['calib_copy_ms']['median'], rec['mfma_issue_floor_ms']):.2f} | {2e-9 * Cn * W * H * D / k['median']:.1f} |")
    d = out["C25"]["patch_features_5x5_one_image_ms"]
    lines += ["", f"les_patch_features_kernel, 5 x 5, one {W} x {H} image: {d['median']:.3f} ms ({d['min']:.3f} .. {d['max']:.3f})."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "C"))
    a = ap.parse_args()
    W, H, D = SHAPE
    if a.child:
        torch = timing.require_gpu("featvol_timing.py")
        print("RESULT " + json.dumps((child_volume if a.child[0] == "volume" else child_baselines)(torch, W, H, D, int(a.child[1]), a.reps)))
        return
    out = dict(note="one MI355X, one run; medians of device-event timings after two warm-up calls", reps=a.reps, shape=f"{W}x{H}x{D}",
               band_efficiency=round(CHUNK / (32 * TILES), 4))
    for key, what, Cn in [("baselines", "baselines", 0)] + [(f"C{c}", "volume", c) for c in CHANNELS]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", what, str(Cn)], capture_output=True, text=True,
                           timeout=CHILD_SECONDS)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"featvol_timing.py: the {key} measurements failed (exit {p.returncode}); nothing further was run")
        out[key] = json.loads(lines[-1][len("RESULT "):])
        if Cn:
            out[key]["mfma_issue_floor_ms"] = round(mfma_floor_ms(W, H, D, Cn), 4)
    timing.write_record(a.out, out)
    print(markdown(out))
    if a.md:
        timing.write_text(a.md, markdown(out))


if __name__ == "__main__":
    main()
