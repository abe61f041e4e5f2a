"""Timing of the three interpolation methods (les_hip_set_interpolation) of the guided-filter cost-volume energy on the GPU: one whole-image
pass of 256 planes at 1500 x 1000, windR 20 (one slab per plane: les_hip_batch_run with out_slabs = 1), and one lock-step of the finest
MidV3 layer's cells (unit = 1 % of the width), at interpolation 0, 1 and 2, on two plane sets:
  clean -- every plane stays inside slices 7 .. 57 over the whole image, so no call of interpolation 2 is flagged;
  wide  -- tools/bf_timing.py's planes (slopes up to 0.05: most of them reach slice 0 or D - 1 somewhere, where the quadratic is NaN),
           so most calls of interpolation 2 are recomputed on the strip kernel.
Prints one JSON line.  Not part of bench.py.

    python tools/interp_timing.py [--planes 256] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timing  # noqa: E402
from localexpstereo_amd import api, pm, synth  # noqa: E402


def timed(fn, reps):
    """Sorted ms of `reps` calls queued back to back, every pair of events recorded before the one synchronise: the one loop tools/timing.py does
    not state (its clock synchronises after every timing); the median is timing.spread's."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--H", type=int, default=1000)
    ap.add_argument("--W", type=int, default=1500)
    ap.add_argument("--D", type=int, default=64)
    args = ap.parse_args()
    H, W, D, n, R = args.H, args.W, args.D, args.planes, 20
    torch.cuda.init()
    g = torch.Generator(device="cuda").manual_seed(1)
    vol = torch.rand((D, H, W), device="cuda", generator=g) * 0.8
    imL = synth.make_guide(H, W, 1234)
    e = api.HipCostVolumeEnergy(imL, imL, vol.data_ptr(), vol.data_ptr(), windR=R, eps=1e-4, th_col=0.5, volumes_on_device=True, shape=(D, H, W))
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    wide = np.zeros((n, 4), np.float32)
    wide[:, 0] = rng.uniform(-0.05, 0.05, n)
    wide[:, 1] = rng.uniform(-0.05, 0.05, n)
    wide[:, 2] = rng.uniform(5, D - 6, n)
    clean = np.zeros((n, 4), np.float32)
    clean[:, 0] = rng.uniform(-0.01, 0.01, n)
    clean[:, 1] = rng.uniform(-0.01, 0.01, n)
    zc = rng.uniform(D / 2 - 12, D / 2 + 12, n)                   # disparity at the image centre
    clean[:, 2] = zc - clean[:, 0] * (W / 2) - clean[:, 1] * (H / 2)
    out = torch.empty((n, H, W), device="cuda")
    full = [(0, 0, W, H)] * n
    b = api.Batch(e, full, full, out_slabs=1)
    unit = int(W * 0.01)
    units, shared, filt, sets = pm.layer_geometry(W, H, R, unit)
    cells = sets[0]
    bl = api.Batch(e, filt[cells], shared[cells])
    cmap = torch.empty((H, W), device="cuda")
    res = dict(shape=[H, W], planes=n, windR=R, finest_layer_unit=unit, finest_layer_cells_per_lockstep=int(len(cells)))
    for name, planes, interp in [(s, p, i) for s, p in (("clean", clean), ("wide", wide)) for i in (0, 1, 2)]:
        d_planes = torch.from_numpy(planes).cuda()
        cp = torch.from_numpy(np.repeat(planes[:1], len(cells), 0)).cuda()
        e.setInterpolationMethod(interp)
        run = lambda: b.run(d_planes.data_ptr(), out.data_ptr(), mode=0, check=True, planes_on_device=True)     # noqa: E731
        run()
        torch.cuda.synchronize()
        ms = timed(run, args.reps)
        step = lambda: bl.run(cp.data_ptr(), cmap.data_ptr(), mode=0, check=True, planes_on_device=True)     # noqa: E731
        step()
        torch.cuda.synchronize()
        ls = timed(step, args.reps * 4)
        res[f"{name}_interp{interp}"] = dict(kernel_kind=b.kernel_kind(0), whole_image_pass_ms=timing.spread(ms, 3)["median"],
                                      whole_image_pass_ms_all=[round(x, 3) for x in ms], lockstep_kernel_kind=bl.kernel_kind(0),
                                      lockstep_ms=timing.spread(ls, 4)["median"])
    for name in ("clean", "wide"):
        for interp in (0, 2):
            res[f"{name}_interp{interp}_over_linear"] = round(res[f"{name}_interp{interp}"]["whole_image_pass_ms"] /
                                                               res[f"{name}_interp1"]["whole_image_pass_ms"], 3)
    b.destroy()
    bl.destroy()
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
