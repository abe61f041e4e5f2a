"""Timing of the bilateral aggregation (csrc/les_bilateral.h) on the GPU: one whole-image pass of 256 planes at 1500 x 1000,
windR 20, cost-volume energy (one slab per plane: les_hip_batch_run with out_slabs = 1), and one lock-step of the finest MidV3 layer's
cells (unit = 1 % of the width).  Prints one JSON line.  Not part of bench.py.

    python tools/bf_timing.py [--planes 256] [--reps 5]
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

VALU_LANE_OPS = 256 * 2.4e9 * 64          # non-packed f32 VALU issue rate of the MI355X (lane-operations / s)


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
    e = api.HipCostVolumeEnergy(imL, imL, vol.data_ptr(), vol.data_ptr(), windR=R, eps=10.0, th_col=0.5, volumes_on_device=True,
                                shape=(D, H, W), filter="BF")
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    planes = np.zeros((n, 4), np.float32)
    planes[:, 0] = rng.uniform(-0.05, 0.05, n)
    planes[:, 1] = rng.uniform(-0.05, 0.05, n)
    planes[:, 2] = rng.uniform(5, D - 6, n)
    d_planes = torch.from_numpy(planes).cuda()
    out = torch.empty((n, H, W), device="cuda")
    full = [(0, 0, W, H)] * n
    b = api.Batch(e, full, full, out_slabs=1)
    assert b.kernel_kind(0) == 2
    run = lambda: b.run(d_planes.data_ptr(), out.data_ptr(), mode=0, check=True, planes_on_device=True)     # noqa: E731
    run()
    torch.cuda.synchronize()
    ms = timed(run, args.reps)
    med = timing.spread(ms, 3)["median"]
    # floor of this kernel in lane-operations per output and plane: per window tap one v_fma_f32, plus one v_sad_u8 and one shift per tap
    # and output shared by the 4 planes of a tile (the LDS reads of weights / costs and the f32 row sums are not counted)
    ops = (2 * R + 1) ** 2 * (1.0 + 2.0 / 4)
    floor_ms = H * W * n * ops / VALU_LANE_OPS * 1e3
    b.destroy()
    # one lock-step of the finest MidV3 layer (unit = 1 % of the width): set 0's cells, one plane each
    unit = int(W * 0.01)
    units, shared, filt, sets = pm.layer_geometry(W, H, R, unit)
    cells = sets[0]
    bl = api.Batch(e, filt[cells], shared[cells])
    cp = torch.from_numpy(np.repeat(planes[:1], len(cells), 0)).cuda()
    cmap = torch.empty((H, W), device="cuda")
    step = lambda: bl.run(cp.data_ptr(), cmap.data_ptr(), mode=0, check=True, planes_on_device=True)     # noqa: E731
    step()
    torch.cuda.synchronize()
    ls = timed(step, args.reps * 4)
    bl.destroy()
    e.close()
    print(json.dumps(dict(shape=[H, W], planes=n, windR=R, whole_image_pass_ms=med, whole_image_pass_ms_all=[round(x, 3) for x in ms],
                          floor_lane_ops_per_output=ops, floor_ms=round(floor_ms, 3), fraction_of_floor=round(floor_ms / med, 3),
                          target_ms=40.0, finest_layer_unit=unit, finest_layer_cells_per_lockstep=int(len(cells)),
                          lockstep_ms=timing.spread(ls, 4)["median"])))


if __name__ == "__main__":
    main()
