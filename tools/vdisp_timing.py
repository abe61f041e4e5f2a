"""Cost of the vertical disparity (Plane::v) in the image-based energy on the GPU: one whole-image pass of 256 planes at 1500 x 1000, windR 20
(one slab per plane: les_hip_batch_run with out_slabs = 1) at v = 0 and at v = 0.37, on the march kernel (windR 20) and on the strip
kernel (windR 30, no march instantiation); and the MidV2 cones run (5 iterations, 2 PatchMatch, one view) at vdisp 0 and at vdisp 2 on
energy and random proposer.  Writes profiles/vdisp_timing.json and prints it.  Not part of bench.py.

    python tools/vdisp_timing.py [--planes 256] [--reps 5] [--no-midv2]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timing  # noqa: E402
from localexpstereo_amd import api, io, stereo, synth  # noqa: E402


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
    ap.add_argument("--no-midv2", action="store_true")
    args = ap.parse_args()
    H, W, n = args.H, args.W, args.planes
    torch.cuda.init()
    imL, imR = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    rng = np.random.default_rng(3)
    planes = np.zeros((n, 4), np.float32)
    planes[:, 0] = rng.uniform(-0.05, 0.05, n)
    planes[:, 1] = rng.uniform(-0.05, 0.05, n)
    planes[:, 2] = rng.uniform(5, 200, n)
    out = torch.empty((n, H, W), device="cuda")
    full = [(0, 0, W, H)] * n
    res = dict(shape=[H, W], planes=n)
    for windR in (20, 30):
        e = api.HipCostVolumeEnergy.naive(imL, imR, windR=windR, max_disp=255.0)
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        b = api.Batch(e, full, full, out_slabs=1)
        ms = {}
        for v in (0.0, 0.37):
            planes[:, 3] = v
            d_planes = torch.from_numpy(planes).cuda()
            run = lambda: b.run(d_planes.data_ptr(), out.data_ptr(), mode=0, check=True, planes_on_device=True)     # noqa: E731
            run()
            torch.cuda.synchronize()
            t = timed(run, args.reps)
            ms[v] = timing.spread(t)["median"]
            res[f"windR{windR}_v{v}"] = dict(kernel_kind=b.kernel_kind(0), whole_image_pass_ms=round(ms[v], 3), all_ms=[round(x, 3) for x in t])
        res[f"windR{windR}_v0.37_over_v0"] = round(ms[0.37] / ms[0.0], 3)
        b.destroy()
        e.close()
    if not args.no_midv2:
        data = io.load_data(os.path.join(ROOT, "tests", "golden", "cones"), ndisp=64)
        for name, kw in (("vdisp0", {}), ("vdisp2", dict(vdisp=2.0, random_vdisp=2.0))):
            stereo.MidV2(data, iterations=1, pmIterations=1, doDual=False, **kw)          # warm-up (compilation of nothing; caches, allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st, lab, raw = stereo.MidV2(data, iterations=5, pmIterations=2, doDual=False, **kw)
            torch.cuda.synchronize()
            _, bad2 = io.Evaluator(data["dispGT"], data["nonocc"], 2.0).evaluate(stereo.disparities(lab))
            res[f"midv2_cones_{name}"] = dict(seconds=round(time.perf_counter() - t0, 3), bad2_nonocc=round(bad2, 3))
    timing.write_record(os.path.join(ROOT, "profiles", "vdisp_timing.json"), res)


if __name__ == "__main__":
    main()
