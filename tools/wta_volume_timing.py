#!/usr/bin/env python
"""Timings of the winner-take-all labels of the aggregated cost volume (csrc/les_wtavol.h) on the MI355X -> profiles/wta_volume_timing.json
(summarised in DESIGN 3.2g).

  python tools/wta_volume_timing.py [--out profiles/wta_volume_timing.json] [--skip-runs]

Recorded:
  * reduction: les_slab_argmin_kernel + the finish over a resident 256-slab volume at 1436 x 992 and 1500 x 1000 in chunks of 32 (8 step launches and
    the finish per timing; the volume, 1.4 - 1.5 GB, is streamed once per timing, so no chunk is re-read from the Infinity Cache), next to
    les_hip_calib_copy_wide over the same number of bytes read (which also writes them) -- each a group of one of tools/timing.py (which states
    the protocol) after 3 warm-up calls;
  * whole_call: les_hip_wta_labels on bench.py's H1 context (U[0,1) volume, guided filter, windR 20) at those sizes with chunks of 16 / 32 / 64, next
    to the H1 pass of the same build (one launch of the 256 fronto-parallel planes into 256 slabs);
  * runs (unless --skip-runs): the two synthetic scenes of tools/e2e_bench.py at 1436 x 992 x 256, two views, MidV3 energy and layers: the Evaluator
    log of a default run (2 PatchMatch + 5 graph-cut iterations) next to labeling="wta" with no PatchMatch iteration, energy per iteration and wall
    clock; and FastGCStereo.wta alone.
Nothing here is a gate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import timing  # noqa: E402

D = 256
SIZES = ((992, 1436), (1000, 1500))


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def time_size(torch, api, synth, h, w, timings):
    P = h * w
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    vol = torch.rand((D, h, w), device="cuda", dtype=torch.float32, generator=gen)
    e = api.HipCostVolumeEnergy(synth.make_guide(h, w, 1234), None, vol.data_ptr(), None, windR=20, eps=1e-4, th_col=0.5, max_disp=D - 1,
                                volumes_on_device=True, shape=(D, h, w))
    stream = torch.cuda.current_stream()
    e.set_stream(stream.cuda_stream)
    out = torch.empty((D, h, w), device="cuda", dtype=torch.float32)
    labels, cost = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w), device="cuda")
    state = torch.empty(e.slab_argmin_state_bytes() // 4, device="cuda")
    rec = dict(shape=[w, h, D], bytes_read=4 * D * P)
    clock = timing.Clock(torch, "cuda")
    one = lambda f: timing.spread(timing.time_one(clock, f, timings, warm=3), 4)

    # ---- the reduction alone, over the raw volume (any resident [256][H][W] floats do)
    def reduce(chunk=32):
        for k0 in range(0, D, chunk):
            e.slab_argmin(vol.data_ptr() + 4 * k0 * P, min(chunk, D - k0), k0, state.data_ptr())
        e.slab_argmin_finish(state.data_ptr(), D, labels.data_ptr(), cost.data_ptr())
    rec["reduction_ms_chunk32"] = one(reduce)
    rec["reduction_ms_one_chunk"] = one(lambda: reduce(D))
    rec["copy_wide_ms"] = one(timing.copy_call(api, 2 * rec["bytes_read"], stream.cuda_stream, wide=True))
    rec["reduction_over_copy"] = round(rec["reduction_ms_chunk32"]["median"] / rec["copy_wide_ms"]["median"], 3)
    rec["reduction_GBps"] = round(rec["bytes_read"] / rec["reduction_ms_chunk32"]["median"] / 1e6, 1)
    _note("reduction", rec["shape"], rec["reduction_ms_chunk32"], rec["reduction_ms_one_chunk"], rec["copy_wide_ms"])

    # ---- the whole call next to the H1 pass of this build
    full = [(0, 0, w, h)] * D
    batch = api.Batch(e, full, full, out_slabs=True)
    planes = torch.from_numpy(synth.fronto_planes(D)).cuda()
    rec["h1_kernel_kind"] = batch.kernel_kind(0)
    rec["h1_ms"] = one(lambda: batch.run(planes.data_ptr(), out.data_ptr(), mode=0, check=False, planes_on_device=True))
    _note("H1", rec["h1_ms"])
    for chunk in (16, 32, 64):
        rec[f"wta_labels_ms_chunk{chunk}"] = one(lambda: e.wta_labels(0, chunk, True, labels.data_ptr(), cost.data_ptr()))
        rec[f"wta_labels_minus_h1_ms_chunk{chunk}"] = round(rec[f"wta_labels_ms_chunk{chunk}"]["median"] - rec["h1_ms"]["median"], 4)
        _note("wta_labels chunk", chunk, rec[f"wta_labels_ms_chunk{chunk}"])
    batch.destroy()
    e.close()
    return rec


def time_runs(torch, api, stereo, lio, e2e_bench, scene):
    h, w = SIZES[0]
    imL, imR, gt, volL = e2e_bench.scene_inputs(scene, h, w, D, "cuda")
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.ingest_volumes(volL, None, device="cuda")
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(D - 1), volumes_on_device=True,
                                shape=(D, h, w), filter=p["filter"])

    def driver():
        st = stereo.FastGCStereo(e, imL, imR, p, device="cuda", seed=1, evaluate_on_device=True)
        st.setEvaluator(lio.Evaluator(gt, np.ones((h, w), bool), 1.0), precision=-1.0)
        stereo._layers(st, (int(w * 0.01), int(w * 0.03), int(w * 0.09)))
        return st

    def rows(st):
        return [dict(index=r["index"], seconds=round(r["time"], 3), energy=round(r["energy"], 1), bad1_all=round(r["all"], 3)) for r in st.log]
    rec = dict(scene=scene, shape=[w, h, D])
    st = driver()
    st.wta((0, 1))                                              # (warms the context's workspace up)
    st = driver()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st.wta((0, 1))
    rec["wta_only"] = dict(wall_seconds=round(time.perf_counter() - t0, 4), seconds=round(st.seconds, 4), rows=[dict(mode=r["mode"], energy=round(r["energy"], 1),
                                                                                                                      bad1_all=round(r["all"], 3) if "all" in r else None) for r in st.log])
    for name, pm_it, labeling in (("default", 2, None), ("wta_start_no_patchmatch", 0, "wta")):
        st = driver()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run(5, (0, 1), pm_it, labeling=labeling)
        rec[name] = dict(wall_seconds=round(time.perf_counter() - t0, 3), seconds=round(st.seconds, 3), pm_iterations=pm_it, gc_iterations=5, log=rows(st))
        _note(scene, name, rec[name]["seconds"], "s, final energy", rec[name]["log"][-2]["energy"], "bad1", rec[name]["log"][-1]["bad1_all"])
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--timings", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true", help="the kernel and whole-call timings only")
    ap.add_argument("--skip-kernels", action="store_true", help="the end-to-end runs only")
    a = ap.parse_args()
    torch = timing.require_gpu("wta_volume_timing.py")
    import e2e_bench
    from localexpstereo_amd import api, io as lio, stereo, synth
    rec = dict(timings=a.timings)
    if not a.skip_kernels:
        rec["sizes"] = [time_size(torch, api, synth, h, w, a.timings) for h, w in SIZES]
    if not a.skip_runs:
        rec["runs"] = [time_runs(torch, api, stereo, lio, e2e_bench, scene) for scene in ("objects", "three_surfaces")]
    timing.write_record(a.out, rec)


if __name__ == "__main__":
    main()
