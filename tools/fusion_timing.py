#!/usr/bin/env python
"""Timings of the fusion moves (csrc/les_pairwise.h) on the MI355X -> profiles/fusion_timing.json (summarised in DESIGN 3.4b).

  python tools/fusion_timing.py [--out profiles/fusion_timing.json]

The synthetic "objects" scene of tools/e2e_bench.py at 1436 x 992 x 256 under the MidV3 energy and layers (1 % / 3 % / 9 % of the width).  The
two label maps are the scene's one-view solutions from seeds 1 and 2 (one PatchMatch and two graph-cut iterations each).  Recorded:
  * graph_kernels: per layer, the device time of a lock-step of les_move_graph_kernel<true> (label map: fusion) next to les_move_graph_kernel<false>
    (one plane per cell: expansion) on the same batches (every disjoint set of the layer; one group of tools/timing.py, which states the
    protocol: one warm-up call, no single launches, 5 rounds of bursts of 20 launches, median), and their ratio;
  * fuse: the whole stereo.FastGCStereo.fuse pass (warm start excluded) and the dense pass inside it (host clock around a synchronise), the share
    of non-submodular pairs, and the three energies E(a), E(b), E(fuse(a, b)) from the device evaluator.
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

H, W, D = 992, 1436, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    torch = timing.require_gpu("fusion_timing.py")
    import e2e_bench
    from localexpstereo_amd import api, gc as lgc, io as lio, pm, stereo
    imL, imR, gt, volL = e2e_bench.scene_inputs("objects", H, W, D, "cuda")
    p = dict(stereo.PARAMS_GF, lambda_=0.5, windR=20, th_col=0.5)
    tl, tr = lio.ingest_volumes(volL, None, device="cuda")
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=20, eps=p["eps"], th_col=0.5, max_disp=float(D - 1), volumes_on_device=True,
                                shape=(D, H, W), filter=p["filter"])

    def driver(seed):
        st = stereo.FastGCStereo(e, imL, imR, p, device="cuda", seed=seed, evaluate_on_device=True)
        st.setEvaluator(lio.Evaluator(gt, np.ones((H, W), bool), 1.0), precision=-1.0)
        stereo._layers(st, (int(W * 0.01), int(W * 0.03), int(W * 0.09)))
        return st

    maps, solve_seconds = [], []
    for seed in (1, 2):
        st = driver(seed)
        st.run(2, (0,), 1)
        maps.append(st.raw_labelings[0])
        solve_seconds.append(round(st.seconds, 3))
    la, lb = maps

    # ---- the two graph kernels on the same batches
    st = driver(1)
    r = pm.PMRunner(e, st.units, st.table, seed=1, device="cuda")
    g = lgc.GraphCut(imL, imR, lambda_=p["lambda_"], th_smooth=p["th_smooth"], omega=p["omega"], epsilon=p["epsilon"])
    r.init_from_labels(la)
    r.begin_gc(g)
    b_dev = torch.from_numpy(np.ascontiguousarray(lb, np.float32)).cuda()
    e.unary_labels(b_dev.data_ptr(), r.prop.data_ptr(), mode=0, check=True)
    pw = g.params
    clock = timing.Clock(torch, "cuda")
    kernels = {}
    for li, layer in enumerate(r.shards):
        rec = dict(locksteps=0, cells=0, nodes=0, fusion_us=[], expansion_us=[])
        for sh in [s for s in layer if s.n]:
            r._gc_buffers(sh)
            sh.batch.propose(api.PROPOSE_EXPANSION, r.labels.data_ptr(), sh.rng.data_ptr(), sh.planes.data_ptr(), m=0)
            fus = lambda: sh.batch.fusion_graph(b_dev.data_ptr(), r.labels.data_ptr(), r.cur.data_ptr(), r.prop.data_ptr(), sh.payload.data_ptr(), mode=0, **pw)
            exp = lambda: sh.batch.expansion_graph(sh.planes.data_ptr(), r.labels.data_ptr(), r.cur.data_ptr(), r.prop.data_ptr(), sh.payload.data_ptr(), mode=0, **pw)
            _, t = timing.time_calls(clock, dict(fusion=fus, expansion=exp), 0, warm=1, burst=a.launches, burst_rounds=a.rounds)
            rec["fusion_us"].append(1e3 * float(np.median(t["fusion"])))
            rec["expansion_us"].append(1e3 * float(np.median(t["expansion"])))
            rec["locksteps"] += 1
            rec["cells"] += sh.n
            rec["nodes"] += sh.graph_nodes
        f_sum, e_sum = sum(rec["fusion_us"]), sum(rec["expansion_us"])
        kernels[f"layer{li}"] = dict(unit=st.units[li], locksteps=rec["locksteps"], cells=rec["cells"], nodes=rec["nodes"], fusion_us_per_lockstep=timing.spread(rec["fusion_us"], 3),
                                     expansion_us_per_lockstep=timing.spread(rec["expansion_us"], 3), fusion_us_layer=round(f_sum, 2), expansion_us_layer=round(e_sum, 2),
                                     ratio=round(f_sum / e_sum, 3))
    r.close(); g.close()

    # ---- the whole pass through the driver, three times (the first one warms the launches up)
    passes = []
    for _ in range(3):
        st = driver(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.fuse(la, [lb])
        wall = time.perf_counter() - t0
        fs = st.fuse_stats[0]
        passes.append(dict(fuse_seconds=round(fs["seconds"], 4), dense_seconds=round(fs["dense_seconds"], 4), driver_seconds_with_warm_start_and_rows=round(wall, 4),
                           cells=fs["cells"], pixels_taken=fs["pixels_taken"], nonsubmodular_pairs=fs["nonsubmodular_pairs"], pairs=fs["pairs"],
                           nonsubmodular_share=round(fs["nonsubmodular_pairs"] / fs["pairs"], 5), E_a=st.log[0]["energy"], E_fused=st.log[1]["energy"],
                           bad1_a=st.log[0]["all"], bad1_fused=st.log[1]["all"]))
    st = driver(1)
    st.fuse(lb, [])
    E_b, bad_b = st.log[0]["energy"], st.log[0]["all"]
    rec = dict(shape=[W, H, D], scene="objects", maps="one-view solutions of seeds 1 and 2 (1 PatchMatch + 2 graph-cut iterations)", solve_seconds=solve_seconds,
               launches_per_timing=a.launches, rounds=a.rounds, graph_kernels=kernels,
               fuse=dict(passes=passes, fuse_seconds=timing.spread([q["fuse_seconds"] for q in passes[1:]], 3), dense_seconds=timing.spread([q["dense_seconds"] for q in passes[1:]], 3),
                         E_a=passes[-1]["E_a"], E_b=E_b, E_fused=passes[-1]["E_fused"], bad1_a=passes[-1]["bad1_a"], bad1_b=bad_b, bad1_fused=passes[-1]["bad1_fused"],
                         nonsubmodular_share=passes[-1]["nonsubmodular_share"]))
    timing.write_record(a.out, rec)
    e.close()


if __name__ == "__main__":
    main()
