"""Kernel + launch logic of localexpstereo_amd/csrc compiled for the CPU SIMT simulator
(tools/hipsim) and compared with the oracle.  Runs without a GPU (-m "not gpu").  The simulator
build is test infrastructure: the same cases run against the real gfx950 build in test_gpu_parity.py."""
import os

import numpy as np
import pytest

from tests import parity_cases as pc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


@pytest.fixture(scope="module")
def cones(sim_lib, oracle_mod):
    pr = pc.cones_pair(sim_lib)
    yield pr
    pr.close()


def test_sim_stats(cones):
    pc.case_stats(cones)


def test_sim_single_calls(cones):
    assert pc.case_single_calls(cones) <= pc.TIGHT


def test_sim_special_planes(cones):
    pc.case_special_planes(cones)


def test_sim_cell_batches_layer0(cones):
    pc.case_cell_batches(cones, unit=8, sets=(0, 7))


def test_sim_cell_batch_multi_strip(sim_lib, oracle_mod):
    # shared regions wider than one strip (44 columns at R=10) and taller than a row block
    pr = pc.synth_pair(sim_lib, 110, 150, 12)
    try:
        pc.case_cell_batches(pr, unit=25, sets=(0, 3), mode=1)
        pc.case_init_cells(pr, unit=30)
    finally:
        pr.close()


def test_sim_kernel_dispatch_and_strip_kernel(sim_lib, oracle_mod, monkeypatch):
    """The march kernel (csrc/les_march.h) serves LayerManager cells and whole-image slabs; targets hugging a filterRect border
    and contexts created with LES_HIP_KERNEL=strip run the fp64 strip kernel -- both against the oracle."""
    pr = pc.synth_pair(sim_lib, 100, 140, 6)
    try:
        layer = pc.om.Layer(pr.W, pr.H, 20, 15)
        cells = layer.sets[3]
        b = pc.api.Batch(pr.e, layer.filter[cells], layer.shared[cells])
        assert b.kernel_kind(0) == 1
        b.destroy()
        b = pc.api.Batch(pr.e, [(20, 20, 100, 70)], [(25, 40, 40, 30)])
        assert b.kernel_kind(0) == 0
        b.destroy()
        planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, 31)
        ref = pr.o.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        got_march = pr.e.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        pc.compare_maps(got_march, ref)
    finally:
        pr.close()
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    pr = pc.synth_pair(sim_lib, 100, 140, 6)
    try:
        b = pc.api.Batch(pr.e, layer.filter[cells], layer.shared[cells])
        assert b.kernel_kind(0) == 0
        b.destroy()
        got_strip = pr.e.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        pc.compare_maps(got_strip, ref)
    finally:
        pr.close()


def test_sim_march_wide_jobs_and_fronto_planes(sim_lib, oracle_mod):
    """Whole-image slabs wider than one wide march job (216 columns): several strips, fronto-parallel (per-job taps) and slanted
    planes, interpolated and integer disparities, both views."""
    pr = pc.synth_pair(sim_lib, 64, 470, 5)
    try:
        planes = np.array([[0, 0, 2, 0], [0, 0, 1.25, 0], [0, 0, -3, 0], [0, 0, 9, 0], [0.004, -0.01, 1.5, 0]], np.float32)
        for mode in (0, 1):
            out = pc.run_slabs(pr, planes, mode=mode, check=True)
            for i in range(len(planes)):
                ref = pr.o.unary((0, 0, pr.W, pr.H), (0, 0, pr.W, pr.H), tuple(planes[i]), mode=mode, check=True)
                pc.compare_maps(out[i], ref)
    finally:
        pr.close()


def test_sim_plane_slabs(cones):
    pc.case_plane_slabs(cones, n=3)


def test_sim_tiled_copy_taps_equal_planar_taps(sim_lib, oracle_mod, monkeypatch):
    assert pc.case_tiled_taps(sim_lib, H=110, W=139, D=12, monkeypatch=monkeypatch) <= pc.TIGHT


def test_sim_grouped_slots(cones):
    worst, kind = pc.case_grouped_slots(cones, unit=10, set_index=2, slots=3)
    assert kind == 1


def test_sim_small_radius(sim_lib, oracle_mod):
    # windR = 4 -> guided-filter radius 2 (a different kernel instantiation), tiny image, min_disp != 0 is not
    # exercised by the reference's shipped modes but the arithmetic (D0) is restated
    pr = pc.synth_pair(sim_lib, 40, 70, 6, windR=4, eps=1e-3, th_col=0.8)
    try:
        layer = pc.om.Layer(pr.W, pr.H, 4, 9)
        cells = layer.sets[0]
        planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, 4)
        ref = pr.o.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        got = pr.e.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        pc.compare_maps(got, ref)
    finally:
        pr.close()


@pytest.mark.parametrize("windR", [2, 4, 6, 8, 10, 14, 17, 30])     # radii 1 (strip kernel), 2, 3 (rings of 6 and 9 rows), 4, 5 (ring longer than the window), 7, 8 (the same), 15 (strip kernel); the GPU sweep runs all
def test_sim_other_radii(sim_lib, oracle_mod, windR):
    pr = pc.synth_pair(sim_lib, 60, 100, 6, windR=windR, eps={2: 1e-2, 4: 1e-3}.get(windR, 1e-4), th_col=0.5)
    try:
        layer = pc.om.Layer(pr.W, pr.H, windR, 13)
        cells = layer.sets[1]
        b = pc.api.Batch(pr.e, layer.filter[cells], layer.shared[cells])
        # guided-filter radii 2 .. 10 have march-kernel instantiations (5, 6, 8, 9: rings longer than the window), 1 and 15 do not
        assert b.kernel_kind(0) == (1 if 2 <= windR // 2 <= 10 else 0)
        b.destroy()
        planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, 8)
        ref = pr.o.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        got = pr.e.unary_batch(layer.filter[cells], layer.shared[cells], planes)
        pc.compare_maps(got, ref)
    finally:
        pr.close()


def test_sim_min_disparity_and_unsupported(sim_lib, oracle_mod):
    """MIN_DISPARITY != 0 (D0 = int(-MIN), LES/CostVolumeEnergy.h:67) and the error path for radii without a kernel."""
    from localexpstereo_amd import api, synth
    pr = pc.synth_pair(sim_lib, 50, 80, 8, max_disp=5.0, min_disp=-2.0)
    try:
        for pl in [(0.0, 0.0, 1.5, 0.0), (0.05, -0.02, -1.25, 0.0), (0.0, 0.0, -3.0, 0.0), (0.0, 0.0, 5.0, 0.0)]:
            fr, tr = (5, 4, 70, 44), (25, 24, 30, 10)
            ref = pr.o.unary(fr, tr, pl)
            got = pr.e.ComputeUnaryPotential(fr, tr, np.full((pr.H, pr.W), np.nan, np.float32), pl)
            pc.compare_maps(got, ref)
    finally:
        pr.close()
    im, vol = synth.make_guide(40, 60, 1), synth.make_volume(4, 40, 60, 2)
    with pytest.raises(api.LesHipError):
        api.HipCostVolumeEnergy(im, None, vol, None, windR=44, lib=sim_lib)      # radius 22: no kernel instantiated


def test_sim_empty_and_errors(cones):
    pc.case_empty_and_errors(cones)


def test_sim_warm_start(sim_lib, oracle_mod):
    pc.case_warm_start(sim_lib, "cpu")


def test_sim_widened_abi_errors(sim_lib, oracle_mod):
    pc.case_widened_abi_errors(sim_lib)


def test_sim_wta(cones):
    pc.case_wta(cones)


def test_sim_matches_golden_fixture(cones):
    g = np.load(os.path.join(pc.om._HERE, "..", "tests", "golden", "golden_unary.npz"))
    for i in range(int(g["n"])):
        fr, tr = tuple(int(v) for v in g[f"fr{i}"]), tuple(int(v) for v in g[f"tr{i}"])
        got = cones.e.ComputeUnaryPotential(fr, tr, np.full((cones.H, cones.W), np.nan, np.float32),
                                            tuple(float(v) for v in g[f"plane{i}"]), mode=int(g[f"mode{i}"]))
        x, y, w, h = tr
        ref = np.full((cones.H, cones.W), np.nan, np.float32)
        ref[y:y + h, x:x + w] = g[f"out{i}"]
        pc.compare_maps(got, ref)


def test_sim_proposers(cones):
    pc.case_proposers(cones, unit=14, set_index=5)


def test_sim_ransac_adaptive_schedule(cones):
    """Chunked candidates with the reference's early stop: planar, noisy and garbage label maps against the oracle, cell by cell."""
    far = pc.case_ransac_schedule(cones, combos=((14, 0.0), (14, 0.3), (14, 3.0), (30, 20.0)))
    assert far[(14, 0.0)] == 0.0, far            # exactly planar regions: the loop ends with its first sample
    assert far[(30, 20.0)] > 0.5, far            # garbage: (nearly) every cell goes through all chunks


def test_sim_pm_iteration(sim_lib, oracle_mod):
    pr = pc.synth_pair(sim_lib, 48, 64, 10)
    try:
        steps, worst = pc.case_pm_iteration(pr, layers_units=(10, 30), plane_exact=True)
        assert steps > 100 and worst <= pc.TIGHT
    finally:
        pr.close()


def test_sim_volume_preparation(cones, sim_lib):
    pc.case_volume_preparation(cones, sim_lib)


def test_sim_expansion_graph_on_device(cones):
    """Pairwise terms / graph capacities on the device (N1): bit-identical to the host construction."""
    from localexpstereo_amd import build
    build.build_host_lib()
    pc.case_expansion_graph(cones)


def test_sim_device_maxflow_widest_cells(sim_lib, oracle_mod):
    """csrc/les_maxflow_cell.h on its widest and tallest cells (250 x 7, 440 x 3, 3 x 70 next to the usual awkward shapes) against the host solver."""
    from localexpstereo_amd import build
    build.build_host_lib()
    pr = pc.synth_pair(sim_lib, 96, 450, 4)
    try:
        pc.case_device_maxflow_edge_cells(pr, seed=5, kind=0)
    finally:
        pr.close()


def test_sim_device_maxflow_edge_cells(cones, monkeypatch):
    """The one-workgroup device max-flows (csrc/les_maxflow_cell.h, and csrc/les_maxflow.h for cells beyond it or on request) on hand-made graphs of
    awkward shapes against the host solver."""
    from localexpstereo_amd import build
    build.build_host_lib()
    pc.case_device_maxflow_edge_cells(cones, kind=0)
    pc.case_device_maxflow_edge_cells(cones, kind=2)                       # (the 48 x 48 cell does not fit les_maxflow_cell.h)
    monkeypatch.setenv("LES_HIP_MAXFLOW_CELL_KERNEL", "0")
    pc.case_device_maxflow_edge_cells(cones, seed=4, kind=2)


def test_sim_refresh_volume(sim_lib, oracle_mod):
    """les_hip_refresh_volume after an in-place refill of a device-resident volume == a context created on the new volume."""
    assert pc.case_refresh_volume(sim_lib) > 0


def test_sim_tiled_device_maxflow(sim_lib, oracle_mod):
    """The region-parallel device max-flow for cells of any size (csrc/les_maxflow_tiled.h): awkward shapes against the host solver,
    small cells against networkx and exhaustive enumeration, cells of several tiles against networkx and the host solver, and the two
    committed crops of real hard lock-steps against the host solver."""
    pr = pc.synth_pair(sim_lib, 140, 210, 4)
    try:
        pc.case_device_maxflow_edge_cells(pr, tiled=True)
        cells, nodes, diff = pc.case_device_maxflow_vs_networkx(pr, seed=5, ncells=6, max_side=24, tiled=True)
        assert diff <= 2e-4 * nodes + 2
        pc.case_device_maxflow_vs_brute_force(pr, seed=9, ncells=10, tiled=True)
        cells, nodes, ties = pc.case_tiled_maxflow_large_cells(pr, shapes=[(100, 70), (65, 31), (210, 1), (1, 140), (31, 65)])
        assert ties <= 2e-4 * nodes + 2
        assert pc.case_tiled_maxflow_hard_cells(pr) > 0
    finally:
        pr.close()


def test_sim_tiled_maxflow_handover(sim_lib, oracle_mod, monkeypatch):
    """Straggler cells of the tiled device max-flow finished by the host cores from their residual graphs: same cuts, same flow values."""
    pr = pc.synth_pair(sim_lib, 140, 210, 4)
    try:
        assert pc.case_tiled_maxflow_handover(pr, monkeypatch, shapes=[(100, 70), (65, 31), (129, 129), (31, 65)]) > 0
    finally:
        pr.close()
    for which in ("cells", "nodes"):                                          # the first selection exceeds the first staging: a fresh context each
        pr = pc.synth_pair(sim_lib, 270, 310, 4)
        try:
            pc.case_tiled_maxflow_handover_staging_growth(pr, monkeypatch, which)
        finally:
            pr.close()


def test_sim_cut_is_a_function_of_the_cell(sim_lib, oracle_mod, monkeypatch):
    """A cell's device cut does not depend on the other cells of its lock-step (their kind, order, number): both one-workgroup kernels and the
    tiled solver with and without the hand-over, against the cell cut alone, bit for bit (tests/parity_cases.py).  Sizes of the simulator pair."""
    from localexpstereo_amd import build
    build.build_host_lib()
    pr = pc.synth_pair(sim_lib, 140, 210, 4)
    try:
        c = pc.case_cut_is_a_function_of_the_cell(pr, "workgroup", [(32, 64), (41, 50), (126, 16), (152, 13), (29, 70), (27, 71), (48, 48), (42, 42), (13, 7), (1, 17), (19, 1)],
                                                  monkeypatch=monkeypatch)
        print("one workgroup per cell:", c)
        c = pc.case_cut_is_a_function_of_the_cell(pr, "tiled", [(100, 70), (65, 31), (210, 1), (1, 140), (31, 65), (64, 30), (40, 40)], monkeypatch=monkeypatch,
                                                  networkx_nodes=2500)
        print("tiled:", c)
        assert c["handed"] > 0
    finally:
        pr.close()


def test_sim_device_maxflow_against_independent_checkers(cones):
    """The same kernel source against networkx and brute force (no product code as the checker); the full-size version runs on the GPU."""
    cells, nodes, diff = pc.case_device_maxflow_vs_networkx(cones, seed=5, ncells=8, max_side=24, kind=0)
    assert diff <= 1e-3 * nodes
    pc.case_device_maxflow_vs_brute_force(cones, seed=9, ncells=12, kind=0)
    os.environ["LES_HIP_MAXFLOW_CELL_KERNEL"] = "0"                          # les_maxflow.h on the same cells
    try:
        cells, nodes, diff = pc.case_device_maxflow_vs_networkx(cones, seed=5, ncells=8, max_side=24, kind=1)
        assert diff <= 1e-3 * nodes
        pc.case_device_maxflow_vs_brute_force(cones, seed=9, ncells=12, kind=1)
    finally:
        del os.environ["LES_HIP_MAXFLOW_CELL_KERNEL"]


def test_sim_exchange_pack_unpack(cones):
    assert pc.case_exchange_pack_unpack(cones) > 0


def test_sim_graph_cut_iterations(sim_lib, oracle_mod, monkeypatch):
    """PatchMatch + graph-cut iterations through the Python driver: simulator proposals / unary costs, host cuts.
    (Driver and host-cut logic are under test: the fiber simulator runs them on the 256-thread strip kernel, ~4x faster than on the
    768-thread march kernel, which test_sim_pm_iteration and the cell-batch cases cover.)"""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    from localexpstereo_amd import build
    build.build_host_lib()
    hist, gap = pc.case_quality_cones_gc(sim_lib, "cpu", units=(12,))
    print("cones crop PM+GC (bad1.0, data, smooth):", hist, "max flow-energy gap", gap)


def test_sim_graph_cut_iteration_with_device_cuts(sim_lib, oracle_mod, monkeypatch):
    """The same driver with the cells cut by the device max-flow kernel (run here by the fiber simulator): the iteration lowers the
    energy and every cell that fits is cut on the "device"."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    from localexpstereo_amd import build
    build.build_host_lib()
    hist, gap = pc.case_quality_cones_gc(sim_lib, "cpu", units=(12,), device_cuts=True, table=[[(pc.api.PROPOSE_EXPANSION, 1), (pc.api.PROPOSE_RANDOM, 1)]],
                                         check_quality=False)      # (two proposals per cell: the energy must go down, convergence is not expected)
    print("cones crop PM+GC with device cuts (bad1.0, data, smooth):", hist)


def test_sim_gc_sets_without_round_trips(sim_lib, oracle_mod, monkeypatch):
    """The finest layer's disjoint sets enqueued without per-lock-step status reads == the per-lock-step path, bit for bit; the roll-back path too."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    from localexpstereo_amd import build
    build.build_host_lib()
    done, rolled = pc.case_gc_sets_without_round_trips(sim_lib, "cpu", monkeypatch)
    assert done > 0 and rolled > 0


def test_sim_two_views_joint_lock_steps(sim_lib, oracle_mod, monkeypatch):
    """Both views advanced in lock-step by pm.PMRunner.gc_iteration_joint (one host team cuts the cells of both) == view after view, bytes equal."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    from localexpstereo_amd import build
    build.build_host_lib()
    pc.case_joint_views(sim_lib, "cpu", units=(16,))


def test_sim_ingest_files(sim_lib, oracle_mod, tmp_path):
    pc.case_ingest_files(sim_lib, "cpu", tmp_path)


def test_sim_post_process(cones):
    """Dual-view post-processing (LR check, fill, weighted median): bit-identical labels."""
    assert pc.case_post_process(cones) > 0.01


def test_sim_naive_energy(sim_lib, oracle_mod):
    """Image-based matching cost of config 1 (NaiveStereoEnergy) through the same kernels."""
    worst = pc.case_naive(sim_lib)
    print("naive energy max abs err", worst)


def test_sim_quality_on_cones_crop(sim_lib):
    """The same end-to-end check through the simulator build (1 iteration: the simulator is slow)."""
    imL, vol, gt = pc.cones_ad_volume()
    assert vol.shape == (64, 96, 120) and (gt > 0).mean() > 0.9
    # ground-truth planes score far better than wrong ones under this volume (sanity of the cost construction)
    ys, xs = np.mgrid[0:96, 0:120]
    d = np.clip(np.rint(gt).astype(int), 0, 63)
    assert float(vol[d, ys, xs][gt > 0].mean()) < 0.5 * float(vol[(d + 7) % 64, ys, xs][gt > 0].mean())
