"""The device-side Evaluator (csrc/les_eval.h): energy, bad-pixel rates and the flow == energy self-check computed from the device-resident
solution -- les_hip_evaluate / les_hip_batch_region_energy, api.DeviceEvaluator, pm.PMRunner.energy, and the opt-in switches of
stereo.FastGCStereo (evaluate_on_device, inner_loop_log, check_flow_energy = "device").  CPU simulator build (-m "not gpu") and MI355X (-m gpu).
The cases, the references and the derivation of the sum tolerance are in tests/eval_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


def _two_proposals():
    return [[(ec.api.PROPOSE_EXPANSION, 1), (ec.api.PROPOSE_RANDOM, 1)]]


# ---------------------------------------------------------------- the references themselves
def test_restatement_matches_per_pixel_loop():
    ec.case_restatement_matches_loop()


def test_restated_coefficient_table_is_the_hosts(host_lib):
    ec.case_table_matches_host()


# ---------------------------------------------------------------- CPU simulator build
def test_sim_terms_bit_for_bit(sim_lib):
    print(ec.case_terms_bit_for_bit(sim_lib))


def test_sim_sums(sim_lib):
    print("worst relative difference to fsum:", ec.case_sums(sim_lib))
    ec.case_nonfinite(sim_lib)


def test_sim_rates(sim_lib):
    print(ec.case_rates(sim_lib))


def test_sim_determinism_and_stream_order(sim_lib):
    ec.case_determinism_and_stream_order(sim_lib, "cpu")


def test_sim_runner_energy(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    ec.case_runner_energy(sim_lib, "cpu")


def test_sim_region_energy(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print("cells checked, of them at the image border:", ec.case_region_energy(sim_lib, "cpu"))


def test_sim_the_check_can_fail(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print("gap of the cut, cells reported for edited masks:", ec.case_check_can_fail(sim_lib, "cpu"))


def test_sim_whole_runs(sim_lib, monkeypatch):
    """The cones crop as test_sim_kernels.py: test_sim_graph_cut_iteration_with_device_cuts (cost-volume energy, one layer of 12-px units, two
    proposals per cell, device cuts), one PatchMatch and two graph-cut iterations through stereo.FastGCStereo.  Measured here: no set raised
    the data term (PatchMatch) or the energy (graph cuts), with device cuts and with host cuts."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    kw = dict(units=(12,), pmInit=1, maxIteration=2, device_cuts=True, table=_two_proposals(), energy="volume")
    print(ec.whole_run_cases(sim_lib, "cpu", kw, 96 * 120))


def test_sim_check_flow_energy_on_the_device_path(sim_lib, monkeypatch):
    """Measured here (one-workgroup cell kernel under the simulator): the solver's own flow value is up to 9.8e-3 off next to the 1e6 terminals of
    invalid proposals (31 of 64 lock-steps miss 1e-5 with it); against the host solver's flow on the same graphs the worst gap is 2.4e-8."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    kw = dict(units=(12,), pmInit=1, maxIteration=2, device_cuts=True, table=_two_proposals(), energy="volume")
    print(ec.check_device_run(sim_lib, "cpu", kw))


def test_sim_inner_loop_log_with_joint_views(sim_lib, monkeypatch):
    """The log rides on pm.PMRunner.gc_iteration_joint unchanged: same labels, a row per view and set."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    from localexpstereo_amd import stereo
    out = []
    for inner in (False, True):
        imL, imR, gt = ec.cones_images()
        e = ec.api.HipCostVolumeEnergy.naive(imL, imR, max_disp=63.0, lib=sim_lib)
        st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=1.0), device="cpu", seed=3, device_cuts=False, inner_loop_log=inner)
        st.setEvaluator(ec.lio.Evaluator(gt, gt > 0, 1.0), precision=0.25)
        st.joint_views, st.concurrent_views = True, False
        st.addLayer(16, [(ec.api.PROPOSE_EXPANSION, 1), (ec.api.PROPOSE_RANSAC, 1)])
        lab, raw = st.run(1, (0, 1), 1)
        e.close()
        out.append((lab, raw, st))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    st = out[1][2]
    assert not out[0][2].inner_log
    for m in (0, 1):
        rows = [r for r in st.inner_log if r["mode"] == m]
        assert len(rows) == 2 * 16 and all(np.isfinite(r["energy"]) for r in rows)
        assert all((r["all"] is None) == (m == 1) for r in rows)
    ec.check_inner_log(st, 1, 1, (0,))


def test_inner_loop_log_refuses_several_ranks(sim_lib):
    from localexpstereo_amd import stereo
    imL, imR, gt = ec.cones_images()
    e = ec.api.HipCostVolumeEnergy.naive(imL, imR, max_disp=63.0, lib=sim_lib)
    try:
        st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=1.0), device="cpu", world=2, inner_loop_log=True)
        st.addLayer(16, [(ec.api.PROPOSE_EXPANSION, 1)])
        with pytest.raises(ValueError, match="single-rank"):
            st.run(0, (0,), 1)
    finally:
        e.close()


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
def test_gpu_terms_sums_rates(host_lib):
    print(ec.case_terms_bit_for_bit(None))
    print("worst relative difference to fsum:", ec.case_sums(None))
    ec.case_nonfinite(None)
    print(ec.case_rates(None))


@pytest.mark.gpu
def test_gpu_determinism_and_stream_order(host_lib):
    ec.case_determinism_and_stream_order(None, "cuda")


@pytest.mark.gpu
def test_gpu_runner_energy(host_lib):
    ec.case_runner_energy(None, "cuda", units=(5, 15, 25))


@pytest.mark.gpu
def test_gpu_region_energy(host_lib):
    print("cells checked, of them at the image border:", ec.case_region_energy(None, "cuda"))


@pytest.mark.gpu
def test_gpu_the_check_can_fail(host_lib):
    print("gap of the cut, cells reported for edited masks:", ec.case_check_can_fail(None, "cuda"))


def _cones():
    pytest.importorskip("PIL")
    from localexpstereo_amd import io as lio
    return lio.load_data(os.path.join(ROOT, "tests", "golden", "cones"), ndisp=64)


@pytest.mark.gpu
def test_gpu_midv2_cones_whole_runs(host_lib):
    """MidV2 on cones, 2 + 2 iterations: device evaluation against the default log, the inner-loop log, and the rise of the energy per set with
    device cuts against host cuts."""
    print(ec.midv_whole_runs("midv2", _cones(), iterations=2, pmIterations=2))


@pytest.mark.gpu
@pytest.mark.parametrize("dual", [False, True])
def test_gpu_objects_whole_runs(host_lib, dual):
    """MidV3 on the synthetic "objects" scene at 1436 x 992 (one PatchMatch and two graph-cut iterations), one view and two views."""
    print(ec.midv_whole_runs("objects", None, iterations=2, pmIterations=1, doDual=dual))


@pytest.mark.gpu
def test_gpu_check_flow_energy_on_the_device_path(host_lib):
    """MidV2's layers on cones with device_cuts="all": the finest two layers by the one-workgroup cell kernel, the coarsest by the tiled solver;
    and once more in a child process with LES_HIP_MAXFLOW_CELL_KERNEL=0 (les_maxflow.h).  Every solver's own worst gap is printed."""
    got = ec.midv_check_device(_cones(), iterations=1, pmIterations=1)
    print("cell kernel + tiled:", got)
    assert got.get("locksteps_checked_cell_kernel", 0) > 0 and got.get("locksteps_checked_tiled", 0) > 0, got
    env = dict(os.environ, LES_HIP_MAXFLOW_CELL_KERNEL="0")
    code = ("import json, os, sys; sys.path.insert(0, %r); from tests import eval_cases as ec; from localexpstereo_amd import io as lio; "
            "d = lio.load_data(os.path.join(%r, 'tests', 'golden', 'cones'), ndisp=64); "
            "print('RESULT ' + json.dumps(ec.midv_check_device(d, iterations=1, pmIterations=1)))") % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got2 = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("les_maxflow.h + tiled:", got2)
    assert got2.get("locksteps_checked_lds_1024", 0) + got2.get("locksteps_checked_lds_512", 0) > 0 and got2.get("locksteps_checked_cell_kernel", 0) == 0, got2
