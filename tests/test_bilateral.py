"""The bilateral ("BF" / "BL") and unfiltered ("") cost aggregation (csrc/les_bilateral.h) against an fp64 restatement of
BilateralFilter::filter (LES/GuidedFilter.h:329-374) on the oracle's raw cost: on the CPU simulator build (-m "not gpu") and on the
MI355X (-m gpu).  Cases: tests/bilateral_cases.py."""
import os

import numpy as np
import pytest

from tests import bilateral_cases as bc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


def test_restatement_matches_reference_loop():
    bc.case_restatement_tiny()


def test_radius0_guided_filter_is_identity(oracle_mod):
    bc.case_radius0_identity(None)


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_sim_bf_single_calls(sim_lib, oracle_mod, naive):
    pr = bc.cones_bf(sim_lib, naive=naive)
    try:
        bc.case_single_calls(pr)
    finally:
        pr.close()


@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_sim_none_single_calls_and_batches_exact(sim_lib, oracle_mod, naive):
    pr = bc.cones_bf(sim_lib, naive=naive, filter="")
    try:
        bc.case_single_calls(pr)
        bc.case_cell_batches(pr, mode=1)
        bc.case_slot_batches(pr, mode=0)
    finally:
        pr.close()


@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_sim_bf_cell_batches_two_layers(sim_lib, oracle_mod, naive):
    pr = bc.cones_bf(sim_lib, naive=naive)
    try:
        bc.case_cell_batches(pr, units=(8, 25), mode=0)
        bc.case_cell_batches(pr, units=(14,), mode=1)
    finally:
        pr.close()


@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_sim_bf_slot_and_slab_batches(sim_lib, oracle_mod, naive):
    pr = bc.cones_bf(sim_lib, naive=naive, filter="BL")
    try:
        bc.case_slot_batches(pr, mode=1)
        bc.case_whole_image_slabs(pr, nplanes=5, mode=0)
    finally:
        pr.close()


@pytest.mark.parametrize("windR,sig2", [(0, 10.0), (1, 1.0), (5, 100.0), (20, 1.0), (20, 100.0), (5, 10.0)])
def test_sim_bf_radius_and_sigma(sim_lib, oracle_mod, windR, sig2):
    pr = bc.synth_bf(sim_lib, 70, 90, 8, windR=windR, sig2=sig2)
    try:
        calls = [c for c in bc.single_calls(pr.H, pr.W, pr.D) if c[1][0] + c[1][2] <= pr.W and c[1][1] + c[1][3] <= pr.H]
        bc.case_single_calls(pr, calls=calls, scratch=False)
        bc.case_slot_batches(pr, unit=12, slots=2, mode=0, windR=max(windR, 1))
    finally:
        pr.close()


def test_sim_errors_and_gf_constructor(sim_lib, oracle_mod):
    bc.case_errors(sim_lib)
    bc.case_gf_through_new_constructor(sim_lib)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
@pytest.mark.parametrize("filt", ["BF", ""], ids=["bf", "none"])
def test_gpu_bf_cases(oracle_mod, naive, filt):
    pr = bc.cones_bf(None, naive=naive, filter=filt)
    try:
        bc.case_single_calls(pr)
        bc.case_cell_batches(pr, units=(8, 25), mode=0)
        bc.case_cell_batches(pr, units=(14,), mode=1)
        bc.case_slot_batches(pr, mode=1)
        bc.case_whole_image_slabs(pr, nplanes=5, mode=0)
    finally:
        pr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("windR,sig2", [(0, 10.0), (1, 1.0), (5, 100.0), (20, 1.0), (20, 100.0), (31, 10.0)])
def test_gpu_bf_radius_and_sigma(oracle_mod, windR, sig2):
    pr = bc.synth_bf(None, 70, 90, 8, windR=windR, sig2=sig2)
    try:
        calls = [c for c in bc.single_calls(pr.H, pr.W, pr.D) if c[1][0] + c[1][2] <= pr.W and c[1][1] + c[1][3] <= pr.H]
        bc.case_single_calls(pr, calls=calls)
        bc.case_slot_batches(pr, unit=12, slots=2, mode=0, windR=max(windR, 1))
    finally:
        pr.close()


@pytest.mark.gpu
def test_gpu_errors_and_gf_constructor(oracle_mod):
    bc.case_errors(None)
    bc.case_gf_through_new_constructor(None)


@pytest.mark.gpu
def test_gpu_bf_whole_image_1436x992(oracle_mod):
    """One whole-image slab batch at the Adirondack-H shape, windR 20, a few planes, against the restatement on sampled rows (image
    borders and interior); the same batch twice is bit-equal."""
    pr = bc.synth_bf(None, 992, 1436, 24, windR=20, sig2=10.0)
    try:
        rows = np.array([0, 7, 19, 20, 21, 400, 977, 991])
        a, worst = bc.case_whole_image_slabs(pr, nplanes=5, mode=0, rows=rows)
        b, _ = bc.case_whole_image_slabs(pr, nplanes=5, mode=0, rows=rows[:1])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        print(f"1436 x 992 whole-image slabs: worst err / bound {worst:.3f}")
    finally:
        pr.close()


@pytest.mark.gpu
def test_gpu_midv2_cones_params_bf():
    """MidV2 on the bundled cones pair with PARAMS_BF (LES/main.cpp:72: lambda 20, windR 20, sig2 10), one view, 2 PatchMatch + 5
    graph-cut iterations: finishes, repeats bit for bit, and its bad-2.0 non-occluded error stays below the 25 % sanity bound."""
    pytest.importorskip("PIL")
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    data = lio.load_data(os.path.join(os.path.dirname(__file__), "golden", "cones"), ndisp=64)
    runs = []
    for _ in range(2):
        st, lab, raw = stereo.MidV2(data, iterations=5, pmIterations=2, doDual=False, params=stereo.PARAMS_BF)
        runs.append(lab)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    disp = stereo.disparities(runs[0])
    _, bad2 = lio.Evaluator(data["dispGT"], data["nonocc"], 2.0).evaluate(disp)
    print("MidV2 cones PARAMS_BF log:", [(r["index"], round(r["energy"]), round(r["all"], 2), round(r["nonocc"], 2)) for r in st.log],
          f"bad-2.0 nonocc {bad2:.2f} %")
    assert bad2 < 25.0
