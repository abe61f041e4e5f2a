"""The dense label-map pass (les_hip_unary_labels, csrc/les_dense.h) compiled for the CPU SIMT simulator (tools/hipsim) against the
per-pixel oracle.  Runs without a GPU (-m "not gpu"), small sizes; the same cases run on the gfx950 build in test_dense_gpu.py."""
import numpy as np
import pytest

from tests import dense_cases as dc
from tests import interp_cases as ic
from tests import parity_cases as pc
from tests import vdisp_cases as vc
from tests.util import load_cones_crop


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


@pytest.mark.parametrize("windR,H,W", [(20, 30, 37), (8, 27, 35), (5, 21, 26), (3, 19, 23)])
def test_sim_dense_oracle_parity(sim_lib, oracle_mod, windR, H, W):
    assert dc.case_oracle_parity(sim_lib, windR, H, W, D=8) <= pc.TIGHT


def test_sim_dense_oracle_parity_radius_12(sim_lib, oracle_mod):
    """windR 24 (radius 12): the dense kernel is instantiated for it too; the result is right whatever the kind reports."""
    from localexpstereo_amd import api, synth
    e = api.HipCostVolumeEnergy(synth.make_guide(20, 27, 1), None, synth.make_volume(8, 20, 27, 2), None, windR=24, lib=sim_lib)
    kind = e.unary_labels_kind(0)
    e.close()
    assert kind in (0, 1)
    assert dc.case_oracle_parity(sim_lib, 24, 20, 27, D=8, expect_kind=kind) <= pc.TIGHT


def test_sim_dense_oracle_parity_radius_15_and_odd_windR(sim_lib, oracle_mod):
    assert dc.case_oracle_parity(sim_lib, 31, 20, 23, D=8, modes=(0,), region=False) <= pc.TIGHT
    assert dc.case_oracle_parity(sim_lib, 9, 21, 25, D=8, modes=(1,)) <= pc.TIGHT


def test_sim_dense_min_disparity(sim_lib, oracle_mod):
    assert dc.case_oracle_parity(sim_lib, 8, 22, 29, D=8, min_disp=-3.0) <= pc.TIGHT


def test_sim_dense_image_based_energy(sim_lib, oracle_mod):
    assert dc.case_naive_oracle(sim_lib, 8, crop=(30, 40)) <= pc.NAIVE_TIGHT


def _scene(H=22, W=31, D=8):
    from localexpstereo_amd import synth
    return synth.make_guide(H, W, 1), synth.make_guide(H, W, 2), synth.make_volume(D, H, W, 3), synth.make_volume(D, H, W, 4)


@pytest.mark.parametrize("interp", [0, 2])
@pytest.mark.parametrize("flt", ["GF", "BF", ""])
def test_sim_dense_interpolation_and_filters(sim_lib, oracle_mod, interp, flt):
    """Interpolation 0 / 2 (end-slice NaNs and their spread included) under every filter, against interp_cases' restatement."""
    imL, imR, volL, volR = _scene()
    md = -2.0 if flt == "GF" else 0.0
    pr = ic.InterpPair(sim_lib, imL, imR, volL, volR, interp, windR=6, filter=flt, min_disp=md)
    try:
        dc.case_context_kinds_restated(pr, 6, min_disp=md)
        if interp == 2:
            lab = dc.planted_labels(pr.H, pr.W, pr.D, 5, min_disp=md)
            assert np.isnan(dc.dense(pr.e, lab, 0, None, False)).any(), "no end-slice NaN in the case: it shows nothing about them"
    finally:
        pr.close()


@pytest.mark.parametrize("flt", ["BF", ""])
def test_sim_dense_linear_bilateral_and_unfiltered(sim_lib, oracle_mod, flt):
    pr = dc.context_pair(sim_lib, 1, flt, 22, 31, 8, 6)
    try:
        dc.case_context_kinds_restated(pr, 6)
    finally:
        pr.close()


@pytest.mark.parametrize("flt", ["GF", "BF", ""])
def test_sim_dense_vertical_disparity(sim_lib, oracle_mod, flt):
    a, b = load_cones_crop()
    pr = vc.VPair(sim_lib, filter=flt, windR=6, ims=(np.ascontiguousarray(a[:24, :30]), np.ascontiguousarray(b[:24, :30])))
    try:
        dc.case_context_kinds_restated(pr, 6, v=2.5)
    finally:
        pr.close()


def test_sim_dense_against_job_route(sim_lib, oracle_mod):
    """The per-pixel-job route (les_hip_unary_batch, untouched by this change) on the same label map."""
    pr = pc.synth_pair(sim_lib, 24, 31, 8, windR=8)
    try:
        assert dc.case_against_job_route(pr.e, dc.planted_labels(24, 31, 8, 4), modes=(0, 1)) <= 2 * pc.TIGHT
    finally:
        pr.close()


def test_sim_dense_kind(sim_lib):
    dc.case_kind_everywhere(sim_lib)


def test_dense_kernel_is_in_the_gfx950_code_object():
    from localexpstereo_amd import build
    so = build.build_hip()
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"les_dense_kernel" in blob


def test_sim_dense_piecewise_constant(sim_lib, oracle_mod):
    pr = pc.synth_pair(sim_lib, 40, 52, 12, windR=8)
    try:
        worst, _ = dc.case_piecewise_constant(pr, K=6, modes=(0, 1))
        assert worst <= pc.TIGHT
    finally:
        pr.close()


def test_sim_dense_optimiser_invariant(sim_lib, oracle_mod):
    assert dc.case_optimiser_invariant(sim_lib, "cpu", H=32, W=40, D=8, units=(6, 18), device_cuts="none") <= 2 * pc.TIGHT


def test_sim_dense_resume(sim_lib, oracle_mod):
    dc.case_resume(sim_lib, "cpu", H=28, W=36, D=8, gc_iters=1, device_cuts="none")


def test_sim_dense_errors(sim_lib):
    dc.case_errors(sim_lib)


def test_sim_dense_two_threads(sim_lib):
    dc.case_two_threads(sim_lib, "cpu", H=26, W=33)
