"""Vertical disparity (Plane::v) in the image-based energy (NaiveStereoEnergy, LES/StereoEnergy.h:704-729) on every device path,
against the numpy restatement of tests/vdisp_cases.py fed through the oracle's guided filter or the bilateral restatement; the vertical
draws of the device proposers; MidV2 with a vertical range on a cones pair shifted by one row.  CPU simulator build (-m "not gpu")
and MI355X (-m gpu)."""
import os

import numpy as np
import pytest

from tests import vdisp_cases as vc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


def test_restatement_matches_reference_loop():
    vc.case_restatement_matches_loop()


def test_restatement_at_v0_is_the_oracle(oracle_mod):
    vc.case_v0_is_the_oracle()


# ---------------------------------------------------------------- CPU simulator build
def test_sim_gf_march(sim_lib, oracle_mod):
    pr = vc.VPair(sim_lib)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(9,), mode=1, kind=1)
        vc.case_slot_and_slab_batches(pr, mode=0, kind=1)
        vc.case_negative_zero(pr)
    finally:
        pr.close()


def test_sim_gf_strip(sim_lib, oracle_mod):
    pr = vc.VPair(sim_lib, windR=30)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(14,), mode=0, windR=30, kind=0)
        vc.case_negative_zero(pr, mode=1)
    finally:
        pr.close()


@pytest.mark.parametrize("filt", ["BF", ""])
def test_sim_bf_and_unfiltered(sim_lib, oracle_mod, filt):
    pr = vc.VPair(sim_lib, filter=filt, windR=20 if filt == "BF" else 0)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(9,), mode=0, kind=2, windR=20)
    finally:
        pr.close()


def test_sim_proposers(sim_lib, oracle_mod):
    vc.case_proposers(sim_lib)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
def test_gpu_gf(oracle_mod):
    pr = vc.VPair(None)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(9, 25), mode=0, kind=1)
        vc.case_cell_batches(pr, units=(14,), mode=1, kind=1)
        vc.case_slot_and_slab_batches(pr, mode=1, kind=1)
        vc.case_negative_zero(pr)
    finally:
        pr.close()
    pr = vc.VPair(None, windR=30)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(14,), mode=1, windR=30, kind=0)
        vc.case_slot_and_slab_batches(pr, mode=0, kind=0)
        vc.case_negative_zero(pr, mode=1)
    finally:
        pr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", ["BF", ""])
def test_gpu_bf_and_unfiltered(oracle_mod, filt):
    pr = vc.VPair(None, filter=filt, windR=20 if filt == "BF" else 0)
    try:
        vc.case_single_calls(pr)
        vc.case_cell_batches(pr, units=(9, 25), mode=1, kind=2, windR=20)
        vc.case_slot_and_slab_batches(pr, mode=0, kind=2)
        vc.case_negative_zero(pr)
    finally:
        pr.close()


@pytest.mark.gpu
def test_gpu_proposers(oracle_mod):
    vc.case_proposers(None)


def _shifted_cones(shift):
    from localexpstereo_amd import io as lio
    data = lio.load_data(os.path.join(os.path.dirname(__file__), "golden", "cones"), ndisp=64)
    if shift:
        imR = data["imR"]
        data["imR"] = np.ascontiguousarray(np.concatenate([imR[:1]] * shift + [imR[:-shift]], 0))     # content moves down: true v = +shift
    return data


def _midv2(data, **kw):
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    st, lab, raw = stereo.MidV2(data, iterations=5, pmIterations=2, doDual=False, **kw)
    _, bad2 = lio.Evaluator(data["dispGT"], data["nonocc"], 2.0).evaluate(stereo.disparities(lab))
    v = stereo.vertical_disparities(lab)[data["nonocc"]]
    return bad2, float(np.median(v)), lab


@pytest.mark.gpu
def test_gpu_midv2_cones_shifted_one_row():
    """cones with imR moved down one row (true v = +1): MidV2 with vdisp 2 on energy and random proposer beats vdisp 0 in bad-2.0
    non-occluded and finds v near 1; on the unshifted pair vdisp 2 costs little.  main.cpp's setting (energy only) is reported and held to
    the same margin.  Measured on MI355X: shifted 11.25 % (vdisp 0) -> 2.52 % (median v 0.967), energy only 2.51 % (median v 0.945);
    unshifted 2.25 % -> 2.36 %.  Bounds: the gain at least 5 points (measured 8.7), the median within 0.1 of 1 (measured 0.033), the
    unshifted loss at most 1 point (measured 0.11)."""
    pytest.importorskip("PIL")
    sh = _shifted_cones(1)
    b0, m0, _ = _midv2(sh)
    b2, m2, lab = _midv2(sh, vdisp=2.0, random_vdisp=2.0)
    be, me, _ = _midv2(sh, vdisp=2.0)
    un = _shifted_cones(0)
    u0, _, _ = _midv2(un)
    u2, um2, _ = _midv2(un, vdisp=2.0, random_vdisp=2.0)
    print(f"shifted: vdisp 0 {b0:.2f} %, vdisp 2 (energy + proposer) {b2:.2f} % median v {m2:.3f}, energy only {be:.2f} % median v {me:.3f}; "
          f"unshifted: vdisp 0 {u0:.2f} %, vdisp 2 {u2:.2f} % median v {um2:.3f}")
    assert b2 < b0 - 5.0
    assert be < b0 - 5.0
    assert abs(m2 - 1.0) <= 0.1
    assert u2 <= u0 + 1.0
