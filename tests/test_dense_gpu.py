"""The dense label-map pass (les_hip_unary_labels, csrc/les_dense.h) on the gfx950 build against the per-pixel oracle (-m gpu, needs an
MI355X).  The cases are tests/dense_cases.py's, shared with the simulator tests."""
import re
import subprocess

import numpy as np
import pytest

from tests import dense_cases as dc
from tests import parity_cases as pc
from tests import vdisp_cases as vc
from tests.util import load_cones_crop

pytestmark = pytest.mark.gpu


# ---- 1. per-pixel oracle parity: sizes that are no multiples of the 8 x 8 tile, both views, check 0 / 1, whole map and inner region
@pytest.mark.parametrize("windR,H,W", [(20, 61, 83), (8, 45, 59), (5, 37, 43), (3, 29, 35)])
def test_gpu_dense_oracle_parity(oracle_mod, windR, H, W):
    assert dc.case_oracle_parity(None, windR, H, W, D=12) <= pc.TIGHT


def test_gpu_dense_oracle_parity_radius_12(oracle_mod):
    from localexpstereo_amd import api, synth
    e = api.HipCostVolumeEnergy(synth.make_guide(20, 27, 1), None, synth.make_volume(8, 20, 27, 2), None, windR=24)
    kind = e.unary_labels_kind(0)
    e.close()
    assert kind in (0, 1)
    assert dc.case_oracle_parity(None, 24, 53, 67, D=12, expect_kind=kind) <= pc.TIGHT


def test_gpu_dense_oracle_parity_radius_15_and_odd_windR(oracle_mod):
    assert dc.case_oracle_parity(None, 31, 40, 47, D=12, checks=(True,)) <= pc.TIGHT
    assert dc.case_oracle_parity(None, 21, 45, 51, D=12, checks=(True,)) <= pc.TIGHT
    assert dc.case_oracle_parity(None, 9, 31, 35, D=8) <= pc.TIGHT


def test_gpu_dense_min_disparity(oracle_mod):
    assert dc.case_oracle_parity(None, 8, 41, 53, D=10, min_disp=-3.0) <= pc.TIGHT


# ---- 2. every kind of context
def test_gpu_dense_image_based_energy(oracle_mod):
    assert dc.case_naive_oracle(None, 20, stride=3) <= pc.NAIVE_TIGHT
    assert dc.case_naive_oracle(None, 8, crop=(50, 70)) <= pc.NAIVE_TIGHT


# (the linear guided filter is the oracle-parity case above)
@pytest.mark.parametrize("interp,flt", [(i, f) for i in (0, 1, 2) for f in ("GF", "BF", "") if (i, f) != (1, "GF")])
def test_gpu_dense_interpolation_and_filters(oracle_mod, interp, flt):
    md = -2.0 if flt == "GF" else 0.0
    pr = dc.context_pair(None, interp, flt, 22, 31, 8, 6, min_disp=md)
    try:
        dc.case_context_kinds_restated(pr, 6, min_disp=md)
        if interp == 2:
            lab = dc.planted_labels(pr.H, pr.W, pr.D, 5, min_disp=md)
            assert np.isnan(dc.dense(pr.e, lab, 0, None, False)).any(), "no end-slice NaN in the case: it shows nothing about them"
    finally:
        pr.close()
    # a larger scene at the shipped windR, a sample of its pixels
    pr = dc.context_pair(None, interp, flt, 70, 90, 16, 20)
    try:
        dc.case_context_kinds_restated(pr, 20, stride=23, modes=(1,), checks=(True,))
    finally:
        pr.close()


@pytest.mark.parametrize("flt", ["GF", "BF", ""])
def test_gpu_dense_vertical_disparity(oracle_mod, flt):
    a, b = load_cones_crop()
    pr = vc.VPair(None, filter=flt, windR=6, ims=(np.ascontiguousarray(a[:24, :30]), np.ascontiguousarray(b[:24, :30])))
    try:
        dc.case_context_kinds_restated(pr, 6, v=2.5)
    finally:
        pr.close()
    pr = vc.VPair(None, filter=flt, windR=20)
    try:
        dc.case_context_kinds_restated(pr, 20, v=2.5, stride=41, modes=(0,), checks=(True,))
    finally:
        pr.close()


def test_gpu_dense_against_job_route(oracle_mod):
    """The per-pixel-job route (les_hip_unary_batch with 1 x 1 targets, untouched by this change): cost volume at the three interpolations and
    the image-based energy with v != 0, at the shipped windR."""
    from localexpstereo_amd import api
    pr = pc.synth_pair(None, 57, 75, 12)
    try:
        lab = dc.planted_labels(57, 75, 12, 4)
        for interp in (1, 0, 2):
            pr.e.setInterpolationMethod(interp)
            assert dc.case_against_job_route(pr.e, lab, modes=(0, 1), checks=(True,)) <= 2 * pc.TIGHT
    finally:
        pr.close()
    imL, imR = load_cones_crop()
    imL, imR = np.ascontiguousarray(imL[:60, :80]), np.ascontiguousarray(imR[:60, :80])
    e = api.HipCostVolumeEnergy.naive(imL, imR, max_disp=31.0)
    try:
        lab = dc.planted_labels(60, 80, 32, 6, v=2.0)
        assert dc.case_against_job_route(e, lab, modes=(0, 1), checks=(True,), tight=pc.NAIVE_TIGHT) <= 2 * pc.NAIVE_TIGHT
    finally:
        e.close()


# ---- 3. the dense kernel is the one that ran
def test_gpu_dense_kind():
    dc.case_kind_everywhere(None)


# ---- 4. piecewise-constant property
def test_gpu_dense_piecewise_constant_mid(oracle_mod):
    pr = pc.synth_pair(None, 375, 450, 64)
    try:
        worst, _ = dc.case_piecewise_constant(pr, K=6, modes=(0, 1))
        assert worst <= pc.TIGHT
    finally:
        pr.close()


def test_gpu_dense_piecewise_constant_adirondack_shape(oracle_mod):
    """1436 x 992 with a 24-slice volume: against the whole-image aggregation of the K planes, and against the per-pixel oracle on every pixel
    within windR of the image border and a seeded sample of 4 000 interior pixels."""
    H, W, D = 992, 1436, 24
    pr = pc.synth_pair(None, H, W, D)
    try:
        worst, lab = dc.case_piecewise_constant(pr, K=6, modes=(0,), block=16)
        assert worst <= pc.TIGHT
        px = dc.border_and_sample(H, W, 20, 4000, 7)
        ref = dc.oracle_pixels(pr.o, lab, 20, 0, True, pixels=px)
        got = dc.dense(pr.e, lab, 0, None, True)
        assert pc.compare_maps(np.where(np.isnan(ref), np.nan, got), ref) <= pc.TIGHT
    finally:
        pr.close()


# ---- 5. the optimiser's invariant
def test_gpu_dense_optimiser_invariant(oracle_mod):
    assert dc.case_optimiser_invariant(None, "cuda", H=96, W=128, D=16, units=(6, 18)) <= 2 * pc.TIGHT


# ---- 6. resume
def test_gpu_dense_resume(oracle_mod):
    dc.case_resume(None, "cuda", H=80, W=104, D=16, gc_iters=2)


def test_gpu_warm_start_is_one_dense_pass(oracle_mod, monkeypatch):
    """PMRunner.init_from_labels and recost build no per-pixel jobs (no batch is created), and recost restores a spoiled cost map."""
    from localexpstereo_amd import api, pm, synth
    H, W, D = 40, 52, 12
    imL, vol = synth.make_guide(H, W, 5), synth.make_volume(D, H, W, 6)
    e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=8, max_disp=D - 1.0)
    r = pm.PMRunner(e, (8,), [[(api.PROPOSE_EXPANSION, 1)]], seed=1, device="cuda")
    made = []
    orig = api.Batch.__init__

    def counting(self, *a, **k):
        made.append(1)
        orig(self, *a, **k)
    monkeypatch.setattr(api.Batch, "__init__", counting)
    try:
        lab = dc.planted_labels(H, W, D, 3)
        r.init_from_labels(lab, rows_per_launch=7)
        first = r.cur.cpu().numpy().copy()
        r.cur.fill_(-1.0)
        r.recost()
        assert not made, "the warm start created batches"
        assert np.array_equal(r.cur.cpu().numpy().view(np.uint32), first.view(np.uint32))
        assert pc.compare_maps(first, dc.oracle_pixels(pc.om.Oracle(imL, None, vol, None, windR=8, max_disp=D - 1.0), lab, 8)) <= pc.TIGHT
    finally:
        r.close()
        e.close()


# ---- 7. errors, threads
def test_gpu_dense_errors():
    dc.case_errors(None)


def test_gpu_dense_two_threads():
    dc.case_two_threads(None, "cuda", H=120, W=150, D=12, windR=20)


# ---- 8. the C++ mirror
def test_gpu_host_demo_warm_start_leg():
    from localexpstereo_amd import build
    build.build_hip()
    demo = build.build_host()
    r = subprocess.run([demo, "run", "200", "140", "24", "1"], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2500:], r.stderr[-1500:])
    assert r.returncode == 0 and "les_host_demo: OK" in r.stdout
    m = re.search(r"warm start: data term of the first run ([0-9.]+), of the run resumed from its labelling ([0-9.]+), (\d+) label differences", r.stdout)
    assert m, "the warm-start leg did not run"
    assert int(m.group(3)) == 0 and abs(float(m.group(1)) - float(m.group(2))) <= 2 * 2 * pc.TIGHT * 200 * 140
