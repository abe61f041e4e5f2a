"""setInterpolationMethod (les_hip_set_interpolation): nearest-slice (0) and quadratic (2) raw costs on every device path, against the
numpy restatement of LES/CostVolumeEnergy.h:99-167 fed through the oracle's guided filter or the bilateral restatement; the per-call
operator against a one-call batch, bit for bit, for every filter, energy and interpolation.  CPU simulator build (-m "not gpu") and
MI355X (-m gpu).  Cases: tests/interp_cases.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import interp_cases as ic
from tests import parity_cases as pc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


def test_restatement_matches_reference_loop():
    ic.case_restatement_matches_loop()


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("interp", [0, 2])
@pytest.mark.parametrize("D,min_disp", [(1, 0.0), (2, -3.0), (64, 0.0), (64, -3.0)])
def test_sim_unfiltered_exact(sim_lib, oracle_mod, interp, D, min_disp):
    ic.case_unfiltered_exact(sim_lib, interp, D, min_disp)


@pytest.mark.parametrize("interp", [0, 2])
def test_sim_gf_single_calls_and_batches(sim_lib, oracle_mod, interp):
    pr = ic.cones_interp(sim_lib, interp)
    try:
        ic.case_gf_single_calls(pr)
        ic.case_cell_batches(pr, units=(8, 25), mode=0, kind=1)
        ic.case_slabs(pr, nplanes=3, mode=1)
    finally:
        pr.close()


@pytest.mark.parametrize("interp", [0, 2])
def test_sim_gf_radius15_strip(sim_lib, oracle_mod, interp):
    pr = ic.cones_interp(sim_lib, interp, windR=30)
    try:
        ic.case_gf_single_calls(pr, scratch=False)
        ic.case_cell_batches(pr, units=(14,), mode=1, windR=30, kind=0)
    finally:
        pr.close()


@pytest.mark.parametrize("interp", [0, 2])
@pytest.mark.parametrize("filt", ["GF", "BF"])
def test_sim_interior_nan(sim_lib, oracle_mod, interp, filt):
    ic.case_interior_nan(sim_lib, interp, filter=filt)


@pytest.mark.parametrize("interp", [0, 2])
def test_sim_bf(sim_lib, oracle_mod, interp):
    pr = ic.cones_interp(sim_lib, interp, filter="BF", sig2=10.0)
    try:
        ic.case_gf_single_calls(pr)
        ic.case_cell_batches(pr, units=(14,), mode=1, kind=2)
    finally:
        pr.close()


def test_sim_routing_flagged_calls(sim_lib, oracle_mod):
    for interp in (0, 2):
        pr = ic.cones_interp(sim_lib, interp)
        try:
            ic.case_routing(pr, mode=0)
        finally:
            pr.close()


def test_sim_mode_switching(sim_lib, oracle_mod):
    pr = ic.cones_interp(sim_lib, 1)
    try:
        ic.case_mode_switching(pr)
    finally:
        pr.close()
    ic.case_naive_refuses(sim_lib)


@pytest.mark.parametrize("name", ic.PATH_CONTEXTS)
def test_sim_one_call_paths_agree(sim_lib, name):
    ic.case_one_call_paths_agree(sim_lib, name)


def test_sim_scratch_cache(sim_lib):
    ic.case_scratch_cache(sim_lib)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 2])
def test_gpu_unfiltered_exact(oracle_mod, interp):
    for D, min_disp in ((1, 0.0), (2, -3.0), (64, 0.0), (64, -3.0)):
        ic.case_unfiltered_exact(None, interp, D, min_disp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 2])
def test_gpu_gf(oracle_mod, interp):
    pr = ic.cones_interp(None, interp)
    try:
        ic.case_gf_single_calls(pr)
        ic.case_cell_batches(pr, units=(8, 25), mode=0, kind=1)
        ic.case_cell_batches(pr, units=(14,), mode=1, kind=1)
        ic.case_slabs(pr, nplanes=5, mode=0)
        ic.case_routing(pr, mode=1)
    finally:
        pr.close()
    pr = ic.cones_interp(None, interp, windR=30)
    try:
        ic.case_gf_single_calls(pr)
        ic.case_cell_batches(pr, units=(14,), mode=0, windR=30, kind=0)
    finally:
        pr.close()
    for filt in ("GF", "BF"):
        ic.case_interior_nan(None, interp, filter=filt)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 2])
def test_gpu_cones_ad_volume(oracle_mod, interp):
    from tests.util import load_cones_crop
    imL, vol, _ = pc.cones_ad_volume(D=64)
    _, imR = load_cones_crop()
    pr = ic.InterpPair(None, imL, imR, vol, vol.copy(), interp, th_col=0.05)
    try:
        ic.case_cell_batches(pr, units=(14,), mode=0, kind=1)
        ic.case_slabs(pr, nplanes=4, mode=0)
    finally:
        pr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 2])
def test_gpu_bf(oracle_mod, interp):
    for filt in ("BF", "BL"):
        pr = ic.cones_interp(None, interp, filter=filt, sig2=10.0)
        try:
            ic.case_gf_single_calls(pr)
            ic.case_cell_batches(pr, units=(8, 25), mode=0, kind=2)
            ic.case_slabs(pr, nplanes=5, mode=1, kind=2)
        finally:
            pr.close()


@pytest.mark.gpu
def test_gpu_mode_switching_and_refresh(oracle_mod):
    pr = ic.cones_interp(None, 1)
    try:
        ic.case_mode_switching(pr)
    finally:
        pr.close()
    ic.case_naive_refuses(None)
    ic.case_refresh_keeps_setting(None, "cuda")


@pytest.mark.gpu
def test_gpu_one_call_paths_agree():
    for name in ic.PATH_CONTEXTS:
        ic.case_one_call_paths_agree(None, name)
    ic.case_scratch_cache(None)


@pytest.mark.gpu
def test_gpu_midv3_interpolation_reaches_the_optimiser():
    """A short MidV3 run at each interpolation repeats bit for bit; 0 and 2 give labelings different from 1."""
    from localexpstereo_amd import stereo, synth
    H, W, D = 96, 160, 24
    imL, imR, gt = synth.make_scene(H, W, D, seed=5)
    volL = synth.ad_volume(imL, imR, D, "cuda").cpu().numpy()
    data = dict(imL=imL, imR=imR, dispGT=gt, nonocc=np.ones((H, W), bool), ndisp=D, gt_prec=-1.0)
    labs = {}
    for interp in (0, 1, 2):
        runs = []
        for _ in range(2):
            st, lab, raw = stereo.MidV3(data, volL, None, iterations=1, pmIterations=1, doDual=False, smooth_weight=0.5, mc_threshold=0.5,
                                        interpolate=interp)
            runs.append(np.ascontiguousarray(lab))
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), f"interpolation {interp} is not repeatable"
        labs[interp] = runs[0]
        print(f"interpolation {interp}:", [(r["index"], float(r["energy"]), float(r["all"])) for r in st.log])
    assert not np.array_equal(labs[0].view(np.uint32), labs[1].view(np.uint32))
    assert not np.array_equal(labs[2].view(np.uint32), labs[1].view(np.uint32))


_CPP = r"""
#include "HipCostVolumeEnergy.h"
#include <cstdio>
#include <vector>
using namespace les_host;
int main()
{
    const int H = 48, W = 64, D = 8;
    std::vector<uint8_t> im((size_t)H * W * 3);
    for (size_t i = 0; i < im.size(); i++) im[i] = (uint8_t)((i * 2654435761u) >> 24);
    std::vector<float> vol((size_t)D * H * W);
    for (size_t i = 0; i < vol.size(); i++) vol[i] = (float)((i * 40503u) % 1000u) / 1000.0f;
    Parameters p;
    p.windR = 10; p.filter_param1 = 1e-4f; p.th_col = 0.5f; p.filterName = "GF";
    HipCostVolumeEnergy e(im.data(), im.data(), W, H, vol.data(), vol.data(), D, p, (float)(D - 1), 0.0f, 0);
    const Rect fr(0, 0, W, H);
    const Plane pl(0.0f, 0.0f, 0.49f, 0.0f);          // fronto-parallel at d = 0.49: nearest reads slice 0, linear mixes slices 0 and 1
    std::vector<float> c1((size_t)H * W), c0((size_t)H * W), c2((size_t)H * W);
    StereoEnergy::Reusable r;
    e.ComputeUnaryPotential(fr, fr, c1.data(), W, pl, r, 0);
    e.setInterpolationMethod(0);
    e.ComputeUnaryPotential(fr, fr, c0.data(), W, pl, r, 0);
    e.setInterpolationMethod(1);
    e.ComputeUnaryPotential(fr, fr, c2.data(), W, pl, r, 0);
    bool thrown = false;
    try { e.setInterpolationMethod(3); } catch (const std::invalid_argument&) { thrown = true; }
    HipNaiveStereoEnergy n(im.data(), im.data(), W, H, p, 7.0f);
    bool nthrown = false;
    try { n.setInterpolationMethod(0); } catch (const std::invalid_argument&) { nthrown = true; }
    int diff01 = 0, diff12 = 0;
    for (size_t i = 0; i < c1.size(); i++) { diff01 += c0[i] != c1[i]; diff12 += c1[i] != c2[i]; }
    printf("diff01 %d diff12 %d thrown %d nthrown %d\n", diff01, diff12, (int)thrown, (int)nthrown);
    return (diff01 > 0 && diff12 == 0 && thrown && nthrown) ? 0 : 1;
}
"""


@pytest.mark.gpu
def test_gpu_host_class_forwards_the_setting(tmp_path):
    """host/HipCostVolumeEnergy.h: setInterpolationMethod reaches the context; the naive subclass and bad values throw."""
    from localexpstereo_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "interp_host.cpp"
    src.write_text(_CPP)
    exe = tmp_path / "interp_host"
    libdir = os.path.dirname(build.HIP_SO)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "localexpstereo_amd", "host"),
                    str(src), "-o", str(exe), "-L", libdir, "-llocalexp_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
