"""Slanted planes fitted to a disparity map (csrc/les_planefit.h): the per-pixel edge-aware weighted least-squares plane fit on the device --
les_hip_fit_planes, api.HipCostVolumeEnergy.fit_planes -- and its drivers: stereo.FastGCStereo.fit_planes, run(labeling="wta+planes" / a disparity
map), wta(slanted=True), MidV2 / MidV3(init="wta+planes").  CPU simulator build (-m "not gpu": the cuts run on the host cores) and MI355X (-m gpu).
The definition, the cases, the references and the tolerances are in tests/planefit_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import planefit_cases as pf

KERNEL_CASES = [(s, r) for s in pf.SHAPES for r in pf.RADII]
KERNEL_IDS = [f"{s[0]}x{s[1]}-r{r}" for s, r in KERNEL_CASES]


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- the reference itself
def test_restatement_matches_per_pixel_loop():
    print("maps checked:", pf.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("kind shares [fallback, fronto, slanted] per (shape, radius):", pf.case_populations_do_what_they_say())


@pytest.mark.parametrize("radius", pf.RADII)
def test_restatement_recovers_exact_planes(radius):
    print("pixels away from / next to the edge:", pf.case_exact_recovery(None, radius, cpu_only=True))


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape,radius", KERNEL_CASES, ids=KERNEL_IDS)
def test_sim_kernel_bit_for_bit(sim_lib, shape, radius):
    print("maps compared:", pf.case_kernel_bit_for_bit(sim_lib, shape, radius))


@pytest.mark.parametrize("radius", pf.RADII)
def test_sim_exact_recovery(sim_lib, radius):
    print("pixels away from / next to the edge:", pf.case_exact_recovery(sim_lib, radius))


def test_sim_independence_and_errors(sim_lib):
    pf.case_independence_and_errors(sim_lib, "cpu")


def test_sim_driver_wta_slanted(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(pf.case_driver_wta(sim_lib, "cpu", "none", full=False))


def test_sim_driver_run(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(pf.case_driver_run(sim_lib, "cpu", "none", full=False))


def test_sim_driver_midv(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(pf.case_driver_midv(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape,radius", KERNEL_CASES, ids=KERNEL_IDS)
def test_gpu_kernel_bit_for_bit(shape, radius):
    print("maps compared:", pf.case_kernel_bit_for_bit(None, shape, radius))


@pytest.mark.gpu
@pytest.mark.parametrize("radius", pf.RADII)
def test_gpu_exact_recovery(radius):
    print("pixels away from / next to the edge:", pf.case_exact_recovery(None, radius))


@pytest.mark.gpu
def test_gpu_independence_and_errors():
    pf.case_independence_and_errors(None, "cuda")


@pytest.mark.gpu
def test_gpu_driver_wta_slanted(host_lib):
    print(pf.case_driver_wta(None, "cuda", "all"))


@pytest.mark.gpu
def test_gpu_driver_run(host_lib):
    print(pf.case_driver_run(None, "cuda", "all"))


@pytest.mark.gpu
def test_gpu_driver_midv(host_lib, monkeypatch):
    print(pf.case_driver_midv(None, "cuda", monkeypatch))
