"""Semi-global matching over a view's cost volume (csrc/les_sgm.h): the transpose, path and read-out kernels behind les_hip_sgm_labels,
api.HipCostVolumeEnergy.sgm_labels, and its users: stereo.FastGCStereo.sgm, run(labeling="sgm" / "sgm+planes"), MidV3(init="sgm").  CPU simulator
build (-m "not gpu": the cuts run on the host cores) and MI355X (-m gpu).  The definition, the cases, the references and the tolerances are in
tests/sgm_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import sgm_cases as sg


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
    print("directions checked:", sg.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("specials placed:", sg.case_populations_hold_what_the_cases_need())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape,K", sg.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sim_kernel_bit_for_bit(sim_lib, shape, K):
    print("outputs compared:", sg.case_kernel_bit_for_bit(sim_lib, shape, K))


def test_sim_order_and_repeat(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    sg.case_order_and_repeat(sim_lib, "cpu")


def test_sim_argument_errors(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print("refusals checked:", sg.case_argument_errors(sim_lib))


def test_sim_quality(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    sg.case_quality(sim_lib, "cpu")


def test_sim_driver_sgm(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(sg.case_driver_sgm(sim_lib, "cpu", "none"))


def test_sim_driver_midv(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(sg.case_driver_midv(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape,K", sg.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gpu_kernel_bit_for_bit(shape, K):
    print("outputs compared:", sg.case_kernel_bit_for_bit(None, shape, K))


@pytest.mark.gpu
def test_gpu_order_and_repeat():
    sg.case_order_and_repeat(None, "cuda")


@pytest.mark.gpu
def test_gpu_argument_errors():
    print("refusals checked:", sg.case_argument_errors(None))


@pytest.mark.gpu
def test_gpu_quality():
    sg.case_quality(None, "cuda")


@pytest.mark.gpu
def test_gpu_driver_sgm(host_lib):
    print(sg.case_driver_sgm(None, "cuda", "all"))


@pytest.mark.gpu
def test_gpu_driver_midv(host_lib, monkeypatch):
    print(sg.case_driver_midv(None, "cuda", monkeypatch))
