"""Winner-take-all labels of the aggregated cost volume (csrc/les_wtavol.h): the streaming arg-min over the slabs of the fronto-parallel planes --
les_hip_slab_argmin, les_hip_slab_argmin_finish -- the whole operation for one view -- les_hip_wta_labels, api.HipCostVolumeEnergy.wta_labels --
and its users: stereo.FastGCStereo.wta, run(labeling="wta"), MidV2 / MidV3(init="wta"), fuse with a WTA map.  CPU simulator build (-m "not gpu":
the cuts run on the host cores) and MI355X (-m gpu).  The definition, the cases, the references and the tolerances are in tests/wtavol_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import wtavol_cases as wv


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
    print("volumes checked:", wv.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("specials placed:", wv.case_populations_hold_what_the_cases_need())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", wv.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sim_kernel_bit_for_bit_and_chunk_independence(sim_lib, shape):
    print("outputs compared:", wv.case_kernel_bit_for_bit(sim_lib, shape))


def test_sim_whole_call(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(wv.case_whole_call(sim_lib, "cpu"))


def test_sim_independence_and_argument_errors(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    wv.case_independence_and_errors(sim_lib, "cpu")


def test_sim_driver_wta(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(wv.case_driver_wta(sim_lib, "cpu", "none"))


def test_sim_driver_midv(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(wv.case_driver_midv(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", wv.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_kernel_bit_for_bit_and_chunk_independence(shape):
    print("outputs compared:", wv.case_kernel_bit_for_bit(None, shape))


@pytest.mark.gpu
def test_gpu_whole_call():
    print(wv.case_whole_call(None, "cuda"))


@pytest.mark.gpu
def test_gpu_independence_and_argument_errors():
    wv.case_independence_and_errors(None, "cuda")


@pytest.mark.gpu
def test_gpu_driver_wta(host_lib):
    print(wv.case_driver_wta(None, "cuda", "all"))


@pytest.mark.gpu
def test_gpu_driver_midv(host_lib, monkeypatch):
    print(wv.case_driver_midv(None, "cuda", monkeypatch))
