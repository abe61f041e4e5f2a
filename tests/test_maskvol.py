"""Valid masks in the cost volumes, the nearest-valid row fill (csrc/les_maskvol.h): les_hip_fill_invalid; api.fill_invalid; io.build_volumes /
io.ingest_volumes(valid=); stereo.MidV3(valid=), stereo.Rectifier.data(valid=True), stereo.FastGCStereo(valid=).  CPU simulator build
(-m "not gpu") and MI355X (-m gpu).  The rule, the cases, the references and why nothing has a tolerance are in tests/maskvol_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import maskvol_cases as mc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


_ids = lambda s: "x".join(str(n) for n in s[:3]) + f"@{s[3]}"


# ---------------------------------------------------------------- the definitions and the references themselves (no device)
def test_restatement_matches_per_entry_loop():
    print("calls checked:", mc.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("rows of each kind:", mc.case_populations())


def test_cut_frames_leave_invalid_borders():
    print("share valid in both views:", mc.case_input_condition())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_ids)
def test_sim_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", mc.case_kernel(sim_lib, shape))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=_ids)
def test_sim_null_masks_are_fill_out_of_view(sim_lib, shape):
    print("calls compared:", mc.case_equals_fill_out_of_view(sim_lib, shape))


def test_sim_properties(sim_lib):
    print("flips:", mc.case_properties(sim_lib))


def test_sim_refusals_launch_nothing(sim_lib):
    print("refused:", mc.case_refusals(sim_lib))


def test_sim_build_volumes(sim_lib):
    print("volumes compared:", mc.case_build_volumes(sim_lib))


def test_sim_ingest_volumes(sim_lib):
    print("calls compared:", mc.case_ingest_volumes(sim_lib))


def test_sim_what_it_buys(sim_lib, host_lib):
    mc.case_what_it_buys(sim_lib)


def test_sim_driver(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(mc.case_driver(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6, device_cuts="none"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_ids)
def test_gpu_kernel_bit_for_bit(shape):
    print("calls compared:", mc.case_kernel(None, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_ids)
def test_gpu_null_masks_are_fill_out_of_view(shape):
    print("calls compared:", mc.case_equals_fill_out_of_view(None, shape))


@pytest.mark.gpu
def test_gpu_properties():
    print("flips:", mc.case_properties(None))


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    print("refused:", mc.case_refusals(None))


@pytest.mark.gpu
def test_gpu_build_volumes():
    print("volumes compared:", mc.case_build_volumes(None))


@pytest.mark.gpu
def test_gpu_ingest_volumes():
    print("calls compared:", mc.case_ingest_volumes(None))


@pytest.mark.gpu
def test_gpu_what_it_buys(host_lib):
    mc.case_what_it_buys(None)


@pytest.mark.gpu
def test_gpu_driver(host_lib, monkeypatch):
    print(mc.case_driver(None, "cuda", monkeypatch))
