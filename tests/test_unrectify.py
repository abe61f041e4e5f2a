"""The way back from the rectified pair to the raw camera (csrc/les_unrectify.h): the inverse map and a label map's geometry on the raw grid --
les_hip_unrectify_map, les_hip_unrectify_labels; api.unrectify_map / api.unrectify_labels; stereo.Rectifier.inverse_maps / .unrectify / .to_raw /
.valid_rect / .crop.  CPU simulator build (-m "not gpu") and MI355X (-m gpu).  The definitions, the cases, the references and why the kernels have
no tolerance are in tests/unrectify_cases.py."""
import pytest

from tests import unrectify_cases as uc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


_ids = lambda s: f"{s[0]}x{s[1]}"


# ---------------------------------------------------------------- the definitions and the references themselves (no device)
def test_restatements_match_per_pixel_loops():
    print("calls checked:", uc.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("pixels of each kind:", uc.case_populations())


def test_forward_of_inverse_is_the_raw_pixel():
    uc.case_consistency()


def test_planes_stay_planes():
    uc.case_planes()


def test_valid_rect_against_brute_force():
    print("rectangle:", uc.case_valid_rect())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_sim_map_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", uc.case_map_kernel(sim_lib, shape))


@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_sim_labels_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", uc.case_labels_kernel(sim_lib, shape))


def test_sim_identity_rig_is_reproject(sim_lib):
    print("calls compared:", uc.case_identity(sim_lib))


def test_sim_refusals_launch_nothing(sim_lib):
    print("refused:", uc.case_refusals(sim_lib))


def test_sim_labels_are_independent(sim_lib):
    print("(changed, touched):", uc.case_independence(sim_lib))


def test_sim_crop(sim_lib):
    print("valid rectangle:", uc.case_crop(sim_lib))


def test_sim_driver(sim_lib, host_lib):
    uc.case_driver(sim_lib)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_gpu_map_kernel_bit_for_bit(shape):
    print("calls compared:", uc.case_map_kernel(None, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_gpu_labels_kernel_bit_for_bit(shape):
    print("calls compared:", uc.case_labels_kernel(None, shape))


@pytest.mark.gpu
def test_gpu_identity_rig_is_reproject():
    print("calls compared:", uc.case_identity(None))


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    print("refused:", uc.case_refusals(None))


@pytest.mark.gpu
def test_gpu_labels_are_independent():
    print("(changed, touched):", uc.case_independence(None))


@pytest.mark.gpu
def test_gpu_crop():
    print("valid rectangle:", uc.case_crop(None))


@pytest.mark.gpu
def test_gpu_driver(host_lib):
    uc.case_driver(None)
