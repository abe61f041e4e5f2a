"""Rectification of a calibrated raw stereo pair (csrc/les_rectify.h): the rectifying transform, the map of raw positions and the sampler --
io.stereo_rectify; les_hip_rectify_map, les_hip_remap; api.rectify_map / api.remap; stereo.Rectifier.  CPU simulator build (-m "not gpu") and
MI355X (-m gpu).  The definitions, the cases, the references and why the kernels have no tolerance are in tests/rectify_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import rectify_cases as rc


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


# ---------------------------------------------------------------- the transform and the references themselves (no device)
def test_identity_rig():
    rc.case_identity_rig()


def test_transform_is_geometrically_consistent():
    print("largest row and disparity error, px:", rc.case_geometry())


def test_transform_refusals():
    print("refused:", rc.case_transform_refusals())


def test_restatements_match_per_pixel_loops():
    print("calls checked:", rc.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("pixels of each kind:", rc.case_populations_do_what_they_say())


def test_round_trip_cap_holds_for_the_restatement():
    rc.case_round_trip_restated()


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_sim_map_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", rc.case_map_kernel(sim_lib, shape))


@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_sim_remap_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", rc.case_remap_kernel(sim_lib, shape))


@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_sim_identity_map_returns_the_source(sim_lib, shape):
    rc.case_identity_map(sim_lib, shape)


def test_sim_refusals_launch_nothing(sim_lib):
    print("refused:", rc.case_refusals(sim_lib))


def test_sim_source_pixels_are_independent(sim_lib):
    print("(changed, touched) per interp:", rc.case_independence(sim_lib))


def test_sim_cones_round_trip(sim_lib):
    rc.case_round_trip(sim_lib)


def test_sim_matcher_needs_it(sim_lib, host_lib):
    rc.case_matcher(sim_lib)


def test_sim_driver(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(rc.case_driver(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6, device_cuts="none"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_gpu_map_kernel_bit_for_bit(shape):
    print("calls compared:", rc.case_map_kernel(None, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_gpu_remap_kernel_bit_for_bit(shape):
    print("calls compared:", rc.case_remap_kernel(None, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", rc.SHAPES, ids=_ids)
def test_gpu_identity_map_returns_the_source(shape):
    rc.case_identity_map(None, shape)


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    print("refused:", rc.case_refusals(None))


@pytest.mark.gpu
def test_gpu_source_pixels_are_independent():
    print("(changed, touched) per interp:", rc.case_independence(None))


@pytest.mark.gpu
def test_gpu_cones_round_trip():
    rc.case_round_trip(None)


@pytest.mark.gpu
def test_gpu_matcher_needs_it(host_lib):
    rc.case_matcher(None)


@pytest.mark.gpu
def test_gpu_driver(host_lib, monkeypatch):
    print(rc.case_driver(None, "cuda", monkeypatch))
