"""The equidistant fisheye camera in the rectification front end and on the way back (csrc/les_fisheye.h): its own atan, sin and cos, the two map
kernels, the model switch -- io.fisheye_theta_max, io.stereo_rectify(model=); les_hip_rectify_map_fisheye, les_hip_unrectify_map_fisheye;
api.fisheye / api.rectify_map_fisheye / api.unrectify_map_fisheye; stereo.Rectifier(model="fisheye").  CPU simulator build (-m "not gpu") and
MI355X (-m gpu).  The definitions, the cases, the references and why the kernels have no tolerance are in tests/fisheye_cases.py."""
import pytest

from tests import fisheye_cases as fc


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


# ---------------------------------------------------------------- the functions, the transform and the references themselves (no device)
def test_restated_functions_are_within_1e15_of_libm():
    fc.case_functions()


def test_theta_max():
    print("the folding lens folds at, rad:", fc.case_theta_max())


def test_transform_model_switch():
    print("refused:", fc.case_transform())


def test_restatements_match_per_pixel_loops():
    print("calls checked:", fc.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("pixels of each kind:", fc.case_populations())


def test_round_trip_holds_for_the_restatement():
    fc.case_round_trip(restated=True)


def test_cones_caps_hold_for_the_restatement():
    fc.case_cones_restated()


def test_timing_tool_states_no_protocol_of_its_own(monkeypatch):
    """tools/timing_fisheye.py under the rules tests/test_timing_harness.py holds every tools/*_timing.py to: the clock, the spread and the
    events are those of tools/timing.py."""
    import os
    from tests import test_timing_harness as th
    th.test_tool_states_no_protocol_of_its_own(os.path.join(th.TOOLS, "timing_fisheye.py"), monkeypatch)


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_ids)
def test_sim_map_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", fc.case_map_kernel(sim_lib, shape))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=_ids)
def test_sim_unmap_kernel_bit_for_bit(sim_lib, shape):
    print("calls compared:", fc.case_unmap_kernel(sim_lib, shape))


def test_sim_round_trip(sim_lib):
    fc.case_round_trip(sim_lib)


def test_sim_refusals_launch_nothing(sim_lib):
    print("refused:", fc.case_refusals(sim_lib))


def test_sim_cones_through_a_fisheye_rig(sim_lib):
    print(fc.case_cones(sim_lib))


def test_sim_matcher_needs_it(sim_lib, host_lib):
    fc.case_matcher(sim_lib)


def test_sim_pinhole_untouched(sim_lib):
    fc.case_pinhole_untouched(sim_lib)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_ids)
def test_gpu_map_kernel_bit_for_bit(shape):
    print("calls compared:", fc.case_map_kernel(None, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.SHAPES, ids=_ids)
def test_gpu_unmap_kernel_bit_for_bit(shape):
    print("calls compared:", fc.case_unmap_kernel(None, shape))


@pytest.mark.gpu
def test_gpu_round_trip():
    fc.case_round_trip(None)


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    print("refused:", fc.case_refusals(None))


@pytest.mark.gpu
def test_gpu_cones_through_a_fisheye_rig():
    print(fc.case_cones(None))


@pytest.mark.gpu
def test_gpu_matcher_needs_it(host_lib):
    fc.case_matcher(None)


@pytest.mark.gpu
def test_gpu_pinhole_untouched():
    fc.case_pinhole_untouched(None)
