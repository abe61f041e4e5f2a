"""The 3D reconstruction (csrc/les_reproject.h): les_hip_reproject, les_hip_mesh, les_hip_mesh_tile, api.HipCostVolumeEnergy.reproject / .mesh,
io.calib3d / write_ply / read_ply, stereo.FastGCStereo.reconstruct.  CPU simulator build (-m "not gpu") and MI355X (-m gpu).  The definition
restated in numpy, the inputs and their shapes are in tests/reproject_cases.py."""
import pytest

from tests import reproject_cases as rc

SHAPES = range(len(rc.SHAPE_IDS))


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- the restatement itself
def test_restatement_matches_pixel_loop():
    print("maps compared:", rc.case_restatement())


def test_plane_identity():
    print("largest error / allowed error:", rc.case_plane_identity())


def test_normal_is_cross_product_direction():
    print("largest 1 - cos:", rc.case_normal_direction())


def test_ply_round_trip():
    print("files compared:", rc.case_ply_round_trip())


def test_mesh_counts_closed_form():
    print("maps counted:", rc.case_mesh_counts())


def test_calib3d():
    import numpy as np
    from localexpstereo_amd import api, io as lio
    cam0 = np.array([[3997.684, 0, 1176.728], [0, 3997.684, 1011.728], [0, 0, 1]], np.float32)
    c = lio.calib3d(dict(cam0=cam0, cam1=cam0, doffs=131.111, baseline=193.001, width=2964))
    want = api.Calib(3997.684, 1176.728, 1011.728, 131.111, 193.001)
    assert bytes(c) == bytes(want) and lio.calib3d(c) is c
    assert bytes(lio.calib3d(dict(f=3997.684, cx=1176.728, cy=1011.728, doffs=131.111, baseline=193.001))) == bytes(want)


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("name", sorted(rc.INPUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=rc.SHAPE_IDS)
def test_sim_device(sim_lib, shape, name):
    print(rc.case_device(sim_lib, name, *rc.shapes(sim_lib)[shape]))


@pytest.mark.parametrize("name", rc.BIG_INPUTS)
def test_sim_device_scan_loops(sim_lib, name):
    print(rc.case_device(sim_lib, name, *rc.big_shape(sim_lib), ptr_forms=False))


def test_sim_refusals(sim_lib):
    print("refusals checked:", rc.case_refusals(sim_lib))


def test_sim_driver(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(rc.case_driver(sim_lib, "cpu"))


def test_sim_midv2_ply(sim_lib, host_lib, monkeypatch):
    from tests import crossview_cases as cv
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(rc.case_midv2_ply(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6, device_cuts="none"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rc.INPUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=rc.SHAPE_IDS)
def test_gpu_device(shape, name):
    print(rc.case_device(None, name, *rc.shapes(None)[shape]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.BIG_INPUTS)
def test_gpu_device_scan_loops(name):
    print(rc.case_device(None, name, *rc.big_shape(None), ptr_forms=False))


@pytest.mark.gpu
def test_gpu_refusals():
    print("refusals checked:", rc.case_refusals(None))


@pytest.mark.gpu
def test_gpu_driver(host_lib):
    print(rc.case_driver(None, "cuda"))


@pytest.mark.gpu
def test_gpu_midv2_ply(host_lib, monkeypatch):
    print(rc.case_midv2_ply(None, "cuda", monkeypatch))
