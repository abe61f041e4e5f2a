"""The speckle filter (csrc/les_speckle.h): les_hip_speckle_mask, les_hip_speckle_tile, les_hip_post_process_speckle,
api.HipCostVolumeEnergy.speckle_mask / post_process(speckle=), stereo.FastGCStereo(speckle=).  CPU simulator build (-m "not gpu", whose workgroups
run on OS threads: the merges race for real) and MI355X (-m gpu).  The definition restated in numpy, the inputs and their shapes are in
tests/speckle_cases.py."""
import pytest

from tests import speckle_cases as sk

# the shapes are functions of the compiled-in tile (les_hip_speckle_tile); the ids name them by what they cover
SHAPE_IDS = ("pixel", "row", "column", "tile", "tile_plus_1", "tiles")
POST = [(guide, views) for guide in ("const", "random") for views in ((0, 1), (0,), (1,))]


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
def test_restatement_matches_flood_fill():
    print("maps compared:", sk.case_restatement(False))


def test_restatement_matches_scipy():
    pytest.importorskip("scipy.sparse.csgraph")
    print("maps compared:", sk.case_restatement(True))


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("name", sorted(sk.INPUTS))
@pytest.mark.parametrize("shape", range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_sim_components(sim_lib, shape, name):
    print(sk.case_components(sim_lib, name, *sk.shapes(sim_lib)[shape]))


@pytest.mark.parametrize("name", sk.BIG_INPUTS)
def test_sim_components_many_workgroups(sim_lib, name):
    print(sk.case_components(sim_lib, name, *sk.big_shape(sim_lib)))


def test_sim_refusals(sim_lib):
    print("refusals checked:", sk.case_refusals(sim_lib))


def test_sim_post_zero(sim_lib):
    print("pixels the post-processing changed:", sk.case_post_zero(sim_lib))


@pytest.mark.parametrize("guide,views", POST)
def test_sim_post_islands(sim_lib, guide, views):
    print(sk.case_post_islands(sim_lib, guide, views))


def test_sim_driver_off(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    sk.case_driver_off(sim_lib, "cpu")


def test_sim_driver_on(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(sk.case_driver_on(sim_lib, "cpu"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sk.INPUTS))
@pytest.mark.parametrize("shape", range(len(SHAPE_IDS)), ids=SHAPE_IDS)
def test_gpu_components(shape, name):
    print(sk.case_components(None, name, *sk.shapes(None)[shape]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sk.BIG_INPUTS)
def test_gpu_components_many_workgroups(name):
    print(sk.case_components(None, name, *sk.big_shape(None)))


@pytest.mark.gpu
def test_gpu_refusals():
    print("refusals checked:", sk.case_refusals(None))


@pytest.mark.gpu
def test_gpu_post_zero():
    print("pixels the post-processing changed:", sk.case_post_zero(None))


@pytest.mark.gpu
@pytest.mark.parametrize("guide,views", POST)
def test_gpu_post_islands(guide, views):
    print(sk.case_post_islands(None, guide, views))


@pytest.mark.gpu
def test_gpu_driver_off(host_lib):
    sk.case_driver_off(None, "cuda")


@pytest.mark.gpu
def test_gpu_driver_on(host_lib):
    print(sk.case_driver_on(None, "cuda"))
