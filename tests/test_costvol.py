"""AD-Census matching-cost volumes built on the device from the stereo pair (csrc/les_costvol.h): les_hip_costvol_tables, les_hip_census,
les_hip_build_cost_volume, api.costvol_tables / census / build_cost_volume, io.build_volumes and stereo.MidV3(volL=None).  CPU simulator build
(-m "not gpu") and MI355X (-m gpu).  The definition restated in numpy, the cases and their shapes are in tests/costvol_cases.py."""
import pytest

from tests import costvol_cases as cc

MODES = (0, 1)


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- 1. the restatement itself
def test_restatement_matches_per_pixel_loop_and_popcount():
    print("popcounts checked:", cc.case_restatement())


# ---------------------------------------------------------------- CPU simulator build
def test_sim_tables(sim_lib):
    print("worst table difference in ulps:", cc.case_tables(sim_lib))


@pytest.mark.parametrize("H,W", cc.CENSUS_SHAPES)
def test_sim_census(sim_lib, H, W):
    print("bits set:", cc.case_census(sim_lib, H, W))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D,H,W,d0", cc.VOLUME_SHAPES)
def test_sim_volume(sim_lib, D, H, W, d0, mode):
    print("mean cost:", cc.case_volume(sim_lib, D, H, W, d0, mode))


def test_sim_volume_unaligned_base(sim_lib):
    """W % 4 == 0 behind a base that is not 16-byte aligned: the dword store path."""
    print("mean cost:", cc.case_volume(sim_lib, 9, 7, 40, 0, 0, lead=cc.GUARD + 1))


def test_sim_symmetry_with_convert_and_fill(sim_lib):
    print("entries the fill replaced:", cc.case_symmetry(sim_lib))


def test_sim_known_answers(sim_lib):
    print("zeros in slice k (left, right):", cc.case_known_answers(sim_lib))


def test_sim_errors(sim_lib):
    print("refused calls of the last group:", cc.case_errors(sim_lib))


def test_sim_quality_cones(sim_lib):
    """Measured (numpy restatement; the device volume is byte-equal to it): winner-take-all bad-1.0 29.0 % against 72.6 % for the plain AD volume
    on the 8 646 counted pixels, bad-2.0 24.2 % against 63.4 %."""
    cc.case_quality(sim_lib)


def test_sim_driver_midv3_from_the_pair(sim_lib, host_lib, monkeypatch):
    """On the simulator the layers are coarsened to cells of 24 / 60 / 120 pixels (cc.case_driver says why); the GPU test runs MidV3's own."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    cc.case_driver(sim_lib, "cpu", monkeypatch, layer_units=(24, 60, 120), device_cuts="none")


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
def test_gpu_tables():
    print("worst table difference in ulps:", cc.case_tables(None))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", cc.CENSUS_SHAPES)
def test_gpu_census(H, W):
    print("bits set:", cc.case_census(None, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D,H,W,d0", cc.VOLUME_SHAPES)
def test_gpu_volume(D, H, W, d0, mode):
    print("mean cost:", cc.case_volume(None, D, H, W, d0, mode))


@pytest.mark.gpu
def test_gpu_volume_unaligned_base():
    print("mean cost:", cc.case_volume(None, 9, 7, 40, 0, 0, lead=cc.GUARD + 1))


@pytest.mark.gpu
def test_gpu_volume_nontemporal_stores(monkeypatch):
    """The other store flavour of the volume kernel (LES_HIP_COSTVOL_NT) writes the same bytes."""
    for nt in ("1", "0"):
        monkeypatch.setenv("LES_HIP_COSTVOL_NT", nt)
        print("mean cost:", cc.case_volume(None, cc.CHUNK + 1, 2, cc.SEGMENT + 8, -2, 0))


@pytest.mark.gpu
def test_gpu_symmetry_with_convert_and_fill():
    print("entries the fill replaced:", cc.case_symmetry(None))


@pytest.mark.gpu
def test_gpu_known_answers():
    print("zeros in slice k (left, right):", cc.case_known_answers(None))


@pytest.mark.gpu
def test_gpu_errors():
    print("refused calls of the last group:", cc.case_errors(None))


@pytest.mark.gpu
def test_gpu_quality_cones():
    cc.case_quality(None)


@pytest.mark.gpu
def test_gpu_driver_midv3_from_the_pair(host_lib, monkeypatch):
    cc.case_driver(None, "cuda", monkeypatch)
