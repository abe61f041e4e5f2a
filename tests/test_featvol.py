"""Correlation cost volumes from feature maps on the matrix cores, and the ZNCC patch descriptor (csrc/les_featvol.h): les_hip_patch_features,
les_hip_build_feature_volume, api.patch_features / build_feature_volume, io.build_volumes(cost="zncc" / features=) and stereo.MidV3's cost / patch /
features.  CPU simulator build (-m "not gpu") and MI355X (-m gpu).  The definitions restated in numpy, the cases and their shapes are in
tests/featvol_cases.py."""
import pytest

from tests import featvol_cases as fc

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
def test_restatement_descriptor_loop_and_exact_fmaf():
    print("fma triples checked against exact rationals, of them wrong when rounded through float64:", fc.case_restatement())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("H,W", fc.DESC_SHAPES)
def test_sim_descriptor(sim_lib, H, W):
    print("flat patches:", fc.case_descriptor(sim_lib, H, W))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,H,W,d0", fc.VOLUME_CASES)
def test_sim_volume_exact(sim_lib, C, D, H, W, d0, mode):
    print("mean cost:", fc.case_volume(sim_lib, C, D, H, W, d0, mode))


@pytest.mark.parametrize("mode", MODES)
def test_sim_volume_one_hot(sim_lib, mode):
    print("ones:", fc.case_one_hot(sim_lib, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.25, 0.75)])
def test_sim_volume_alpha_beta(sim_lib, alpha, beta, mode):
    print("mean cost:", fc.case_volume(sim_lib, 25, fc.CHUNK + 1, 1, 33, -3, mode, alpha=alpha, beta=beta))


@pytest.mark.parametrize("mode", MODES)
def test_sim_volume_unaligned_bases(sim_lib, mode):
    """W % 4 == 0 behind a volume base that is not 16-byte aligned (the dword store path), and feature maps that are not either."""
    print("mean cost:", fc.case_volume(sim_lib, 3, 9, 2, 40, 0, mode, lead=fc.GUARD + 1, feat_lead=1))
    print("mean cost:", fc.case_volume(sim_lib, 3, 9, 2, 40, 0, mode, feat_lead=3))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,H,W,d0", fc.REAL_CASES)
def test_sim_volume_real(sim_lib, C, D, H, W, d0, mode):
    fc.case_real(sim_lib, C, D, H, W, d0, mode)


def test_sim_symmetry(sim_lib):
    print("entries compared:", fc.case_symmetry(sim_lib))


def test_sim_errors(sim_lib):
    print("refused calls of the last group:", fc.case_errors(sim_lib))
    print("refused keyword sets:", fc.case_python_errors(sim_lib))


def test_sim_quality_cones(sim_lib):
    """Measured on the simulator build (its volume is byte-equal to the numpy chain): winner-take-all bad-1.0 8.3 % for ZNCC 5 x 5 against 29.0 %
    for AD-Census on the 8 646 counted pixels."""
    fc.case_quality(sim_lib)


def test_sim_driver_midv3_zncc_and_features(sim_lib, host_lib, monkeypatch):
    """On the simulator the layers are coarsened as in test_costvol.test_sim_driver_midv3_from_the_pair; the GPU test runs MidV3's own."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    fc.case_driver(sim_lib, "cpu", monkeypatch, layer_units=(24, 60, 120), device_cuts="none")


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", fc.DESC_SHAPES)
def test_gpu_descriptor(H, W):
    print("flat patches:", fc.case_descriptor(None, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,H,W,d0", fc.VOLUME_CASES)
def test_gpu_volume_exact(C, D, H, W, d0, mode):
    print("mean cost:", fc.case_volume(None, C, D, H, W, d0, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_volume_one_hot(mode):
    print("ones:", fc.case_one_hot(None, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.25, 0.75)])
def test_gpu_volume_alpha_beta(alpha, beta, mode):
    print("mean cost:", fc.case_volume(None, 25, fc.CHUNK + 1, 1, 33, -3, mode, alpha=alpha, beta=beta))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_volume_unaligned_bases(mode):
    print("mean cost:", fc.case_volume(None, 3, 9, 2, 40, 0, mode, lead=fc.GUARD + 1, feat_lead=1))
    print("mean cost:", fc.case_volume(None, 3, 9, 2, 40, 0, mode, feat_lead=3))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,H,W,d0", fc.REAL_CASES)
def test_gpu_volume_real(C, D, H, W, d0, mode):
    """Asserts the derived bound; prints how many entries differ from the numpy fmaf chain (DESIGN 3.2k records the count)."""
    fc.case_real(None, C, D, H, W, d0, mode)


@pytest.mark.gpu
def test_gpu_symmetry():
    print("entries compared:", fc.case_symmetry(None))


@pytest.mark.gpu
def test_gpu_errors():
    print("refused calls of the last group:", fc.case_errors(None))
    print("refused keyword sets:", fc.case_python_errors(None))


@pytest.mark.gpu
def test_gpu_quality_cones():
    fc.case_quality(None)


@pytest.mark.gpu
def test_gpu_driver_midv3_zncc_and_features(host_lib, monkeypatch):
    fc.case_driver(None, "cuda", monkeypatch)
