"""The confidence of a label map under the aggregated cost volume (csrc/les_confidence.h): the streaming own / rival reduction over the slabs of
the fronto-parallel planes -- les_hip_slab_confidence, les_hip_slab_confidence_finish -- the whole operation for one view -- les_hip_confidence,
api.HipCostVolumeEnergy.confidence -- the post-processing with the caller's masks -- les_hip_post_process_masked -- and their users:
stereo.FastGCStereo(confidence=, min_confidence=), FastGCStereo.confidence, io.sparsification.  CPU simulator build (-m "not gpu") and MI355X
(-m gpu).  The definition, the cases, the references and the tolerances are in tests/confidence_cases.py."""
import pytest

from tests import confidence_cases as cf

POST_VIEWS = ((0, 1), (0,), (1,))


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- the references themselves
def test_restatement_matches_per_pixel_loop():
    print("volumes checked:", cf.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("specials checked:", cf.case_populations_hold_what_the_cases_need())


def test_sparsification_by_hand():
    print(cf.case_sparsification())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", cf.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sim_kernel_bit_for_bit_and_chunk_independence(sim_lib, shape):
    print("outputs compared:", cf.case_kernel_bit_for_bit(sim_lib, shape))


def test_sim_whole_call(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(cf.case_whole_call(sim_lib, "cpu"))


def test_sim_argument_errors(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print("refusals checked:", cf.case_argument_errors(sim_lib, "cpu"))


@pytest.mark.parametrize("views", POST_VIEWS, ids=lambda v: "views_" + "".join(map(str, v)))
def test_sim_post_process_masked(sim_lib, views):
    print(cf.case_post_masked(sim_lib, views))


def test_sim_drivers(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(cf.case_drivers(sim_lib, "cpu"))


def test_sim_ranks_errors(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(cf.case_ranks_errors(sim_lib, "cpu"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", cf.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_kernel_bit_for_bit_and_chunk_independence(shape):
    print("outputs compared:", cf.case_kernel_bit_for_bit(None, shape))


@pytest.mark.gpu
def test_gpu_whole_call():
    print(cf.case_whole_call(None, "cuda"))


@pytest.mark.gpu
def test_gpu_argument_errors():
    print("refusals checked:", cf.case_argument_errors(None, "cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("views", POST_VIEWS, ids=lambda v: "views_" + "".join(map(str, v)))
def test_gpu_post_process_masked(views):
    print(cf.case_post_masked(None, views))


@pytest.mark.gpu
def test_gpu_drivers(host_lib):
    print(cf.case_drivers(None, "cuda"))


@pytest.mark.gpu
def test_gpu_ranks_errors(host_lib):
    print(cf.case_ranks_errors(None, "cuda"))
