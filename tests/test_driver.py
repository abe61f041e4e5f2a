"""The driver above the kernels (localexpstereo_amd/stereo.py): its entry points agree where they make the same calls, and each closes every
runner, graph-cut context and device evaluator it made, also when it raises.  CPU simulator build (-m "not gpu": the cuts run on the host cores)
and MI355X (-m gpu).  The cases are in tests/driver_cases.py."""
import pytest

from tests import driver_cases as dc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- CPU simulator build
def test_sim_entry_points_agree(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    dc.case_entry_points_agree(sim_lib, "cpu", "none")


def test_sim_everything_made_is_closed(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print("made and closed:", dc.case_everything_closed(sim_lib, "cpu", "none", monkeypatch))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
def test_gpu_entry_points_agree(host_lib):
    dc.case_entry_points_agree(None, "cuda", "all")


@pytest.mark.gpu
def test_gpu_everything_made_is_closed(host_lib, monkeypatch):
    print("made and closed:", dc.case_everything_closed(None, "cuda", "all", monkeypatch))
