"""Fusion moves on the device (csrc/les_pairwise.h): two label maps fused by graph cuts -- les_hip_batch_fusion_graph, les_hip_batch_apply_masks_labels,
api.Batch.fusion_graph / apply_masks_labels, pm.PMRunner.fuse, stereo.FastGCStereo.fuse.  CPU simulator build (-m "not gpu": the cuts run on the
host cores) and MI355X (-m gpu: the device solvers).  The definition, the cases, the references and the tolerances are in tests/fusion_cases.py."""
import pytest

from tests import fusion_cases as fc


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
def test_restatement_matches_per_pair_loop():
    print("cells checked:", fc.case_restatement_matches_loop())


def test_cut_cost_is_the_truncated_energy():
    """Measured here: worst |cut - E'| 1.8e-14 over 40 instances x 4096 labellings; about 5 % of the pairs are non-submodular."""
    print("worst |cut - E'|, share of non-submodular pairs:", fc.case_enumeration())


# ---------------------------------------------------------------- CPU simulator build
def test_sim_payload_flow0_counts(sim_lib):
    print("non-submodular pairs counted:", fc.case_payload(sim_lib))


def test_sim_pin_to_the_expansion_chain(sim_lib):
    print("pairs one rounding below zero:", fc.case_pin_to_expansion(sim_lib))


def test_sim_one_plane_nonfinite(sim_lib):
    print("words compared, NaN words:", fc.case_one_plane_nonfinite(sim_lib))


def test_sim_apply_and_flow_against_energy(sim_lib, host_lib):
    print("cells equal / bounded, pixels moved:", fc.case_apply_and_energy(sim_lib))


def test_sim_runner_and_driver_fuse(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(fc.case_runner_fuse(sim_lib, "cpu", "none"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
def test_gpu_payload_flow0_counts(host_lib):
    print("non-submodular pairs counted:", fc.case_payload(None))


@pytest.mark.gpu
def test_gpu_pin_to_the_expansion_chain(host_lib):
    print("pairs one rounding below zero:", fc.case_pin_to_expansion(None))


@pytest.mark.gpu
def test_gpu_one_plane_nonfinite(host_lib):
    print("words compared, NaN words:", fc.case_one_plane_nonfinite(None))


@pytest.mark.gpu
def test_gpu_device_cuts_on_fusion_payloads(host_lib):
    print("cells enumerated:", fc.case_device_cuts(None))


@pytest.mark.gpu
def test_gpu_apply_and_flow_against_energy(host_lib):
    print("cells equal / bounded, pixels moved:", fc.case_apply_and_energy(None))


@pytest.mark.gpu
def test_gpu_runner_and_driver_fuse(host_lib):
    print(fc.case_runner_fuse(None, "cuda", "all"))
