"""Cross-view fusion (csrc/les_crossview.h): a view's label map warped into the other view on the device -- les_hip_warp_labels,
api.HipCostVolumeEnergy.warp_labels -- and fused there: pm.PMRunner.fuse with a device map, stereo.FastGCStereo.cross_fuse and cross_view=.  CPU
simulator build (-m "not gpu": the cuts run on the host cores) and MI355X (-m gpu).  The definition, the cases, the references and the tolerances
are in tests/crossview_cases.py."""
import pytest

from tests import crossview_cases as cv

@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


@pytest.fixture(scope="module")
def host_lib():
    from localexpstereo_amd import build
    return build.build_host_lib()


# ---------------------------------------------------------------- the reference itself
def test_restatement_matches_per_pixel_loop():
    print("maps checked, hit pixels:", cv.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("specials placed:", cv.case_populations_do_what_they_say())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", cv.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sim_kernel_bit_for_bit(sim_lib, shape):
    print("maps compared:", cv.case_kernel_bit_for_bit(sim_lib, shape))


def test_sim_kernel_widest_row(sim_lib):
    print("maps compared:", cv.case_kernel_bit_for_bit(sim_lib, cv.WIDEST))


@pytest.mark.parametrize("shape", cv.SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sim_landing_bound(sim_lib, shape):
    print("hit pixels, worst ratio to the bound:", cv.case_landing_bound(sim_lib, shape))


def test_sim_independence_and_width_limit(sim_lib):
    cv.case_independence(sim_lib, "cpu")
    cv.case_width_limit(sim_lib)


def test_sim_cross_fuse(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    cv.case_cross_fuse(sim_lib, "cpu", "none")


def test_sim_driver_midv2(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    cv.case_driver_midv2(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6)


def test_sim_driver_midv3_from_the_pair(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    cv.case_driver_midv3(sim_lib, "cpu", monkeypatch, layers=cv.sim_layers, filterRadious=6)


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", cv.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_kernel_bit_for_bit(shape):
    print("maps compared:", cv.case_kernel_bit_for_bit(None, shape))


@pytest.mark.gpu
def test_gpu_kernel_widest_row():
    """The stated limit is served, not only enforced: 65536 bytes of dynamic LDS launch."""
    print("maps compared:", cv.case_kernel_bit_for_bit(None, cv.WIDEST))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", cv.SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_landing_bound(shape):
    print("hit pixels, worst ratio to the bound:", cv.case_landing_bound(None, shape))


@pytest.mark.gpu
def test_gpu_independence_and_width_limit():
    cv.case_independence(None, "cuda")
    cv.case_width_limit(None)


@pytest.mark.gpu
def test_gpu_cross_fuse(host_lib):
    cv.case_cross_fuse(None, "cuda", "all")


@pytest.mark.gpu
def test_gpu_driver_midv2(host_lib, monkeypatch):
    cv.case_driver_midv2(None, "cuda", monkeypatch)


@pytest.mark.gpu
def test_gpu_driver_midv3_from_the_pair(host_lib, monkeypatch):
    cv.case_driver_midv3(None, "cuda", monkeypatch)
