"""View synthesis and the photometric check (csrc/les_view.h): a label map rendered as the image of a camera anywhere on the baseline, two renders
blended with their holes filled, and the colour difference between every pixel and the point of the other image its label names --
les_hip_render_view, les_hip_blend_views, les_hip_photo_error; api.HipCostVolumeEnergy.render_view / .blend_views / .photo_error;
stereo.FastGCStereo.synthesize / .photo_error / max_photo_error=; io.photometric.  CPU simulator build (-m "not gpu") and MI355X (-m gpu).  The
definitions, the cases, the references and why there is no tolerance are in tests/view_cases.py."""
import pytest

from tests import view_cases as vc


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    build.build_host_lib()
    return build.build_sim()


_ids = lambda s: f"{s[0]}x{s[1]}"


# ---------------------------------------------------------------- the references themselves
def test_restatements_match_per_pixel_loops():
    print("calls checked:", vc.case_restatement_matches_loop())


def test_populations_hold_what_the_cases_need():
    print("(src, fill) seen:", vc.case_populations_do_what_they_say())


def test_photometric_summary():
    print(vc.case_photometric_summary())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("shape", vc.SHAPES, ids=_ids)
def test_sim_kernels_bit_for_bit(sim_lib, shape):
    print("calls compared:", vc.case_kernels_bit_for_bit(sim_lib, shape))


def test_sim_kernels_widest_row(sim_lib):
    print("calls compared:", vc.case_widest_row(sim_lib))


def test_sim_hits_are_the_label_warps(sim_lib):
    print("hit pixels:", vc.case_warp_hits(sim_lib))


def test_sim_rows_are_independent(sim_lib):
    vc.case_independence(sim_lib)


def test_sim_refusals_launch_nothing(sim_lib):
    vc.case_refusals(sim_lib)


def test_sim_cones_render_and_photometric_error(sim_lib):
    vc.case_cones(sim_lib)


def test_sim_driver(sim_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    vc.case_driver(sim_lib, "cpu")


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("shape", vc.SHAPES, ids=_ids)
def test_gpu_kernels_bit_for_bit(shape):
    print("calls compared:", vc.case_kernels_bit_for_bit(None, shape))


@pytest.mark.gpu
def test_gpu_kernels_widest_row():
    """The stated limit is served, not only enforced: 65536 bytes of dynamic LDS launch."""
    print("calls compared:", vc.case_widest_row(None))


@pytest.mark.gpu
def test_gpu_hits_are_the_label_warps():
    print("hit pixels:", vc.case_warp_hits(None))


@pytest.mark.gpu
def test_gpu_rows_are_independent():
    vc.case_independence(None)


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    vc.case_refusals(None)


@pytest.mark.gpu
def test_gpu_cones_render_and_photometric_error():
    vc.case_cones(None)


@pytest.mark.gpu
def test_gpu_driver():
    vc.case_driver(None, "cuda")
