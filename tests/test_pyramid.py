"""A half-resolution solve as a start (csrc/les_pyramid.h): les_hip_pool_image, les_hip_pool_volume, les_hip_upsample_labels, les_hip_create_half,
les_hip_get_image, api.pool_image / pool_volume / HipCostVolumeEnergy.half / upsample_labels, stereo.FastGCStereo.run(labeling="half") and
MidV2 / MidV3(init="half").  CPU simulator build (-m "not gpu") and MI355X (-m gpu).  The definitions restated in numpy, the cases and their shapes
are in tests/pyramid_cases.py."""
import pytest

from tests import crossview_cases as cv
from tests import pyramid_cases as pc

GUIDES = ("random", "const", "edge")
# (naive, filter, interpolation): the cost-volume energy at every filter and interpolation, the image-based one (it has no interpolation) at every filter
HALF_KINDS = [(False, f, i) for f in pc.FILTERS for i in (0, 1, 2)] + [(True, f, 1) for f in pc.FILTERS]


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
def test_restatement_matches_per_pixel_loops():
    print("comparisons:", pc.case_restatement())


# ---------------------------------------------------------------- CPU simulator build
@pytest.mark.parametrize("H,W", pc.IMAGE_SHAPES)
def test_sim_pool_image(sim_lib, H, W):
    print("sum:", pc.case_pool_image(sim_lib, H, W))


@pytest.mark.parametrize("D,H,W", pc.VOLUME_SHAPES)
def test_sim_pool_volume(sim_lib, D, H, W):
    print("mean:", pc.case_pool_volume(sim_lib, D, H, W))


def test_sim_pool_volume_unaligned_base(sim_lib):
    """W % 4 == 0 behind an input base that is not 16-byte aligned, then behind an output base that is not 8-byte aligned: the dword path."""
    print("mean:", pc.case_pool_volume(sim_lib, *pc.UNALIGNED, lead=pc.GUARD + 1))
    print("mean:", pc.case_pool_volume(sim_lib, *pc.UNALIGNED, out_lead=pc.GUARD + 1))


def test_sim_pool_volume_nonfinite(sim_lib):
    print("NaN, inf outputs:", pc.case_pool_volume_nonfinite(sim_lib))


def test_sim_pool_errors(sim_lib):
    print("refused:", pc.case_pool_errors(sim_lib))


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("mind", pc.MIN_DISPS)
@pytest.mark.parametrize("half_shape,full_shape", pc.UPSAMPLE_SHAPES)
def test_sim_upsample(sim_lib, half_shape, full_shape, mind, guide):
    counts = pc.case_upsample(sim_lib, half_shape, full_shape, mind, guide)
    print("kinds [kept, clamped, non-finite]:", counts)
    if full_shape == (33, 66):
        assert all(c > 0 for c in counts), counts


def test_sim_upsample_errors(sim_lib):
    print("refused:", pc.case_upsample_errors(sim_lib))


@pytest.mark.parametrize("mind", pc.MIN_DISPS)
@pytest.mark.parametrize("naive,filt,interp", HALF_KINDS)
def test_sim_create_half(sim_lib, naive, filt, interp, mind):
    print("finite values compared:", pc.case_create_half(sim_lib, naive, filt, interp, mind))


def test_sim_create_half_errors(sim_lib):
    pc.case_create_half_errors(sim_lib)


@pytest.mark.parametrize("which", ("MidV3", "MidV2"))
def test_sim_driver(sim_lib, host_lib, monkeypatch, which):
    """On the simulator the layers are coarsened (crossview_cases.sim_layers) and every cut runs on the host, as costvol_cases.case_driver does and
    for its reason.  Measured there with seed 3 (the seed was chosen here; any seed leaves this room, since a random start's energy is dominated
    by the 1e6 of its invalid labels): start row energy 5 621.9 ("half") against 1.298e9 (random) for MidV3, 44 562.8 against 2.419e9 for MidV2."""
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(pc.case_driver(sim_lib, "cpu", monkeypatch, which, layers=cv.sim_layers, filterRadious=6, device_cuts="none"))


def test_sim_driver_two_levels(sim_lib, host_lib, monkeypatch):
    monkeypatch.setenv("LES_HIP_KERNEL", "strip")
    print(pc.case_driver(sim_lib, "cpu", monkeypatch, "MidV3", layers=cv.sim_layers, two_levels=True, filterRadious=6, device_cuts="none"))


def test_sim_driver_refusals(sim_lib, host_lib):
    pc.case_driver_refusals(sim_lib, "cpu")


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", pc.IMAGE_SHAPES)
def test_gpu_pool_image(H, W):
    print("sum:", pc.case_pool_image(None, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,W", pc.VOLUME_SHAPES)
def test_gpu_pool_volume(D, H, W):
    print("mean:", pc.case_pool_volume(None, D, H, W))


@pytest.mark.gpu
def test_gpu_pool_volume_unaligned_base():
    print("mean:", pc.case_pool_volume(None, *pc.UNALIGNED, lead=pc.GUARD + 1))
    print("mean:", pc.case_pool_volume(None, *pc.UNALIGNED, out_lead=pc.GUARD + 1))


@pytest.mark.gpu
def test_gpu_pool_volume_plain_loads(monkeypatch):
    """The other load flavour of the volume pool (LES_HIP_PYRAMID_NT) gives the same bytes."""
    for nt in ("1", "0"):
        monkeypatch.setenv("LES_HIP_PYRAMID_NT", nt)
        print("mean:", pc.case_pool_volume(None, pc.CHUNK + 3, 5, pc.SEGMENT + 8))


@pytest.mark.gpu
def test_gpu_pool_volume_nonfinite():
    print("NaN, inf outputs:", pc.case_pool_volume_nonfinite(None))


@pytest.mark.gpu
def test_gpu_pool_errors():
    print("refused:", pc.case_pool_errors(None))


@pytest.mark.gpu
@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("mind", pc.MIN_DISPS)
@pytest.mark.parametrize("half_shape,full_shape", pc.UPSAMPLE_SHAPES)
def test_gpu_upsample(half_shape, full_shape, mind, guide):
    counts = pc.case_upsample(None, half_shape, full_shape, mind, guide)
    print("kinds [kept, clamped, non-finite]:", counts)
    if full_shape == (33, 66):
        assert all(c > 0 for c in counts), counts


@pytest.mark.gpu
def test_gpu_upsample_errors():
    print("refused:", pc.case_upsample_errors(None))


@pytest.mark.gpu
@pytest.mark.parametrize("mind", pc.MIN_DISPS)
@pytest.mark.parametrize("naive,filt,interp", HALF_KINDS)
def test_gpu_create_half(naive, filt, interp, mind):
    print("finite values compared:", pc.case_create_half(None, naive, filt, interp, mind))


@pytest.mark.gpu
def test_gpu_create_half_errors():
    pc.case_create_half_errors(None)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("MidV3", "MidV2"))
def test_gpu_driver(host_lib, monkeypatch, which):
    print(pc.case_driver(None, "cuda", monkeypatch, which))


@pytest.mark.gpu
def test_gpu_driver_two_levels(host_lib, monkeypatch):
    print(pc.case_driver(None, "cuda", monkeypatch, "MidV3", two_levels=True))


@pytest.mark.gpu
def test_gpu_driver_refusals(host_lib):
    pc.case_driver_refusals(None, "cuda")
