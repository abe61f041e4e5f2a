"""Every compiled unary-cost kernel instantiation (csrc/les_hip_march_tables.inc) against its reference, at every radius, route and job
cut: the march kernel's wide and narrow entries at radii 2 .. 10 (interpolation 0 / 1 / 2, the image-based energy with v = 0 and v != 0,
whole-image slabs and LayerManager cells, every forced cut bit-identical), every strip-kernel family at every radius, awkward image
shapes for every filter, and the product against the plain build.  CPU simulator build (-m "not gpu": each instantiation once, at the
smallest shape that reaches it) and MI355X (-m gpu: the full matrix at shapes that split jobs).  Cases: tests/instantiation_cases.py."""
import os

import pytest

from tests import instantiation_cases as ns

MARCH_RADII = sorted(ns.MARCH_BY)
STRIP_CASES = [(f, R, None) for f in ns.STRIP_FAMILIES for R in ns.STRIP_RADII] + \
              [("strip", R, v) for R, vs in ns.STRIP_VARIANTS.items() for v in vs]


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


@pytest.fixture(scope="module")
def tally():
    t = ns.Tally()
    yield t
    print("\n" + t.report())


def test_census_matches_the_matrix():
    """The instantiations the tables compile are exactly the ones this file runs (LES_MARCH_LAB entries excluded)."""
    compiled, tested = ns.census(), ns.matrix()
    assert compiled - tested == set(), f"compiled but never tested: {sorted(compiled - tested)}"
    assert tested - compiled == set(), f"tested but not compiled: {sorted(tested - compiled)}"
    cases = {("march", R, (wgc, nj, ns.MARCH_BY[R])) for R in MARCH_RADII for wgc, nj in ns.MARCH_ENTRIES.values()}
    cases |= {(f, R, v or 0) for f, R, v in STRIP_CASES}
    assert cases == tested


def test_census_sees_an_added_entry():
    text = open(ns.TABLES).read()
    added = text.replace("LES_MARCH_ENTRY(10, 256, 1, 7),", "LES_MARCH_ENTRY(10, 256, 1, 7), LES_MARCH_ENTRY(11, 256, 1, 8),", 1)
    assert ("march", 11, (256, 1, 8)) in ns.census(added) - ns.matrix()
    added = text.replace("LES_STRIP_ENTRY(10, 8, 128, 21, 6, 2),", "LES_STRIP_ENTRY(10, 8, 128, 21, 6, 2), LES_STRIP_ENTRY(10, 9, 96, 21, 3, 2),", 1)
    assert ("strip", 10, 9) in ns.census(added) - ns.matrix()
    added = text.replace("LES_INTERP_ENTRY(15, 96, 16, 6, 2, SRC_)", "LES_INTERP_ENTRY(15, 96, 16, 6, 2, SRC_), LES_INTERP_ENTRY(20, 96, 16, 6, 2, SRC_)", 1)
    assert {("nearest", 20, 0), ("quadratic", 20, 0)} <= ns.census(added) - ns.matrix()
    lab = "#if defined(LES_MARCH_LAB)\n    LES_MARCH_ENTRY(11, 256, 1, 8),\n#endif\n"
    assert ns.census(text.replace("const MarchEntry kMarch[] = {\n", "const MarchEntry kMarch[] = {\n" + lab, 1)) == ns.census(text)


def test_workgroup_count_restatement():
    """groups() on hand-checked cuts: a 45-column target is 23 + 22 at TW <= 44, rows balanced, narrow jobs padded to pairs."""
    from localexpstereo_amd import api
    t = api._rects([(0, 0, 45, 10)])
    assert ns.groups(t, 10, "narrow", 1 << 30) == 1 and ns.groups(t, 10, "narrow", 4) == 2      # 1 column strip x 3 row chunks -> 2 pairs
    assert ns.groups(api._rects([(0, 0, 217, 7)]), 10, "wide", 1 << 30) == 2                    # TW 216: 109 + 108
    assert ns.groups(api._rects([(0, 0, 88, 7)] * 3), 10, "narrow", 7) == 2


# ---------------------------------------------------------------- CPU simulator build
def sim_shape(R):
    """Small enough for the simulator; tall enough that the ring wraps and rows BY / BY + 1 cut the targets into several jobs."""
    return 2 * ns.MARCH_BY[R] + 3, 4 * R + 9


@pytest.mark.parametrize("R", MARCH_RADII)
def test_sim_march_volume(sim_lib, oracle_mod, tally, R):
    H, W = sim_shape(R)
    ns.case_march_volume(sim_lib, R, H, W, 8, tally)


@pytest.mark.parametrize("R", MARCH_RADII)
def test_sim_march_interp_and_image(sim_lib, oracle_mod, tally, R):
    H, W = sim_shape(R)
    which = ("default", "wide", "narrow", f"narrow-rows{ns.MARCH_BY[R]}")
    ns.case_march_interp(sim_lib, R, H, W, 8, tally, which=which)
    ns.case_march_naive(sim_lib, R, H, W, tally, which=which)


@pytest.mark.parametrize("fam,R,variant", STRIP_CASES, ids=[f"{f}-R{R}" + (f"-v{v}" if v else "") for f, R, v in STRIP_CASES])
def test_sim_strip(sim_lib, oracle_mod, tally, fam, R, variant):
    W = ns.strip_tw(R) + 1 if variant is None else 50
    ns.case_strip_family(sim_lib, fam, R, 7, W, 8, tally, variant=variant)


SIM_SHAPES = [(1, 37), (37, 1), (2, 2), (5, 7), (4, 23), (5, 23), (9, 4), (9, 5), (6, 119), (6, 120), (6, 121), (6, 247), (6, 248), (6, 249)]


@pytest.mark.parametrize("filt", ["GF", "GF-strip", "BF", ""])
@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_sim_shapes(sim_lib, oracle_mod, tally, filt, naive):
    """Radius 2: thin and tiny images, H / W = 2R and 2R + 1, W = TW - 1, TW, TW + 1 of both march entries (each forced on the march)."""
    for H, W in SIM_SHAPES:
        ns.case_shape(sim_lib, H, W, 2, filt.split("-")[0], naive, tally, strip=filt.endswith("strip"))


# ---------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("R", MARCH_RADII)
def test_gpu_march_matrix(oracle_mod, tally, R):
    """Every cut, every route; W = wide TW + 1 splits both entries' jobs, H spans several row blocks of every forced row count."""
    H, W = 3 * ns.MARCH_BY[R] + 4 * R + 5, 256 - 4 * R + 1
    ns.case_march_volume(None, R, H, W, 12, tally)
    ns.case_march_interp(None, R, H, W, 12, tally)
    ns.case_march_naive(None, R, H, W, tally)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,R,variant", STRIP_CASES, ids=[f"{f}-R{R}" + (f"-v{v}" if v else "") for f, R, v in STRIP_CASES])
def test_gpu_strip(oracle_mod, tally, fam, R, variant):
    W = 2 * ns.strip_tw(R, variant or 0) + 1
    ns.case_strip_family(None, fam, R, 2 * R + 9, W, 12, tally, variant=variant)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 10])
@pytest.mark.parametrize("filt", ["GF", "GF-strip", "BF", ""])
@pytest.mark.parametrize("naive", [False, True], ids=["volume", "image"])
def test_gpu_shapes(oracle_mod, tally, R, filt, naive):
    for H, W in ns.shapes(R):
        ns.case_shape(None, H, W, R, filt.split("-")[0], naive, tally, strip=filt.endswith("strip"))


@pytest.mark.gpu
@pytest.mark.parametrize("R", MARCH_RADII)
def test_gpu_plain_build_every_radius(oracle_mod, R):
    """The inline-assembly paths (DPP scan, role C's loads with hand-kept vmcnt, v_cvt_rpi_i32_f32) at every radius and both entries:
    bit-identical to libles_plain.so on interpolation 1 and 2 and the image-based energy.  (Small radii have the largest stage-2 scale,
    so role C's quantised a, b reach [2^23, 2^24), where a rounding of x + 0.5 to float before the floor differs from the instruction.)"""
    from localexpstereo_amd import build
    assert os.path.exists(build.PLAIN_SO), "libles_plain.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    for entry in ns.MARCH_ENTRIES:
        n = ns.case_plain_vs_product(build.PLAIN_SO, R, entry, 2 * (3 * ns.MARCH_BY[R]) + 8 * R + 3, 2 * (256 - 4 * R) + 3)
        assert n > 0
