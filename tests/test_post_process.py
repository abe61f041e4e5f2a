"""Dual-view post-processing (csrc/les_post.h: consistency check, fill, colour-weighted median) against the oracle (bit for bit)
and an independent fp64 restatement, at every weighted-median kernel variant and its edges, on the CPU simulator build
(-m "not gpu") and on the MI355X (-m gpu).  Cases: tests/post_cases.py."""
import time

import numpy as np
import pytest

from tests import post_cases as pc

F32 = np.float32

# windR -> les_weighted_median_kernel<NMAX, NT>: <256,64> up to 7, <1024,256> 8 .. 15, <2048,256> 16 .. 22, <4096,256> 23 .. 31
SWEEP = [0, 1, 2, 7, 8, 15, 16, 22, 23, 31]


@pytest.fixture(scope="module")
def sim_lib():
    from localexpstereo_amd import build
    return build.build_sim()


def _report(label, stats):
    print(f"{label}: " + "; ".join(f"{'LR'[v]} failed {s['failed']} changed {s['changed']} near-ties {s['near_ties']} "
                                   f"(picks moved {s['near_tie_moves']})" for v, s in enumerate(stats)))


def _sweep_scene(windR):
    H, W = (24, 40) if windR >= 16 else (30, 52)
    im = (pc.image(H, W, 100 + windR), pc.image(H, W, 200 + windR))
    return pc.scene_surfaces(H, W, 7 + windR), im


# ------------------------------------------------------------------------------------------------ shared bodies
def run_sweep(lib, windR):
    scene, (imL, imR) = _sweep_scene(windR)
    st = pc.case_post_process(lib, scene, imL, imR, windR)
    assert all(s["failed"] > 0 and s["changed"] > 0 for s in st), st
    H, W = imL.shape[:2]
    st2 = pc.case_post_process(lib, pc.scene_crossing(H, W, windR), imL, imR, windR, omega=1e6)
    assert windR == 0 or sum(s["tie_picks"] for s in st2) > 0, st2
    _report(f"windR {windR} surfaces", st)
    _report(f"windR {windR} crossing", st2)
    return st + st2


def run_filters(lib):
    """windR 0 and 1 in bilateral contexts, windR 4 and 20 in guided-filter contexts (radius 2 and 10)."""
    for windR, filt in ((0, "BF"), (1, "BF"), (4, "GF"), (20, "GF")):
        scene, (imL, imR) = _sweep_scene(windR)
        st = pc.case_post_process(lib, scene, imL, imR, windR, filter=filt)
        assert all(s["failed"] > 0 for s in st)


def run_shapes(lib):
    out = []
    for H, W, windR in ((5, 255, 3), (5, 256, 8), (5, 257, 16), (4, 257, 23)):
        im = (pc.image(H, W, 5), pc.image(H, W, 6))
        st = pc.case_post_process(lib, pc.scene_surfaces(H, W, 3), *im, windR)
        assert all(s["failed"] > 0 for s in st)
        out += st
    for H, W in ((1, 40), (40, 1), (1, 1)):
        im = pc.image(max(H, 8), max(W, 8), 9)[:H, :W].copy()
        for windR in (0, 2, 16):
            st = pc.case_post_process(lib, pc.scene_corners(H, W), im, im, windR)
            assert st[0]["failed"] > 0
    for H, W, windR in ((9, 11, 16), (9, 11, 31), (17, 13, 23)):
        im = (pc.image(H, W, 11), pc.image(H, W, 12, colours=3))
        st = pc.case_post_process(lib, pc.scene_surfaces(H, W, 5), *im, windR)
        st2 = pc.case_post_process(lib, pc.scene_corners(H, W), *im, windR)
        for s in st + st2:
            assert s["failed"] > 0
        out += st + st2
    for H, W, windR in ((20, 30, 2), (20, 30, 8)):
        im = (pc.image(H, W, 13), pc.image(H, W, 14))
        LL, LR = pc.scene_corners(H, W)
        st = pc.case_post_process(lib, (LL, LR), *im, windR)
        fl, _ = pc.lr_check_ref(pc.disparities(LL), pc.disparities(LR), 1.5)
        assert all(fl[y, x] == 255 for y in (0, H - 1) for x in (0, W - 1))
        assert st[0]["one_side"] > 0
    return out


def run_special_scenes(lib, windRs=(4, 20)):
    out = []
    im = np.full((12, 16, 3), 100, np.uint8)
    for windR in windRs:
        st = pc.case_post_process(lib, pc.scene_signed_zero(), im, im, windR)
        assert all(s["failed"] > 0 and s["tie_picks"] > 0 for s in st), st
        out += st
    im = (pc.image(14, 20, 21), pc.image(14, 20, 22))
    for windR in windRs:
        for sign in (1.0, -1.0):
            st = pc.case_post_process(lib, pc.scene_nonfinite(nan_sign=sign), *im, windR)
            assert st[0]["no_donor"] >= 20 and st[0]["nan_windows"] >= 20, st
            out += st
        st = pc.case_post_process(lib, pc.scene_nonfinite(extra=True), *im, windR)
        assert st[0]["one_side"] > 0 and st[1]["fill_ties"] > 0 and st[1]["inf_windows"] > 0 and st[1]["nan_windows"] > 0, st
        out += st
    imr = (pc.image(26, 33, 23), pc.image(26, 33, 24))
    for windR in (2, 9, 17):
        st = pc.case_post_process(lib, pc.scene_random_nonfinite(26, 33, windR), *imr, windR)
        assert all(s["nan_windows"] > 0 and s["inf_windows"] > 0 for s in st), st
        out += st
    return out


def run_weights(lib):
    """omega 0.05: colours at least 8 apart in L1 within the window, every off-centre weight underflows to 0 and the median keeps
    the centre's own post-fill label; omega 1e6: near-uniform weights (a plain median), with repeated colours; omega 10."""
    H, W = 24, 30
    ys, xs = np.mgrid[0:H, 0:W]
    distinct = np.stack([(xs * 8) % 256, (ys * 8) % 256, np.full_like(xs, 50)], -1).astype(np.uint8)
    LL, LR = pc.scene_surfaces(H, W, 41)
    assert np.all(pc.weight_table(0.05)[8:] == 0)
    for windR in (3, 8):
        pc.case_post_process(lib, (LL, LR), distinct, distinct, windR, omega=0.05)
        ref, _, _ = pc.post_process_ref(LL, LR, distinct, distinct, windR, 1.5, 0.05)
        fl, _ = pc.lr_check_ref(pc.disparities(LL), pc.disparities(LR), 1.5)
        failb = np.where(fl > 0, 255, 0).astype(np.uint8)
        filled, _ = pc.fill_ref(LL, failb, pc.dilate3(failb))
        assert failb.any() and np.array_equal(ref[0].view(np.uint32), filled.view(np.uint32))
    out = []
    for colours in (0, 2, 5):
        im = (pc.image(H, W, 31, colours), pc.image(H, W, 32, colours))
        for omega in (10.0, 1e6):
            for windR in (4, 12):
                st = pc.case_post_process(lib, (LL, LR), *im, windR, omega=omega)
                assert all(s["changed"] > 0 for s in st)
                out += st
    for thr in (1.0, 1.5):
        im = (pc.image(H, W, 33, 4), pc.image(H, W, 34, 4))
        out += pc.case_post_process(lib, (LL, LR), *im, 6, thr=thr)
    return out


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_matches_reference_loop():
    """The vectorised restatement equals the literal per-pixel loop, bit for bit, on tiny scenes (ties, signed zeros, NaN, inf)."""
    cases = [(pc.scene_surfaces(9, 13, 2), pc.image(9, 13, 1), pc.image(9, 13, 2, colours=3)),
             (pc.scene_signed_zero(), np.full((12, 16, 3), 100, np.uint8), np.full((12, 16, 3), 100, np.uint8)),
             (pc.scene_nonfinite(extra=True), pc.image(14, 20, 3), pc.image(14, 20, 4)),
             (pc.scene_crossing(10, 14, 1), pc.image(10, 14, 5), pc.image(10, 14, 6)),
             (pc.scene_random_nonfinite(8, 11, 3), pc.image(8, 11, 7), pc.image(8, 11, 8)),
             (pc.scene_corners(1, 9), pc.image(8, 9, 9)[:1].copy(), pc.image(8, 9, 9)[:1].copy())]
    for (LL, LR), imL, imR in cases:
        for windR, omega, thr in ((0, 10.0, 1.5), (2, 10.0, 1.0), (4, 1e6, 1.5), (7, 0.05, 1.5)):
            ref, _, _ = pc.post_process_ref(LL, LR, imL, imR, windR, thr, omega)
            loop = pc.post_process_loop(LL, LR, imL, imR, windR, thr, omega)
            for a, b in zip(ref, loop):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_order_is_total():
    """-0 and +0 tie and NaNs of either sign rank after +inf, in the restatement's sort."""
    LL = np.zeros((1, 5, 4), F32)
    LL[0, :, 2] = [np.copysign(np.nan, -1.0), np.inf, -0.0, 0.0, np.nan]
    failb = np.zeros((1, 5), np.uint8)
    failb[0, 2] = 255
    LL = pc.tag(LL, LL.copy())[0]
    im = np.zeros((1, 5, 3), np.uint8)
    out, _, _ = pc.median_ref(LL, failb, im, 2, 1e6)
    # sorted: -0 (scan 2), +0 (3), inf (1), NaN (0), NaN (4); five equal weights -> the third, +inf
    assert out[0, 2, 3] == LL[0, 1, 3]


# ------------------------------------------------------------------------------------------------ CPU simulator build
def test_sim_consistency_check_edges(sim_lib, oracle_mod):
    assert pc.case_consistency_edges(sim_lib) > 20


@pytest.mark.parametrize("windR", SWEEP)
def test_sim_windR_sweep(sim_lib, oracle_mod, windR):
    run_sweep(sim_lib, windR)


def test_sim_filters(sim_lib, oracle_mod):
    run_filters(sim_lib)


def test_sim_shapes(sim_lib, oracle_mod):
    run_shapes(sim_lib)


def test_sim_signed_zero_nan_inf(sim_lib, oracle_mod):
    _report("special scenes", run_special_scenes(sim_lib)[:2])


def test_sim_weights(sim_lib, oracle_mod):
    run_weights(sim_lib)


# ------------------------------------------------------------------------------------------------ MI355X
@pytest.mark.gpu
def test_gpu_consistency_check_edges(oracle_mod):
    assert pc.case_consistency_edges(None) > 20


@pytest.mark.gpu
@pytest.mark.parametrize("windR", SWEEP)
def test_gpu_windR_sweep(oracle_mod, windR):
    run_sweep(None, windR)


@pytest.mark.gpu
def test_gpu_filters_shapes_scenes_weights(oracle_mod):
    run_filters(None)
    run_shapes(None)
    run_special_scenes(None, windRs=(4, 20, 31))
    run_weights(None)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,windR", [(992, 1436, 20), (450, 375, 31)], ids=["1436x992_r20", "375x450_r31"])
def test_gpu_large_against_oracle(oracle_mod, H, W, windR):
    """Large two-view post-processing against the oracle, bit for bit, and a repeat run bit-equal."""
    from oracle import oracle as om
    imL, imR = pc.image(H, W, 51), pc.image(H, W, 52)
    LL, LR = pc.scene_surfaces(H, W, 53)
    e = pc.context(None, imL, imR, windR)
    try:
        t0 = time.perf_counter()
        got = e.post_process_host(LL, LR, threshold=1.5, omega=10.0)
        t1 = time.perf_counter()
        again = e.post_process_host(LL, LR, threshold=1.5, omega=10.0)
    finally:
        e.close()
    t2 = time.perf_counter()
    ora = om.post_process(LL, LR, imL, imR, windR=windR, threshold=1.5, omega=10.0)
    t3 = time.perf_counter()
    fl, fr = pc.lr_check_ref(pc.disparities(LL), pc.disparities(LR), 1.5)
    for v in range(2):
        assert np.array_equal(got[v].view(np.uint32), again[v].view(np.uint32)), "a repeated post-processing differs"
        same = (got[v].view(np.uint32) == ora[v].view(np.uint32)).all(-1)
        assert same.all(), f"view {'LR'[v]}: {int((~same).sum())} pixels differ from the oracle"
    changed = (got[0].view(np.uint32) != LL.view(np.uint32)).any(-1).mean()
    assert (fl > 0).mean() > 0.01 and changed > 0.005
    print(f"{W} x {H} windR {windR}: failed {(fl > 0).mean():.3f} / {(fr > 0).mean():.3f}, changed {changed:.3f}; "
          f"device {t1 - t0:.2f} s, oracle {t3 - t2:.2f} s")
