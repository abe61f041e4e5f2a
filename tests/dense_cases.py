"""Cases of the dense label-map pass (les_hip_unary_labels, csrc/les_dense.h) shared by the simulator tests (-m "not gpu") and the MI355X
tests (-m gpu), in the style of parity_cases.py.

The reference of every case is the per-pixel operator: one call per pixel p with filterRect = (p +- windR) clipped to the image, a 1 x 1
target at p and the pixel's own plane -- evaluated by the CPU oracle (Oracle.unary_batch) for the guided filter on a linearly read volume
and on the image-based energy with v == 0, by the restatements of interp_cases / vdisp_cases / bilateral_cases for the other kinds of
context.  Tolerances are those modules' own (parity_cases.compare_maps with TIGHT / NAIVE_TIGHT, interp_cases.compare)."""
import threading

import numpy as np

from localexpstereo_amd import api, synth
from tests import bilateral_cases as bc
from tests import interp_cases as ic
from tests import parity_cases as pc
from tests.util import load_cones_crop

F32 = np.float32
FILL = ic.FILL


# ------------------------------------------------------------------------------------------------ helpers
def pixel_jobs(H, W, windR, pixels=None, region=None):
    """(filterRects, targetRects, ys, xs) of the per-pixel calls: every pixel of `region` (x, y, w, h; None: the image) or the listed (y, x)."""
    if pixels is None:
        x0, y0, w, h = (0, 0, W, H) if region is None else region
        ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
        ys, xs = ys.ravel(), xs.ravel()
    else:
        ys, xs = np.asarray(pixels, np.int64).reshape(-1, 2).T
    fx0, fy0 = np.maximum(xs - windR, 0), np.maximum(ys - windR, 0)
    fx1, fy1 = np.minimum(xs + windR + 1, W), np.minimum(ys + windR + 1, H)
    frs = np.stack([fx0, fy0, fx1 - fx0, fy1 - fy0], 1).astype(np.int32)
    trs = np.stack([xs, ys, np.ones_like(xs), np.ones_like(ys)], 1).astype(np.int32)
    return frs, trs, ys, xs


def as_map(labels, H, W):
    return np.ascontiguousarray(np.asarray(labels).view(F32).reshape(H, W, 4))


def dense(e, labels, mode=0, region=None, check=True, fill=np.nan):
    """les_hip_unary_labels on a host label map: upload, one dense pass into a map pre-filled with `fill`, download."""
    H, W = e.H, e.W
    lab = as_map(labels, H, W)
    bl, bc_ = api.DeviceBuffer(e, H * W * 16), api.DeviceBuffer(e, H * W * 4)
    try:
        bl.upload(lab)
        bc_.upload(np.full((H, W), fill, F32))
        e.unary_labels(bl.ptr, bc_.ptr, mode=mode, region=region, check=check)
        e.synchronize()
        return bc_.download((H, W), F32)
    finally:
        bl.free()
        bc_.free()


def oracle_pixels(o, labels, windR, mode=0, check=True, pixels=None, region=None):
    """The per-pixel oracle: H x W map, NaN where no call was made."""
    lab = as_map(labels, o.H, o.W)
    frs, trs, ys, xs = pixel_jobs(o.H, o.W, windR, pixels, region)
    return o.unary_batch(frs, trs, lab[ys, xs], mode=mode, check=check)


def planted_labels(H, W, D, seed, min_disp=0.0, v=0.0):
    """A different plane at every pixel plus the special ones: NaN, +inf, an out-of-range c, a plane that leaves [min_disp, max_disp] on part
    of its window, an invalid label."""
    lab = as_map(pc._label_map(H, W, D, seed, noise=0.3), H, W).copy()
    lab[..., 2] += F32(min_disp)
    rng = np.random.default_rng(seed + 1)
    if v:
        lab[..., 3] = rng.uniform(-v, v, (H, W)).astype(F32)
        lab[::3, ::2, 3] = 0.0
        lab[1::4, 1::3, 3] = -0.0
    lab[H // 2, W // 3] = (np.nan, 0.0, 1.0, 0.0)
    lab[H // 3, W // 2] = (0.0, 0.0, np.inf, 0.0)
    lab[2, W - 3] = (0.0, 0.0, 1e9, 0.0)
    lab[H - 2, 1] = (0.0, 0.0, -50.0, 0.0)
    lab[H // 2 + 1, W // 2 + 2] = (0.31, 0.0, min_disp + 1.0 - 0.31 * (W // 2 + 2), 0.0)      # in range at the pixel, out of range across its window
    lab[3, 4] = (0.0, 0.0, 500.0, 0.0)
    lab[1, 1] = (0.0, 0.0, min_disp + 0.2, 0.0)                  # the first slice: the quadratic read (interpolation 2) is NaN at every pixel
    lab[H - 1, W - 1] = (0.0, 0.27, min_disp + (D - 2) - 0.27 * (H - 1), 0.0)
    return lab


def inner_region(H, W):
    return (3, 2, W - 7, H - 5)


def check_written(got, region, H, W, fill_is_nan=True):
    """Pixels outside the region still hold the fill value."""
    m = np.ones((H, W), bool)
    if region is not None:
        x, y, w, h = region
        m[y:y + h, x:x + w] = False
    else:
        m[:] = False
    assert np.all(np.isnan(got[m])) if fill_is_nan else np.all(got[m] == FILL), "pixels outside the region were written"
    return ~m


# ------------------------------------------------------------------------------------------------ 1. per-pixel oracle parity
def case_oracle_parity(lib, windR, H, W, D=12, min_disp=0.0, modes=(0, 1), checks=(True, False), region=True, sample=None, expect_kind=1):
    """Cost volume, linear interpolation, guided filter: whole map and a region strictly inside it against Oracle.unary_batch.
    sample: evaluate the oracle on that many seeded pixels only (plus the planted ones), the dense pass still on every pixel."""
    max_disp = D - 1 + min_disp
    pr = pc.synth_pair(lib, H, W, D, windR=windR, max_disp=max_disp, min_disp=min_disp)
    worst = 0.0
    try:
        lab = planted_labels(H, W, D, 3 + windR, min_disp=min_disp)
        pixels = None
        if sample is not None:
            rng = np.random.default_rng(windR)
            pixels = np.stack([rng.integers(0, H, sample), rng.integers(0, W, sample)], 1)
            special = [(H // 2, W // 3), (H // 3, W // 2), (2, W - 3), (H - 2, 1), (H // 2 + 1, W // 2 + 2), (3, 4), (H - 1, W - 1), (0, 0), (0, W - 1), (H - 1, 0)]
            pixels = np.unique(np.concatenate([pixels, np.array(special)]), axis=0)
        for mode in modes:
            assert pr.e.unary_labels_kind(mode) == expect_kind
            for check in checks:
                ref = oracle_pixels(pr.o, lab, windR, mode, check, pixels=pixels)
                got = dense(pr.e, lab, mode, None, check)
                assert not np.isnan(got).any(), "the whole-map pass left pixels unwritten"
                got_s = got if pixels is None else np.where(np.isnan(ref), np.nan, got)      # compare where the oracle was evaluated
                worst = max(worst, pc.compare_maps(got_s, ref))
                if check:
                    assert got[3, 4] == F32(1e6)
                if region and pixels is None:
                    rg = inner_region(H, W)
                    gr = dense(pr.e, lab, mode, rg, check)
                    inside = check_written(gr, rg, H, W)
                    assert np.array_equal(gr[inside].view(np.uint32), got[inside].view(np.uint32)), "a region pass differs from the whole-map pass"
    finally:
        pr.close()
    return worst


# ------------------------------------------------------------------------------------------------ 2. every kind of context
def _restated(pr, lab, windR, mode, check, region=None, pixels=None):
    """Expected map / tolerance scale / written mask from a pair's own restatement (interp_cases.expected_batch)."""
    frs, trs, ys, xs = pixel_jobs(pr.H, pr.W, windR, pixels, region)
    ref, S, written = ic.expected_batch(pr, frs, trs, lab[ys, xs], mode, check)
    return ref[0], S[0], written[0]


class LinearFiltered:
    """bilateral_cases.BfPair (bilateral / unfiltered aggregation of the LINEARLY read volume: the oracle's own gather) behind the interface of
    interp_cases.InterpPair, whose restatement covers interpolation 0 and 2 only."""

    def __init__(self, lib, H, W, D, windR, flt):
        self.bp = bc.synth_bf(lib, H, W, D, windR=windR, filter=flt)
        self.e, self.H, self.W, self.D, self.filter = self.bp.e, self.bp.H, self.bp.W, self.bp.D, flt

    def expected(self, fr, tr, plane, mode, check, out):
        return self.bp.expected(tuple(int(v) for v in fr), tuple(int(v) for v in tr), tuple(float(v) for v in plane), mode, check, out=out)[1]

    def close(self):
        self.bp.close()


def context_pair(lib, interp, flt, H, W, D, windR, min_disp=0.0):
    """The pair whose restatement is the reference of a cost-volume context at interpolation `interp` and filter `flt`."""
    if interp == 1 and flt != "GF":
        return LinearFiltered(lib, H, W, D, windR, flt)
    return ic.InterpPair(lib, synth.make_guide(H, W, 1), synth.make_guide(H, W, 2), synth.make_volume(D, H, W, 3), synth.make_volume(D, H, W, 4), interp,
                         windR=windR, filter=flt, min_disp=min_disp)


def case_context_kinds_restated(pr, windR, v=0.0, modes=(0, 1), checks=(True, False), stride=1, seed=5, min_disp=0.0):
    """A pair of interp_cases / vdisp_cases / bilateral-through-InterpPair: the dense pass against the pair's restatement of the per-pixel
    calls (every stride-th pixel of a seeded order plus the image corners)."""
    H, W, D = pr.H, pr.W, pr.D
    lab = planted_labels(H, W, D, seed, min_disp=min_disp, v=v)
    pixels = None
    if stride > 1:
        ys, xs = np.mgrid[0:H, 0:W]
        sel = (ys * 7 + xs * 3) % stride == 0
        sel[[0, 0, -1, -1], [0, -1, 0, -1]] = True
        sel[H // 2, W // 3] = sel[H // 3, W // 2] = sel[3, 4] = True
        pixels = np.stack([ys[sel], xs[sel]], 1)
    worst = 0.0
    for mode in modes:
        assert pr.e.unary_labels_kind(mode) == 1
        for check in checks:
            ref, S, written = _restated(pr, lab, windR, mode, check, pixels=pixels)
            got = dense(pr.e, lab, mode, None, check, fill=FILL)
            worst = max(worst, ic.compare(pr, got, ref, S, written))
    return worst


def case_naive_oracle(lib, windR, modes=(0, 1), stride=1, crop=None):
    """Image-based energy, v == 0, on the cones crop: against the oracle's per-pixel calls with NAIVE_TIGHT."""
    imL, imR = load_cones_crop()
    if crop is not None:
        imL, imR = np.ascontiguousarray(imL[:crop[0], :crop[1]]), np.ascontiguousarray(imR[:crop[0], :crop[1]])
    pr = pc.NaivePair(lib, imL, imR, 31.0, windR=windR)
    worst = 0.0
    try:
        H, W = pr.H, pr.W
        lab = planted_labels(H, W, 32, 9)
        ys, xs = np.mgrid[0:H, 0:W]
        sel = (ys * 5 + xs * 3) % stride == 0
        pixels = np.stack([ys[sel], xs[sel]], 1)
        for mode in modes:
            assert pr.e.unary_labels_kind(mode) == 1
            ref = oracle_pixels(pr.o, lab, windR, mode, True, pixels=pixels)
            got = dense(pr.e, lab, mode, None, True)
            worst = max(worst, pc.compare_maps(np.where(np.isnan(ref), np.nan, got), ref, tight=pc.NAIVE_TIGHT))
    finally:
        pr.close()
    return worst


def case_against_job_route(e, lab, modes=(0, 1), checks=(True, False), windR=None, tight=pc.TIGHT):
    """Any context against the per-pixel-job route this change does not touch (les_hip_unary_batch with 1 x 1 targets): sentinel and NaN sets
    exact, values within 2 x `tight` (each side is within `tight` of the oracle)."""
    H, W = e.H, e.W
    windR = e.params.windR if windR is None else windR
    frs, trs, ys, xs = pixel_jobs(H, W, windR)
    worst = 0.0
    for mode in modes:
        for check in checks:
            ref = e.unary_batch(frs, trs, lab[ys, xs], mode=mode, check=check)
            got = dense(e, lab, mode, None, check)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN sets differ"
            m = ~np.isnan(ref)
            assert np.array_equal(got[m] == F32(1e6), ref[m] == F32(1e6)), "1e6 sentinels differ"
            v = m & (ref != F32(1e6))
            err = np.abs(got[v].astype(np.float64) - ref[v]).max() if v.any() else 0.0
            assert err <= 2 * tight, f"dense pass vs job route: {err:.3e}"
            worst = max(worst, float(err))
    return worst


# ------------------------------------------------------------------------------------------------ 3. which kernel ran
def case_kind_everywhere(lib, windRs=tuple(range(2, 22)) + (24,), H=24, W=30, D=6):
    """unary_labels_kind is 1 for the guided filter at every windR 2 .. 21 (and what the build instantiated at 24: this build has it) on both
    energies and all three interpolations, and for BF / ""."""
    imL, imR = synth.make_guide(H, W, 1), synth.make_guide(H, W, 2)
    volL, volR = synth.make_volume(D, H, W, 3), synth.make_volume(D, H, W, 4)
    for windR in windRs:
        e = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=windR, lib=lib)
        for interp in (0, 1, 2):
            e.setInterpolationMethod(interp)
            assert e.unary_labels_kind(0) == 1 and e.unary_labels_kind(1) == 1, (windR, interp)
        assert e.unary_labels_kind(2) == -1
        e.close()
        e = api.HipCostVolumeEnergy.naive(imL, imR, windR=windR, max_disp=5.0, lib=lib)
        assert e.unary_labels_kind(0) == 1 and e.unary_labels_kind(1) == 1, windR
        e.close()
    for flt in ("BF", ""):
        e = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=20, eps=10.0, lib=lib, filter=flt)
        assert e.unary_labels_kind(0) == 1
        e.close()
        e = api.HipCostVolumeEnergy.naive(imL, imR, windR=20, eps=10.0, max_disp=5.0, lib=lib, filter=flt)
        assert e.unary_labels_kind(1) == 1
        e.close()


# ------------------------------------------------------------------------------------------------ 4. piecewise-constant property
def block_labels(H, W, D, K, seed, block=4, invalid=True):
    """K planes in block x block tiles (one of them invalid): (label map, planes, index map)."""
    rng = np.random.default_rng(seed)
    planes = pc.random_planes(K, D, H, W, seed, slant=0.15)
    planes[:, 2] = rng.uniform(1, D - 2, K) - planes[:, 0] * W / 2 - planes[:, 1] * H / 2
    if invalid:
        planes[K - 1] = (0.0, 0.0, 500.0, 0.0)
    ys, xs = np.mgrid[0:H, 0:W]
    idx = rng.integers(0, K, ((H + block - 1) // block, (W + block - 1) // block))[ys // block, xs // block]
    return np.ascontiguousarray(planes[idx]), planes, idx


def case_piecewise_constant(pr, K=6, seed=13, block=4, modes=(0,), check=True, tight=True, nthreads=0):
    """Fact 1: on a piecewise-constant label map the dense pass equals the whole-image aggregation of each distinct plane sampled where that
    plane is the label (Oracle.aggregate_planes)."""
    H, W, D = pr.H, pr.W, pr.D
    lab, planes, idx = block_labels(H, W, D, K, seed, block)
    worst = 0.0
    for mode in modes:
        whole = pr.o.aggregate_planes(planes, mode=mode, check=check, nthreads=nthreads)
        ref = np.take_along_axis(whole, idx[None], 0)[0]
        got = dense(pr.e, lab, mode, None, check)
        worst = max(worst, pc.compare_maps(got, ref, tight=tight))
    return worst, lab


def border_and_sample(H, W, windR, n, seed):
    """(y, x) of every pixel within windR of the image border plus n seeded interior pixels."""
    ys, xs = np.mgrid[0:H, 0:W]
    border = (ys < windR) | (ys >= H - windR) | (xs < windR) | (xs >= W - windR)
    rng = np.random.default_rng(seed)
    iy, ix = rng.integers(windR, H - windR, n), rng.integers(windR, W - windR, n)
    return np.unique(np.concatenate([np.stack([ys[border], xs[border]], 1), np.stack([iy, ix], 1)]), axis=0)


# ------------------------------------------------------------------------------------------------ 5. the optimiser's invariant
def assert_is_cost_of_labels(runner, tight=pc.TIGHT):
    """unary_labels(labels) equals the runner's cost map: sentinels identical, |diff| <= 2 x tight."""
    import torch
    e = runner.e
    out = torch.full((e.H, e.W), float("nan"), dtype=torch.float32, device=runner.device)
    e.unary_labels(runner.labels.data_ptr(), out.data_ptr(), mode=runner.mode, check=True)
    e.synchronize()
    got, cur = out.cpu().numpy(), runner.cur.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got == F32(1e6), cur == F32(1e6)), "sentinels differ"
    v = cur != F32(1e6)
    err = float(np.abs(got[v].astype(np.float64) - cur[v]).max())
    assert err <= 2 * tight, f"cost map is not the cost of its labels: {err:.3e}"
    return err


def case_optimiser_invariant(lib, device, H=48, W=64, D=12, units=(6, 18), gc=True, device_cuts=None):
    """Fact 2: after init_labels() + one PatchMatch iteration, and after one graph-cut iteration, cur == unary_labels(labels)."""
    from localexpstereo_amd import gc as gcm
    from localexpstereo_amd import pm
    imL, vol = synth.make_guide(H, W, 5), synth.make_volume(D, H, W, 6)
    e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=8, eps=1e-4, th_col=0.5, max_disp=D - 1.0, lib=lib)
    table = [[(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANDOM, 2)] for _ in units]
    r = pm.PMRunner(e, units, table, seed=3, device=device)
    worst = 0.0
    try:
        r.init_labels()
        r.iteration(0)
        r._sync()
        worst = max(worst, assert_is_cost_of_labels(r))
        if gc:
            g = gcm.GraphCut(imL, None, lambda_=1.0)
            r.device_cuts = device_cuts
            r.begin_gc(g)
            r.gc_iteration(1)
            r._sync()
            worst = max(worst, assert_is_cost_of_labels(r))
            g.close()
    finally:
        r.close()
        e.close()
    return worst


# ------------------------------------------------------------------------------------------------ 6. resume
def _driver(lib, device, imL, imR, volL, volR, windR=8, units=(8,), seed=3, **kw):
    from localexpstereo_amd import stereo
    e = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=windR, eps=1e-4, th_col=0.5, lib=lib)
    st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=1.0, windR=windR), device=device, seed=seed, device_cuts=kw.pop("device_cuts", None), **kw)
    for u in units:
        st.addLayer(u, [(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANDOM, 2)])
    return e, st


def case_resume(lib, device, H=40, W=52, D=12, gc_iters=2, device_cuts=None):
    """run A = run(gc_iters, pmInit=1); run B = run(0, pmInit=0, labeling=A's raw labelling): B returns A's labels unchanged and its row 0
    data equals A's last data within H W 2 TIGHT.  Two views with the dict form: each view gets its own map.  recost_after_post changes only
    the last row, whose data is the sum of unary_labels(final labels)."""
    imL, imR = synth.make_guide(H, W, 5), synth.make_guide(H, W, 7)
    volL, volR = synth.make_volume(D, H, W, 6), synth.make_volume(D, H, W, 8)
    bound = H * W * 2 * pc.TIGHT
    e, A = _driver(lib, device, imL, imR, volL, volR, device_cuts=device_cuts)
    labA, rawA = A.run(gc_iters, (0,), 1)
    e.close()
    assert np.array_equal(labA, rawA)                                        # one view: no post-processing
    e, B = _driver(lib, device, imL, imR, volL, volR, device_cuts=device_cuts)
    labB, rawB = B.run(0, (0,), 0, labeling=rawA)
    e.close()
    assert np.array_equal(rawB.view(np.uint32), rawA.view(np.uint32)) and np.array_equal(labB.view(np.uint32), rawA.view(np.uint32))
    assert [r["index"] for r in B.log] == [0]
    assert abs(B.log[0]["data"] - A.log[-1]["data"]) <= bound, (B.log[0]["data"], A.log[-1]["data"])

    # two views
    e, A2 = _driver(lib, device, imL, imR, volL, volR, device_cuts=device_cuts)
    lab2, raw2 = A2.run(1, (0, 1), 1)
    e.close()
    assert sorted(A2.raw_labelings) == [0, 1] and np.array_equal(A2.raw_labelings[0], raw2)
    assert not np.array_equal(A2.raw_labelings[0], A2.raw_labelings[1])
    e, B2 = _driver(lib, device, imL, imR, volL, volR, device_cuts=device_cuts)
    B2.run(0, (0, 1), 0, labeling=dict(A2.raw_labelings))
    for m in (0, 1):
        assert np.array_equal(B2.raw_labelings[m].view(np.uint32), A2.raw_labelings[m].view(np.uint32)), f"view {m} did not resume from its own map"
    assert abs(B2.log[0]["data"] - A2.log[-2]["data"]) <= bound              # (A2's last row is the one after the post-processing)
    try:
        B2.run(0, (0, 1), 0, labeling={0: A2.raw_labelings[0]})
        raise AssertionError("a dict without the right view's map was accepted")
    except ValueError:
        pass
    # a single array keeps the reference's meaning: every view starts from it
    B2.run(0, (0, 1), 0, labeling=A2.raw_labelings[0])
    assert np.array_equal(B2.raw_labelings[1].view(np.uint32), A2.raw_labelings[0].view(np.uint32))
    e.close()

    # recost_after_post
    e, C = _driver(lib, device, imL, imR, volL, volR, device_cuts=device_cuts, recost_after_post=True)
    labC, rawC = C.run(1, (0, 1), 1)
    assert np.array_equal(labC.view(np.uint32), lab2.view(np.uint32)) and np.array_equal(rawC.view(np.uint32), raw2.view(np.uint32))
    assert len(C.log) == len(A2.log)
    for a, c in zip(A2.log[:-1], C.log[:-1]):
        assert a["index"] == c["index"] and a["data"] == c["data"] and (a["smooth"] == c["smooth"] or (a["smooth"] != a["smooth"] and c["smooth"] != c["smooth"]))
    final = dense(e, labC, 0, None, True)
    want = float(final.astype(np.float64).sum())
    assert abs(C.log[-1]["data"] - want) <= 1e-6 * max(1.0, abs(want)), (C.log[-1]["data"], want)
    changed = (labC != rawC).any(-1)
    assert changed.any()
    e.close()
    return abs(B.log[0]["data"] - A.log[-1]["data"])


# ------------------------------------------------------------------------------------------------ 7. errors, regions, threads
def case_errors(lib, H=30, W=41, D=6):
    imL = synth.make_guide(H, W, 1)
    vol = synth.make_volume(D, H, W, 3)
    e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=8, lib=lib)           # view 1 has no data
    bl, bcst = api.DeviceBuffer(e, H * W * 16), api.DeviceBuffer(e, H * W * 4)
    try:
        lab = planted_labels(H, W, D, 2)
        bl.upload(lab)
        bcst.upload(np.full((H, W), FILL, F32))

        def fails(*a, **k):
            try:
                e.unary_labels(*a, **k)
            except api.LesHipError as ex:
                assert "error -1" in str(ex) or "error 1" in str(ex) or "liblocalexp_hip error" in str(ex)
                assert len(e.L.les_hip_last_error()) > 0
                return True
            return False
        assert fails(bl.ptr, bcst.ptr, mode=1)                                    # view without data
        assert fails(bl.ptr, bcst.ptr, mode=2)
        for rg in ((-1, 0, 4, 4), (0, 0, W + 1, 2), (W - 2, 0, 3, 3), (0, H - 1, 2, 2), (0, 0, -1, 3)):
            assert fails(bl.ptr, bcst.ptr, region=rg), rg
        assert e.L.les_hip_unary_labels(e.h, 0, None, None, api.C.c_void_p(bcst.ptr), 1) != 0          # null pointers
        assert e.L.les_hip_unary_labels(e.h, 0, None, api.C.c_void_p(bl.ptr), None, 1) != 0
        assert e.L.les_hip_unary_labels(None, 0, None, api.C.c_void_p(bl.ptr), api.C.c_void_p(bcst.ptr), 1) != 0
        assert e.L.les_hip_unary_labels_kind(None, 0) == -1
        e.synchronize()
        assert np.all(bcst.download((H, W), F32) == FILL), "a refused call wrote"
        for rg in ((5, 5, 0, 3), (5, 5, 3, 0), (0, 0, 0, 0)):                       # empty regions: OK, nothing written
            e.unary_labels(bl.ptr, bcst.ptr, region=rg)
        e.synchronize()
        assert np.all(bcst.download((H, W), F32) == FILL), "an empty region wrote"
    finally:
        bl.free()
        bcst.free()
        e.close()


def case_two_threads(lib, device, H=40, W=52, D=8, windR=8):
    """Concurrent calls from two host threads with per-thread streams on one context: the single-thread result bit for bit."""
    import torch
    dev = torch.device(device)
    pr = pc.synth_pair(lib, H, W, D, windR=windR)
    try:
        labs = [torch.as_tensor(planted_labels(H, W, D, 20 + m)).to(dev) for m in (0, 1)]
        single = []
        for m in (0, 1):
            out = torch.full((H, W), float("nan"), dtype=torch.float32, device=dev)
            pr.e.unary_labels(labs[m].data_ptr(), out.data_ptr(), mode=m)
            pr.e.synchronize()
            single.append(out.cpu().numpy())
        outs = [torch.full((H, W), float("nan"), dtype=torch.float32, device=dev) for _ in (0, 1)]
        streams = [torch.cuda.Stream(dev) if dev.type == "cuda" else None for _ in (0, 1)]
        errs = []

        def work(m):
            try:
                pr.e.set_thread_stream(streams[m].cuda_stream if streams[m] is not None else 0, True)
                for _ in range(3):
                    pr.e.unary_labels(labs[m].data_ptr(), outs[m].data_ptr(), mode=m)
                pr.e.synchronize()
                pr.e.set_thread_stream(0, False)
            except Exception as ex:          # noqa: BLE001
                errs.append(ex)
        ths = [threading.Thread(target=work, args=(m,)) for m in (0, 1)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        for m in (0, 1):
            assert np.array_equal(outs[m].cpu().numpy().view(np.uint32), single[m].view(np.uint32)), f"view {m}: threaded result differs"
    finally:
        pr.close()
