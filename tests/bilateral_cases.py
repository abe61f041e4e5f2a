"""Cases of the bilateral ("BF" / "BL") and unfiltered ("") aggregation, shared by the simulator tests (-m "not gpu") and the MI355X
tests (-m gpu) in test_bilateral.py.  The library (`lib` = the HIP build on the GPU box, the CPU SIMT-simulator build of the same sources
in the build container) is compared with an fp64 numpy restatement of BilateralFilter::filter (LES/GuidedFilter.h:329-374) applied to the
oracle's raw cost.

Tolerance: |dev - ref| <= 1e-5 * sum w |raw| + 1e-6 per pixel; the written set and the 1e6 sentinels exact; "" bit for bit.
"""
import ctypes as C

import numpy as np

from localexpstereo_amd import api, synth
from oracle import oracle as om
from tests.util import load_cones_crop

RTOL_SUM = 1e-5
ATOL = 1e-6
SENT = np.float32(1e6)


# ------------------------------------------------------------------------------------------------ restatement
def bf_ref(guide, raw, R, sig2, rows=None):
    """fp64 BilateralFilter::filter on a sub-region: guide = I(filterRect) (h x w x 3, 0..255), raw = the cost patch (h x w).
    Returns (q, S) for the output rows `rows` (all by default): q = sum over the window clipped to the sub-region of
    exp(-|dI|_1 / sig2) raw, S = the same sum of w |raw| (the scale of the tolerance).  Vectorised over the window offsets."""
    G = np.asarray(guide, np.float64)
    P = np.asarray(raw, np.float64)
    h, w = P.shape
    rows = np.arange(h) if rows is None else np.asarray(rows)
    q = np.zeros((len(rows), w))
    S = np.zeros((len(rows), w))
    Gp = G[rows]
    for dy in range(-R, R + 1):
        ty = rows + dy
        ok = (ty >= 0) & (ty < h)
        if not ok.any():
            continue
        ro, rt = np.nonzero(ok)[0], ty[ok]
        for dx in range(-R, R + 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            if x0 >= x1:
                continue
            d = np.abs(G[rt, x0 + dx:x1 + dx] - Gp[ro, x0:x1]).sum(-1)
            wt = np.exp(-d / sig2)
            t = P[rt, x0 + dx:x1 + dx]
            q[ro, x0:x1] += wt * t
            S[ro, x0:x1] += wt * np.abs(t)
    return q, S


def bf_loop(guide, raw, R, sig2):
    """Literal per-pixel transcription of BilateralFilter::filter (LES/GuidedFilter.h:355-371): patch = window & filterDomain,
    w = exp(-channelSum(|I(patch) - I(y, x)|) / sig2), q = p(patch).dot(w)."""
    I = np.asarray(guide, np.float64)
    p = np.asarray(raw, np.float64)
    h, w = p.shape
    q = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            y0, y1, x0, x1 = max(y - R, 0), min(y + R + 1, h), max(x - R, 0), min(x + R + 1, w)
            wt = np.exp(-np.abs(I[y0:y1, x0:x1] - I[y, x]).sum(-1) / sig2)
            q[y, x] = float((p[y0:y1, x0:x1] * wt).sum())
    return q


# ------------------------------------------------------------------------------------------------ contexts
class BfPair:
    """Library context with a filter + the oracle's raw cost of the same energy (volume: Oracle.gather; image-based: the guided filter
    at radius 0, which is the identity -- checked by case_radius0_identity)."""

    def __init__(self, lib, imL, imR, volL=None, volR=None, windR=20, sig2=10.0, filter="BF", th_col=0.5, max_disp=None, naive=False):
        self.imL, self.imR = np.ascontiguousarray(imL, np.uint8), np.ascontiguousarray(imR, np.uint8)
        self.H, self.W = self.imL.shape[:2]
        self.R = windR if filter in ("BF", "BL") else 0
        self.sig2, self.filter, self.naive = float(sig2), filter, naive
        if naive:
            self.o = om.Oracle.naive(imL, imR, max_disp, windR=1)
            self.e = api.HipCostVolumeEnergy.naive(imL, imR, windR=windR, eps=sig2, max_disp=max_disp, lib=lib, filter=filter)
            self.D = int(max_disp) + 1
        else:
            self.o = om.Oracle(imL, imR, volL, volR, windR=20, th_col=th_col, max_disp=max_disp)
            self.e = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=windR, eps=sig2, th_col=th_col, max_disp=max_disp, lib=lib, filter=filter)
            self.D = volL.shape[0]

    def close(self):
        self.e.close()

    def raw(self, fr, plane, mode):
        if self.naive:
            x, y, w, h = fr
            return self.o.unary(fr, fr, plane, mode=mode, check=False)[y:y + h, x:x + w].copy()
        return self.o.gather(fr, plane, mode)

    def expected(self, fr, tr, plane, mode, check, out=None):
        """(map, S): the restatement's H x W output of one call (NaN outside the target) and its tolerance scale."""
        out = np.full((self.H, self.W), np.nan, np.float64) if out is None else out
        S = np.zeros((self.H, self.W))
        x, y, w, h = fr
        tx, ty, tw, th = tr
        if tw <= 0 or th <= 0:
            return out, S
        raw = self.raw(fr, plane, mode)
        im = self.imL if mode == 0 else self.imR
        sub = slice(ty - y, ty - y + th), slice(tx - x, tx - x + tw)
        if self.R == 0:
            q = raw.astype(np.float64)
            s = np.abs(q)
        else:
            q, s = bf_ref(im[y:y + h, x:x + w], raw, self.R, self.sig2, rows=np.arange(ty - y, ty - y + th))
            q, s = q[:, sub[1]], s[:, sub[1]]
            q = q.astype(np.float32).astype(np.float64)          # the reference stores the double sum as float
        if self.R == 0:
            q, s = q[sub], s[sub]
        if check:
            valid = self.o.valid_mask(tr, plane).astype(bool)
            q = np.where(valid, q, float(SENT))
        out[ty:ty + th, tx:tx + tw] = q
        S[ty:ty + th, tx:tx + tw] = s
        return out, S


def compare(got, ref, S, exact=False):
    """Written set, sentinels exact; values within 1e-5 sum w |raw| + 1e-6 (exact: bit for bit)."""
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "set of written pixels differs"
    m = ~np.isnan(ref)
    assert np.array_equal(got[m] == SENT, ref[m] == float(SENT)), "1e6 sentinels differ"
    v = m & (ref != float(SENT))
    if exact:
        assert np.array_equal(got[v].astype(np.float32).view(np.uint32), ref[v].astype(np.float32).view(np.uint32)), "unfiltered cost is not the raw cost bit for bit"
        return 0.0
    err = np.abs(got[v].astype(np.float64) - ref[v])
    bound = RTOL_SUM * S[v] + ATOL
    assert np.all(err <= bound), f"bilateral parity: worst err / bound {np.max(err / bound):.3f}, max abs err {err.max():.3e}"
    return float(np.max(err / bound)) if err.size else 0.0


def cones_bf(lib, naive=False, **kw):
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    if naive:
        return BfPair(lib, imL, imR, naive=True, max_disp=31.0, **kw)
    return BfPair(lib, imL, imR, synth.make_volume(16, H, W, 42), synth.make_volume(16, H, W, 43), **kw)


def synth_bf(lib, H, W, D, **kw):
    return BfPair(lib, synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235), synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43), **kw)


def random_planes(n, D, H, W, seed, slant=0.3):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = rng.uniform(-slant, slant, n)
    p[:, 1] = rng.uniform(-slant, slant, n)
    zc = rng.uniform(-2, D + 1, n)
    p[:, 2] = zc - p[:, 0] * rng.uniform(0, W, n) - p[:, 1] * rng.uniform(0, H, n)
    return p


# ------------------------------------------------------------------------------------------------ cases
def case_restatement_tiny():
    """The vectorised restatement equals the literal per-pixel loop of the reference (sub-region of 9 x 11, R = 3 and R = 0)."""
    rng = np.random.default_rng(5)
    I = rng.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    p = rng.uniform(-0.5, 2.0, (9, 11)).astype(np.float32)
    for R, sig2 in ((3, 10.0), (0, 1.0), (6, 100.0)):
        q, _ = bf_ref(I, p, R, sig2)
        assert np.allclose(q, bf_loop(I, p, R, sig2), rtol=1e-13, atol=1e-13)


def case_radius0_identity(lib):
    """The guided filter at radius 0 (windR = 1) is the identity on the oracle's volume energy: the image-based raw cost is taken from it."""
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    o = om.Oracle(imL, imR, synth.make_volume(16, H, W, 42), synth.make_volume(16, H, W, 43), windR=1, th_col=0.5)
    for fr, pl, mode in (((0, 0, W, H), (0.01, 0.02, 2.125, 0.0), 0), ((19, 22, 82, 74), (0.05, -0.03, 4.25, 0.0), 1)):
        x, y, w, h = fr
        got = o.unary(fr, fr, pl, mode=mode, check=False)[y:y + h, x:x + w]
        assert np.array_equal(got, o.gather(fr, pl, mode))


def single_calls(H, W, D):
    return [
        (0, (0, 0, 62, 62), (0, 0, 42, 42), (0.0, 0.0, 3.0, 0.0)),                    # filterRect clipped by the image corner
        (0, (19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 4.25, 0.0)),
        (1, (W - 62, H - 62, 62, 62), (W - 42, H - 42, 42, 42), (-0.11, 0.07, 9.5, 0.0)),
        (0, (0, 0, W, H), (0, 0, W, H), (0.01, 0.02, 2.125, 0.0)),                     # whole image
        (1, (30, 0, 90, 60), (50, 0, 50, 40), (0.3, 0.2, -20.0, 0.0)),                 # mostly invalid
        (1, (5, 5, 30, 30), (5, 5, 30, 30), (0.0, 0.0, 2.5, 0.0)),                     # target == filterRect: touches every border
        (0, (10, 12, 50, 40), (10, 30, 20, 22), (0.02, 0.0, 4.0, 0.0)),                # target on the left / bottom filterRect border
        (0, (40, 40, 41, 41), (60, 60, 1, 1), (0.02, 0.01, 5.0, 0.0)),                 # 1 x 1 target
        (1, (40, 40, 41, 41), (40, 40, 1, 1), (0.0, 0.01, 6.0, 0.0)),                  # 1 x 1 target in the filterRect corner
        (0, (10, 8, 80, 70), (30, 28, 40, 30), (float("nan"), 0.0, 1.0, 0.0)),         # NaN plane
    ]


def case_single_calls(pr, calls=None, scratch=True):
    """les_hip_unary_one (and les_hip_unary_one_scratch) for individual calls, both views, check 0 / 1."""
    worst = 0.0
    sc = pr.e.scratch() if scratch else None
    try:
        for mode, fr, tr, pl in (calls or single_calls(pr.H, pr.W, pr.D)):
            for check in (True, False):
                ref, S = pr.expected(fr, tr, pl, mode, check)
                got = pr.e.ComputeUnaryPotential(fr, tr, np.full((pr.H, pr.W), np.nan, np.float32), pl, mode=mode, check=check)
                worst = max(worst, compare(got, ref, S, exact=pr.R == 0))
                if sc is not None:
                    got = pr.e.ComputeUnaryPotentialScratch(sc, fr, tr, np.full((pr.H, pr.W), np.nan, np.float32), pl, mode=mode, check=check)
                    compare(got, ref, S, exact=pr.R == 0)
    finally:
        if sc is not None:
            pr.e.scratch_free(sc)
    return worst


def case_cell_batches(pr, units=(8, 25), mode=0, seed=3, windR=20):
    """One lock-step of a disjoint set of LayerManager cells per layer (les_hip_unary_batch: a prepared batch, out_slabs = 0)."""
    worst = 0.0
    for li, unit in enumerate(units):
        layer = om.Layer(pr.W, pr.H, windR, unit)
        for s in (0, len(layer.sets) - 1):
            cells = layer.sets[s]
            frs, trs = layer.filter[cells], layer.shared[cells]
            planes = random_planes(len(cells), pr.D, pr.H, pr.W, seed + 10 * li + s)
            for check in (True, False):
                ref, S = np.full((pr.H, pr.W), np.nan), np.zeros((pr.H, pr.W))
                for f, t, pl in zip(frs, trs, planes):
                    _, s_ = pr.expected(tuple(f), tuple(t), tuple(pl), mode, check, out=ref)
                    S = np.maximum(S, s_)
                got = pr.e.unary_batch(frs, trs, planes, mode=mode, check=check)
                worst = max(worst, compare(got, ref, S, exact=pr.R == 0))
    return worst


def run_batch(pr, frs, trs, planes, out_slabs, mode, check):
    """A prepared batch run into device memory (les_hip_batch_run), read back as [slabs][H][W]."""
    n = len(frs)
    nslab = 1 if out_slabs == 0 else (n + out_slabs - 1) // out_slabs
    b = api.Batch(pr.e, frs, trs, out_slabs=out_slabs)
    buf = api.DeviceBuffer(pr.e, nslab * pr.H * pr.W * 4)
    try:
        assert b.kernel_kind(mode) == 2
        buf.fill(0xFF)                        # NaN: unwritten
        b.run(planes, buf.ptr, mode=mode, check=check)
        pr.e.synchronize()
        return buf.download((nslab, pr.H, pr.W), np.float32)
    finally:
        buf.free()
        b.destroy()


def case_slot_batches(pr, unit=8, slots=5, mode=1, seed=7, windR=20):
    """out_slabs = k: the cells of a disjoint set times `slots` proposal slots in one launch (calls i and i + k share their rects: tiles
    of several planes), and out_slabs = 1: one slab per call."""
    layer = om.Layer(pr.W, pr.H, windR, unit)
    cells = layer.sets[0]
    k = len(cells)
    frs, trs = np.tile(layer.filter[cells], slots), np.tile(layer.shared[cells], slots)
    planes = random_planes(k * slots, pr.D, pr.H, pr.W, seed)
    planes[k + 1] = (np.nan, 0.0, 1.0, 0.0)
    worst = 0.0
    for out_slabs in (k, 1):
        for check in (True, False):
            got = run_batch(pr, frs, trs, planes, out_slabs, mode, check)
            for sl in range(got.shape[0]):
                ref, S = np.full((pr.H, pr.W), np.nan), np.zeros((pr.H, pr.W))
                for i in range(sl * out_slabs, min((sl + 1) * out_slabs, k * slots)):
                    _, s_ = pr.expected(tuple(frs[i]), tuple(trs[i]), tuple(planes[i]), mode, check, out=ref)
                    S = np.maximum(S, s_)
                worst = max(worst, compare(got[sl], ref, S, exact=pr.R == 0))
    return worst


def case_whole_image_slabs(pr, nplanes=5, mode=0, seed=11, rows=None):
    """One whole-image slab per plane (every call the same rects: tiles of up to four planes, then one), against the restatement on
    `rows` (all rows by default).  Returns the output for a repeatability check."""
    full = [(0, 0, pr.W, pr.H)] * nplanes
    planes = random_planes(nplanes, pr.D, pr.H, pr.W, seed, slant=0.05)
    got = run_batch(pr, full, full, planes, 1, mode, True)
    rows = np.arange(pr.H) if rows is None else np.asarray(rows)
    im = pr.imL if mode == 0 else pr.imR
    worst = 0.0
    for i in range(nplanes):
        raw = pr.raw((0, 0, pr.W, pr.H), tuple(planes[i]), mode)
        if pr.R == 0:
            q, S = raw[rows].astype(np.float64), np.abs(raw[rows].astype(np.float64))
        else:
            q, S = bf_ref(im, raw, pr.R, pr.sig2, rows=rows)
            q = q.astype(np.float32).astype(np.float64)
        valid = pr.o.valid_mask((0, 0, pr.W, pr.H), tuple(planes[i])).astype(bool)[rows]
        ref = np.where(valid, q, float(SENT))
        worst = max(worst, compare(got[i][rows], ref, S, exact=pr.R == 0))
    return got, worst


def case_errors(lib):
    """windR outside 0 .. 31 -> LES_HIP_ERR_UNSUPPORTED (3); sig2 <= 0 -> LES_HIP_ERR_ARG (1); unknown names refused in Python."""
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    vol = synth.make_volume(4, H, W, 42)
    for kw, code in ((dict(windR=32, eps=10.0), 3), (dict(windR=-1, eps=10.0), 1), (dict(windR=20, eps=0.0), 1), (dict(windR=20, eps=-1.0), 1)):
        try:
            api.HipCostVolumeEnergy(imL, imR, vol, vol, lib=lib, filter="BF", **kw)
        except api.LesHipError as ex:
            assert f"error {code}:" in str(ex), str(ex)
        else:
            raise AssertionError(f"{kw} was accepted")
        try:
            api.HipCostVolumeEnergy.naive(imL, imR, max_disp=31.0, lib=lib, filter="BL", **kw)
        except api.LesHipError as ex:
            assert f"error {code}:" in str(ex), str(ex)
        else:
            raise AssertionError(f"naive {kw} was accepted")
    for good in (dict(windR=31, eps=10.0), dict(windR=0, eps=1.0)):
        api.HipCostVolumeEnergy(imL, imR, vol, vol, lib=lib, filter="BF", **good).close()
    api.HipCostVolumeEnergy(imL, imR, vol, vol, lib=lib, filter="", windR=0, eps=0.0).close()
    for bad in ("GFfloat", "bf", None):
        try:
            api.HipCostVolumeEnergy(imL, imR, vol, vol, lib=lib, filter=bad)
        except ValueError:
            pass
        else:
            raise AssertionError(f"filter {bad!r} was accepted")


def case_gf_through_new_constructor(lib):
    """A guided-filter context made by les_hip_create_filtered(..., LES_HIP_FILTER_GF, ...) gives the bits of les_hip_create."""
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    vl, vr = synth.make_volume(16, H, W, 42), synth.make_volume(16, H, W, 43)
    a = api.HipCostVolumeEnergy(imL, imR, vl, vr, windR=20, eps=1e-4, th_col=0.5, lib=lib)
    b = api.HipCostVolumeEnergy.__new__(api.HipCostVolumeEnergy)
    b.L, b.H, b.W, b.D, b.params, b.filter, b.h = a.L, a.H, a.W, a.D, a.params, api.FILTER_GF, None
    h = C.c_void_p()
    b._chk(a.L.les_hip_create_filtered(C.byref(h), C.byref(a.params), api.FILTER_GF, api._ptr(a.imL), api._ptr(a.imR), api._ptr(np.ascontiguousarray(vl)),
                                       api._ptr(np.ascontiguousarray(vr))))
    b.h = h
    try:
        layer = om.Layer(W, H, 20, 8)
        cells = layer.sets[2]
        planes = random_planes(len(cells), 16, H, W, 21)
        for mode in (0, 1):
            ga = a.unary_batch(layer.filter[cells], layer.shared[cells], planes, mode=mode)
            gb = b.unary_batch(layer.filter[cells], layer.shared[cells], planes, mode=mode)
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
            fr, tr, pl = (19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 4.25, 0.0)
            ga = a.ComputeUnaryPotential(fr, tr, np.full((H, W), np.nan, np.float32), pl, mode=mode)
            gb = b.ComputeUnaryPotential(fr, tr, np.full((H, W), np.nan, np.float32), pl, mode=mode)
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
        ba = api.Batch(b, layer.filter[cells], layer.shared[cells])
        assert ba.kernel_kind(0) in (0, 1)
        ba.destroy()
    finally:
        a.close()
        b.close()
