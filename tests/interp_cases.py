"""setInterpolationMethod (LES/CostVolumeEnergy.h:45-48, :99-167) on the device: nearest-slice (0) and three-point quadratic (2) raw
costs, shared by the simulator tests (-m "not gpu") and the MI355X tests (-m gpu) of tests/test_interpolation.py.

The raw cost is restated in numpy f32 (gather_np) and checked bit for bit against a literal per-pixel loop written from the reference
(gather_loop).  The reference converts with (int) on a double; its platform (MSVC x86-64, cvttsd2si) returns INT_MIN for NaN, +-inf
and values outside [-2^31, 2^31), and cvt(t) + D0 wraps as int32.  The guided filter of a restated raw patch comes from the oracle's
own filter (Oracle.filter_subregion), the bilateral one from tests/bilateral_cases.py's restatement."""
import math

import numpy as np

from localexpstereo_amd import api, synth
from oracle import oracle as om
from tests import bilateral_cases as bc
from tests import parity_cases as pc
from tests.util import load_cones_crop

SENT = np.float32(1e6)
F32 = np.float32
INT_MIN = -(2 ** 31)


# ------------------------------------------------------------------------------------------------ restatements
def cvt_msvc(t):
    """(int) of a double as cvttsd2si computes it: truncation inside [-2^31, 2^31), INT_MIN elsewhere (NaN included)."""
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (t >= -2.0 ** 31) & (t < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, t, 0.0)), INT_MIN).astype(np.int64)


def wrap32(k):
    return ((np.asarray(k, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def gather_np(vol, fr, plane, interp, D0, th_col):
    """Raw cost min(C, th_col) of `plane` on filterRect fr = (x, y, w, h) at interpolation 0 or 2, f32 [h][w]."""
    x0, y0, w, h = fr
    D = vol.shape[0]
    a, b, c = F32(plane[0]), F32(plane[1]), F32(plane[2])
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    with np.errstate(all="ignore"):
        d_base = (b * ys.astype(F32) + c).astype(F32)                         # float d_base = b * y + c
        d = (a * xs.astype(F32)[None, :] + d_base[:, None]).astype(F32)       # float d = a * x + d_base
        k = wrap32(cvt_msvc(d.astype(np.float64) + 0.5) + int(D0))            # (int)(d + 0.5) + D0: the add in double
        e = np.broadcast_to(d_base[:, None], d.shape) if interp == 0 else d
        bad = np.isnan(e) | np.isinf(e)
        Y, X = np.meshgrid(ys, xs, indexing="ij")
        kc = np.clip(k, 0, D - 1)
        C = vol[kc, Y, X].astype(F32)
        if interp == 2:
            k1, k3 = np.maximum(kc - 1, 0), np.minimum(kc + 1, D - 1)
            y1, y2, y3 = vol[k1, Y, X], vol[kc, Y, X], vol[k3, Y, X]
            r1, r2, r3 = k1.astype(F32), kc.astype(F32), k3.astype(F32)
            A = y1 / (r1 - r2) / (r1 - r3)
            B = y2 / (r2 - r1) / (r2 - r3)
            Cq = y3 / (r3 - r1) / (r3 - r2)
            r = (A + B) + Cq
            p = -((A * (r2 + r3) + B * (r1 + r3)) + Cq * (r1 + r2))
            q = ((A * r2) * r3 + (B * r1) * r3) + (Cq * r1) * r2
            dd = d + F32(D0)
            Q = ((r * dd) * dd + p * dd) + q
            C = Q.astype(F32)
        C = np.where(k < 0, vol[0, Y, X], np.where(k >= D, vol[D - 1, Y, X], np.where(bad, SENT, C))).astype(F32)
        return np.where(F32(th_col) < C, F32(th_col), C).astype(F32)


def _cvt_scalar(t):
    if t != t or not (-2.0 ** 31 <= t < 2.0 ** 31):
        return INT_MIN
    return int(math.trunc(t))


def gather_loop(vol, fr, plane, interp, D0, th_col):
    """LES/CostVolumeEnergy.h:99-167 line by line, one pixel at a time with f32 scalars."""
    x0, y0, w, h = fr
    D = vol.shape[0]
    out = np.zeros((h, w), F32)
    a, b, c = F32(plane[0]), F32(plane[1]), F32(plane[2])
    th = F32(th_col)
    with np.errstate(all="ignore"):
        for y in range(y0, y0 + h):
            d_base = F32(b * F32(y) + c)
            for x in range(x0, x0 + w):
                if interp == 0:
                    dv = _cvt_scalar(float(F32(a * F32(x) + d_base)) + 0.5)
                    dv = int(wrap32(dv + D0))
                    if dv < 0:
                        C = vol[0, y, x]
                    elif dv >= D:
                        C = vol[D - 1, y, x]
                    elif math.isnan(d_base) or math.isinf(d_base):
                        C = SENT
                    else:
                        C = vol[dv, y, x]
                else:
                    d = F32(a * F32(x) + d_base)
                    d2 = int(wrap32(_cvt_scalar(float(d) + 0.5) + D0))
                    if d2 < 0:
                        C = vol[0, y, x]
                    elif d2 >= D:
                        C = vol[D - 1, y, x]
                    elif math.isnan(d) or math.isinf(d):
                        C = SENT
                    else:
                        d3 = min(d2 + 1, D - 1)
                        d1 = max(d2 - 1, 0)
                        y1, y2, y3 = vol[d1, y, x], vol[d2, y, x], vol[d3, y, x]
                        rd1, rd2, rd3 = F32(d1), F32(d2), F32(d3)
                        aa = F32(F32(y1 / F32(rd1 - rd2)) / F32(rd1 - rd3))
                        bb = F32(F32(y2 / F32(rd2 - rd1)) / F32(rd2 - rd3))
                        cc = F32(F32(y3 / F32(rd3 - rd1)) / F32(rd3 - rd2))
                        r = F32(F32(aa + bb) + cc)
                        p = F32(-F32(F32(F32(aa * F32(rd2 + rd3)) + F32(bb * F32(rd1 + rd3))) + F32(cc * F32(rd1 + rd2))))
                        q = F32(F32(F32(F32(aa * rd2) * rd3) + F32(F32(bb * rd1) * rd3)) + F32(F32(cc * rd1) * rd2))
                        d = F32(d + F32(D0))
                        C = F32(F32(F32(F32(r * d) * d) + F32(p * d)) + q)
                out[y - y0, x - x0] = th if th < C else C          # std::min(C, th_col)
    return out


def same_bits(a, b):
    """Equal as f32 bit patterns, except that every NaN equals every NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


# ------------------------------------------------------------------------------------------------ planes
def special_planes(D, D0, H, W):
    """(a, b, c) planes named by what they exercise (the 4th component is unused by the gather)."""
    ulp_below = float(np.nextafter(F32(0.5), F32(0)))
    P = []
    for d in (0.0, 1.0, 2.0, float(D - 1 - D0), 0.5, 1.5, -0.5, ulp_below, -ulp_below, -1.0, -0.75, -1.49, float(D) - D0 - 0.5):
        P.append((0.0, 0.0, d))                                      # fronto-parallel: integer, half-integer, +-(0.5 - ulp), (-1.5, -0.5]
    P += [(0.9, -0.4, 1.0), (-1.7, 0.3, float(D)), (0.25, 0.25, -3.0)]                  # steep planes
    P += [(0.0, 0.0, float(-D0)), (0.0, 0.0, float(D - 1 - D0)), (0.01, 0.0, float(-D0) - 0.2)]  # slices 0 and D - 1 (mode 2: NaN)
    P += [(float("nan"), 0.0, 1.0), (0.0, float("nan"), 1.0), (0.0, 0.0, float("inf")), (0.0, 0.0, -float("inf")),
          (float("inf"), 0.0, 0.0), (0.0, 0.0, 3e9), (0.0, 0.0, -3e9), (0.0, 0.0, 2.0 ** 31), (0.0, 0.0, -2.0 ** 31 - D0 + 0.0),
          (1e9, 0.0, 0.0)]                                                               # NaN, +-inf, |d| >= 2^31
    return [(F32(a), F32(b), F32(c), F32(0.0)) for a, b, c in P]


# ------------------------------------------------------------------------------------------------ cases
def case_restatement_matches_loop():
    """gather_np == gather_loop bit for bit on small scenes, every special plane and random ones, both modes, D 1 / 2 / 5, D0 0 / 3."""
    rng = np.random.default_rng(5)
    for D in (1, 2, 5):
        for D0 in (0, 3):
            vol = rng.uniform(0.0, 1.0, (D, 6, 9)).astype(F32)
            vol[:, 2, 3] = rng.uniform(0.0, 1.0, D).astype(F32) * 40.0     # a pixel above th_col
            planes = special_planes(D, D0, 6, 9) + [tuple(p) for p in pc.random_planes(6, D, 6, 9, 7 + D)]
            for pl in planes:
                for interp in (0, 2):
                    for fr in ((0, 0, 9, 6), (2, 1, 5, 4)):
                        got, ref = gather_np(vol, fr, pl, interp, D0, 0.6), gather_loop(vol, fr, pl, interp, D0, 0.6)
                        assert same_bits(got, ref), (D, D0, pl, interp, fr)


class InterpPair:
    """A library context of filter `filter` at interpolation `interp` plus the oracle (its guided filter, validity) over the same scene."""

    def __init__(self, lib, imL, imR, volL, volR, interp, windR=20, eps=1e-4, th_col=0.5, min_disp=0.0, filter="GF", sig2=10.0):
        self.imL, self.imR = imL, imR
        self.vol = (np.ascontiguousarray(volL, F32), np.ascontiguousarray(volR, F32))
        self.D, self.H, self.W = self.vol[0].shape
        self.D0 = int(-min_disp)
        self.th_col, self.interp, self.filter = th_col, interp, filter
        max_disp = float(self.D - 1 + min_disp)
        self.o = om.Oracle(imL, imR, volL, volR, windR=windR, eps=eps, th_col=th_col, max_disp=max_disp, min_disp=min_disp)
        self.R = windR if filter in ("BF", "BL") else 0
        self.sig2 = sig2
        self.e = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=windR, eps=sig2 if filter in ("BF", "BL") else eps, th_col=th_col,
                                         max_disp=max_disp, min_disp=min_disp, lib=lib, filter=filter, interpolate=interp)

    def close(self):
        self.e.close()

    def raw(self, fr, plane, mode):
        return gather_np(self.vol[mode], tuple(int(v) for v in fr), plane, self.interp, self.D0, self.th_col)

    def expected(self, fr, tr, plane, mode, check, out):
        """Writes the expected output of one call into `out` (H x W float64, target rect only); returns the tolerance scale map."""
        x, y, w, h = (int(v) for v in fr)
        tx, ty, tw, th = (int(v) for v in tr)
        S = np.zeros((self.H, self.W))
        if tw <= 0 or th <= 0:
            return S
        raw = self.raw(fr, plane, mode)
        sub = slice(ty - y, ty - y + th), slice(tx - x, tx - x + tw)
        if self.filter == "GF":
            q = self.o.filter_subregion((x, y, w, h), raw, mode)[sub].astype(np.float64)
            s = np.abs(q)
        elif self.R == 0:
            q = raw[sub].astype(np.float64)
            s = np.abs(q)
        else:
            im = self.imL if mode == 0 else self.imR
            q, s = bc.bf_ref(im[y:y + h, x:x + w], raw, self.R, self.sig2, rows=np.arange(ty - y, ty - y + th))
            q, s = q[:, sub[1]].astype(np.float32).astype(np.float64), s[:, sub[1]]
        if check:
            q = np.where(self.o.valid_mask((tx, ty, tw, th), tuple(plane)).astype(bool), q, float(SENT))
        out[ty:ty + th, tx:tx + tw] = q
        S[ty:ty + th, tx:tx + tw] = s
        return S


def compare(pr, got, ref, S, written):
    """got vs ref on the written pixels: NaN sets equal, 1e6 sentinels equal, finite values within the filter's tolerance (bit for bit
    for the unfiltered energy).  Returns the largest absolute error."""
    got, ref = np.asarray(got)[written], np.asarray(ref)[written]
    S = S[written]
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"NaN outputs differ at {int((gn != rn).sum())} of {got.size} pixels"
    v = ~rn
    assert np.array_equal(got[v] == SENT, ref[v] == float(SENT)), "1e6 sentinels differ"
    v &= ref != float(SENT)
    if not v.any():
        return 0.0
    if pr.filter == "":
        assert np.array_equal(got[v].astype(F32).view(np.uint32), ref[v].astype(F32).view(np.uint32)), "raw cost not bit for bit"
        return 0.0
    err = np.abs(got[v].astype(np.float64) - ref[v])
    if pr.filter == "GF":
        assert np.all(err <= pc.RTOL * np.abs(ref[v]) + pc.ATOL), f"parity: max abs err {err.max():.3e}"
    else:
        bound = bc.RTOL_SUM * S[v] + bc.ATOL
        assert np.all(err <= bound), f"bilateral parity: worst err / bound {np.max(err / bound):.3f}"
    return float(err.max())


FILL = np.float32(-7.25)      # what an unwritten pixel holds (NaN is a legitimate output here)


def run_calls(pr, calls, check, scratch=None):
    """Single calls (les_hip_unary_one, and les_hip_unary_one_scratch when `scratch`) against the restatement."""
    worst = 0.0
    for mode, fr, tr, pl in calls:
        ref = np.full((pr.H, pr.W), np.nan)
        S = pr.expected(fr, tr, pl, mode, check, ref)
        written = np.zeros((pr.H, pr.W), bool)
        written[tr[1]:tr[1] + tr[3], tr[0]:tr[0] + tr[2]] = True
        outs = [pr.e.ComputeUnaryPotential(fr, tr, np.full((pr.H, pr.W), FILL, F32), pl, mode=mode, check=check)]
        if scratch is not None:
            outs.append(pr.e.ComputeUnaryPotentialScratch(scratch, fr, tr, np.full((pr.H, pr.W), FILL, F32), pl, mode=mode, check=check))
        for got in outs:
            assert np.all(got[~written] == FILL), "pixels outside the target were written"
            worst = max(worst, compare(pr, got, ref, S, written))
    return worst


def run_batch(pr, frs, trs, planes, mode, check, out_slabs=0, kind=None):
    """One prepared batch (les_hip_batch_run) into device memory, [slabs][H][W]; kind: the les_hip_batch_kernel_kind expected."""
    n = len(frs)
    nslab = 1 if out_slabs == 0 else n // out_slabs
    b = api.Batch(pr.e, frs, trs, out_slabs=out_slabs)
    buf = api.DeviceBuffer(pr.e, nslab * pr.H * pr.W * 4)
    try:
        if kind is not None:
            assert b.kernel_kind(mode) == kind, (b.kernel_kind(mode), kind)
        buf.fill(0xFF)
        b.run(planes, buf.ptr, mode=mode, check=check)
        pr.e.synchronize()
        return buf.download((nslab, pr.H, pr.W), F32)
    finally:
        buf.free()
        b.destroy()


def expected_batch(pr, frs, trs, planes, mode, check, out_slabs=0):
    nslab = 1 if out_slabs == 0 else len(frs) // out_slabs
    ref, S = np.full((nslab, pr.H, pr.W), np.nan), np.zeros((nslab, pr.H, pr.W))
    for i, (f, t, pl) in enumerate(zip(frs, trs, planes)):
        sl = 0 if out_slabs == 0 else i // out_slabs
        S[sl] = np.maximum(S[sl], pr.expected(tuple(f), tuple(t), tuple(pl), mode, check, ref[sl]))
    written = np.zeros(ref.shape, bool)
    for i, t in enumerate(trs):
        sl = 0 if out_slabs == 0 else i // out_slabs
        written[sl, t[1]:t[1] + t[3], t[0]:t[0] + t[2]] = True
    return ref, S, written


def check_batch(pr, frs, trs, planes, mode, check, out_slabs=0, kind=None):
    got = run_batch(pr, frs, trs, planes, mode, check, out_slabs, kind)
    ref, S, written = expected_batch(pr, frs, trs, planes, mode, check, out_slabs)
    worst = 0.0
    for sl in range(got.shape[0]):
        worst = max(worst, compare(pr, got[sl], ref[sl], S[sl], written[sl]))
    return got, worst


def synth_scene(H, W, D, seed=42):
    return synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235), synth.make_volume(D, H, W, seed), synth.make_volume(D, H, W, seed + 1)


def case_unfiltered_exact(lib, interp, D, min_disp, H=22, W=37):
    """"" context: the device raw cost equals the restatement bit for bit (NaN positions included), single calls and one batch, both views,
    check 0 / 1, every special plane."""
    imL, imR, vL, vR = synth_scene(H, W, D)
    pr = InterpPair(lib, imL, imR, vL, vR, interp, windR=0, min_disp=min_disp, filter="")
    try:
        planes = special_planes(D, pr.D0, H, W)
        fr, tr = (2, 1, W - 5, H - 3), (4, 3, W - 10, H - 7)
        for check in (False, True):
            calls = [(m, fr, tr, pl) for m in (0, 1) for pl in planes]
            run_calls(pr, calls, check)
            for m in (0, 1):
                check_batch(pr, [fr] * len(planes), [tr] * len(planes), planes, m, check, out_slabs=1, kind=2)
    finally:
        pr.close()


def cones_interp(lib, interp, filter="GF", D=16, **kw):
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    return InterpPair(lib, imL, imR, synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43), interp, filter=filter, **kw)


def gf_single_calls(H, W, D):
    return [
        (0, (0, 0, 62, 62), (0, 0, 42, 42), (0.0, 0.0, 3.0, 0.0)),
        (0, (19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 4.25, 0.0)),
        (1, (W - 62, H - 62, 62, 62), (W - 42, H - 42, 42, 42), (-0.11, 0.07, 9.5, 0.0)),
        (1, (30, 0, 90, 60), (50, 0, 50, 40), (0.3, 0.2, -20.0, 0.0)),                  # mostly clamped to slice 0
        (0, (10, 12, 50, 40), (10, 30, 20, 22), (0.02, 0.0, 4.0, 0.0)),                 # tight rects: strip kernel
        (1, (5, 5, 60, 50), (25, 25, 20, 10), (0.0, 0.0, float(D - 1), 0.0)),            # slice D - 1 (mode 2: all NaN)
        (0, (10, 8, 80, 70), (30, 28, 40, 30), (float("nan"), 0.0, 1.0, 0.0)),
    ]


def case_gf_single_calls(pr, scratch=True):
    H, W, D = pr.H, pr.W, pr.D
    sc = pr.e.scratch() if scratch else None
    try:
        for check in (True, False):
            run_calls(pr, gf_single_calls(H, W, D), check, scratch=sc)
    finally:
        if sc is not None:
            pr.e.scratch_free(sc)


def case_cell_batches(pr, units=(8, 25), mode=0, seed=3, windR=20, kind=None):
    """One lock-step of a disjoint set of LayerManager cells per layer; kind: the kernel kind every batch must report."""
    for li, unit in enumerate(units):
        layer = om.Layer(pr.W, pr.H, windR, unit)
        for s in (0, len(layer.sets) - 1):
            cells = layer.sets[s]
            frs, trs = layer.filter[cells], layer.shared[cells]
            planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, seed + 10 * li + s)
            for check in (True, False):
                check_batch(pr, frs, trs, planes, mode, check, kind=kind)


def case_slabs(pr, nplanes=4, mode=0, seed=11, kind=None):
    full = [(0, 0, pr.W, pr.H)] * nplanes
    planes = pc.random_planes(nplanes, pr.D, pr.H, pr.W, seed, slant=0.05)
    planes[-1] = (0.0, 0.0, 0.0, 0.0)                      # fronto-parallel on slice 0 (mode 2: NaN everywhere)
    return check_batch(pr, full, full, planes, mode, True, out_slabs=1, kind=kind)[0]


def interior_nan_volume(H, W, D, seed=42):
    """A volume whose slice 3 holds one NaN in the image interior: a fronto-parallel plane at d = 3 reads it at one pixel."""
    v = synth.make_volume(D, H, W, seed)
    v[3, H // 2, W // 2] = np.nan
    return v


def case_interior_nan(lib, interp, filter="GF", H=60, W=70, D=8):
    """One NaN inside a filterRect: the filtered output is NaN exactly where the reference's filter spreads it."""
    imL, imR = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    vL = interior_nan_volume(H, W, D)
    pr = InterpPair(lib, imL, imR, vL, vL.copy(), interp, filter=filter, windR=10 if filter == "GF" else 3)
    try:
        pl = (F32(0.0), F32(0.0), F32(3.0), F32(0.0))
        calls = [(0, (0, 0, W, H), (0, 0, W, H), pl), (1, (5, 4, 55, 50), (15, 14, 35, 30), pl)]
        for check in (False, True):
            run_calls(pr, calls, check)
    finally:
        pr.close()


def case_routing(pr, mode=0, seed=5):
    """Interpolation 0 runs the march kernel wherever interpolation 1 does; interpolation 2 too (its flagged calls on the strip kernel).
    A batch that mixes clean calls with calls on slice 0 / D - 1 (NaN raw costs: flagged) gives the restatement everywhere."""
    layer = om.Layer(pr.W, pr.H, 20, 14)
    cells = layer.sets[5]
    frs, trs = layer.filter[cells], layer.shared[cells]
    planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, seed, slant=0.02)
    planes[:, 2] = np.clip(planes[:, 2], 2.0, pr.D - 3.0)
    planes[::3] = (0.0, 0.0, 0.0, 0.0)                     # slice 0
    planes[1::5] = (0.0, 0.0, float(pr.D - 1), 0.0)        # slice D - 1
    interp = pr.e.interpolate
    pr.e.setInterpolationMethod(1)
    b = api.Batch(pr.e, frs, trs)
    kind1 = b.kernel_kind(mode)
    b.destroy()
    pr.e.setInterpolationMethod(interp)
    assert kind1 == 1, "the scene must put LayerManager cells on the march kernel"
    check_batch(pr, frs, trs, planes, mode, True, kind=kind1)
    check_batch(pr, frs, trs, planes, mode, False, kind=kind1)


def case_mode_switching(pr, mode=1, seed=9):
    """A batch created at interpolation 1, run at 0, 2 and 1 again: the last run equals the first bit for bit; each run equals the run of a
    fresh context at that interpolation.  The setting survives refresh_volume; bad values give LES_HIP_ERR_ARG."""
    layer = om.Layer(pr.W, pr.H, 20, 25)
    cells = layer.sets[0]
    frs, trs = layer.filter[cells], layer.shared[cells]
    planes = pc.random_planes(len(cells), pr.D, pr.H, pr.W, seed)
    n = len(frs)
    pr.e.setInterpolationMethod(1)
    b = api.Batch(pr.e, frs, trs)
    buf = api.DeviceBuffer(pr.e, pr.H * pr.W * 4)
    outs = {}
    try:
        for k, m in enumerate((1, 0, 2, 1)):
            pr.e.setInterpolationMethod(m)
            buf.fill(0xFF)
            b.run(planes, buf.ptr, mode=mode, check=True)
            pr.e.synchronize()
            outs[k] = buf.download((pr.H, pr.W), F32)
    finally:
        buf.free()
        b.destroy()
    assert same_bits(outs[0], outs[3]), "back at interpolation 1 the batch does not give what it gave before"
    assert not same_bits(outs[0], outs[1]) and not same_bits(outs[0], outs[2]), "the setting did not reach the prepared batch"
    for k, m in ((1, 0), (2, 2)):
        pr.e.setInterpolationMethod(m)
        fresh = pr.e.unary_batch(frs, trs, planes, mode=mode, check=True)
        w = np.zeros((pr.H, pr.W), bool)
        for t in trs:
            w[t[1]:t[1] + t[3], t[0]:t[0] + t[2]] = True
        assert same_bits(outs[k][w], fresh[w]), f"interpolation {m}: the old batch and a new one differ"
    for bad in (-1, 3, 7):
        rc = pr.e.L.les_hip_set_interpolation(pr.e.h, bad)
        assert rc == 1, f"interpolation {bad}: rc {rc}"
    pr.e.setInterpolationMethod(pr.interp)
    return n


def case_refresh_keeps_setting(lib, device, interp=2, H=60, W=80, D=8):
    """A volumes_on_device context: the setting survives les_hip_refresh_volume (same volume refilled: same output)."""
    import torch
    imL, imR, vL, vR = synth_scene(H, W, D)
    tl, tr_ = torch.from_numpy(vL).to(device), torch.from_numpy(vR).to(device)
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr_.data_ptr(), windR=10, th_col=0.5, max_disp=D - 1.0, device=tl.device.index or 0,
                                volumes_on_device=True, shape=(D, H, W), lib=lib, interpolate=interp)
    o = om.Oracle(imL, imR, vL, vR, windR=10, th_col=0.5, max_disp=D - 1.0)
    try:
        fr = tr = (0, 0, W, H)
        pl = (F32(0.01), F32(-0.02), F32(3.3), F32(0.0))
        before = e.ComputeUnaryPotential(fr, tr, np.zeros((H, W), F32), pl, mode=0, check=False)
        torch.cuda.synchronize()
        tl.copy_(torch.from_numpy(vL).to(device))
        torch.cuda.synchronize()
        e.refresh_volume(0)
        after = e.ComputeUnaryPotential(fr, tr, np.zeros((H, W), F32), pl, mode=0, check=False)
        assert same_bits(before, after)
        ref = o.filter_subregion(fr, gather_np(vL, fr, pl, interp, 0, 0.5), 0)
        assert np.all(np.abs(after - ref) <= pc.RTOL * np.abs(ref) + pc.ATOL)
    finally:
        e.close()


def case_naive_refuses(lib):
    imL, imR = load_cones_crop()
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=20, max_disp=31.0, lib=lib)
    try:
        for m in (0, 1, 2):
            assert e.L.les_hip_set_interpolation(e.h, m) == 1
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ one call, three entry points
# The per-call operator (les_hip_unary_one_scratch, les_hip_unary_one) and a one-call prepared batch (les_hip_batch_run) route the same
# call through the same kernels: their target rects agree bit for bit, NaN sets included.
PATH_CONTEXTS = [f"gf{windR}_interp{i}" for windR in (20, 30) for i in (0, 1, 2)] + [f"gf_nan_interp{i}" for i in (0, 1, 2)] + \
                ["naive_gf20", "naive_gf30"] + [f"{f}_interp{i}" for f in ("bf", "none") for i in (0, 1, 2)] + ["naive_bf", "naive_none"]


def path_context(lib, name):
    """(energy, calls) of one context kind of PATH_CONTEXTS; calls: (filterRect, targetRect, plane), each run in both views."""
    from tests import vdisp_cases as vc
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    D = 16
    if name.startswith("naive"):
        filt, windR = {"naive_gf20": ("GF", 20), "naive_gf30": ("GF", 30), "naive_bf": ("BF", 5), "naive_none": ("", 0)}[name]
        e = api.HipCostVolumeEnergy.naive(imL, imR, windR=windR, eps=10.0 if filt == "BF" else 1e-4, max_disp=31.0, lib=lib, filter=filt)
        return e, [(fr, tr, pl) for _, fr, tr, pl in vc.mixed_calls(H, W)]
    interp = int(name[-1])
    if name.startswith("gf_nan"):
        # an interior NaN in view 0 only: view 0 runs the strip kernel (+ the NaN spread at 0 / 2), view 1 the march kernel
        e = api.HipCostVolumeEnergy(imL, imR, interior_nan_volume(H, W, D), synth.make_volume(D, H, W, 43), windR=20, max_disp=D - 1.0, lib=lib,
                                    interpolate=interp)
        pl = (0.0, 0.0, 3.0, 0.0)
        return e, [((0, 0, W, H), (0, 0, W, H), pl), ((19, 22, 82, 74), (39, 42, 42, 34), pl), ((5, 4, 55, 50), (15, 14, 35, 30), pl)]
    filt, windR = {"gf20": ("GF", 20), "gf30": ("GF", 30), "bf": ("BF", 5), "none": ("", 0)}[name.split("_")[0]]
    e = api.HipCostVolumeEnergy(imL, imR, synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43), windR=windR,
                                eps=10.0 if filt == "BF" else 1e-4, max_disp=D - 1.0, lib=lib, filter=filt, interpolate=interp)
    calls = [(fr, tr, pl) for _, fr, tr, pl in gf_single_calls(H, W, D)]
    calls += [((19, 22, 82, 74), (39, 42, 42, 34), (0.0, 0.0, 0.0, 0.0)), ((19, 22, 82, 74), (39, 42, 42, 34), (0.01, 0.0, float(D - 1), 0.0))]
    return e, calls


def one_call_three_ways(e, sc, fr, tr, pl, mode, check):
    """The target rect of one call through les_hip_unary_one_scratch, les_hip_unary_one and a one-call prepared batch; asserts that
    the three agree bit for bit and returns the first."""
    H, W = e.H, e.W
    x, y, w, h = tr
    sub = (slice(y, y + h), slice(x, x + w))
    outs = [e.ComputeUnaryPotentialScratch(sc, fr, tr, np.full((H, W), FILL, F32), pl, mode=mode, check=check)[sub],
            e.ComputeUnaryPotential(fr, tr, np.full((H, W), FILL, F32), pl, mode=mode, check=check)[sub]]
    b = api.Batch(e, [fr], [tr])
    buf = api.DeviceBuffer(e, H * W * 4)
    try:
        buf.fill(0xFF)
        b.run([pl], buf.ptr, mode=mode, check=check)
        e.synchronize()
        outs.append(buf.download((H, W), F32)[sub])
    finally:
        buf.free()
        b.destroy()
    for name, o in zip(("les_hip_unary_one", "one-call batch"), outs[1:]):
        assert same_bits(outs[0], o), f"les_hip_unary_one_scratch and {name} differ: {fr} {tr} {pl} mode {mode} check {check}"
    return outs[0]


def case_one_call_paths_agree(lib, name):
    """Every call of the context kind `name`, both views, check 0 / 1, through one scratch (its cached rect pairs are revisited with
    the other view and the other check)."""
    e, calls = path_context(lib, name)
    sc = e.scratch()
    try:
        for check in (True, False):
            for fr, tr, pl in calls:
                for mode in (0, 1):
                    one_call_three_ways(e, sc, fr, tr, pl, mode, check)
    finally:
        e.scratch_free(sc)
        e.close()


def case_scratch_cache(lib):
    """One scratch through more than 16 rect pairs and back to the first (eviction); a cached pair after a change of interpolation; a
    bilateral scratch alternating between two rect pairs."""
    imL, imR = load_cones_crop()
    H, W = imL.shape[:2]
    D = 16
    pl = (0.02, -0.01, 6.5, 0.0)
    e = api.HipCostVolumeEnergy(imL, imR, synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43), windR=20, max_disp=D - 1.0, lib=lib)
    sc = e.scratch()
    try:
        pairs = [((x, y, 44, 44), (x + 2 * (k % 3), y + 3, 20, 18)) for k, (y, x) in enumerate((y, x) for y in (0, 20, 40) for x in (0, 12, 24, 36, 48, 60))]
        assert len(set(pairs)) > 16
        first = [one_call_three_ways(e, sc, fr, tr, pl, 0, True) for fr, tr in pairs]
        again = one_call_three_ways(e, sc, pairs[0][0], pairs[0][1], pl, 0, True)
        assert same_bits(first[0], again), "the first rect pair gives other bits after its eviction"
        fr, tr = (19, 22, 82, 74), (39, 42, 42, 34)
        outs = []
        for interp in (1, 0, 2, 1):
            e.setInterpolationMethod(interp)
            outs.append(one_call_three_ways(e, sc, fr, tr, pl, 1, True))
        assert same_bits(outs[0], outs[3]) and not same_bits(outs[0], outs[1]), "the cached pair does not follow the interpolation"
    finally:
        e.scratch_free(sc)
        e.close()
    e = api.HipCostVolumeEnergy(imL, imR, synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43), windR=5, eps=10.0, max_disp=D - 1.0,
                                lib=lib, filter="BF")
    sc = e.scratch()
    try:
        pairs = [((0, 0, 60, 50), (10, 10, 30, 25)), ((40, 30, 70, 60), (50, 45, 40, 30))]
        outs = [one_call_three_ways(e, sc, fr, tr, pl, k % 2, True) for k in range(3) for fr, tr in pairs]
        assert same_bits(outs[0], outs[4]) and same_bits(outs[1], outs[5]), "a bilateral rect pair gives other bits on its second visit"
    finally:
        e.scratch_free(sc)
        e.close()
