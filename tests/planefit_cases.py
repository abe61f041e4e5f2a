"""Cases of tests/test_planefit.py: slanted planes fitted to a disparity map (csrc/les_planefit.h: les_hip_fit_planes; api.HipCostVolumeEnergy.fit_planes;
stereo.FastGCStereo.fit_planes, run(labeling="wta+planes" / a disparity map), wta(slanted=True)) on the CPU simulator build and on the MI355X.

The definition, restated from csrc/les_planefit.h.  I: the view's 8-bit image; d: H x W disparities -- of a label map (a, b, c, v): d = (a x + b y) + c
rounded to f32 after every operation, v the label's; of a disparity map: the map, v = 0.  wtab[k] = f32(exp(-k / sig)), k = 0 .. 765 (sig = 0: ones).
For the target p = (x, y), d0 = d(p):
    d0 not finite: the fallback's label ((0, 0, mind, 0) without a fallback map), kind 0.
    taps s = p + (dx, dy), |dx|, |dy| <= r, inside the image, dy outer, dx inner, ascending; taken iff d(s) is finite and, in f32,
        |d(s) - d0| <= gate0 + gate_slope * max(|dx|, |dy|);  w = wtab[|I(p) - I(s)|_1], delta = f32(d(s) - d0); in f64, every operation rounded:
        S += w, Sx += w dx, Sy += w dy, Sxx += (w dx) dx, Sxy += (w dx) dy, Syy += (w dy) dy, Sd += w delta, Sxd += (w delta) dx, Syd += (w delta) dy, n += 1
    C00 = Syy S - Sy Sy, C01 = Sx Sy - Sxy S, C02 = Sxy Sy - Syy Sx, C11 = Sxx S - Sx Sx, C12 = Sxy Sx - Sxx Sy, C22 = Sxx Syy - Sxy Sxy
    det = (Sxx C00 + Sxy C01) + Sx C02;  a = ((C00 Sxd + C01 Syd) + C02 Sd) / det, b = ((C01 Sxd + C11 Syd) + C12 Sd) / det, c' = ((C02 Sxd + C12 Syd) + C22 Sd) / det
    accepted iff n >= min_support, det > 1e-3 ((S S) S), |c'| <= gate0, af = f32(a) and bf = f32(b) finite with |af|, |bf| <= max_slope,
        cf = f32((d0 + c') - (af x + bf y)) (in f64) finite, and (af, bf, cf, 0) is a valid label at p (IsValiLabel, LES/StereoEnergy.h:560-610)
    accepted: (af, bf, cf, v), kind 2; else if mind <= d0 <= maxd: (0, 0, d0, v), kind 1; else the fallback's label, kind 0.

References, none of them the code under test: the vectorised numpy restatement below (one array operation per tap, in tap order; a tap that is not
taken adds +0.0, which changes no bit of a sum that is never -0), itself held to a literal per-pixel loop.  Tolerances: labels and kind are compared
byte for byte everywhere; the energies of the driver case by <=, as a fusion move never raises the energy.

The mixed map (population test) is fitted with max_slope = 0.45: with the default gate (1, 0.5) no window can hold a slope above 1.5, so the default
max_slope = 2 can refuse nothing."""
import functools
import math

import numpy as np

from localexpstereo_amd import api
from tests import crossview_cases as cv
from tests import eval_cases as ec

F, D = np.float32, np.float64
SHAPES = ((5, 7), (1, 40), (33, 70), (19, 77))      # (H, W): below the window at every radius, one partial tile; only collinear support; several tiles;
                                                    # 3 x 2 tiles of 8 x 32, a multiple in neither direction
RADII = (1, 5, 15)
MIND, MAXD = 0.0, 63.0
DEFAULTS = dict(api.FIT_DEFAULTS)
MIXED = dict(DEFAULTS, max_slope=0.45)


def params_of(**kw):
    q = dict(DEFAULTS, **kw)
    assert set(q) == set(DEFAULTS)
    return q


def weight_table(sig):
    if sig == 0:
        return np.ones(766, F)
    return np.array([math.exp(-k / float(F(sig))) for k in range(766)], D).astype(F)


def disparities_of(labels):
    H, W = labels.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        return ((labels[..., 0] * xs.astype(F) + labels[..., 1] * ys.astype(F)) + labels[..., 2]).astype(F)


def label_valid(a, b, c, xs, ys, mind, maxd):
    """label_valid of csrc/les_kernels.h with v = 0, f32 in its order."""
    with np.errstate(all="ignore"):
        ds = ((xs.astype(F) * a + ys.astype(F) * b) + F(1) * c) + F(0) * F(0)
        a5, b5 = a * F(5), b * F(5)
        ok = (ds >= mind) & (ds <= maxd)
        for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            d = (ds + a5 if sa > 0 else ds - a5)
            d = (d + b5 if sb > 0 else d - b5)
            ok &= (d >= mind) & (d <= maxd)
    return ok


# ------------------------------------------------------------------------------------------------ restatement, numpy
def fit_restate(img, src, fallback=None, mind=MIND, maxd=MAXD, **params):
    """src: H x W x 4 labels or H x W disparities -> (out H x W x 4, kind H x W u8, info: boolean maps of what happened at each target)"""
    q = params_of(**params)
    r, ms = int(q["radius"]), int(q["min_support"])
    g0, gs, smax = F(q["gate0"]), F(q["gate_slope"]), F(q["max_slope"])
    mind, maxd = F(mind), F(maxd)
    if src.ndim == 3:
        d, v = disparities_of(src), src[..., 3].copy()
    else:
        d, v = src.astype(F), np.zeros(src.shape, F)
    H, W = d.shape
    tab = weight_table(q["sig"]).astype(D)
    dp = np.full((H + 2 * r, W + 2 * r), np.nan, F)
    dp[r:r + H, r:r + W] = d
    ip = np.zeros((H + 2 * r, W + 2 * r, 3), np.int32)
    ip[r:r + H, r:r + W] = img
    ic = img.astype(np.int32)
    fin0 = np.isfinite(d)
    n = np.zeros((H, W), np.int64)
    S, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd = (np.zeros((H, W), D) for _ in range(9))
    info = dict(nonfinite_tap=np.zeros((H, W), bool), on_gate=np.zeros((H, W), bool), beyond_gate=np.zeros((H, W), bool))
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ds = dp[r + dy:r + dy + H, r + dx:r + dx + W]
                inside = np.zeros((H, W), bool)
                inside[max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)] = True
                delta = (ds - d).astype(F)
                lim = F(g0 + F(gs * F(max(abs(dx), abs(dy)))))
                fin = np.isfinite(ds)
                taken = fin0 & fin & (np.abs(delta) <= lim)
                info["nonfinite_tap"] |= fin0 & inside & ~fin
                info["on_gate"] |= taken & (np.abs(delta) == lim)
                info["beyond_gate"] |= fin0 & fin & (np.abs(delta) == np.nextafter(lim, F(np.inf)))
                sad = np.abs(ic - ip[r + dy:r + dy + H, r + dx:r + dx + W]).sum(-1)
                w = np.where(taken, tab[sad], 0.0)
                wd = w * np.where(taken, delta, F(0)).astype(D)
                fx, fy = D(dx), D(dy)
                wx, wy = w * fx, w * fy
                n += taken
                S += w; Sx += wx; Sy += wy
                Sxx += wx * fx; Sxy += wx * fy; Syy += wy * fy
                Sd += wd; Sxd += wd * fx; Syd += wd * fy
        C00, C01, C02 = Syy * S - Sy * Sy, Sx * Sy - Sxy * S, Sxy * Sy - Syy * Sx
        C11, C12, C22 = Sxx * S - Sx * Sx, Sxy * Sx - Sxx * Sy, Sxx * Syy - Sxy * Sxy
        det = (Sxx * C00 + Sxy * C01) + Sx * C02
        a = ((C00 * Sxd + C01 * Syd) + C02 * Sd) / det
        b = ((C01 * Sxd + C11 * Syd) + C12 * Sd) / det
        c = ((C02 * Sxd + C12 * Syd) + C22 * Sd) / det
        ys, xs = np.mgrid[0:H, 0:W]
        ok_n = fin0 & (n >= ms)
        ok_det = ok_n & (det > D(1e-3) * ((S * S) * S))
        ok_c = ok_det & (np.abs(c) <= D(g0))
        af, bf = a.astype(F), b.astype(F)
        ok_s = ok_c & np.isfinite(af) & np.isfinite(bf) & (np.abs(af) <= smax) & (np.abs(bf) <= smax)
        cf = ((d.astype(D) + c) - (af.astype(D) * xs.astype(D) + bf.astype(D) * ys.astype(D))).astype(F)
        ok_f = ok_s & np.isfinite(cf)
        ok = ok_f & label_valid(af, bf, cf, xs, ys, mind, maxd)
        in_range = fin0 & (d >= mind) & (d <= maxd)
    info.update(nonfinite_d0=~fin0, support_refused=fin0 & ~ok_n, det_refused=ok_n & ~ok_det, c_refused=ok_det & ~ok_c, slope_refused=ok_c & ~ok_s,
                valid_refused=ok_f & ~ok, out_of_range=fin0 & ~in_range, n=n)
    fb = fallback if fallback is not None else np.broadcast_to(np.array([0, 0, mind, 0], F), (H, W, 4))
    kind = np.where(ok, 2, np.where(in_range, 1, 0)).astype(np.uint8)
    out = np.array(fb, F, copy=True)
    k1 = kind == 1
    out[k1] = np.stack([np.zeros(k1.sum(), F), np.zeros(k1.sum(), F), d[k1], v[k1]], -1)
    k2 = kind == 2
    out[k2] = np.stack([af[k2], bf[k2], cf[k2], v[k2]], -1)
    return out, kind, info


def fit_loop(img, src, fallback=None, mind=MIND, maxd=MAXD, **params):
    """The same by a literal per-pixel transcription of the definition.  Python floats are IEEE doubles; an f32 result of two f32 operands is the
    f64 result rounded to f32 (53 >= 2 x 24 + 2 bits: the double rounding is innocuous)."""
    q = params_of(**params)
    r, ms = int(q["radius"]), int(q["min_support"])
    g0, gs, smax = float(F(q["gate0"])), float(F(q["gate_slope"])), float(F(q["max_slope"]))
    mind, maxd = float(F(mind)), float(F(maxd))
    f32 = lambda t: float(F(t))
    H, W = src.shape[:2]
    if src.ndim == 3:
        dl = [[f32(f32(f32(float(src[y, x, 0]) * x) + f32(float(src[y, x, 1]) * y)) + float(src[y, x, 2])) for x in range(W)] for y in range(H)]
        vl = src[..., 3]
    else:
        dl = [[float(src[y, x]) for x in range(W)] for y in range(H)]
        vl = np.zeros((H, W), F)
    tab = [float(t) for t in weight_table(q["sig"])]
    im = img.astype(int).tolist()
    lim = [f32(g0 + f32(gs * float(k))) for k in range(r + 1)]
    out, kind = np.zeros((H, W, 4), F), np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                d0 = dl[y][x]
                k = 0
                if math.isfinite(d0):
                    n = 0
                    S = Sx = Sy = Sxx = Sxy = Syy = Sd = Sxd = Syd = 0.0
                    pc = im[y][x]
                    for dy in range(-r, r + 1):
                        if not 0 <= y + dy < H:
                            continue
                        for dx in range(-r, r + 1):
                            if not 0 <= x + dx < W:
                                continue
                            ds = dl[y + dy][x + dx]
                            if not math.isfinite(ds):
                                continue
                            delta = f32(ds - d0)
                            if not abs(delta) <= lim[max(abs(dx), abs(dy))]:
                                continue
                            ps = im[y + dy][x + dx]
                            w = tab[abs(pc[0] - ps[0]) + abs(pc[1] - ps[1]) + abs(pc[2] - ps[2])]
                            wx, wy, wd = w * dx, w * dy, w * delta
                            n += 1
                            S += w; Sx += wx; Sy += wy
                            Sxx += wx * dx; Sxy += wx * dy; Syy += wy * dy
                            Sd += wd; Sxd += wd * dx; Syd += wd * dy
                    accepted = False
                    if n >= ms:
                        S, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd = (D(t) for t in (S, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd))       # (numpy: inf / 0 do not raise)
                        C00, C01, C02 = Syy * S - Sy * Sy, Sx * Sy - Sxy * S, Sxy * Sy - Syy * Sx
                        C11, C12, C22 = Sxx * S - Sx * Sx, Sxy * Sx - Sxx * Sy, Sxx * Syy - Sxy * Sxy
                        det = (Sxx * C00 + Sxy * C01) + Sx * C02
                        if det > D(1e-3) * ((S * S) * S):
                            a = ((C00 * Sxd + C01 * Syd) + C02 * Sd) / det
                            b = ((C01 * Sxd + C11 * Syd) + C12 * Sd) / det
                            c = ((C02 * Sxd + C12 * Syd) + C22 * Sd) / det
                            af, bf = F(a), F(b)
                            if abs(c) <= g0 and np.isfinite(af) and np.isfinite(bf) and abs(af) <= smax and abs(bf) <= smax:
                                cf = F((D(d0) + c) - (D(af) * D(x) + D(bf) * D(y)))
                                one = lambda t: np.array([[t]])
                                if np.isfinite(cf) and label_valid(one(af), one(bf), one(cf), one(x), one(y), F(mind), F(maxd))[0, 0]:
                                    out[y, x] = (af, bf, cf, vl[y, x])
                                    accepted, k = True, 2
                    if not accepted and mind <= d0 <= maxd:
                        out[y, x] = (0, 0, d0, vl[y, x])
                        k = 1
                if k == 0:
                    out[y, x] = fallback[y, x] if fallback is not None else (0, 0, mind, 0)
                kind[y, x] = k
    return out, kind


# ------------------------------------------------------------------------------------------------ images and maps
def images(H, W, seed):
    """Both views' images: blocks of one colour plus three grey levels of noise (weights between 0 and 1), one pixel of white in a black block (a
    support that is nearly a single tap)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (0, 1):
        base = np.repeat(np.repeat(rng.integers(0, 200, (-(-H // 6), -(-W // 9), 3)), 6, 0), 9, 1)[:H, :W]
        im = (base + rng.integers(0, 4, (H, W, 3))).astype(np.uint8)
        if H >= 19 and W >= 45:
            im[3:14, 34:45] = 0
            im[8, 39] = 255
        out.append(np.ascontiguousarray(im))
    return out


def fallback_map(H, W, seed):
    lab = ec.cell_labels(H, W, seed, cell=4, maxd=30.0, slant=0.3)
    lab[..., 3] = np.random.default_rng(seed).uniform(-1, 1, (H, W)).astype(F)
    return np.ascontiguousarray(lab)


def mixed_labels(H, W, seed):
    """The mixed label map: slanted cells of 11 x 11 pixels (slopes up to 0.3), then, where the shape has room,
        columns < 33        an inverted pyramid d = 10.9 + 0.5 max(|x - 16|, |y - 16|) around (16, 16) with d = 10 at its tip: every tap of the tip passes
                            the gate and the fit passes more than gate0 above it; its faces have slope 0.5 (refused at max_slope 0.45)
        rows 3 .. 13, columns 34 .. 44   a flat block at d = 0 under the black block of the images (its centre is the white pixel): one neighbour of
                            (5, 36) is exactly on the gate (1.5), the opposite one an ulp beyond (d0 = 0: the differences are exact)
        the last 12 columns a plane of slope 0.3 through d = 1: valid disparities whose +-5 a corners leave the range, then disparities below 0
    and over all of it 10 % isolated disparities in range (no support), 6 % non-finite ones, 4 % isolated ones out of range."""
    rng = np.random.default_rng(seed)
    lab = ec.cell_labels(H, W, seed, cell=11, maxd=30.0, slant=0.3)
    lab[..., 2] += F(6)
    ys, xs = np.mgrid[0:H, 0:W]
    big = H >= 19 and W >= 45

    def flat(mask, d):
        lab[mask] = 0
        lab[..., 2][mask] = np.broadcast_to(d, (H, W))[mask].astype(F)
    if big:
        pyr = xs < 33
        cheb = np.maximum(np.abs(xs - 16), np.abs(ys - min(16, H // 2)))
        flat(pyr, F(10.9) + F(0.5) * cheb.astype(F))
        flat(pyr & (cheb == 0), F(10))
        flat((ys >= 3) & (ys < 14) & (xs >= 34) & (xs < 45), F(0))
        edge = xs >= W - 12
        lab[edge] = 0
        lab[..., 0][edge] = F(-0.3)
        lab[..., 2][edge] = F(1.0) + F(0.3) * F(W - 8)          # d = 1 at column W - 8, falling to the right
    u = rng.uniform(0, 1, (H, W))
    keep = np.zeros((H, W), bool)
    if big:
        keep[3:14, 34:45] = True
        keep[max(0, min(16, H // 2) - 1):min(16, H // 2) + 2, 15:18] = True
    salt = (u < 0.10) & ~keep
    flat(salt, rng.uniform(35.0, 63.0, (H, W)))
    bad = (u >= 0.10) & (u < 0.16) & ~keep
    flat(bad, rng.choice(np.array([np.nan, np.inf, -np.inf], F), (H, W)))
    far = (u >= 0.16) & (u < 0.20) & ~keep
    flat(far, rng.choice(np.array([-40.0, 100.0, 1e30], F), (H, W)))
    if big:
        lab[5, 37] = (0, 0, F(1.5), 0)
        lab[5, 35] = (0, 0, np.nextafter(F(1.5), F(np.inf)), 0)
    lab[..., 3] = rng.uniform(-1, 1, (H, W)).astype(F)
    return np.ascontiguousarray(lab)


@functools.lru_cache(maxsize=None)
def scene(shape):
    """(images of both views, mixed labels, their disparities, fallback) of a shape: computed once, shared, left unchanged."""
    H, W = shape
    ims = images(H, W, 50 + W)
    lab = mixed_labels(H, W, 60 + W)
    disp = disparities_of(lab)
    fb = fallback_map(H, W, 70 + W)
    for a in ims + [lab, disp, fb]:
        a.setflags(write=False)
    return ims, lab, disp, fb


@functools.lru_cache(maxsize=None)
def expected(shape, radius, mode, form, fallback=True, **params):
    """The restated (out, kind, info) of the mixed map of a shape: computed once, shared, left unchanged."""
    ims, lab, disp, fb = scene(shape)
    out, kind, info = fit_restate(ims[mode], lab if form == "labels" else disp, fb if fallback else None, **dict(MIXED, radius=radius, **params))
    out.setflags(write=False); kind.setflags(write=False)
    return out, kind, info


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the restatement itself (CPU only)
def case_restatement_matches_loop():
    checked = 0
    for shape, radii in (((5, 7), RADII), ((33, 70), (1, 5))):
        ims, lab, disp, fb = scene(shape)
        for radius in radii:
            for mode, form in ((0, "labels"), (1, "disp")) if shape == (33, 70) and radius == 5 else ((radius % 2, "labels" if radius == 5 else "disp"),):
                src = lab if form == "labels" else disp
                for extra, fallback in (({}, fb), (dict(sig=0.0), None)) if radius == 5 else (({}, fb),):
                    want = fit_restate(ims[mode], src, fallback, **dict(MIXED, radius=radius, **extra))
                    got = fit_loop(ims[mode], src, fallback, **dict(MIXED, radius=radius, **extra))
                    assert same(want[0], got[0]) and same(want[1], got[1]), (shape, radius, mode, form, extra)
                    checked += 1
    # the largest radius once, on the rows of 33 x 70 that hold the pyramid's tip (the loop is slow)
    ims, lab, disp, fb = scene((33, 70))
    rows = slice(6, 27)
    want = fit_restate(ims[0][rows], lab[rows], fb[rows], **dict(MIXED, radius=15))
    got = fit_loop(ims[0][rows], lab[rows], fb[rows], **dict(MIXED, radius=15))
    assert same(want[0], got[0]) and same(want[1], got[1])
    return checked + 1


# ------------------------------------------------------------------------------------------------ 2. populations
def case_populations_do_what_they_say():
    """Every special is present in the mixed maps the kernel tests use, at every radius, and each kind holds 5 % of the pixels or more."""
    seen = {}
    for shape in ((33, 70), (19, 77)):
        for radius in RADII:
            for mode in (0, 1):
                for form in ("labels", "disp"):
                    out, kind, info = expected(shape, radius, mode, form)
                    share = [float((kind == k).mean()) for k in range(3)]
                    assert min(share) >= 0.05, (shape, radius, mode, form, share)
                    for name in ("nonfinite_d0", "nonfinite_tap", "on_gate", "beyond_gate", "det_refused", "c_refused", "slope_refused", "valid_refused",
                                 "out_of_range", "support_refused"):
                        assert info[name].any(), (shape, radius, mode, form, name)
                    # the constructed ones are where they were put
                    assert info["on_gate"][5, 36] and info["beyond_gate"][5, 36] and info["det_refused"][8, 39], (shape, radius)
                    tip = (min(16, shape[0] // 2), 16)
                    assert info["c_refused"][tip] and kind[tip] == 1
                    # kind 0 carries the fallback bit for bit, kind 1 its own disparity, v is the centre label's (0 from a disparity map)
                    ims, lab, disp, fb = scene(shape)
                    assert same(out[kind == 0], fb[kind == 0])
                    assert same(out[kind == 1][:, 2], disp[kind == 1]) and (out[kind == 1][:, :2] == 0).all()
                    assert same(out[kind != 0][:, 3], lab[kind != 0][:, 3] if form == "labels" else np.zeros(int((kind != 0).sum()), F))
                    seen[(shape, radius)] = share
    # 1 x 40: only collinear support, no slanted fit anywhere; 5 x 7 has all three kinds' code paths reachable at least (kinds 0 and 1 present)
    for radius in RADII:
        out, kind, info = expected((1, 40), radius, 0, "disp")
        assert not (kind == 2).any() and (kind == 1).any() and (kind == 0).any()
        assert info["det_refused"].any() or radius == 1, radius          # (radius 1: three taps at most, refused for their number)
    return seen


# ------------------------------------------------------------------------------------------------ device harness
class Dev:
    """An energy context over the shape's images (image-based cost, no aggregation: any image size) and device buffers for the maps."""

    def __init__(self, lib, shape, ims, mind=MIND, maxd=MAXD):
        H, W = shape
        self.e = api.HipCostVolumeEnergy.naive(ims[0], ims[1], windR=0, max_disp=maxd, min_disp=mind, lib=lib, filter="")
        self.H, self.W = H, W
        P = H * W
        self.lab, self.fb, self.out = (api.DeviceBuffer(self.e, P * 16) for _ in range(3))
        self.disp, self.kind = api.DeviceBuffer(self.e, max(16, P * 4)), api.DeviceBuffer(self.e, max(16, P))

    def fit(self, src, fb, mode, in_place=False, with_kind=True, **params):
        """-> (out, kind or None) of one call; in_place: d_out is the d_fallback buffer."""
        labels = src.ndim == 3
        (self.lab if labels else self.disp).upload(src)
        if fb is not None:
            self.fb.upload(fb)
        self.out.fill(0x5A); self.kind.fill(0x5A)
        dst = self.fb if in_place else self.out
        self.e.fit_planes_ptr(mode, self.lab.ptr if labels else None, None if labels else self.disp.ptr, self.fb.ptr if fb is not None else None, dst.ptr,
                              self.kind.ptr if with_kind else None, **params)
        self.e.synchronize()
        kind = self.kind.download((self.H, self.W), np.uint8)
        if not with_kind:
            assert (kind == 0x5A).all()
        return dst.download((self.H, self.W, 4), F), kind if with_kind else None

    def close(self):
        for b in (self.lab, self.fb, self.out, self.disp, self.kind):
            b.free()
        self.e.close()


def describe(got, want, what):
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(-1) if got.ndim == 3 else got != want
    if not diff.any():
        return ""
    y, x = np.argwhere(diff)[0]
    return f"{int(diff.sum())} {what} differ from the restatement, first at ({y}, {x}): got {got[y, x]}, want {want[y, x]}"


# ------------------------------------------------------------------------------------------------ 3. kernel against the restatement
def case_kernel_bit_for_bit(lib, shape, radius):
    ims, lab, disp, fb = scene(shape)
    d = Dev(lib, shape, ims)
    n = 0
    try:
        for mode in (0, 1):
            for form in ("labels", "disp"):
                src = lab if form == "labels" else disp
                want, want_kind, _ = expected(shape, radius, mode, form)
                q = dict(MIXED, radius=radius)
                got, kind = d.fit(src, fb, mode, **q)
                msg = describe(got, want, "planes") or describe(kind, want_kind, "kinds")
                assert not msg, f"{shape}, radius {radius}, view {mode}, {form}: {msg}"
                n += 1
        # out is the fallback buffer and no kind map; no fallback map; sig = 0 (all weights 1)
        want, want_kind, _ = expected(shape, radius, 1, "labels")
        got, _ = d.fit(lab, fb, 1, in_place=True, with_kind=False, **dict(MIXED, radius=radius))
        assert same(got, want), (shape, radius, "in place")
        want, want_kind, _ = expected(shape, radius, 0, "disp", fallback=False)
        got, kind = d.fit(disp, None, 0, **dict(MIXED, radius=radius))
        assert same(got, want) and same(kind, want_kind), (shape, radius, "no fallback")
        want, want_kind, _ = expected(shape, radius, 0, "labels", sig=0.0)
        got, kind = d.fit(lab, fb, 0, **dict(MIXED, radius=radius, sig=0.0))
        msg = describe(got, want, "planes") or describe(kind, want_kind, "kinds")
        assert not msg, f"{shape}, radius {radius}, sig 0: {msg}"
        # the default parameters (max_slope 2)
        want, want_kind, _ = fit_restate(ims[0], lab, fb, radius=radius)
        got, kind = d.fit(lab, fb, 0, radius=radius)
        assert same(got, want) and same(kind, want_kind), (shape, radius, "defaults")
        n += 4
    finally:
        d.close()
    return n


# ------------------------------------------------------------------------------------------------ 4. exact recovery
RECOVER = dict(sig=10.0, gate0=0.5, gate_slope=0.5)
PLANES = ((F(10 / 64), F(-6 / 64), F(40 + 13 / 64)), (F(-8 / 64), F(12 / 64), F(150 + 5 / 64)))      # (a, b, c): multiples of 1 / 64


@functools.lru_cache(maxsize=None)
def recovery_scene(shape):
    """Two planes that meet at the vertical edge between columns W // 2 - 1 and W // 2, which the guide shows (black | white); the disparities are
    exact in f32 (multiples of 1 / 64 below 256) and jump by about a hundred at the edge."""
    H, W = shape
    xe = W // 2
    ys, xs = np.mgrid[0:H, 0:W]
    side = (xs >= xe).astype(int)
    lab = np.zeros((H, W, 4), F)
    for k, (a, b, c) in enumerate(PLANES):
        lab[side == k] = (a, b, c, F(0.25 * (k + 1)))
    d = disparities_of(lab)
    exact = lab[..., 0].astype(D) * xs + lab[..., 1].astype(D) * ys + lab[..., 2].astype(D)
    assert (d.astype(D) == exact).all() and np.abs(d).max() < 256 and (d * 64 == np.rint(d * 64)).all()
    im = np.where(side[..., None] == 1, 255, 0).astype(np.uint8) * np.ones((1, 1, 3), np.uint8)
    for a in (lab, d, im):
        a.setflags(write=False)
    return np.ascontiguousarray(im), lab, d, side


def check_recovery(shape, radius, out, kind, form):
    im, lab, d, side = recovery_scene(shape)
    H, W = shape
    xe = W // 2
    ys, xs = np.mgrid[0:H, 0:W]
    inner = (ys >= radius) & (ys < H - radius) & (xs >= radius) & (xs < W - radius) & ((xs + radius < xe) | (xs - radius >= xe))
    assert inner.sum() > 0, (shape, radius)
    assert (kind[inner] == 2).all(), (shape, radius, form, int((kind[inner] != 2).sum()))
    assert same(out[inner][:, :3], lab[inner][:, :3]), (shape, radius, form)
    assert same(out[inner][:, 3], lab[inner][:, 3] if form == "labels" else np.zeros(int(inner.sum()), F))
    # next to the edge, away from the image border: still the pixel's own side's plane (the other side's taps fail the gate: the jump is about 100)
    near = (ys >= radius) & (ys < H - radius) & (xs >= radius) & (xs < W - radius) & ~inner
    assert (kind[near] == 2).all() and same(out[near][:, :3], lab[near][:, :3]), (shape, radius, form)
    return int(inner.sum()), int(near.sum())


RECOVERY_SHAPES = {1: (9, 14), 5: (19, 45), 15: (37, 70)}


def case_exact_recovery(lib, radius, cpu_only=False):
    shape = RECOVERY_SHAPES[radius]
    im, lab, d, side = recovery_scene(shape)
    counts = None
    for form, src in (("labels", lab), ("disp", d)):
        want, want_kind, _ = fit_restate(im, src, None, 0.0, 255.0, radius=radius, **RECOVER)
        counts = check_recovery(shape, radius, want, want_kind, form)                # the restatement satisfies it before the device is asked
    if cpu_only:
        return counts
    dev = Dev(lib, shape, [im, im], 0.0, 255.0)
    try:
        for form, src in (("labels", lab), ("disp", d)):
            got, kind = dev.fit(src, None, 1, radius=radius, **RECOVER)
            check_recovery(shape, radius, got, kind, form)
            want, want_kind, _ = fit_restate(im, src, None, 0.0, 255.0, radius=radius, **RECOVER)
            assert same(got, want) and same(kind, want_kind)
    finally:
        dev.close()
    return counts


# ------------------------------------------------------------------------------------------------ 5. independence, argument errors
def case_independence_and_errors(lib, device):
    """The same map on a second stream, beside another enqueued kernel (a 64 MB streaming copy on the context's stream) and after calls with other
    values of sig (the context's table cache: more values than it keeps) gives the same bytes; bad arguments are refused with the stated codes and
    nothing is written."""
    shape, radius = (19, 77), 5
    ims, lab, disp, fb = scene(shape)
    H, W = shape
    d = Dev(lib, shape, ims)
    n = 1 << 24
    big = [api.DeviceBuffer(d.e, 4 * n) for _ in range(2)]
    try:
        want, want_kind, _ = expected(shape, radius, 0, "labels")
        q = dict(MIXED, radius=radius)
        got, kind = d.fit(lab, fb, 0, **q)
        assert same(got, want) and same(kind, want_kind)
        big[0].fill(1)
        side = None
        if device == "cuda":
            import torch
            side = torch.cuda.Stream()
            d.e.set_thread_stream(side.cuda_stream)
        try:
            got, kind = d.fit(lab, fb, 0, **q)                                                        # a second stream
            assert same(got, want) and same(kind, want_kind)
            d.lab.upload(lab); d.fb.upload(fb); d.out.fill(0x5A); d.kind.fill(0x5A)
            d.e._chk(d.e.L.les_hip_calib_copy(api.C.c_void_p(big[0].ptr), api.C.c_void_p(big[1].ptr), n, 0, None))       # default stream: runs beside
            d.e.fit_planes_ptr(0, d.lab.ptr, None, d.fb.ptr, d.out.ptr, d.kind.ptr, **q)
            d.e.synchronize()
            assert same(d.out.download((H, W, 4), F), want) and same(d.kind.download((H, W), np.uint8), want_kind)
        finally:
            if side is not None:
                d.e.set_thread_stream(0, bind=False)
                import torch
                torch.cuda.synchronize()
        # other parameters in between: ten values of sig (the cache keeps eight), another radius and gate
        for k in range(10):
            other, _ = d.fit(lab, fb, 0, **dict(q, sig=0.5 + k, radius=1 + k % 3, gate0=2.0))
        want0, kind0, _ = expected(shape, radius, 0, "labels", sig=0.0)
        got, kind = d.fit(lab, fb, 0, **dict(q, sig=0.0))
        assert same(got, want0) and same(kind, kind0)
        got, kind = d.fit(lab, fb, 0, **q)
        assert same(got, want) and same(kind, want_kind)
        # argument errors: nothing launched, the outputs keep their guard bytes
        d.out.fill(0x5A); d.kind.fill(0x5A)
        L, Dp, Fb, O, K = d.lab.ptr, d.disp.ptr, d.fb.ptr, d.out.ptr, d.kind.ptr
        assert api.FIT_MAX_RADIUS == 15
        bad = [((0, L, Dp, Fb, O, K), {}), ((0, None, None, Fb, O, K), {}), ((0, L, None, Fb, None, K), {}), ((2, L, None, Fb, O, K), {}), ((-1, L, None, Fb, O, K), {}),
               ((0, O, None, Fb, O, K), {}), ((0, None, O, Fb, O, K), {}), ((0, L, None, Fb, O, K), dict(radius=0)), ((0, L, None, Fb, O, K), dict(sig=-1.0)),
               ((0, L, None, Fb, O, K), dict(sig=float("nan"))), ((0, L, None, Fb, O, K), dict(gate0=0.0)), ((0, L, None, Fb, O, K), dict(gate_slope=-0.5)),
               ((0, L, None, Fb, O, K), dict(max_slope=0.0)), ((0, L, None, Fb, O, K), dict(min_support=2)), ((0, L, None, Fb, O, K), dict(gate0=float("inf")))]
        for args, kw in bad:
            try:
                d.e.fit_planes_ptr(*args, **kw)
                raise AssertionError(f"fit_planes_ptr{args} {kw} was accepted")
            except api.LesHipError as ex:
                assert f"error {api.LES_HIP_ERR_ARG}" in str(ex), str(ex)
        try:
            d.e.fit_planes_ptr(0, L, None, Fb, O, K, radius=api.FIT_MAX_RADIUS + 1)
            raise AssertionError("a radius above the limit was accepted")
        except api.LesHipError as ex:
            assert f"error {api.LES_HIP_ERR_UNSUPPORTED}" in str(ex), str(ex)
        d.e.synchronize()
        assert (d.out.download((H * W * 16,), np.uint8) == 0x5A).all() and (d.kind.download((H * W,), np.uint8) == 0x5A).all()
        # the largest radius is served (case_kernel_bit_for_bit runs it); the tensor form returns the same bytes
        t_out, t_kind = d.e.fit_planes(lab, mode=0, fallback=fb, with_kind=True, device=device, **q)
        t_disp = d.e.fit_planes(disp, mode=0, fallback=fb, device=device, **q)
        d.e.synchronize()
        assert same(t_out.cpu().numpy(), want) and same(t_kind.cpu().numpy(), want_kind) and same(t_disp.cpu().numpy(), expected(shape, radius, 0, "disp")[0])
    finally:
        for b in big:
            b.free()
        d.close()


# ------------------------------------------------------------------------------------------------ 6. drivers, on the cones crop
def case_driver_wta(lib, device, device_cuts, full=True):
    """stereo.FastGCStereo on the cones crop (crossview_cases.driver: image-based energy, both views, two layers): fit_planes of the WTA map and
    wta(slanted=True).  full: also the two-view call with the post-processing (the GPU leg; on the fibre simulator every fusion takes seconds)."""
    out = {}
    st, e = cv.driver(lib, device, device_cuts, evaluate_on_device=True)
    try:
        imL, imR, gt = ec.cones_images()
        lab_w, raw_w = st.wta((0, 1), post_process=False)
        wta = dict(st.raw_labelings)
        wta_rows = list(st.log)
        # fit_planes of the WTA map: checked on the restatement first, then the device map is that restatement
        want, want_kind, _ = fit_restate(imL, wta[0], wta[0], 0.0, 63.0)
        share = float((want_kind == 2).mean())
        print(f"cones crop, planes fitted to the left WTA map: kind 2 on {100 * share:.1f} % of the pixels, kind 1 on {100 * float((want_kind == 1).mean()):.1f} %")
        assert share > 0.5, share
        fitted, kind = e.fit_planes(wta[0], mode=0, fallback=wta[0], with_kind=True, device=device)
        e.synchronize()
        assert same(fitted.cpu().numpy(), want) and same(kind.cpu().numpy(), want_kind)
        assert same(st.fit_planes(disparities_of(wta[0]), 0), fit_restate(imL, disparities_of(wta[0]), None, 0.0, 63.0)[0])
        # wta(slanted=True): per view a fusion of the WTA map and its fitted map; the energy does not rise
        st.wta((0, 1), post_process=False, slanted=True)
        slanted = dict(st.raw_labelings)
        for m in (0, 1):
            im = imL if m == 0 else imR
            fit_m = fit_restate(im, wta[m], wta[m], 0.0, 63.0)[0]
            own = (slanted[m].view(np.uint32) == wta[m].view(np.uint32)).all(-1)
            other = (slanted[m].view(np.uint32) == fit_m.view(np.uint32)).all(-1)
            assert (own | other).all(), (m, int((~(own | other)).sum()))
            E0, E1 = cv.energy_of(st, e, device, wta[m], m), cv.energy_of(st, e, device, slanted[m], m)
            print(f"view {m}: energy of wta() {E0:.2f}, of wta(slanted=True) {E1:.2f}; pixels that took the fitted label {int((~own).sum())}; "
                  f"kind pixels [fallback, fronto, slanted] {st.slant_stats[m]['kind_pixels']}")
            assert E1 <= E0, (m, E0, E1)
            assert st.slant_stats[m]["kind_pixels"][2] > 0 and sum(st.slant_stats[m]["kind_pixels"]) == im.shape[0] * im.shape[1]
            out[f"view{m}"] = dict(E_wta=E0, E_slanted=E1, taken=int((~own).sum()))
        d_gt = np.where(gt > 0, gt, np.nan)
        bad = lambda lab: float((np.abs(disparities_of(lab) - d_gt)[gt > 0] > 1.0).mean() * 100)
        print(f"left view bad-1.0: wta() {bad(wta[0]):.2f} %, wta(slanted=True) {bad(slanted[0]):.2f} %; rows of wta(): {[round(r['energy'], 1) for r in wta_rows]}, "
              f"of wta(slanted=True): {[round(r['energy'], 1) for r in st.log]}")
        if full:          # two views with the post-processing run end to end
            lab_s, raw_s = st.wta((0, 1), slanted=True)
            assert same(raw_s, slanted[0]) and np.isfinite(lab_s).all()
        st3, e3 = cv.driver(lib, device, device_cuts)
        try:
            st3.units, st3.table = [], []
            try:
                st3.wta((0,), slanted=True)
                raise AssertionError("wta(slanted=True) without layers was accepted")
            except ValueError:
                pass
        finally:
            e3.close()
    finally:
        e.close()
    return out


def case_driver_run(lib, device, device_cuts, full=True):
    """run(labeling="wta+planes") and run(labeling=<a disparity map>) on the cones crop.  full: also the "wta" run it is printed next to and the dict
    form (the GPU leg)."""
    out = {}
    st, e = cv.driver(lib, device, device_cuts, evaluate_on_device=True)
    try:
        imL, imR, gt = ec.cones_images()
        d_gt = np.where(gt > 0, gt, np.nan)
        bad = lambda lab: float((np.abs(disparities_of(lab) - d_gt)[gt > 0] > 1.0).mean() * 100)
        st.wta((0,), post_process=False)
        wta = dict(st.raw_labelings)
        # run(labeling="wta+planes"): bit-identical on repeat; without graph-cut iterations it is the WTA start
        st.log = []
        lab_a, raw_a = st.run(1, (0,), 0, labeling="wta+planes")
        rows_a, stats_a = list(st.log), dict(st.slant_stats)
        st.log = []
        lab_b, raw_b = st.run(1, (0,), 0, labeling="wta+planes")
        assert same(lab_a, lab_b) and same(raw_a, raw_b) and [r["energy"] for r in rows_a] == [r["energy"] for r in st.log]
        assert stats_a[0]["kind_pixels"] == st.slant_stats[0]["kind_pixels"] and stats_a[0]["pixels_taken"] == st.slant_stats[0]["pixels_taken"]
        print(f"run(1, pmInit=0, labeling='wta+planes'): energy {rows_a[0]['energy']:.1f} -> {rows_a[-1]['energy']:.1f}, bad-1.0 {bad(lab_a):.2f} %; "
              f"fusion: {stats_a[0]['pixels_taken']} pixels taken, kind pixels {stats_a[0]['kind_pixels']}")
        out.update(start=rows_a[0]["energy"], end=rows_a[-1]["energy"])
        if full:
            st.log = []
            lab_p, _ = st.run(1, (0,), 0, labeling="wta")
            print(f"run(1, pmInit=0, labeling='wta'): energy {st.log[0]['energy']:.1f} -> {st.log[-1]['energy']:.1f}, bad-1.0 {bad(lab_p):.2f} %")
        st.log = []
        lab_0, _ = st.run(0, (0,), 0, labeling="wta+planes")
        assert same(lab_0, wta[0]) and not st.slant_stats
        # a disparity map as the start labelling == the fitted map as the start labelling, also in a dict
        dmap = disparities_of(wta[0])
        st.log = []
        lab_d, raw_d = st.run(1, (0,), 0, labeling=dmap)
        st.log = []
        lab_f, raw_f = st.run(1, (0,), 0, labeling=st.fit_planes(dmap, 0))
        assert same(lab_d, lab_f) and same(raw_d, raw_f)
        if full:
            st.log = []
            lab_g, raw_g = st.run(1, (0,), 0, labeling={0: dmap})
            assert same(lab_g, lab_d)
        # what is refused
        try:
            st.run(1, (0,), 0, labeling="wta+plane")
            raise AssertionError("an unknown start was accepted")
        except ValueError:
            pass
        st2, e2 = cv.driver(lib, device, device_cuts, world=2)
        try:
            for fn in (lambda: st2.wta((0,), slanted=True), lambda: st2.run(1, (0,), 0, labeling="wta+planes")):
                try:
                    fn()
                    raise AssertionError("world = 2 was accepted")
                except NotImplementedError:
                    pass
        finally:
            e2.close()
    finally:
        e.close()
    return out


def case_driver_midv(lib, device, monkeypatch, layers=None, **opts):
    """MidV2 / MidV3(init="wta+planes") run end to end and report the fusion.  layers, opts: as crossview_cases.case_driver_midv2."""
    from localexpstereo_amd import stereo
    from tests import costvol_cases as cc
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    kw = dict(iterations=1, pmIterations=0, device=device, lib=lib, **opts)
    st2, lab2, _ = stereo.MidV2(cv.cones_data(), init="wta+planes", **kw)
    assert np.isfinite(lab2).all() and sorted(st2.slant_stats) == [0]
    imL, imR, gt = cc.cones_pair()
    data3 = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
    st3, lab3, _ = stereo.MidV3(data3, None, None, doDual=True, init="wta+planes", evaluate_on_device=True, **kw)
    assert lab3.shape == gt.shape + (4,) and np.isfinite(lab3).all() and sorted(st3.slant_stats) == [0, 1]
    print(f"MidV3 from the pair, init='wta+planes': energy {st3.log[0]['energy']:.1f} -> {st3.log[1]['energy']:.1f}, all {st3.log[0]['all']:.2f} -> {st3.log[1]['all']:.2f} %; "
          f"kind pixels {[st3.slant_stats[m]['kind_pixels'] for m in (0, 1)]}")
    assert st3.log[1]["energy"] <= st3.log[0]["energy"]
    return dict(midv3_start=st3.log[0]["energy"], midv3_after=st3.log[1]["energy"])
