"""Cases of tests/test_unrectify.py: the way back from the rectified pair to the raw camera (csrc/les_unrectify.h: les_hip_unrectify_map,
les_hip_unrectify_labels; api.unrectify_map / api.unrectify_labels; stereo.Rectifier.inverse_maps / .unrectify / .to_raw / .valid_rect / .crop) on
the CPU simulator build and on the MI355X.

The definitions, restated from csrc/les_unrectify.h (camera model, conventions and the forward map: tests/rectify_cases.py).  Every operation
fp64, rounded, in this order; each output rounded to f32 once; every NaN stored is 0x7fc00000.
  distort   xx = x x, yy = y y, xy = x y, r2 = xx + yy; num = 1 + r2 (k1 + r2 (k2 + r2 k3)), den = 1 + r2 (k4 + r2 (k5 + r2 k6)); den finite and
            != 0 or (NaN, NaN); rad = num / den; ex = (x rad + (2 p1) xy) + p2 (r2 + 2 xx), ey = (y rad + p1 (r2 + 2 yy)) + (2 p2) xy.
  map       inv[v][u] = (xs, ys): xd = (u - cxr) / fx, yd = (v - cyr) / fy; x = xd, y = yd; `steps` times (ex, ey) = distort(x, y),
            x = x - (ex - xd), y = y - (ey - yd); (ex, ey) = distort(x, y) once more; converged iff |fx (ex - xd)| <= tol and |fy (ey - yd)| <= tol
            or (NaN, NaN); X = (R0 x + R1 y) + R2, Y, Z alike; Z > 0 or (NaN, NaN); xs = f (X / Z) + cx, ys = f (Y / Z) + cy; a NaN in either
            rounded coordinate: (NaN, NaN).
  labels    (xs, ys) the map entry as fp64; inside iff 0 <= xs <= W - 1 and 0 <= ys <= H - 1; xi = min(floor(xs + 0.5), W - 1), yi alike;
            (a, b, c, .) = labels[yi][xi]; dropped = drop[yi][xi] != 0; d = (a xs + b ys) + c; D = d + doffs; Zr = (f baseline) / D; valid iff
            inside, d finite, D > 0, not dropped, Zr <= z_max when z_max > 0; Xr = ((xs - cx) Zr) / f, Yr = ((ys - cy) Zr) / f;
            P_j = (M[3j] Xr + M[3j+1] Yr) + M[3j+2] Zr; nr = (a f, b f, ((a cx + b cy) + c) + doffs), n_j = (M[3j] nrx + M[3j+1] nry) + M[3j+2] nrz;
            normal = -n / sqrt((nx nx + ny ny) + nz nz); disparity = d; valid 255 / 0; NaN in every float output of an invalid pixel.

References, none of them the code under test: the vectorised numpy restatements below, themselves held to literal per-pixel loops; the camera
model rectify_cases.project for the geometric tests.  Tolerances: none for the kernels -- every output is compared bit for bit (fp64 add,
multiply, divide, sqrt and floor are correctly rounded on both sides, the order is fixed, nothing is contracted, each output is rounded once).

Shapes: raw grids (1, 1), (3, 5), (17, 67), (64, 257) -- the last crosses a workgroup of 256 within a row --, rectified sizes (1, 1), (9, 300)
and (17, 67), steps 1, 20, 64, tol 1e-3 and 1e-6."""
import ctypes as C
import functools
import itertools

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import io as lio
from tests import crossview_cases as cv
from tests import pyramid_cases as pc
from tests import rectify_cases as rc
from tests.rectify_cases import D, F, QNAN, cones_setup, first_diff, map_inputs, same

SHAPES = rc.SHAPES                            # raw grids
SIZES = [(1, 1), (9, 300), (17, 67)]          # rectified label maps
STEPS = (1, 20, 64)
TOLS = (1e-3, 1e-6)
OUTPUTS = ("points", "normals", "disparity", "valid")


# ------------------------------------------------------------------------------------------------ restatement, numpy
def _distort_ordered(coef, x, y):
    k1, k2, p1, p2, k3, k4, k5, k6 = coef
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
    rad = num / den
    ex = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
    ey = (y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
    return ex, ey, den


def inv_parts(K, dist, R, f, cx, cy, Hs, Ws, steps=api.UNRECTIFY_STEPS, tol=api.UNRECTIFY_TOL):
    """-> (inv Hs x Ws x 2 f32, dict(pole: a den that is 0 or not finite in some evaluation, converged, Z, den: that of the last evaluation):
    what the NaN branches test)"""
    R = np.asarray(R, D).reshape(9)
    coef = tuple(rc._coefficients(dist))
    fx, fy, cxr, cyr, f, cx, cy, tol = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy, tol))
    vs, us = np.mgrid[0:Hs, 0:Ws]
    with np.errstate(all="ignore"):
        xd, yd = (us.astype(D) - cxr) / fx, (vs.astype(D) - cyr) / fy
        x, y = xd, yd
        pole = np.zeros((Hs, Ws), bool)
        for _ in range(steps):
            ex, ey, den = _distort_ordered(coef, x, y)
            pole |= ~np.isfinite(den) | (den == 0.0)
            x, y = x - (ex - xd), y - (ey - yd)
        ex, ey, den = _distort_ordered(coef, x, y)
        pole |= ~np.isfinite(den) | (den == 0.0)
        converged = (np.abs(fx * (ex - xd)) <= tol) & (np.abs(fy * (ey - yd)) <= tol)
        X = (R[0] * x + R[1] * y) + R[2]
        Y = (R[3] * x + R[4] * y) + R[5]
        Z = (R[6] * x + R[7] * y) + R[8]
        xs, ys = (f * (X / Z) + cx).astype(F), (f * (Y / Z) + cy).astype(F)
        ok = ~pole & converged & (Z > 0.0) & ~np.isnan(xs) & ~np.isnan(ys)
    out = np.full((Hs, Ws, 2), QNAN, F)
    out[ok, 0], out[ok, 1] = xs[ok], ys[ok]
    return out, dict(pole=pole, converged=converged & ~pole, Z=Z, den=den)


def inv_restate(K, dist, R, f, cx, cy, Hs, Ws, steps=api.UNRECTIFY_STEPS, tol=api.UNRECTIFY_TOL):
    return inv_parts(K, dist, R, f, cx, cy, Hs, Ws, steps, tol)[0]


def inv_loop(K, dist, R, f, cx, cy, Hs, Ws, steps=api.UNRECTIFY_STEPS, tol=api.UNRECTIFY_TOL):
    """The same by a literal per-pixel transcription (numpy's float64 scalars: IEEE doubles, and a division by zero is no exception)."""
    R = [D(v) for v in np.asarray(R, D).reshape(9)]
    k1, k2, p1, p2, k3, k4, k5, k6 = rc._coefficients(dist)
    fx, fy, cxr, cyr, f, cx, cy, tol = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy, tol))
    one, two = D(1.0), D(2.0)
    out = np.full((Hs, Ws, 2), QNAN, F)

    def dist_(x, y):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        num = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        den = one + r2 * (k4 + r2 * (k5 + r2 * k6))
        if not np.isfinite(den) or den == 0.0:
            return None
        rad = num / den
        return (x * rad + (two * p1) * xy) + p2 * (r2 + two * xx), (y * rad + p1 * (r2 + two * yy)) + (two * p2) * xy

    def pixel(u, v):
        xd, yd = (D(u) - cxr) / fx, (D(v) - cyr) / fy
        x, y = xd, yd
        for _ in range(steps):
            e = dist_(x, y)
            if e is None:
                return None
            x, y = x - (e[0] - xd), y - (e[1] - yd)
        e = dist_(x, y)
        if e is None or not (abs(fx * (e[0] - xd)) <= tol and abs(fy * (e[1] - yd)) <= tol):
            return None
        X = (R[0] * x + R[1] * y) + R[2]
        Y = (R[3] * x + R[4] * y) + R[5]
        Z = (R[6] * x + R[7] * y) + R[8]
        if not Z > 0.0:
            return None
        xs, ys = F(f * (X / Z) + cx), F(f * (Y / Z) + cy)
        return (xs, ys) if xs == xs and ys == ys else None

    with np.errstate(all="ignore"):
        for v in range(Hs):
            for u in range(Ws):
                p = pixel(u, v)
                if p is not None:
                    out[v, u] = p
    return out


def lab_parts(labels, drop, inv, M, f, cx, cy, doffs, baseline, z_max=None):
    """labels H x W x 4 f32, drop H x W u8 or None, inv Hs x Ws x 2 f32 -> (dict(points, normals, disparity, valid), dict of the populations)"""
    H, W = labels.shape[:2]
    M = np.asarray(M, D).reshape(9)
    f, cx, cy, doffs, baseline = (D(v) for v in (f, cx, cy, doffs, baseline))
    zm = F(z_max if z_max is not None else 0.0)
    xs, ys = inv[..., 0].astype(D), inv[..., 1].astype(D)
    with np.errstate(all="ignore"):
        inside = (xs >= 0.0) & (xs <= D(W - 1)) & (ys >= 0.0) & (ys <= D(H - 1))
        xs, ys = np.where(inside, xs, 0.0), np.where(inside, ys, 0.0)
        xi, yi = np.minimum(np.floor(xs + 0.5).astype(np.int64), W - 1), np.minimum(np.floor(ys + 0.5).astype(np.int64), H - 1)
        lab = labels[yi, xi].astype(D)
        a, b, c = lab[..., 0], lab[..., 1], lab[..., 2]
        dropped = (drop[yi, xi] != 0) if drop is not None else np.zeros(inside.shape, bool)
        d = (a * xs + b * ys) + c
        Dd = d + doffs
        Zr = (f * baseline) / Dd
        far = ~(Zr <= D(zm)) if zm > 0 else np.zeros(inside.shape, bool)
        valid = inside & np.isfinite(d) & (Dd > 0.0) & ~dropped & ~far
        Xr, Yr = ((xs - cx) * Zr) / f, ((ys - cy) * Zr) / f
        nr = (a * f, b * f, ((a * cx + b * cy) + c) + doffs)
        P = [(M[3 * j] * Xr + M[3 * j + 1] * Yr) + M[3 * j + 2] * Zr for j in range(3)]
        N = [(M[3 * j] * nr[0] + M[3 * j + 1] * nr[1]) + M[3 * j + 2] * nr[2] for j in range(3)]
        ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
        points, normals = np.stack(P, -1).astype(F), np.stack([-n / ln for n in N], -1).astype(F)
        disparity = d.astype(F)
    points[~valid], normals[~valid], disparity[~valid] = QNAN, QNAN, QNAN
    kinds = dict(inside=inside, outside=~inside, dropped=inside & dropped, nonfinite=inside & ~np.isfinite(d), behind=inside & np.isfinite(d) & ~(Dd > 0.0),
                 far=inside & np.isfinite(d) & (Dd > 0.0) & ~dropped & far, valid=valid, taps=(yi, xi))
    return dict(points=points, normals=normals, disparity=disparity, valid=np.where(valid, 255, 0).astype(np.uint8)), kinds


def lab_restate(*a, **kw):
    return lab_parts(*a, **kw)[0]


def lab_loop(labels, drop, inv, M, f, cx, cy, doffs, baseline, z_max=None):
    """The same by a literal per-pixel transcription."""
    H, W = labels.shape[:2]
    Hs, Ws = inv.shape[:2]
    M = [D(v) for v in np.asarray(M, D).reshape(9)]
    f, cx, cy, doffs, baseline = (D(v) for v in (f, cx, cy, doffs, baseline))
    zm = F(z_max if z_max is not None else 0.0)
    out = dict(points=np.full((Hs, Ws, 3), QNAN, F), normals=np.full((Hs, Ws, 3), QNAN, F), disparity=np.full((Hs, Ws), QNAN, F), valid=np.zeros((Hs, Ws), np.uint8))
    with np.errstate(all="ignore"):
        for v in range(Hs):
            for u in range(Ws):
                xs, ys = D(inv[v, u, 0]), D(inv[v, u, 1])
                if not (xs >= 0.0 and xs <= D(W - 1) and ys >= 0.0 and ys <= D(H - 1)):
                    continue
                xi, yi = min(int(np.floor(xs + D(0.5))), W - 1), min(int(np.floor(ys + D(0.5))), H - 1)
                a, b, c = (D(t) for t in labels[yi, xi, :3])
                d = (a * xs + b * ys) + c
                Dd = d + doffs
                Zr = (f * baseline) / Dd
                if not np.isfinite(d) or not Dd > 0.0 or (drop is not None and drop[yi, xi] != 0) or (zm > 0 and not Zr <= D(zm)):
                    continue
                Xr, Yr = ((xs - cx) * Zr) / f, ((ys - cy) * Zr) / f
                nr = (a * f, b * f, ((a * cx + b * cy) + c) + doffs)
                P = [(M[3 * j] * Xr + M[3 * j + 1] * Yr) + M[3 * j + 2] * Zr for j in range(3)]
                N = [(M[3 * j] * nr[0] + M[3 * j + 1] * nr[1]) + M[3 * j + 2] * nr[2] for j in range(3)]
                ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
                out["points"][v, u], out["normals"][v, u] = [F(p) for p in P], [F(-n / ln) for n in N]
                out["disparity"][v, u], out["valid"][v, u] = F(d), 255
    return out


# ------------------------------------------------------------------------------------------------ inputs
def inv_inputs(name, shape):
    """The views of rectify_cases.map_inputs as inverse-map arguments (K, dist, R = M^T, f, cx, cy), plus two rigs of this file: "zero" and
    "overflow" with the raw camera at focal length 2 and centre 0, so that raw pixel (2, 0) / (4, 0) has r2 = 1 / 4 exactly in the first
    evaluation (den = 0; r2 k6 = +inf), as map_inputs' rigs of these names have on the rectified side."""
    if name in ("zero inv", "overflow inv"):
        H, W = shape
        coef = (0.1, 0, 0, 0, 0, -1.0) if name == "zero inv" else (0.1, 0, 0, 0, 0, 0, 0, 1e308)
        return [(rc.pinhole(2.0, 2.0, 0.0, 0.0), coef, np.eye(3), 0.6 * max(H, W) + 1.0, 0.5 * (W - 1), 0.5 * (H - 1))]
    return [(K, dist, np.ascontiguousarray(np.asarray(M).T), f, cx, cy) for K, dist, M, f, cx, cy in map_inputs(name, shape)]


INV_RIGS = rc.RIGS + ("zero inv", "overflow inv")


def five_geometry(shape):
    """The calibration the labels kernel is tested with: view 1 of rig "five" for a raw grid of `shape` -> dict(M, f, cx, cy, doffs, baseline)"""
    v0, v1 = map_inputs("five", shape)
    return dict(M=np.ascontiguousarray(v1[2]), f=v1[3], cx=v1[4], cy=v1[5], doffs=v1[4] - v0[4], baseline=1.0)


@functools.lru_cache(maxsize=None)
def label_inputs(size, shape):
    """-> (labels H x W x 4 f32, drop H x W u8, z_max): slanted planes whose D = d + doffs takes both signs over the frame, one entry in twelve
    not finite, one pixel in five dropped, and a z_max near the median depth of the finite ones."""
    H, W = size
    g = five_geometry(shape)
    rng = np.random.default_rng(3000 + 17 * H + W + 3 * shape[0] + shape[1])
    lab = np.zeros((H, W, 4), F)
    lab[..., 0], lab[..., 1] = rng.uniform(-0.3, 0.3, (H, W)), rng.uniform(-0.3, 0.3, (H, W))
    ys, xs = np.mgrid[0:H, 0:W]
    d = rng.uniform(-0.5 * 20.0, 20.0, (H, W)) - g["doffs"]                  # the disparity at the pixel itself: D in -10 .. 20
    lab[..., 2] = d - (lab[..., 0] * xs + lab[..., 1] * ys)
    lab[..., 3] = rng.uniform(-1.0, 1.0, (H, W))                            # (the fourth entry is not read)
    flat = lab[..., :3].reshape(-1)
    bad = rng.random(flat.size) < 1.0 / 36.0
    flat[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    lab[..., :3] = flat.reshape(H, W, 3)
    if size == (1, 1):
        lab[0, 0, :3] = (0.125, -0.25, 6.0 - g["doffs"])                    # one label: make it a good one
    drop = np.where(rng.random((H, W)) < 0.2, rng.integers(1, 256, (H, W)), 0).astype(np.uint8)
    if size == (1, 1):
        drop[0, 0] = 0
    z_max = float(g["f"] * g["baseline"] / 6.0)                              # D = 6: about a third of the pixels with D > 0 lie beyond
    lab.setflags(write=False)
    drop.setflags(write=False)
    return lab, drop, z_max


INV_KINDS = ("rig", "edges", "random")


@functools.lru_cache(maxsize=None)
def inv_input(shape, size, kind):
    """An inverse map of raw grid `shape` against a label map of `size`: "rig": view 1 of rig "five" at tol 1e-6 (real positions, NaN where
    not converged), shifted so that the label map lies in its middle; "edges", "random": rectify_cases.hand_map (borders, -0, +-0.5, NaN, +-inf,
    +-1e30, +-3e9; uniform positions from -1 to the size)."""
    if kind != "rig":
        return rc.hand_map(shape, size, kind)
    K, dist, R, f, cx, cy = inv_inputs("five", shape)[1]
    inv = inv_restate(K, dist, R, f, 0.5 * (size[1] - 1), 0.5 * (size[0] - 1), *shape, steps=20, tol=1e-6)
    inv.setflags(write=False)
    return inv


# ------------------------------------------------------------------------------------------------ 1 - 5. host tests
def case_restatement_matches_loop(shape=(5, 7)):
    n = 0
    for name in INV_RIGS:
        for args in inv_inputs(name, shape):
            for steps, tol in ((1, 1e-3), (20, 1e-3), (20, 1e-6)):
                a, b = inv_restate(*args, *shape, steps, tol), inv_loop(*args, *shape, steps, tol)
                assert same(a, b), (name, steps, tol, first_diff(a, b))
                n += 1
    g = five_geometry(shape)
    for size in SIZES + [(5, 7)]:
        lab, drop, z_max = label_inputs(size, shape)
        for kind in INV_KINDS:
            for dr, zm in itertools.product((None, drop), (None, z_max)):
                a, b = lab_restate(lab, dr, inv_input(shape, size, kind), z_max=zm, **g), lab_loop(lab, dr, inv_input(shape, size, kind), z_max=zm, **g)
                for k in OUTPUTS:
                    assert same(a[k], b[k]), (size, kind, k, first_diff(a[k], b[k]))
                n += 1
    return n


def case_populations():
    """Each kind of pixel the device cases need occurs in their inputs; every population is non-empty."""
    seen = {}

    def add(k, m):
        seen[k] = seen.get(k, 0) + int(np.count_nonzero(m))

    for shape in SHAPES[2:]:
        Hs, Ws = shape
        for name in INV_RIGS:
            for args in inv_inputs(name, shape):
                for steps, tol in itertools.product(STEPS, TOLS):
                    inv, p = inv_parts(*args, Hs, Ws, steps, tol)
                    nan = np.isnan(inv[..., 0])
                    assert same(nan, np.isnan(inv[..., 1]))
                    add("stored", ~nan)
                    add("not converged", ~p["pole"] & ~p["converged"])
                    add(f"pole ({name})", p["pole"])
                    add(f"Z <= 0 ({name})", p["converged"] & ~(p["Z"] > 0.0))
                    if name == "identity":
                        assert not nan.any() and same(inv, rc.identity_map(Hs, Ws)), shape
                    if name == "five":
                        assert (~nan).any(), (shape, steps, tol)
                        add(f"not converged (five, {steps} steps, tol {tol}) {shape}", ~p["pole"] & ~p["converged"])
                        add(f"converged (five, {steps} steps, tol {tol}) {shape}", p["converged"])
                    if name == "pole":                                            # the pole of rad lies inside the raw frame: den takes both signs
                        add("den < 0 (pole)", p["den"] < 0.0)
                        add("den > 0 (pole)", p["den"] > 0.0)
                    if name == "zero inv":
                        assert p["pole"][0, 2] and nan[0, 2], shape
                    if name == "overflow inv":
                        assert p["pole"][0, 4] and nan[0, 4] and not nan[0, 0], shape
        g = five_geometry(shape)
        for size in SIZES:
            lab, drop, z_max = label_inputs(size, shape)
            for kind in INV_KINDS:
                out, k = lab_parts(lab, drop, inv_input(shape, size, kind), z_max=z_max, **g)
                for name in ("inside", "outside", "dropped", "nonfinite", "behind", "far", "valid"):
                    add(f"{name} {size}", k[name])
                add("converged and inside", k["inside"] & (kind == "rig"))
                add("converged and outside", k["outside"] & ~np.isnan(inv_input(shape, size, kind)[..., 0]) & (kind == "rig"))
                assert np.isnan(out["points"][out["valid"] == 0]).all() and np.isfinite(out["disparity"][out["valid"] == 255]).all()
    need = ["stored", "not converged", "den < 0 (pole)", "den > 0 (pole)", "pole (zero inv)", "pole (overflow inv)", "Z <= 0 (behind)", "converged and inside", "converged and outside"]
    need += [f"{name} {size}" for size in SIZES[1:] for name in ("inside", "outside", "dropped", "nonfinite", "behind", "far", "valid")]
    need += [f"{name} (1, 1)" for name in ("inside", "outside", "valid")]
    need += [f"{k} (five, 20 steps, tol 1e-06) {shape}" for shape in SHAPES[2:] for k in ("converged", "not converged")]      # the small shapes too
    for k in need:
        assert seen.get(k, 0) > 0, (k, seen)
    return seen


def forward(K, dist, R, f, cx, cy, xs, ys):
    """The forward formula in its continuous form: a rectified position -> the raw pixel."""
    ray = np.stack([(xs - cx) / f, (ys - cy) / f, np.ones_like(xs)], 1) @ np.asarray(R, D).reshape(3, 3)          # (rows times R: R^T applied)
    return rc.project(np.asarray(K, D), np.concatenate([np.asarray(dist, D).reshape(-1), np.zeros(8)])[:8], ray)


def cones_views():
    s = cones_setup()
    tr = s["transform"]
    return [(tr[f"K{m}"], tr[f"dist{m}"], tr[f"R{m}"], tr["f"], tr[f"cx{m}"], tr["cy"]) for m in (0, 1)]


def case_consistency():
    """The forward formula at the stored (xs, ys) of every converged raw pixel returns (u, v) within tol + 1e-4 px: the residual bound plus the
    f32 rounding of (xs, ys) through the map's local stretch.  Measured here (numpy restatement): cones rig 7.3e-6 px at tol 1e-3 and 1e-6; rig
    "five" at 64 x 257 9.96e-4 at tol 1e-3 and 9.7e-6 at tol 1e-6 (the first is the residual bound itself)."""
    worst = {}
    rigs = [("cones", rc.RAW_SIZE, v) for v in cones_views()] + [("five", (64, 257), v) for v in inv_inputs("five", (64, 257))]
    for name, (Hs, Ws), args in rigs:
        for tol in TOLS:
            inv = inv_restate(*args, Hs, Ws, 20, tol)
            ok = ~np.isnan(inv[..., 0])
            assert ok.any(), (name, tol)
            vs, us = np.nonzero(ok)
            uv = forward(*args, inv[ok][:, 0].astype(D), inv[ok][:, 1].astype(D))
            err = float(np.abs(uv - np.stack([us, vs], 1)).max())
            worst[(name, tol)] = max(worst.get((name, tol), 0.0), err)
            assert err <= tol + 1e-4, (name, tol, err)
    print("largest forward error of a converged pixel, px:", worst)
    return worst


PLANES = [((0.0, 0.0, 1.0), 2.0), ((0.3, -0.2, 1.0), 1.5), ((-0.4, 0.5, 1.0), 3.0), ((0.1, 0.6, 0.9), 1.0)]
PLANE_REL, PLANE_PX = 4 * 1.5e-7, 4 * 8.7e-6        # four times the figures of case_planes' docstring ...
PLANE_REL_MAX, PLANE_PX_MAX = 1e-4, api.UNRECTIFY_TOL + 1e-4      # ... and neither may be looser than this


def case_planes():
    """A 3D plane n . P = h of the left raw frame, written as the constant rectified label it is, comes back as points on that plane that
    project onto their own raw pixels.  Measured with the restatement (cones rig, view 0, labels rounded to f32, 4 planes): |n . P - h| / h
    at most 1.5e-7, |project(K, dist, P) - (u, v)| at most 8.7e-6 px; the caps are four times these (the f32 rounding of labels and outputs
    moves with the plane)."""
    assert PLANE_REL <= PLANE_REL_MAX and PLANE_PX <= PLANE_PX_MAX
    s = cones_setup()
    tr = s["transform"]
    H, W = s["gt"].shape
    Hs, Ws = rc.RAW_SIZE
    K, dist, R0, f, cx, cy = cones_views()[0]
    inv = inv_restate(K, dist, R0, f, cx, cy, Hs, Ws)
    worst = [0.0, 0.0]
    for n, h in PLANES:
        n = np.array(n, D)
        nr = R0 @ n                                                           # the plane in the rectified frame: nr . Q = h
        s_ = f * tr["baseline"] / h
        lab = np.zeros((H, W, 4), F)
        lab[..., 0], lab[..., 1], lab[..., 2] = s_ * nr[0] / f, s_ * nr[1] / f, s_ * (nr[2] - (nr[0] * cx + nr[1] * cy) / f) - tr["doffs"]
        out = lab_restate(lab, None, inv, R0.T, f, cx, cy, tr["doffs"], tr["baseline"])
        ok = out["valid"] == 255
        assert ok.sum() >= 8000, int(ok.sum())
        P = out["points"][ok].astype(D)
        vs, us = np.nonzero(ok)
        rel = float(np.abs(P @ n - h).max() / h)
        px = float(np.abs(rc.project(K, dist, P) - np.stack([us, vs], 1)).max())
        nrm = out["normals"][ok].astype(D)
        assert np.abs(nrm + n / np.linalg.norm(n)).max() <= 1e-6                 # the unit normal, facing the camera (f32 outputs)
        worst = [max(worst[0], rel), max(worst[1], px)]
        assert rel <= PLANE_REL and px <= PLANE_PX, (n, h, rel, px)
    print("planes: largest |n . P - h| / h and reprojection error, px:", worst)
    return worst


def brute_rect(mask):
    """The largest all-True rectangle by trying every one; the tie rule of stereo.largest_rect."""
    H, W = mask.shape
    best_key, best = None, (0, 0, 0, 0)
    for y0 in range(H):
        for x0 in range(W):
            for h in range(1, H - y0 + 1):
                for w in range(1, W - x0 + 1):
                    if mask[y0:y0 + h, x0:x0 + w].all():
                        key = (-h * w, y0, x0, -h)
                        if best_key is None or key < best_key:
                            best_key, best = key, (y0, x0, h, w)
    return best


def five_valid(shape=(64, 257)):
    """Where both forward maps of the rig of five_rectifier are valid (numpy restatement)."""
    H, W = shape
    tr = lio.stereo_rectify(*five_rig(shape))
    both = np.ones(shape, bool)
    shares = []
    for m in (0, 1):
        v = rc.valid_of(rc.map_restate(tr[f"K{m}"], tr[f"dist{m}"], tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], H, W), H, W)
        shares.append(float(v.mean()))
        both &= v
    return both, shares


def case_valid_rect():
    from localexpstereo_amd import stereo
    rng = np.random.default_rng(5)
    for i in range(200):
        H, W = int(rng.integers(1, 8)), int(rng.integers(1, 10))
        mask = rng.random((H, W)) < (0.5 + 0.45 * rng.random())
        if i < 3:
            mask[:] = (False, True, True)[i]                                  # empty, full
        got, want = stereo.largest_rect(mask), brute_rect(mask)
        assert got == want, (mask.astype(int).tolist(), got, want)
    both, shares = five_valid()
    H, W = both.shape
    y0, x0, h, w = stereo.largest_rect(both)
    print("rig five at 64 x 257: valid shares", shares, "both", float(both.mean()), "rectangle (y0, x0, h, w)", (y0, x0, h, w))
    assert 0.0 < shares[0] < 1.0 and 0.0 < shares[1] < 1.0
    assert h > 0 and w > 0 and both[y0:y0 + h, x0:x0 + w].all()
    for ya, xa, yb, xb in ((y0 - 1, x0, y0 + h, x0 + w), (y0, x0 - 1, y0 + h, x0 + w), (y0, x0, y0 + h + 1, x0 + w), (y0, x0, y0 + h, x0 + w + 1)):
        assert ya < 0 or xa < 0 or yb > H or xb > W or not both[ya:yb, xa:xb].all(), (ya, xa, yb, xb)
    return (y0, x0, h, w)


# ------------------------------------------------------------------------------------------------ device harness
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def dev_inv(lib, K, dist, R, f, cx, cy, Hs, Ws, steps, tol):
    out = pc.Guarded(lib, Hs * Ws * 2)
    api.unrectify_map(api.camera(K, dist), R, f, cx, cy, out.ptr, Hs, Ws, steps=steps, tol=tol, lib=lib)
    return out.check().view(F).reshape(Hs, Ws, 2)


def dev_labels(lib, labels, drop, inv, g, z_max=None, skip=None):
    """-> dict of the four outputs; `skip`: the output whose pointer is NULL (its buffer must keep the guard pattern)"""
    H, W = labels.shape[:2]
    Hs, Ws = inv.shape[:2]
    lb, mp = pc.Guarded(lib, labels.size, fill=labels), pc.Guarded(lib, inv.size, fill=inv)
    dr = pc.Guarded(lib, drop.size, words=False, fill=drop) if drop is not None else None
    bufs = dict(points=pc.Guarded(lib, Hs * Ws * 3), normals=pc.Guarded(lib, Hs * Ws * 3), disparity=pc.Guarded(lib, Hs * Ws), valid=pc.Guarded(lib, Hs * Ws, words=False))
    ptr = {k: (None if k == skip else b.ptr) for k, b in bufs.items()}
    api.unrectify_labels(lb.ptr, H, W, dr.ptr if dr is not None else None, mp.ptr, Hs, Ws, g["M"], g["f"], g["cx"], g["cy"], g["doffs"], g["baseline"], ptr["valid"],
                         points_dev_ptr=ptr["points"], normals_dev_ptr=ptr["normals"], disparity_dev_ptr=ptr["disparity"], z_max=z_max, lib=lib)
    out = {}
    for k, b in bufs.items():
        o = b.check()
        if k == skip:
            assert (o == b.g).all(), f"{k}: a NULL output was written"
            continue
        out[k] = o.reshape(Hs, Ws) if k == "valid" else o.view(F).reshape((Hs, Ws, 3) if k != "disparity" else (Hs, Ws))
    assert same(lb.check().view(F).reshape(labels.shape), labels) and same(mp.check().view(F).reshape(inv.shape), inv)
    assert dr is None or same(dr.check().reshape(drop.shape), drop)
    return out


# ------------------------------------------------------------------------------------------------ 6. the map kernel
def case_map_kernel(lib, shape):
    Hs, Ws = shape
    n = 0
    for name in INV_RIGS:
        for args in inv_inputs(name, shape):
            for steps, tol in itertools.product(STEPS, TOLS):
                got, want = dev_inv(lib, *args, Hs, Ws, steps, tol), inv_restate(*args, Hs, Ws, steps, tol)
                assert same(got, want), f"inverse map {Hs}x{Ws} {name} steps {steps} tol {tol}: {first_diff(got, want)}"
                n += 1
    return n


# ------------------------------------------------------------------------------------------------ 7. the labels kernel
def case_labels_kernel(lib, shape):
    g = five_geometry(shape)
    n = 0
    for size in SIZES:
        lab, drop, z_max = label_inputs(size, shape)
        for kind in INV_KINDS:
            inv = inv_input(shape, size, kind)
            variants = [(dr, zm, None) for dr, zm in itertools.product((None, drop), (None, z_max))]
            if kind == "edges":
                variants += [(drop, z_max, k) for k in OUTPUTS[:3]]              # each optional output NULL in turn
            for dr, zm, skip in variants:
                got, want = dev_labels(lib, lab, dr, inv, g, zm, skip), lab_restate(lab, dr, inv, z_max=zm, **g)
                for k, o in got.items():
                    assert same(o, want[k]), f"labels {shape} from {size} {kind} drop {dr is not None} z_max {zm} without {skip}: {k}: {first_diff(o, want[k])}"
                n += 1
    return n


# ------------------------------------------------------------------------------------------------ 8. the identity rig
def identity_rectifier(lib, shape, **kw):
    """A power-of-two focal length, dyadic centres, doffs and baseline: every operation of both directions is exact."""
    from localexpstereo_amd import stereo
    H, W = shape
    K0, K1 = rc.pinhole(128.0, 128.0, 0.5 * (W - 1), 0.5 * (H - 1)), rc.pinhole(128.0, 128.0, 0.5 * (W - 1) + 4.0, 0.5 * (H - 1))      # doffs = 4
    return stereo.Rectifier(K0, (), K1, (), np.eye(3), (-0.25, 0.0, 0.0), raw_size=shape, device=_dev(lib), lib=lib, **kw)


def case_identity(lib, shape=(17, 67)):
    """With the identity rig unrectify IS reproject -- points, normals and the valid byte, byte for byte, both views, with a drop map and a
    z_max -- and to_raw returns its input."""
    import torch
    H, W = shape
    rect = identity_rectifier(lib, shape)
    assert rect.transform["doffs"] == 4.0 and rect.transform["baseline"] == 0.25
    for m in (0, 1):
        assert same(rect.inverse_maps[m].cpu().numpy(), rc.identity_map(H, W)), m
    rng = np.random.default_rng(31)
    lab = np.zeros((H, W, 4), F)                                                # small dyadic entries; D = d + 4 takes both signs
    lab[..., 0], lab[..., 1], lab[..., 2] = rng.integers(-4, 5, (H, W)) / 8.0, rng.integers(-4, 5, (H, W)) / 8.0, rng.integers(-64, 160, (H, W)) / 4.0
    drop = (rng.random((H, W)) < 0.2).astype(np.uint8) * 255
    im = rc.source(shape, 3, seed=2)
    e = api.HipCostVolumeEnergy.naive(im, im, windR=2, max_disp=63.0, lib=lib, filter="")
    n = 0
    try:
        for m, dr, zm in itertools.product((0, 1), (None, drop), (None, 4.0)):
            want = [t.cpu().numpy() for t in e.reproject(lab, rect.calib, mode=m, drop=dr, z_max=zm, device=torch.device(_dev(lib)))]
            e.synchronize()
            got = rect.unrectify(lab, viewMode=m, drop=dr, z_max=zm)
            assert 0 < (want[2] != 0).sum() < H * W
            for k, w in zip(("points", "normals"), want):
                assert same(got[k], w), f"view {m} {k}: {first_diff(got[k], w)}"
            assert same(got["valid"], want[2] != 0) and same(got["depth"], want[0][..., 2])
            n += 1
    finally:
        e.close()
    for src in (im, np.ascontiguousarray(im[..., 0])):
        for interp in api.INTERP_NAMES:
            out, valid = rect.to_raw(src, viewMode=1, interp=interp)
            assert same(out, src) and valid.all(), (src.shape, interp)
    # device in, device out, the same bytes
    out, valid = rect.to_raw(torch.from_numpy(im.copy()).to(_dev(lib)))
    assert torch.is_tensor(out) and same(out.cpu().numpy(), im) and bool(valid.all())
    host, tens = rect.unrectify(lab, drop=drop), rect.unrectify(torch.from_numpy(lab.copy()).to(_dev(lib)), drop=torch.from_numpy(drop.copy()).to(_dev(lib)))
    assert sorted(tens) == sorted(host) == ["depth", "disparity", "normals", "points", "valid"]
    for k, t in tens.items():
        assert torch.is_tensor(t) and same(np.ascontiguousarray(t.cpu().numpy()), np.ascontiguousarray(host[k])), k
    return n


# ------------------------------------------------------------------------------------------------ 9. refusals
def case_refusals(lib):
    L = api.load(lib)
    vp = C.c_void_p
    H, W, Hs, Ws = 3, 5, 4, 6
    sizes = dict(lab=(H * W * 4, True), drop=(H * W, False), inv=(Hs * Ws * 2, True), pts=(Hs * Ws * 3, True), nrm=(Hs * Ws * 3, True), dsp=(Hs * Ws, True),
                 val=(Hs * Ws, False))
    bufs = {k: pc.Guarded(lib, n, words=w) for k, (n, w) in sizes.items()}
    p = {k: b.ptr for k, b in bufs.items()}
    cam = api.camera(rc.pinhole(10.0, 10.0, 2.0, 1.0), rc.DIST8)
    eye = (C.c_double * 9)(*np.eye(3).reshape(9))
    ARG, UNSUP = api.LES_HIP_ERR_ARG, api.LES_HIP_ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")

    def umap(cam_=cam, R=eye, f=10.0, steps=20, tol=1e-3, d_map=p["inv"], Hs_=Hs, Ws_=Ws):
        return L.les_hip_unrectify_map(C.byref(cam_) if cam_ is not None else None, R, f, 2.0, 1.0, steps, tol, vp(d_map) if d_map else None, Hs_, Ws_, 0, None)

    def ulab(lab=p["lab"], H_=H, W_=W, drop=p["drop"], inv=p["inv"], Hs_=Hs, Ws_=Ws, M=eye, f=10.0, baseline=1.0, val=p["val"]):
        o = lambda a: vp(a) if a else None
        return L.les_hip_unrectify_labels(o(lab), H_, W_, o(drop), o(inv), Hs_, Ws_, M, f, 2.0, 1.0, 0.5, baseline, 0.0, o(p["pts"]), o(p["nrm"]), o(p["dsp"]), o(val),
                                          0, None)

    cams = [api.camera(rc.pinhole(fx, fy, 2.0, 1.0)) for fx, fy in ((0.0, 10.0), (10.0, -1.0), (nan, 10.0), (10.0, inf))]
    refused = [umap(cam_=None), umap(R=None), umap(d_map=None), umap(Hs_=0), umap(Ws_=0), umap(Hs_=-2), umap(Ws_=-1), umap(f=0.0), umap(f=nan), umap(f=inf),
               umap(f=-1.0), umap(d_map=p["inv"] + 4), umap(steps=0), umap(steps=-1), umap(steps=65), umap(tol=0.0), umap(tol=-1e-3), umap(tol=nan)]
    refused += [umap(cam_=c) for c in cams]
    refused += [ulab(lab=None), ulab(inv=None), ulab(M=None), ulab(val=None), ulab(H_=0), ulab(W_=0), ulab(H_=-1), ulab(Hs_=0), ulab(Ws_=0), ulab(Ws_=-3),
                ulab(inv=p["inv"] + 4), ulab(lab=p["lab"] + 4), ulab(f=0.0), ulab(f=nan), ulab(f=inf), ulab(baseline=0.0), ulab(baseline=-1.0), ulab(baseline=nan),
                ulab(baseline=inf)]
    assert refused == [ARG] * len(refused), refused
    assert L.les_hip_last_error() != b""
    big = [umap(Hs_=65536), ulab(Hs_=65536), ulab(H_=46341, W_=46341), ulab(H_=1 << 16, W_=1 << 15), ulab(H_=2, W_=2 ** 30)]      # the grid; H W >= 2^31
    assert big == [UNSUP] * len(big), big
    for k, b in bufs.items():
        assert (b.check() == b.g).all(), f"a refused call wrote {k}"
    for call in (lambda: api.unrectify_map(cam, np.eye(3), 10.0, 2.0, 1.0, p["inv"], Hs, Ws, steps=0, lib=lib),
                 lambda: api.unrectify_labels(p["lab"], H, W, None, p["inv"], Hs, Ws, np.eye(3), 10.0, 2.0, 1.0, 0.5, 0.0, p["val"], lib=lib)):
        try:
            call()
            raise AssertionError("accepted")
        except api.LesHipError as ex:
            assert f"error {ARG}" in str(ex)
    # a good call still works afterwards: the map first, then the labels through it (the label buffer holds the guard pattern: NaN labels, all invalid)
    assert umap() == api.LES_HIP_OK and ulab() == api.LES_HIP_OK
    assert not (bufs["inv"].check() == bufs["inv"].g).all() and (bufs["val"].check() == 0).all()
    return len(refused) + len(big)


# ------------------------------------------------------------------------------------------------ 10. independence
def case_independence(lib, shape=(17, 67), size=(9, 300)):
    """Changing one label changes only the raw pixels whose (yi, xi) is that pixel."""
    rng = np.random.default_rng(23)
    inv = np.stack([rng.uniform(140.0, 150.0, shape), rng.uniform(2.0, 6.0, shape)], -1).astype(F)          # dense around the label that changes
    g = five_geometry(shape)
    lab = np.zeros(size + (4,), F)
    lab[..., 0], lab[..., 1], lab[..., 2] = rng.uniform(-0.01, 0.01, size), rng.uniform(-0.01, 0.01, size), rng.uniform(20.0, 40.0, size) - g["doffs"]
    y0, x0 = 4, 145
    lab2 = lab.copy()
    lab2[y0, x0, :3] = (0.02, -0.03, 55.0)
    k = lab_parts(lab, None, inv, **g)[1]
    touched = k["inside"] & (k["taps"][0] == y0) & (k["taps"][1] == x0)
    a, b = dev_labels(lib, lab, None, inv, g), dev_labels(lib, lab2, None, inv, g)
    assert (a["valid"] == 255).all() and (b["valid"] == 255).all()
    changed = (a["disparity"] != b["disparity"]) | (a["points"] != b["points"]).any(-1) | (a["normals"] != b["normals"]).any(-1)
    assert touched.any() and not touched.all() and same(changed, touched), (int(changed.sum()), int(touched.sum()))
    return int(changed.sum()), int(touched.sum())


# ------------------------------------------------------------------------------------------------ 11. crop
def five_rig(shape):
    """K0, dist0, K1, dist1, R, T of rectify_cases.map_inputs("five", shape)."""
    H, W = shape
    f, cx, cy = 0.6 * max(H, W) + 1.0, 0.5 * (W - 1), 0.5 * (H - 1)
    return (rc.pinhole(1.02 * f, 0.98 * f, cx + 1.3, cy - 0.7), rc.DIST8, rc.pinhole(0.97 * f, 1.01 * f, cx - 0.9, cy + 1.1), rc.DIST8B, rc.rot(5.0, -5.0, 5.0),
            (-1.0, 0.05, -0.03))


def case_crop(lib, shape=(64, 257)):
    from localexpstereo_amd import stereo
    H, W = shape
    rect = stereo.Rectifier(*five_rig(shape), raw_size=shape, device=_dev(lib), lib=lib, tol=1e-6)
    rawL, rawR = rc.source(shape, 3, seed=3), rc.source(shape, 3, seed=4)
    full = rect.rectify(rawL, rawR)
    assert not full["validL"].all() and not full["validR"].all()
    both = five_valid(shape)[0]
    assert same(full["validL"] & full["validR"], both)
    best = rect.valid_rect()
    assert best == stereo.largest_rect(both) and best[2] > 0 and best[3] > 0
    for r in ((3, 10, 20, 100), best, None):
        c = rect.crop(r)
        y0, x0, h, w = best if r is None else r
        got = c.rectify(rawL, rawR)
        for k in ("imL", "imR", "validL", "validR"):
            assert same(got[k], np.ascontiguousarray(full[k][y0:y0 + h, x0:x0 + w])), (r, k)
        if r != (3, 10, 20, 100):
            assert got["validL"].all() and got["validR"].all()
        tr, tc = rect.transform, c.transform
        assert c.size == (h, w) and c.raw_size == rect.raw_size
        assert (tc["cx0"], tc["cx1"], tc["cy"]) == (tr["cx0"] - x0, tr["cx1"] - x0, tr["cy"] - y0) and all(tc[k] == tr[k] for k in ("f", "doffs", "baseline"))
        assert (c.calib.cx, c.calib.cy) == (F(tr["cx0"] - x0), F(tr["cy"] - y0))
        assert (c.calib.f, c.calib.doffs, c.calib.baseline) == (rect.calib.f, rect.calib.doffs, rect.calib.baseline)
        assert (rect.calib.cx, rect.calib.cy) == (F(tr["cx0"]), F(tr["cy"]))             # the parent is untouched
    # the crop's way back: its inverse maps come from the shifted intrinsics, and unrectify works on it unchanged
    y0, x0, h, w = best
    c = rect.crop()
    tc = c.transform
    rng = np.random.default_rng(41)
    lab = np.zeros((h, w, 4), F)
    lab[..., 0], lab[..., 2] = rng.uniform(-0.05, 0.05, (h, w)), rng.uniform(5.0, 30.0, (h, w))
    for m in (0, 1):
        inv = inv_restate(tc[f"K{m}"], tc[f"dist{m}"], tc[f"R{m}"], tc["f"], tc[f"cx{m}"], tc["cy"], H, W, 20, 1e-6)
        assert same(c.inverse_maps[m].cpu().numpy(), inv), m
        want = lab_restate(lab, None, inv, tc[f"R{m}"].T, tc["f"], tc[f"cx{m}"], tc["cy"], tc["doffs"], tc["baseline"])
        got = c.unrectify(lab, viewMode=m)
        for k in OUTPUTS[:3]:
            assert same(got[k], want[k]), (m, k, first_diff(got[k], want[k]))
        assert same(got["valid"], want["valid"] == 255) and got["valid"].any() and not got["valid"].all()
    for bad in ((0, 0, 0, 5), (-1, 0, 3, 3), (0, 0, H + 1, 3), (2, 250, 3, 8)):
        try:
            rect.crop(bad)
            raise AssertionError(f"accepted {bad}")
        except ValueError:
            pass
    return best


# ------------------------------------------------------------------------------------------------ 12. the driver
# Measured on the CPU simulator build with the numpy restatements of both directions (case_driver(sim_lib, restated=True)): bad-1.0 of the one-view
# wta on the rectified grid 15.36 % of 11 462 pixels, on the raw grid 14.91 % of 11 106 pixels (76.0 % of the 14 688 raw pixels lie inside the
# rectified frame): a difference of 0.45 points; with the labels shifted by +3 disparities 99.38 %.  The margin is that difference plus one
# percentage point: the rates move by single pixels on a crop this small.
DRIVER_DIFFERENCE = 0.004530
DRIVER_MARGIN = DRIVER_DIFFERENCE + 0.01


def wta_labels(lib, imL, imR):
    """The one-view wta label map of rectify_cases.wta_bad1 (the same settings)."""
    from localexpstereo_amd import stereo
    device = _dev(lib)
    H, W = imL.shape[:2]
    tl, tr = lio.build_volumes(imL, imR, 64, device=device, lib=lib)
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=cv.WINDR, th_col=0.5, max_disp=63.0, volumes_on_device=True, shape=(64, H, W), lib=lib)
    try:
        st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=0.5, windR=cv.WINDR, th_col=0.5), device=device, seed=3, device_cuts="none")
        st.concurrent_views = False
        for u, t in zip(cv.UNITS, cv.TABLE):
            st.addLayer(u, t)
        lab, _ = st.wta((0,))
    finally:
        e.close()
    del tl, tr
    return np.ascontiguousarray(lab, F)


def case_driver(lib, restated=False):
    """The raw cones pair: Rectifier.data -> one-view wta -> unrectify, against the truth's disparity sent through the numpy restatement of the
    labels definition as fronto-parallel labels.  restated: the numpy restatements in the place of the Rectifier (the measurement of the margin).
    Measured (simulator build, restatements): see DRIVER_DIFFERENCE."""
    from localexpstereo_amd import stereo
    s = cones_setup()
    tr, gt = s["transform"], s["gt"]
    H, W = gt.shape
    Hs, Ws = rc.RAW_SIZE
    K, dist, R0, f, cx, cy = cones_views()[0]
    geom = dict(M=R0.T, f=f, cx=cx, cy=cy, doffs=tr["doffs"], baseline=tr["baseline"])
    inv = inv_restate(K, dist, R0, f, cx, cy, Hs, Ws)
    known = (gt > 0) & np.isfinite(gt)
    truth_lab = np.zeros((H, W, 4), F)
    truth_lab[..., 2] = np.where(known, gt, 0.0)
    truth = lab_restate(truth_lab, (~known).astype(np.uint8), inv, **geom)
    inside = float((lab_parts(truth_lab, None, inv, **geom)[1]["inside"]).mean())
    if restated:
        imL, imR, validL, _ = rc.cones_restated()
        unrect = lambda lab: {k: (v == 255 if k == "valid" else v) for k, v in lab_restate(lab, None, inv, **geom).items()}
    else:
        rect = rc.cones_rectifier(lib)
        data = rect.data(s["rawL"], s["rawR"], 64)
        imL, imR, validL = data["imL"], data["imR"], data["nonocc"]
        assert same(rect.inverse_maps[0].cpu().numpy(), inv)
        unrect = lambda lab: rect.unrectify(lab, viewMode=0)
    lab = wta_labels(lib, imL, imR)
    rate_rect = float((np.abs(stereo.disparities(lab) - gt)[known & validL] > 1.0).mean())

    def raw_rate(labels):
        got = unrect(labels)
        mask = got["valid"] & (truth["valid"] == 255)
        return float((np.abs(got["disparity"] - truth["disparity"])[mask] > 1.0).mean()), int(mask.sum())

    rate_raw, pixels = raw_rate(lab)
    shifted = lab.copy()
    shifted[..., 2] += 3.0
    rate_shifted, _ = raw_rate(shifted)
    out = dict(pixels=pixels, raw_pixels=Hs * Ws, inside=inside, rectified=rate_rect, raw=rate_raw, shifted=rate_shifted)
    print("one-view wta on the raw cones pair, bad-1.0:", out, "margin", DRIVER_MARGIN)
    assert pixels >= 8000, out
    assert abs(rate_raw - rate_rect) <= DRIVER_MARGIN, out
    assert rate_shifted > rate_raw + DRIVER_MARGIN, out
    return out
