"""Cases of tests/test_rectify.py: the rectification front end (csrc/les_rectify.h: les_hip_rectify_map, les_hip_remap; api.rectify_map / api.remap;
io.stereo_rectify; stereo.Rectifier) on the CPU simulator build and on the MI355X.

The definitions, restated from csrc/les_rectify.h.  Conventions: the rig is X1 = R X0 + T (one point in the left and the right raw camera
frame); pixel centres sit at integer coordinates; doffs = cx1 - cx0; baseline = |T|.
  camera    (X, Y, Z) -> x' = X / Z, y' = Y / Z, r2 = x'^2 + y'^2, rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
            x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2), y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y', u = fx x'' + cx, v = fy y'' + cy.
  map       every operation fp64, rounded, in this order: xr = (x - cx) / f, yr = (y - cy) / f; X = (M0 xr + M1 yr) + M2, Y, Z alike; Z > 0 or
            (NaN, NaN); xp = X / Z, yp = Y / Z, xx = xp xp, yy = yp yp, xy = xp yp, r2 = xx + yy; num = 1 + r2 (k1 + r2 (k2 + r2 k3)),
            den = 1 + r2 (k4 + r2 (k5 + r2 k6)); den finite and != 0 or (NaN, NaN); rad = num / den; xd = (xp rad + (2 p1) xy) + p2 (r2 + 2 xx),
            yd = (yp rad + p1 (r2 + 2 yy)) + (2 p2) xy; u = fx xd + cxr, v = fy yd + cyr, each rounded to f32 once; a NaN in either: (NaN, NaN).
  remap     valid iff 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1 (a NaN fails, -0 passes); invalid: 0 in every channel, valid 0.  With U, V the
            coordinates as fp64: nearest: the tap (min(floor(U + 0.5), Ws - 1), min(floor(V + 0.5), Hs - 1)); linear: x0 = floor(U), tx = U - x0,
            x1 = min(x0 + 1, Ws - 1), rows alike, s = (1 - ty) ((1 - tx) p00 + tx p01) + ty ((1 - tx) p10 + tx p11); cubic: taps x0 - 1 .. x0 + 2
            clamped, w0 = ((-0.5 t + 1) t - 0.5) t, w1 = ((1.5 t - 2.5) t) t + 1, w2 = ((-1.5 t + 2) t + 0.5) t, w3 = ((0.5 t - 0.5) t) t,
            h_j = ((wx0 p_j0 + wx1 p_j1) + wx2 p_j2) + wx3 p_j3, s = ((wy0 h_0 + wy1 h_1) + wy2 h_2) + wy3 h_3; out = floor(s + 0.5) clamped to 0 .. 255.

References, none of them the code under test: the vectorised numpy restatements below, themselves held to literal per-pixel loops; the camera
model `project`, written once more in the issue's form for the geometric test.  Tolerances: none for the kernels -- every output is compared
bit for bit (fp64 add, multiply, divide and floor are correctly rounded on both sides, the order is fixed, nothing is contracted, and each
coordinate is rounded to f32 once).  The transform is held to 1e-9 px (fp64 on coordinates of order 1e3 through a few dozen operations: an
expected error of order 1e-11, with two orders of margin) and the identity rig to 1e-15.

Shapes: destinations (1, 1), (3, 5), (17, 67), (64, 257) -- the widths straddle a workgroup of 256 --, sources (9, 300) and (1, 1), 1 and 3
channels, all three interpolations."""
import functools
import math

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import io as lio
from tests import costvol_cases as cc
from tests import crossview_cases as cv
from tests import pyramid_cases as pc

F, D = np.float32, np.float64
QNAN = np.uint32(0x7FC00000).view(F)
SHAPES = [(1, 1), (3, 5), (17, 67), (64, 257)]
SOURCES = [(9, 300), (1, 1)]
CHANNELS = (1, 3)
INTERPS = (0, 1, 2)
GUARD = pc.GUARD_BYTE


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def first_diff(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return f"{len(bad)} elements differ, first at {bad[0].tolist() if len(bad) else None}"


# ------------------------------------------------------------------------------------------------ geometry helpers (test only)
def rot(rx, ry, rz):
    """Rz Ry Rx of angles in degrees."""
    a, b, c = (math.radians(v) for v in (rx, ry, rz))
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pinhole(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def distort(dist, x, y):
    """The camera model's distortion of normalised coordinates, in the issue's form."""
    k1, k2, p1, p2, k3, k4, k5, k6 = np.concatenate([np.asarray(dist, D), np.zeros(8 - len(dist))])
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def project(K, dist, P):
    """Points N x 3 of the camera's frame -> pixels N x 2."""
    xd, yd = distort(dist, P[:, 0] / P[:, 2], P[:, 1] / P[:, 2])
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


# ------------------------------------------------------------------------------------------------ restatement, numpy
def _coefficients(dist):
    return (D(v) for v in np.concatenate([np.asarray(dist, D).reshape(-1), np.zeros(8)])[:8])


def map_parts(K, dist, M, f, cx, cy, H, W):
    """-> (map H x W x 2 f32, Z, den: the fp64 intermediates the NaN branches test)"""
    M = np.asarray(M, D).reshape(9)
    k1, k2, p1, p2, k3, k4, k5, k6 = _coefficients(dist)
    fx, fy, cxr, cyr = D(K[0, 0]), D(K[1, 1]), D(K[0, 2]), D(K[1, 2])
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        xr, yr = (xs.astype(D) - D(cx)) / D(f), (ys.astype(D) - D(cy)) / D(f)
        X = (M[0] * xr + M[1] * yr) + M[2]
        Y = (M[3] * xr + M[4] * yr) + M[5]
        Z = (M[6] * xr + M[7] * yr) + M[8]
        xp, yp = X / Z, Y / Z
        xx, yy, xy = xp * xp, yp * yp, xp * yp
        r2 = xx + yy
        num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
        rad = num / den
        xd = (xp * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (yp * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        u, v = (fx * xd + cxr).astype(F), (fy * yd + cyr).astype(F)
        ok = (Z > 0.0) & np.isfinite(den) & (den != 0.0) & ~np.isnan(u) & ~np.isnan(v)
    out = np.full((H, W, 2), QNAN, F)
    out[ok, 0], out[ok, 1] = u[ok], v[ok]
    return out, Z, den


def map_restate(K, dist, M, f, cx, cy, H, W):
    return map_parts(K, dist, M, f, cx, cy, H, W)[0]


def map_loop(K, dist, M, f, cx, cy, H, W):
    """The same by a literal per-pixel transcription (numpy's float64 scalars: IEEE doubles, and a division by zero is no exception)."""
    M = [D(v) for v in np.asarray(M, D).reshape(9)]
    k1, k2, p1, p2, k3, k4, k5, k6 = _coefficients(dist)
    fx, fy, cxr, cyr, f, cx, cy = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy))
    out = np.full((H, W, 2), QNAN, F)
    one, two = D(1.0), D(2.0)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                xr, yr = (D(x) - cx) / f, (D(y) - cy) / f
                X = (M[0] * xr + M[1] * yr) + M[2]
                Y = (M[3] * xr + M[4] * yr) + M[5]
                Z = (M[6] * xr + M[7] * yr) + M[8]
                if not Z > 0.0:
                    continue
                xp, yp = X / Z, Y / Z
                xx, yy, xy = xp * xp, yp * yp, xp * yp
                r2 = xx + yy
                num = one + r2 * (k1 + r2 * (k2 + r2 * k3))
                den = one + r2 * (k4 + r2 * (k5 + r2 * k6))
                if not np.isfinite(den) or den == 0.0:
                    continue
                rad = num / den
                xd = (xp * rad + (two * p1) * xy) + p2 * (r2 + two * xx)
                yd = (yp * rad + p1 * (r2 + two * yy)) + (two * p2) * xy
                u, v = F(fx * xd + cxr), F(fy * yd + cyr)
                if u == u and v == v:
                    out[y, x] = (u, v)
    return out


def cubic_weights(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t]


def valid_of(mp, Hs, Ws):
    U, V = mp[..., 0].astype(D), mp[..., 1].astype(D)
    with np.errstate(invalid="ignore"):
        return (U >= 0.0) & (U <= D(Ws - 1)) & (V >= 0.0) & (V <= D(Hs - 1))


def tap_indices(mp, Hs, Ws, interp):
    """-> (ok, list of (rows, cols) H x W int arrays of every tap of the valid pixels; garbage where not ok)"""
    ok = valid_of(mp, Hs, Ws)
    U, V = np.where(ok, mp[..., 0].astype(D), 0.0), np.where(ok, mp[..., 1].astype(D), 0.0)
    if interp == 0:
        return ok, [(np.minimum(np.floor(V + 0.5).astype(np.int64), Hs - 1), np.minimum(np.floor(U + 0.5).astype(np.int64), Ws - 1))]
    x0, y0 = np.floor(U).astype(np.int64), np.floor(V).astype(np.int64)
    offs = (0, 1) if interp == 1 else (-1, 0, 1, 2)
    return ok, [(np.clip(y0 + dy, 0, Hs - 1), np.clip(x0 + dx, 0, Ws - 1)) for dy in offs for dx in offs]


def remap_parts(src, mp, interp):
    """src Hs x Ws x C u8, mp H x W x 2 f32 -> (dst H x W x C u8, valid H x W u8, s: the unrounded fp64 sums, None for nearest)"""
    Hs, Ws, C = src.shape
    ok, taps = tap_indices(mp, Hs, Ws, interp)
    U, V = np.where(ok, mp[..., 0].astype(D), 0.0), np.where(ok, mp[..., 1].astype(D), 0.0)
    p = src.astype(D)
    s = None
    if interp == 0:
        dst = src[taps[0][0], taps[0][1]].copy()
    else:
        tx, ty = (U - np.floor(U))[..., None], (V - np.floor(V))[..., None]
        if interp == 1:
            p00, p01, p10, p11 = (p[r, c] for r, c in taps)
            top = (1.0 - tx) * p00 + tx * p01
            bot = (1.0 - tx) * p10 + tx * p11
            s = (1.0 - ty) * top + ty * bot
        else:
            wx, wy = cubic_weights(tx), cubic_weights(ty)
            for j in range(4):
                q = [p[r, c] for r, c in taps[4 * j:4 * j + 4]]
                h = ((wx[0] * q[0] + wx[1] * q[1]) + wx[2] * q[2]) + wx[3] * q[3]
                s = wy[0] * h if j == 0 else s + wy[j] * h
        dst = np.clip(np.floor(s + 0.5), 0.0, 255.0).astype(np.uint8)
    dst[~ok] = 0
    return dst, ok.astype(np.uint8), s


def remap_restate(src, mp, interp):
    return remap_parts(src, mp, interp)[:2]


def remap_loop(src, mp, interp):
    """The same by a literal per-pixel transcription (Python floats are IEEE doubles)."""
    Hs, Ws, C = src.shape
    H, W = mp.shape[:2]
    dst, valid = np.zeros((H, W, C), np.uint8), np.zeros((H, W), np.uint8)
    rnd = lambda s: int(min(max(math.floor(s + 0.5), 0), 255))
    cl = lambda i, n: min(max(i, 0), n - 1)
    for y in range(H):
        for x in range(W):
            U, V = float(mp[y, x, 0]), float(mp[y, x, 1])
            if not (U >= 0.0 and U <= float(Ws - 1) and V >= 0.0 and V <= float(Hs - 1)):
                continue
            valid[y, x] = 1
            if interp == 0:
                dst[y, x] = src[min(math.floor(V + 0.5), Hs - 1), min(math.floor(U + 0.5), Ws - 1)]
                continue
            x0, y0 = math.floor(U), math.floor(V)
            tx, ty = U - x0, V - y0
            for k in range(C):
                px = lambda yy, xx: float(src[cl(yy, Hs), cl(xx, Ws), k])
                if interp == 1:
                    top = (1.0 - tx) * px(y0, x0) + tx * px(y0, x0 + 1)
                    bot = (1.0 - tx) * px(y0 + 1, x0) + tx * px(y0 + 1, x0 + 1)
                    s = (1.0 - ty) * top + ty * bot
                else:
                    wx, wy = cubic_weights(tx), cubic_weights(ty)
                    h = [((wx[0] * px(y0 - 1 + j, x0 - 1) + wx[1] * px(y0 - 1 + j, x0)) + wx[2] * px(y0 - 1 + j, x0 + 1)) + wx[3] * px(y0 - 1 + j, x0 + 2)
                         for j in range(4)]
                    s = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3]
                dst[y, x, k] = rnd(s)
    return dst, valid


# ------------------------------------------------------------------------------------------------ inputs
RIGS = ("identity", "five", "behind", "pole", "zero", "overflow")
DIST8 = (0.21, -0.13, 0.004, -0.003, 0.05, 0.11, -0.07, 0.02)               # all eight non-zero
DIST8B = (-0.17, 0.09, -0.002, 0.005, -0.03, 0.06, 0.04, -0.01)


@functools.lru_cache(maxsize=None)
def map_inputs(name, shape):
    """-> list of (K, dist, M, f, cx, cy): the views of rig `name` for a destination of `shape`.  The rectified focal length is 0.6 of the longer
    side, so that the rays span about +-40 degrees at every shape."""
    H, W = shape
    f, cx, cy = 0.6 * max(H, W) + 1.0, 0.5 * (W - 1), 0.5 * (H - 1)
    K0, K1 = pinhole(1.02 * f, 0.98 * f, cx + 1.3, cy - 0.7), pinhole(0.97 * f, 1.01 * f, cx - 0.9, cy + 1.1)
    eye = np.eye(3)
    if name == "identity":                   # a power-of-two focal length and dyadic centres: every operation is exact, the map is the identity map
        return [(pinhole(128.0, 128.0, cx, cy), (), eye, 128.0, cx, cy)]
    if name == "five":
        tr = lio.stereo_rectify(K0, DIST8, K1, DIST8B, rot(5.0, -5.0, 5.0), (-1.0, 0.05, -0.03))
        return [(tr[f"K{m}"], tr[f"dist{m}"], tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"]) for m in (0, 1)]
    if name == "behind":                     # Z = -sin(100 deg) xr + cos(100 deg): in front only left of xr = -0.18
        return [(K0, DIST8[:5], rot(0.0, 100.0, 0.0), f, cx, cy)]
    if name == "pole":                       # 1 - 4 r2 = 0 on the circle r = 0.5, inside the field of view
        return [(K0, (0.1, 0, 0, 0, 0, -4.0), eye, f, cx, cy)]
    if name == "zero":                       # pixel (2, 0): xr = 1, yr = 0, r2 = 1, den = 1 + 1 (-1) = 0 exactly
        return [(K0, (0.1, 0, 0, 0, 0, -1.0), eye, 2.0, 0.0, 0.0)]
    if name == "overflow":                   # pixel (4, 0): r2 = 4, r2 k6 = +inf
        return [(K0, (0.1, 0, 0, 0, 0, 0, 0, 1e308), eye, 2.0, 0.0, 0.0)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def source(size, channels, seed=0):
    """Random bytes, a third of them pushed to 0 or 255 so that the cubic's over- and undershoot reach the clamp."""
    rng = np.random.default_rng(900 + 7 * size[0] + size[1] + channels + seed)
    im = rng.integers(0, 256, size + (channels,), dtype=np.uint8)
    ends = rng.integers(0, 6, size + (channels,))
    im[ends == 0], im[ends == 1] = 0, 255
    im.setflags(write=False)
    return im


MAPS = ("integers", "edges", "random", "constant")


def edge_pool(n):
    """The coordinates a hand-built map holds along an axis of n source pixels."""
    last = F(n - 1)
    vals = [0.0, last, -0.0, -1e-7, -1e-45, np.nextafter(last, F(np.inf), dtype=F), last + F(1e-3) * max(last, F(1)), 0.5, 1.5, -0.5, last - F(0.5),
            last - F(1.5), last + F(0.5), np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 0.25 * float(last), 0.75 * float(last)]
    return np.array(vals, F)


@functools.lru_cache(maxsize=None)
def hand_map(shape, size, kind):
    H, W = shape
    Hs, Ws = size
    rng = np.random.default_rng(1000 + 13 * H + W + 5 * Hs + Ws)
    mp = np.zeros((H, W, 2), F)
    if kind == "integers":
        mp[..., 0], mp[..., 1] = rng.integers(0, Ws, (H, W)), rng.integers(0, Hs, (H, W))
    elif kind == "edges":                    # every pair of pool values while the map has room, the rest random pairs
        pu, pv = edge_pool(Ws), edge_pool(Hs)
        iu, iv = rng.integers(0, len(pu), H * W), rng.integers(0, len(pv), H * W)
        n = min(H * W, len(pu) * len(pv))
        order = rng.permutation(len(pu) * len(pv))[:n]
        iu[:n], iv[:n] = order // len(pv), order % len(pv)
        mp[..., 0], mp[..., 1] = pu[iu].reshape(H, W), pv[iv].reshape(H, W)
    elif kind == "random":
        mp[..., 0], mp[..., 1] = rng.uniform(-1.0, Ws, (H, W)), rng.uniform(-1.0, Hs, (H, W))
    elif kind == "constant":
        mp[..., 0], mp[..., 1] = min(1.25, Ws - 1.0), min(2.5, Hs - 1.0)
    else:
        raise KeyError(kind)
    mp.setflags(write=False)
    return mp


def identity_map(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], -1).astype(F)


# ------------------------------------------------------------------------------------------------ 1 - 4. host tests
def case_identity_rig(B=0.12):
    K = pinhole(700.0, 705.0, 320.5, 240.25)
    tr = lio.stereo_rectify(K, (), K, None, np.eye(3), (-B, 0.0, 0.0))
    assert np.abs(tr["R0"] - np.eye(3)).max() <= 1e-15 and np.abs(tr["R1"] - np.eye(3)).max() <= 1e-15
    assert tr["doffs"] == 0.0 and tr["baseline"] == B and tr["f"] == 705.0 and tr["cx0"] == tr["cx1"] == 320.5 and tr["cy"] == 240.25
    c = tr["calib"]
    assert isinstance(c, api.Calib) and (c.f, c.cx, c.cy, c.doffs, c.baseline) == (F(705.0), F(320.5), F(240.25), F(0.0), F(B))
    tr = lio.stereo_rectify(K, (), K, (), np.eye(3), (-B, 0.0, 0.0), f=650.0, principal=(300.0, 310.0, 200.0))
    assert (tr["f"], tr["cx0"], tr["cx1"], tr["cy"], tr["doffs"]) == (650.0, 300.0, 310.0, 200.0, 10.0)
    return tr


GEOMETRY_RIGS = [((5.0, 5.0, 5.0), (-0.2, 0.01, -0.02)), ((-5.0, 3.0, -4.0), (-0.5, -0.06, 0.04)), ((2.0, -5.0, 1.0), (-0.1, 0.03, 0.03)),
                 ((0.0, 0.0, 0.0), (-0.3, 0.1, -0.1))]


def case_geometry():
    """A rectified pair: every point has one row in both views, and x_left - x_right = f baseline / Z - doffs.  -> the largest errors, px"""
    K0, K1 = pinhole(1010.0, 1005.0, 640.5, 361.2), pinhole(995.0, 1001.0, 633.1, 355.8)
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for angles, T in GEOMETRY_RIGS:
        R, T = rot(*angles), np.array(T)
        for kw in ({}, dict(f=900.0, principal=(600.0, 650.0, 340.0))):
            tr = lio.stereo_rectify(K0, DIST8, K1, DIST8B, R, T, **kw)
            P0 = np.stack([rng.uniform(-1.5, 1.5, 1000), rng.uniform(-1.0, 1.0, 1000), rng.uniform(2.0, 20.0, 1000)], 1)       # in front of both cameras
            P1 = P0 @ R.T + T
            assert (P1[:, 2] > 1.0).all()
            raw = project(K0, DIST8, P0), project(K1, DIST8B, P1)                # where the raw cameras see the points
            assert all(np.isfinite(r).all() for r in raw)
            Q0, Q1 = P0 @ tr["R0"].T, P1 @ tr["R1"].T                              # the points in the two rectified frames
            f, cy = tr["f"], tr["cy"]
            x0, y0 = f * Q0[:, 0] / Q0[:, 2] + tr["cx0"], f * Q0[:, 1] / Q0[:, 2] + cy
            x1, y1 = f * Q1[:, 0] / Q1[:, 2] + tr["cx1"], f * Q1[:, 1] / Q1[:, 2] + cy
            rows = float(np.abs(y0 - y1).max())
            disp = float(np.abs((x0 - x1) - (f * tr["baseline"] / Q0[:, 2] - tr["doffs"])).max())
            worst = [max(worst[0], rows), max(worst[1], disp)]
            assert rows <= 1e-9 and disp <= 1e-9, (angles, rows, disp)
            for Rm in (tr["R0"], tr["R1"]):
                assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Rm) - 1.0) <= 1e-14
            # the rectified frames are what the map kernel's M undoes: a rectified pixel's ray, through M and the camera, is the raw pixel
            for m, (K, dist, x, y) in enumerate(((K0, DIST8, x0, y0), (K1, DIST8B, x1, y1))):
                ray = np.stack([(x - tr[f"cx{m}"]) / f, (y - cy) / f, np.ones_like(x)], 1) @ tr[f"R{m}"]          # (rows times R: R^T applied)
                assert np.abs(project(K, dist, ray) - raw[m]).max() <= 1e-9
            c = tr["calib"]
            assert (c.f, c.cx, c.cy, c.doffs, c.baseline) == (F(tr["f"]), F(tr["cx0"]), F(cy), F(tr["doffs"]), F(tr["baseline"]))
    return worst


def case_transform_refusals():
    from localexpstereo_amd import stereo
    K = pinhole(700.0, 700.0, 320.0, 240.0)
    skew = K.copy()
    skew[0, 1] = 0.5
    good = (K, (), K, (), np.eye(3), (-0.1, 0.0, 0.0))
    lio.stereo_rectify(*good)
    bad = [(K, (), K, (), np.eye(3), (0.0, -0.1, 0.0)), (K, (), K, (), rot(0, 0, 2.0), (-0.05, 0.1, 0.01)),           # vertical rigs
           (skew, (), K, (), np.eye(3), (-0.1, 0.0, 0.0)), (K, (), skew, (), np.eye(3), (-0.1, 0.0, 0.0)),            # a skewed K
           (K, np.zeros(9), K, (), np.eye(3), (-0.1, 0.0, 0.0)), (K, (), K, np.ones(9), np.eye(3), (-0.1, 0.0, 0.0)),  # a 9-element dist
           (K, (), K, (), np.eye(3), (0.1, 0.0, 0.0))]                                                                # the cameras swapped
    for args in bad:
        try:
            lio.stereo_rectify(*args)
            raise AssertionError(f"accepted: {args}")
        except ValueError:
            pass
    try:
        stereo.Rectifier(*good, raw_size=(4, 4), interp="lanczos", device="cpu")
        raise AssertionError("an unknown interpolation was accepted")
    except ValueError:
        pass
    return len(bad)


def case_restatement_matches_loop(shape=(5, 7)):
    n = 0
    for name in RIGS:
        for args in map_inputs(name, shape):
            assert same(map_restate(*args, *shape), map_loop(*args, *shape)), name
            n += 1
    for size in SOURCES + [(5, 7)]:
        for C in CHANNELS:
            for kind in MAPS:
                for interp in INTERPS:
                    a, b = remap_restate(source(size, C), hand_map(shape, size, kind), interp), remap_loop(source(size, C), hand_map(shape, size, kind), interp)
                    assert same(a[0], b[0]) and same(a[1], b[1]), (size, C, kind, interp)
                    n += 1
    return n


def case_populations_do_what_they_say():
    """Each kind of pixel the device cases need occurs: in the maps of the map kernel, and in the hand-built maps of the sampler."""
    seen = {}
    for shape in SHAPES[2:]:
        H, W = shape
        for name in RIGS:
            for args in map_inputs(name, shape):
                mp, Z, den = map_parts(*args, H, W)
                nan = np.isnan(mp[..., 0])
                assert same(nan, np.isnan(mp[..., 1]))
                if name in ("identity", "five"):
                    assert not nan.any(), (shape, name)
                elif name == "behind":
                    assert (Z <= 0).any() and (Z > 0).any() and same(nan, Z <= 0), (shape, name)
                elif name == "pole":
                    assert (den < 0).any() and (den > 0).any() and np.isfinite(mp).all(), (shape, name)
                elif name == "zero":
                    assert den[0, 2] == 0.0 and nan[0, 2] and same(nan, den == 0.0) and nan.sum() <= 4, (shape, name)          # (the lattice points of the circle)
                else:
                    assert np.isinf(den[0, 4]) and nan[0, 4] and same(nan, np.isinf(den)) and not nan[0, :2].any(), (shape, name)
        # "identity" is the identity map where the intrinsics agree
        K, dist, M, f, cx, cy = map_inputs("identity", shape)[0]
        assert same(map_restate(K, dist, M, f, cx, cy, H, W), identity_map(H, W)), shape
        for size in SOURCES:
            Hs, Ws = size
            mp = np.concatenate([hand_map(shape, size, k) for k in ("edges", "random", "integers")])
            u, v = mp[..., 0], mp[..., 1]
            ok = valid_of(mp, Hs, Ws)
            with np.errstate(invalid="ignore"):
                kinds = {"interior": ok & (u > 0) & (u < Ws - 1) & (v > 0) & (v < Hs - 1), "left": ok & (u == 0), "right": ok & (u == Ws - 1), "top": ok & (v == 0),
                         "bottom": ok & (v == Hs - 1), "minus zero": ok & (u == 0) & np.signbit(u), "half": ok & ((u - np.floor(u)) == 0.5),
                         "nan": np.isnan(u) | np.isnan(v), "+inf": np.isposinf(u) | np.isposinf(v), "-inf": np.isneginf(u) | np.isneginf(v),
                         "huge": (np.abs(u) >= 2.0 ** 31) & np.isfinite(u), "just below": (u < 0) & (u > -1e-6), "just above": (u > Ws - 1) & (u < Ws - 1 + 0.5),
                         "below": u <= -0.5, "above": u >= Ws - 0.5}
            for k, m in kinds.items():
                if size == (1, 1) and k in ("interior", "half"):
                    continue                 # a one-pixel source has neither
                assert m.any(), (shape, size, k)
                if k not in ("interior", "left", "right", "top", "bottom", "minus zero", "half"):
                    assert not ok[m].any(), (shape, size, k)
                seen[k] = seen.get(k, 0) + int(m.sum())
            const = hand_map(shape, size, "constant")
            assert len(np.unique(const.reshape(-1, 2), axis=0)) == 1 and valid_of(const, Hs, Ws).all()
    # the cubic's sums leave 0 .. 255 on both sides, so the clamp works
    mp = hand_map((64, 257), (9, 300), "random")
    s = remap_parts(source((9, 300), 3), mp, 2)[2]
    ok = valid_of(mp, 9, 300)
    assert (s[ok] < -0.5).any() and (s[ok] > 255.5).any()
    return seen


# ------------------------------------------------------------------------------------------------ device harness
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def dev_map(lib, K, dist, M, f, cx, cy, H, W):
    out = pc.Guarded(lib, H * W * 2)
    api.rectify_map(api.camera(K, dist), M, f, cx, cy, out.ptr, H, W, lib=lib)
    return out.check().view(F).reshape(H, W, 2)


def dev_remap(lib, src, mp, interp, want_valid=True):
    Hs, Ws, C = src.shape
    H, W = mp.shape[:2]
    s, m = pc.Guarded(lib, src.size, words=False, fill=src), pc.Guarded(lib, mp.size, fill=mp)
    d, v = pc.Guarded(lib, H * W * C, words=False), pc.Guarded(lib, H * W, words=False)
    api.remap(s.ptr, Hs, Ws, C, m.ptr, d.ptr, v.ptr if want_valid else None, H, W, interp=interp, lib=lib)
    dst, valid = d.check().reshape(H, W, C), v.check().reshape(H, W)
    assert same(s.check().reshape(src.shape), src) and same(m.check().view(F).reshape(mp.shape), mp)
    if not want_valid:
        assert (valid == GUARD).all()
    return dst, valid


# ------------------------------------------------------------------------------------------------ 5. the map kernel
def case_map_kernel(lib, shape):
    H, W = shape
    n = 0
    for name in RIGS:
        for args in map_inputs(name, shape):
            got, want = dev_map(lib, *args, H, W), map_restate(*args, H, W)
            assert same(got, want), f"map {H}x{W} {name}: {first_diff(got, want)}"
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ 6. the sampler
def case_remap_kernel(lib, shape):
    H, W = shape
    n = 0
    for size in SOURCES:
        for C in CHANNELS:
            src = source(size, C)
            for kind in MAPS:
                mp = hand_map(shape, size, kind)
                for interp in INTERPS:
                    got, want = dev_remap(lib, src, mp, interp), remap_restate(src, mp, interp)
                    assert same(got[0], want[0]) and same(got[1], want[1]), f"remap {H}x{W} from {size} x {C} {kind} interp {interp}: {first_diff(got[0], want[0])}"
                    n += 1
    got = dev_remap(lib, source(SOURCES[0], 3), hand_map(shape, SOURCES[0], "edges"), 1, want_valid=False)            # without a valid map
    assert same(got[0], remap_restate(source(SOURCES[0], 3), hand_map(shape, SOURCES[0], "edges"), 1)[0])
    return n + 1


# ------------------------------------------------------------------------------------------------ 7. the identity map
def case_identity_map(lib, shape):
    H, W = shape
    for C in CHANNELS:
        src = source(shape, C, seed=1)
        for interp in INTERPS:
            dst, valid = dev_remap(lib, src, identity_map(H, W), interp)
            assert same(dst, src) and (valid == 1).all(), (shape, C, interp)
    for name in ("nearest", "linear", "cubic"):                       # the names of api.INTERP_NAMES
        assert same(dev_remap(lib, source(shape, 3, seed=1), identity_map(H, W), name)[0], source(shape, 3, seed=1))


# ------------------------------------------------------------------------------------------------ 8. refusals
def case_refusals(lib):
    import ctypes as C
    L = api.load(lib)
    vp = C.c_void_p
    H, W, Hs, Ws = 3, 5, 4, 6
    bufs = [pc.Guarded(lib, n, words=w) for n, w in ((Hs * Ws * 3, False), (H * W * 2, True), (H * W * 3, False), (H * W, False))]
    src, mp, dst, val = (b.ptr for b in bufs)
    cam = api.camera(pinhole(10.0, 10.0, 2.0, 1.0), DIST8)
    bad_cam = api.camera(pinhole(0.0, 10.0, 2.0, 1.0))
    M = (C.c_double * 9)(*np.eye(3).reshape(9))
    ARG, UNSUP = api.LES_HIP_ERR_ARG, api.LES_HIP_ERR_UNSUPPORTED

    def rmap(cam_=cam, M_=M, f=10.0, d_map=mp, H_=H, W_=W):
        return L.les_hip_rectify_map(C.byref(cam_) if cam_ is not None else None, M_, f, 2.0, 1.0, vp(d_map) if d_map else None, H_, W_, 0, None)

    def rem(s=src, Hs_=Hs, Ws_=Ws, ch=3, m=mp, d=dst, v=val, H_=H, W_=W, interp=1):
        return L.les_hip_remap(vp(s) if s else None, Hs_, Ws_, ch, vp(m) if m else None, vp(d) if d else None, vp(v) if v else None, H_, W_, interp, 0, None)

    refused = [rmap(cam_=None), rmap(M_=None), rmap(d_map=None), rmap(H_=0), rmap(W_=0), rmap(H_=-2), rmap(W_=-1), rmap(f=0.0), rmap(f=float("nan")),
               rmap(f=float("inf")), rmap(cam_=bad_cam), rmap(d_map=mp + 4),
               rem(s=None), rem(m=None), rem(d=None), rem(Hs_=0), rem(Ws_=0), rem(Hs_=-1), rem(H_=0), rem(W_=0), rem(W_=-3), rem(ch=0), rem(ch=2), rem(ch=4),
               rem(interp=-1), rem(interp=3), rem(m=mp + 4), rem(d=src)]
    assert refused == [ARG] * len(refused), refused
    assert L.les_hip_last_error() != b""
    big = [rem(Hs_=46341, Ws_=46341, ch=1), rem(Hs_=32768, Ws_=21846, ch=3), rem(Hs_=1, Ws_=2 ** 31 - 1, ch=3), rmap(H_=65536), rem(H_=65536)]      # Hs Ws channels >= 2^31; the grid
    assert big == [UNSUP] * len(big), big
    for b in bufs:
        assert (b.check() == b.g).all(), "a refused call wrote"
    for call in (lambda: api.remap(src, Hs, Ws, 2, mp, dst, val, H, W, lib=lib), lambda: api.rectify_map(cam, np.eye(3), 0.0, 0.0, 0.0, mp, H, W, lib=lib)):
        try:
            call()
            raise AssertionError("accepted")
        except api.LesHipError as ex:
            assert f"error {ARG}" in str(ex)
    # a good call still works afterwards
    assert rmap() == api.LES_HIP_OK and rem() == api.LES_HIP_OK
    assert not (bufs[1].check() == bufs[1].g).all() and (bufs[3].check() != GUARD).all()
    return len(refused) + len(big)


# ------------------------------------------------------------------------------------------------ 9. independence
def case_independence(lib, shape=(17, 67), size=(9, 300)):
    """Changing one source pixel changes only destination pixels whose taps include it."""
    Hs, Ws = size
    rng = np.random.default_rng(21)
    mp = np.stack([rng.uniform(140.0, 150.0, shape), rng.uniform(2.0, 6.0, shape)], -1).astype(F)       # dense around the pixel that changes
    src = source(size, 3)
    y0, x0 = 4, 145
    src2 = src.copy()
    src2[y0, x0] ^= 0xFF
    out = {}
    for interp in INTERPS:
        ok, taps = tap_indices(mp, Hs, Ws, interp)
        touched = ok & np.any([(r == y0) & (c == x0) for r, c in taps], 0)
        a, b = dev_remap(lib, src, mp, interp), dev_remap(lib, src2, mp, interp)
        changed = (a[0] != b[0]).any(-1)
        assert touched.any() and not touched.all() and changed.any() and not changed[~touched].any(), interp
        assert same(a[1], b[1])
        out[interp] = (int(changed.sum()), int(touched.sum()))
    assert out[0][1] < out[1][1] < out[2][1]
    return out


# ------------------------------------------------------------------------------------------------ 10 - 12. the cones crop
RAW_SIZE = (108, 136)                    # the raw frames: the 96 x 120 crop with a border of 6 / 8 pixels, so that the rig's shifts stay inside
CONES_F = 150.0                          # the focal length the crop is given, pixels: a field of view of 44 degrees
CONES_RIG = dict(angles=(1.0, -0.8, 1.2), T=(-0.16, 0.004, -0.003), dist0=(-0.06, 0.02, 0.0008, -0.0006), dist1=(-0.05, 0.015, -0.0007, 0.0005))
UNDISTORT_STEPS = 20


@functools.lru_cache(maxsize=None)
def cones_setup():
    """The cones crop as the rectified truth, and the rig that looks at it: rotations of about 1 degree, mild distortion.  -> dict(imL, imR, gt,
    K0, K1, R, T, f, principal, rawL, rawR, transform)."""
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    f, principal = CONES_F, (0.5 * (W - 1), 0.5 * (W - 1), 0.5 * (H - 1))
    Hs, Ws = RAW_SIZE
    K0 = pinhole(152.0, 149.0, 0.5 * (Ws - 1) + 0.8, 0.5 * (Hs - 1) - 0.6)
    K1 = pinhole(148.5, 151.0, 0.5 * (Ws - 1) - 1.1, 0.5 * (Hs - 1) + 0.7)
    R, T = rot(*CONES_RIG["angles"]), np.array(CONES_RIG["T"])
    tr = lio.stereo_rectify(K0, CONES_RIG["dist0"], K1, CONES_RIG["dist1"], R, T, f=f, principal=principal)
    raws = []
    for m, (K, dist, im) in enumerate(((K0, CONES_RIG["dist0"], imL), (K1, CONES_RIG["dist1"], imR))):
        # every raw pixel -> its undistorted ray (a fixed-count fixed-point inversion of the distortion) -> the rectified frame -> the truth image
        vs, us = np.mgrid[0:Hs, 0:Ws].astype(D)
        xd, yd = (us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1]
        x, y = xd.copy(), yd.copy()
        for _ in range(UNDISTORT_STEPS):
            ex, ey = distort(dist, x, y)
            x, y = x - (ex - xd), y - (ey - yd)
        Q = np.stack([x, y, np.ones_like(x)], -1) @ tr[f"R{m}"].T
        px, py = f * Q[..., 0] / Q[..., 2] + principal[m], f * Q[..., 1] / Q[..., 2] + principal[2]
        px, py = np.clip(px, 0.0, W - 1.0), np.clip(py, 0.0, H - 1.0)                      # beyond the truth: its border pixel
        x0, y0 = np.minimum(np.floor(px).astype(int), W - 2), np.minimum(np.floor(py).astype(int), H - 2)
        tx, ty = (px - x0)[..., None], (py - y0)[..., None]
        p = im.astype(D)
        val = (1 - ty) * ((1 - tx) * p[y0, x0] + tx * p[y0, x0 + 1]) + ty * ((1 - tx) * p[y0 + 1, x0] + tx * p[y0 + 1, x0 + 1])
        raw = np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
        raw.setflags(write=False)
        raws.append(raw)
    return dict(imL=imL, imR=imR, gt=gt, K0=K0, K1=K1, R=R, T=T, f=f, principal=principal, rawL=raws[0], rawR=raws[1], transform=tr)


def cones_rectifier(lib, interp="linear"):
    from localexpstereo_amd import stereo
    s = cones_setup()
    return stereo.Rectifier(s["K0"], CONES_RIG["dist0"], s["K1"], CONES_RIG["dist1"], s["R"], s["T"], raw_size=RAW_SIZE, size=s["gt"].shape, f=s["f"],
                            principal=s["principal"], interp=interp, device=_dev(lib), lib=lib)


@functools.lru_cache(maxsize=None)
def cones_restated(interp=1):
    """The numpy restatement of the whole chain on the raw cones pair -> (imL, imR, validL, validR)"""
    s = cones_setup()
    tr = s["transform"]
    H, W = s["gt"].shape
    out = []
    for m, raw in ((0, s["rawL"]), (1, s["rawR"])):
        mp = map_restate(tr[f"K{m}"], tr[f"dist{m}"], tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], H, W)
        out.append(remap_restate(raw, mp, interp))
    return out[0][0], out[1][0], out[0][1] != 0, out[1][1] != 0


def raw_crop(raw):
    """The raw frame's centre crop of the truth's size: the raw pair as a user without rectification would feed it to the matcher."""
    (Hs, Ws), (H, W) = RAW_SIZE, cones_setup()["gt"].shape
    return np.ascontiguousarray(raw[(Hs - H) // 2:(Hs - H) // 2 + H, (Ws - W) // 2:(Ws - W) // 2 + W])


def mad(a, b, mask):
    return float(np.abs(a[mask].astype(D) - b[mask].astype(D)).mean())


def round_trip_figures(imL, imR, validL, validR):
    s = cones_setup()
    both = validL & validR
    return dict(valid_both=float(both.mean()), rect_L=mad(imL, s["imL"], both), rect_R=mad(imR, s["imR"], both),
                raw_L=mad(raw_crop(s["rawL"]), s["imL"], both), raw_R=mad(raw_crop(s["rawR"]), s["imR"], both))


def case_round_trip_restated():
    """The cap holds for the numpy restatement alone: at least 90 % of the pixels are valid in both views."""
    fig = round_trip_figures(*cones_restated())
    print("cones round trip, numpy restatement:", fig)
    assert fig["valid_both"] >= 0.9, fig
    return fig


def case_round_trip(lib):
    """The raw cones pair through stereo.Rectifier against the original pair and against the numpy restatement of the whole chain.
    Measured (linear; the device returns the restatement's bytes, so there is one set of figures): every pixel valid in both views; mean
    absolute difference to the original pair 4.59 (left) and 4.66 (right) grey levels, against 16.83 and 22.34 for the raw pair's centre crop."""
    s = cones_setup()
    rect = cones_rectifier(lib)
    got = rect.rectify(s["rawL"], s["rawR"])
    want = cones_restated()
    for k, w in zip(("imL", "imR", "validL", "validR"), want):
        assert same(got[k], w), f"{k}: {first_diff(got[k], w)}"
    fig, fig_np = round_trip_figures(got["imL"], got["imR"], got["validL"], got["validR"]), round_trip_figures(*want)
    print("cones round trip, device:", fig)
    print("cones round trip, numpy restatement:", fig_np)
    assert fig["valid_both"] >= 0.9, fig
    assert fig == fig_np, (fig, fig_np)
    # `far below`: at most half.  Two bilinear resamplings blur by a few grey levels; a pair displaced by f tan(1 deg) = 2.6 px and more on a
    # textured image differs like unrelated texture, tens of grey levels.
    assert fig["rect_L"] <= 0.5 * fig["raw_L"] and fig["rect_R"] <= 0.5 * fig["raw_R"], fig
    assert got["calib"] is rect.calib and rect.transform["doffs"] == 0.0
    # device frames in, device tensors out, the same bytes; the other interpolations restate too
    import torch
    dev = torch.device(_dev(lib))
    tens = rect.rectify(torch.from_numpy(s["rawL"].copy()).to(dev), torch.from_numpy(s["rawR"].copy()).to(dev))
    assert torch.is_tensor(tens["imL"]) and same(tens["imL"].cpu().numpy(), want[0]) and same(tens["validR"].cpu().numpy(), want[3])
    for name, interp in (("nearest", 0), ("cubic", 2)):
        other = cones_rectifier(lib, name).rectify(s["rawL"], s["rawR"])
        assert same(other["imL"], cones_restated(interp)[0]) and same(other["imR"], cones_restated(interp)[1]), name
    try:
        rect.rectify(s["rawL"][:-1], s["rawR"])
        raise AssertionError("a frame of another size was accepted")
    except ValueError:
        pass
    return fig


# Measured on the CPU simulator build with the numpy restatement of the rectification fed into wta_bad1 (case_matcher(sim_lib,
# rectified=cones_restated())): bad-1.0 over 11 462 pixels: original pair 11.72 %, rectified pair 15.36 %, raw pair 97.98 %.  The margin is
# that excess plus one percentage point: two resamplings blur, and the rate moves by single pixels on a crop this small.
MATCHER_EXCESS = 0.036468
MATCHER_MARGIN = MATCHER_EXCESS + 0.01


def wta_bad1(lib, imL, imR, gt, mask):
    """bad-1.0 of the one-view wta (AD-Census volumes, 64 disparities, th_col 0.5, guided filter of crossview_cases.WINDR: sgm_cases.driver's
    settings) over `mask`."""
    from localexpstereo_amd import stereo
    device = _dev(lib)
    H, W = gt.shape
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
    return float((np.abs(stereo.disparities(lab) - gt)[mask] > 1.0).mean())


def case_matcher(lib, rectified=None):
    """The matcher needs the front end: bad-1.0 of the one-view wta against the ground truth over the known pixels valid in both views, on the
    original pair, the rectified pair and the raw pair (its centre crop).  rectified: (imL, imR, validL, validR) to use in the place of the
    Rectifier's output (the measurement of the margin feeds the numpy restatement).
    Measured (simulator build, numpy restatement of the rectification; 11 462 pixels): original 11.72 %, rectified 15.36 %, raw 97.98 %; the
    rectified pair may exceed the original by MATCHER_MARGIN = 3.65 + 1 points, and the raw pair must exceed the rectified one by more."""
    s = cones_setup()
    if rectified is None:
        r = cones_rectifier(lib).rectify(s["rawL"], s["rawR"])
        rectified = (r["imL"], r["imR"], r["validL"], r["validR"])
    imL, imR, validL, validR = rectified
    gt = s["gt"]
    mask = (gt > 0) & np.isfinite(gt) & validL & validR
    out = dict(pixels=int(mask.sum()), original=wta_bad1(lib, s["imL"], s["imR"], gt, mask), rectified=wta_bad1(lib, imL, imR, gt, mask),
               raw=wta_bad1(lib, raw_crop(s["rawL"]), raw_crop(s["rawR"]), gt, mask))
    print("one-view wta on the cones crop, bad-1.0:", out, "margin", MATCHER_MARGIN)
    assert out["pixels"] >= 8000, out
    assert out["rectified"] <= out["original"] + MATCHER_MARGIN, out
    assert out["raw"] > out["rectified"] + MATCHER_MARGIN, out
    return out


def case_driver(lib, device, monkeypatch, layers=None, **opts):
    """Rectifier.data into MidV3 for one iteration, then reconstruct with the rectifier's calibration: it runs, the points are finite where valid,
    and with the identity rig MidV3 returns the bytes it returns for the unrectified input.  layers, opts: as crossview_cases.case_driver_midv2."""
    from localexpstereo_amd import stereo
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    kw = dict(iterations=1, pmIterations=1, device=device, lib=lib, **opts)
    s = cones_setup()
    rect = cones_rectifier(lib)
    data = rect.data(s["rawL"], s["rawR"], 64)
    assert sorted(data) == ["dispGT", "gt_prec", "imL", "imR", "ndisp", "nonocc"]                  # io.load_data's keys
    assert data["ndisp"] == 64 and data["gt_prec"] == -1.0 and not data["dispGT"].any() and data["dispGT"].dtype == F
    assert data["nonocc"].dtype == bool and same(data["nonocc"], cones_restated()[2]) and same(data["imL"], cones_restated()[0])
    run, lab, raw = stereo.MidV3(data, **kw)
    H, W = lab.shape[:2]
    assert lab.shape == s["gt"].shape + (4,) and np.isfinite(lab).all()
    e = api.HipCostVolumeEnergy.naive(data["imL"], data["imR"], windR=2, max_disp=63.0, lib=lib, filter="")
    try:
        st = stereo.FastGCStereo(e, data["imL"], data["imR"], dict(lambda_=run.p["lambda_"], th_smooth=run.p["th_smooth"], windR=2), device=device, seed=1)
        r = st.reconstruct(lab, rect.calib, conf=data["nonocc"], min_confidence=0.5)
    finally:
        e.close()
    assert r["valid"].any() and not r["valid"][~data["nonocc"]].any()
    assert np.isfinite(r["points"][r["valid"]]).all() and np.isnan(r["points"][~r["valid"]]).all()
    # metric: Z = f baseline / (d + doffs), in the unit of T
    Z = CONES_F * rect.transform["baseline"] / (stereo.disparities(lab).astype(D) + rect.transform["doffs"])
    assert np.allclose(r["points"][..., 2][r["valid"]], Z[r["valid"]], rtol=1e-5)
    # the identity rig changes nothing
    K = pinhole(128.0, 128.0, 0.5 * (W - 1), 0.5 * (H - 1))                                       # (exact arithmetic: see map_inputs("identity"))
    ident = stereo.Rectifier(K, (), K, (), np.eye(3), (-0.16, 0.0, 0.0), raw_size=(H, W), device=device, lib=lib)
    same_data = ident.data(s["imL"], s["imR"], 64)
    assert same(same_data["imL"], s["imL"]) and same(same_data["imR"], s["imR"]) and same_data["nonocc"].all()
    _, lab_i, raw_i = stereo.MidV3(same_data, **kw)
    _, lab_p, raw_p = stereo.MidV3(dict(imL=s["imL"], imR=s["imR"], dispGT=np.zeros((H, W), F), nonocc=np.ones((H, W), bool), ndisp=64, gt_prec=-1.0), **kw)
    assert same(lab_i, lab_p) and same(raw_i, raw_p)
    return dict(vertices=int(r["valid"].sum()), pixels=H * W)
