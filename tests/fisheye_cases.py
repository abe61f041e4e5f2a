"""Cases of tests/test_fisheye.py: the equidistant fisheye camera in the rectification front end and on the way back (csrc/les_fisheye.h:
les_hip_rectify_map_fisheye, les_hip_unrectify_map_fisheye; api.fisheye / api.rectify_map_fisheye / api.unrectify_map_fisheye;
io.fisheye_theta_max; io.stereo_rectify(model="fisheye"); stereo.Rectifier(model="fisheye")) on the CPU simulator build and on the MI355X.

The definitions, restated from csrc/les_fisheye.h (conventions, the rig and the sampler: tests/rectify_cases.py).  Every operation fp64,
rounded, in this order; each output rounded to f32 once; every NaN stored is 0x7fc00000.
  camera    (X, Y, Z) -> a = X / Z, b = Y / Z, r = sqrt(a^2 + b^2), theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 +
            k4 theta^8), u = fx (theta_d / r) a + cx, v = fy (theta_d / r) b + cy (r = 0: the principal point); no pixel beyond theta_max.
  fe_atan   r >= 0: big = r > 1, t = big ? 1 / r : r; mid = t > T8 = sqrt(2.0) - 1.0; s = mid ? (t - 1) / (t + 1) : t; z = s s; p = 1 / 39, for
            n = 18 .. 0: p = 1 / (2 n + 1) - z p; a = s p; mid: a = pi/4 + a; big: a = pi/2 - a.
  fe_sincos 0 <= theta <= pi: q = floor(theta / (pi/2) + 0.5), y = theta - q (pi/2), z = y y; S = -1 / 19!, for k = 17, 15 .. 3: S = +-1 / k! + z S
            (+ where (k - 1) / 2 is even), sin_y = y + (y z) S; C = 1 / 20!, for k = 18, 16 .. 2: C = +-1 / k! + z C (+ where k / 2 is even),
            cos_y = 1 + z C; q = 0: (sin_y, cos_y), q = 1: (cos_y, -sin_y), q = 2: (-sin_y, -cos_y).
  map       xr = (x - cx) / f, yr = (y - cy) / f; X = (M0 xr + M1 yr) + M2, Y, Z alike; Z > 0 or (NaN, NaN); a = X / Z, b = Y / Z,
            r = sqrt(a a + b b); theta = fe_atan(r); theta <= theta_max or (NaN, NaN); t2 = theta theta, P = 1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)));
            theta_d = theta P; s = r > 0 ? theta_d / r : 1; u = fx (a s) + cxr, v = fy (b s) + cyr, each rounded to f32 once; a NaN in either: (NaN, NaN).
  inverse   xd = (u - cxr) / fx, yd = (v - cyr) / fy; theta_d = sqrt(xd xd + yd yd); theta = theta_d; `steps` times: t2, P as above,
            Q = 1 + t2 (3 k1 + t2 (5 k2 + t2 (7 k3 + t2 (9 k4)))) with the products rounded first, Q finite and > 0 or (NaN, NaN),
            theta = theta - (theta P - theta_d) / Q; once more e = theta P - theta_d; converged iff |fx e| <= tol and |fy e| <= tol or (NaN, NaN);
            0 <= theta <= theta_max or (NaN, NaN); (sn, cs) = fe_sincos(theta); g = theta_d > 0 ? sn / theta_d : 1; ray = (xd g, yd g, cs);
            X = (R0 rx + R1 ry) + R2 rz, Y, Z alike; Z > 0 or (NaN, NaN); xs = f (X / Z) + cx, ys = f (Y / Z) + cy, each rounded to f32 once.

References, none of them the code under test: the vectorised numpy restatements below, themselves held to literal per-pixel loops; the camera
model `project`, written once more in its plain form with math.atan (and math.sin / math.cos for the functions) for the accuracy, the round
trip and the rendering of the raw frames.  Tolerances: none for the kernels -- every output is compared bit for bit (fp64 add, multiply,
divide, sqrt and floor are correctly rounded on both sides, the order is fixed, nothing is contracted, each coordinate is rounded to f32
once, and atan, sin and cos are the restated ones on both sides).  The restated functions are held to 1e-15 of math.atan / sin / cos.

Shapes: rectify_cases.SHAPES, (1, 1), (3, 5), (17, 67), (64, 257), for both maps, with intrinsics scaled to the shape so that every shape spans
+-72 degrees horizontally; lenses k = 0, a four-coefficient lens, that lens with a field of view of 100 degrees, and a lens that folds back
at 59.79 degrees; an identity rotation and one of 60 degrees; steps 1, 3, 10."""
import ctypes as C
import functools
import itertools
import math

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import io as lio
from tests import costvol_cases as cc
from tests import pyramid_cases as pc
from tests import rectify_cases as rc
from tests import unrectify_cases as uc
from tests.rectify_cases import D, F, QNAN, first_diff, same

SHAPES = rc.SHAPES
STEPS = (1, 3, 10)
TOL = api.UNRECTIFY_TOL

# ------------------------------------------------------------------------------------------------ the three functions, restated
ONE = D(1.0)
PI2, PI4 = D(math.pi) / D(2.0), D(math.pi) / D(4.0)          # the doubles nearest pi / 2 and pi / 4 (halving is exact)
T8 = D(np.sqrt(D(2.0))) - ONE
ATAN_COEF = [ONE / D(2 * n + 1) for n in range(20)]          # 1, 1/3 .. 1/39
FACT = [ONE / D(math.factorial(k)) for k in range(21)]       # 1 / k!; k! is a double up to 22!


def fe_atan(r):
    r = np.asarray(r, D)
    with np.errstate(all="ignore"):
        big = r > 1.0
        t = np.where(big, ONE / r, r)
        mid = t > T8
        s = np.where(mid, (t - ONE) / (t + ONE), t)
        z = s * s
        p = ATAN_COEF[19]
        for n in range(18, -1, -1):
            p = ATAN_COEF[n] - z * p
        a = s * p
        a = np.where(mid, PI4 + a, a)
        a = np.where(big, PI2 - a, a)
    return a


def fe_sincos(theta):
    theta = np.asarray(theta, D)
    with np.errstate(all="ignore"):
        q = np.floor(theta / PI2 + D(0.5))
        y = theta - q * PI2
        z = y * y
        S = -FACT[19]
        for k in range(17, 1, -2):
            S = (FACT[k] if ((k - 1) // 2) % 2 == 0 else -FACT[k]) + z * S
        sin_y = y + (y * z) * S
        Cc = FACT[20]
        for k in range(18, 0, -2):
            Cc = (FACT[k] if (k // 2) % 2 == 0 else -FACT[k]) + z * Cc
        cos_y = ONE + z * Cc
    return np.where(q == 0, sin_y, np.where(q == 1, cos_y, -sin_y)), np.where(q == 0, cos_y, np.where(q == 1, -sin_y, -cos_y))


def fe_atan_scalar(r):
    """fe_atan by a literal transcription on one numpy float64 scalar."""
    big = r > 1.0
    t = ONE / r if big else r
    mid = t > T8
    s = (t - ONE) / (t + ONE) if mid else t
    z = s * s
    p = ONE / D(39.0)
    for n in range(18, -1, -1):
        p = ONE / D(2 * n + 1) - z * p
    a = s * p
    if mid:
        a = PI4 + a
    if big:
        a = PI2 - a
    return a


def fe_sincos_scalar(theta):
    q = np.floor(theta / PI2 + D(0.5))
    y = theta - q * PI2
    z = y * y
    S = -(ONE / D(math.factorial(19)))
    for k in (17, 15, 13, 11, 9, 7, 5, 3):
        c = ONE / D(math.factorial(k))
        S = (c if k in (17, 13, 9, 5) else -c) + z * S
    sin_y = y + (y * z) * S
    Cc = ONE / D(math.factorial(20))
    for k in (18, 16, 14, 12, 10, 8, 6, 4, 2):
        c = ONE / D(math.factorial(k))
        Cc = (c if k in (16, 12, 8, 4) else -c) + z * Cc
    cos_y = ONE + z * Cc
    return (sin_y, cos_y) if q == 0 else ((cos_y, -sin_y) if q == 1 else (-sin_y, -cos_y))


def neighbours(vals, lo, hi):
    """vals with the doubles on either side of each, kept to [lo, hi]."""
    out = []
    for v in vals:
        v = D(v)
        out += [np.nextafter(v, D(-np.inf)), v, np.nextafter(v, D(np.inf))]
    out = np.array(out, D)
    return out[(out >= lo) & (out <= hi)]


def atan_grid():
    """220 001 points of [0, 1e6] -- dense where the branches change, geometric beyond --, with 0, 1, T8, 1 / T8, their neighbours and inf."""
    g = np.concatenate([np.linspace(0.0, 4.0, 200001), np.geomspace(4.0, 1e6, 20000), neighbours([0.0, 1.0, T8, ONE / T8, 1e6], 0.0, 1e6), [np.inf]])
    return g.astype(D)


def sincos_grid():
    """400 001 points of [0, pi] with the multiples of pi / 4 and their neighbours."""
    return np.concatenate([np.linspace(0.0, math.pi, 400001), neighbours([j * math.pi / 4.0 for j in range(5)], 0.0, math.pi)]).astype(D)


FUNCTION_BOUND = 1e-15          # absolute; the issue's: 2.3e-16 measured against numpy's library, times four for another libm


def case_functions():
    """The restated fe_atan and fe_sincos against math.atan / math.sin / math.cos, absolute error at most 1e-15; the vectorised forms are the
    scalar transcriptions, bit for bit, on a subsample and at every special point.
    Measured here: fe_atan 2.22e-16 over [0, 1e6] and inf; fe_sincos 2.22e-16 (sin) and 2.22e-16 (cos) over [0, pi]."""
    g = atan_grid()
    got = fe_atan(g)
    err_atan = float(np.abs(got - np.array([math.atan(v) for v in g])).max())
    assert got[0] == 0.0 and got[-1] == PI2 and np.isnan(fe_atan(D(np.nan)))
    t = sincos_grid()
    sn, cs = fe_sincos(t)
    err_sin = float(np.abs(sn - np.array([math.sin(v) for v in t])).max())
    err_cos = float(np.abs(cs - np.array([math.cos(v) for v in t])).max())
    print("largest absolute differences to math.atan, math.sin, math.cos:", err_atan, err_sin, err_cos)
    assert err_atan <= FUNCTION_BOUND and err_sin <= FUNCTION_BOUND and err_cos <= FUNCTION_BOUND, (err_atan, err_sin, err_cos)
    # every branch occurs
    with np.errstate(all="ignore"):
        tt = np.where(g > 1.0, 1.0 / g, g)
    q = np.floor(t / PI2 + 0.5)
    assert (g > 1.0).any() and (g <= 1.0).any() and (tt > T8).any() and (tt <= T8).any() and all((q == j).any() for j in (0, 1, 2))
    # the vectorised forms are the scalar ones
    with np.errstate(all="ignore"):
        sub = np.concatenate([g[::97], g[-40:]])
        assert same(fe_atan(sub), np.array([fe_atan_scalar(v) for v in sub], D))
        sub = np.concatenate([t[::173], t[-40:]])
        pairs = np.array([fe_sincos_scalar(v) for v in sub], D)
        assert same(fe_sincos(sub)[0], np.ascontiguousarray(pairs[:, 0])) and same(fe_sincos(sub)[1], np.ascontiguousarray(pairs[:, 1]))
    return err_atan, err_sin, err_cos


# ------------------------------------------------------------------------------------------------ the camera model in its plain form
def _k4(k):
    return np.concatenate([np.asarray(() if k is None else k, D).reshape(-1), np.zeros(4)])[:4]


def project(K, k, P):
    """Points N x 3 of the camera's frame (Z > 0) -> pixels N x 2: the model as the issue writes it, with math.atan."""
    k1, k2, k3, k4 = _k4(k)
    a, b = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r = np.sqrt(a * a + b * b)
    th = np.array([math.atan(v) for v in r])
    th_d = th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    with np.errstate(all="ignore"):
        s = np.where(r > 0, th_d / r, 1.0)
    return np.stack([K[0, 0] * s * a + K[0, 2], K[1, 1] * s * b + K[1, 2]], 1)


def forward(K, k, R, f, cx, cy, xs, ys):
    """A rectified position -> the raw pixel, in the plain form."""
    ray = np.stack([(xs - cx) / f, (ys - cy) / f, np.ones_like(xs)], 1) @ np.asarray(R, D).reshape(3, 3)          # (rows times R: R^T applied)
    return project(np.asarray(K, D), k, ray)


def unproject(K, k, us, vs, steps=30):
    """Raw pixels -> unit rays of the camera's frame, by an fp64 Newton inversion of the radial polynomial with `steps` steps (numpy's sin, cos)."""
    k1, k2, k3, k4 = _k4(k)
    xd, yd = (us - K[0, 2]) / K[0, 0], (vs - K[1, 2]) / K[1, 1]
    th_d = np.sqrt(xd * xd + yd * yd)
    th = th_d.copy()
    for _ in range(steps):
        t2 = th * th
        th = th - (th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - th_d) / (1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4))))
    with np.errstate(all="ignore"):
        g = np.where(th_d > 0, np.sin(th) / th_d, 1.0)
    return np.stack([xd * g, yd * g, np.cos(th)], -1)


# ------------------------------------------------------------------------------------------------ the kernels, restated
def _poly(k, t2):
    return ONE + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))


def map_parts(K, k, theta_max, M, f, cx, cy, H, W):
    """-> (map H x W x 2 f32, dict(Z, r, theta: the fp64 intermediates the branches test))"""
    M = np.asarray(M, D).reshape(9)
    k = [D(v) for v in _k4(k)]
    fx, fy, cxr, cyr, theta_max = D(K[0, 0]), D(K[1, 1]), D(K[0, 2]), D(K[1, 2]), D(theta_max)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        xr, yr = (xs.astype(D) - D(cx)) / D(f), (ys.astype(D) - D(cy)) / D(f)
        X = (M[0] * xr + M[1] * yr) + M[2]
        Y = (M[3] * xr + M[4] * yr) + M[5]
        Z = (M[6] * xr + M[7] * yr) + M[8]
        a, b = X / Z, Y / Z
        r = np.sqrt(a * a + b * b)
        theta = fe_atan(r)
        theta_d = theta * _poly(k, theta * theta)
        s = np.where(r > 0.0, theta_d / r, ONE)
        u, v = (fx * (a * s) + cxr).astype(F), (fy * (b * s) + cyr).astype(F)
        ok = (Z > 0.0) & (theta <= theta_max) & ~np.isnan(u) & ~np.isnan(v)
    out = np.full((H, W, 2), QNAN, F)
    out[ok, 0], out[ok, 1] = u[ok], v[ok]
    return out, dict(Z=Z, r=r, theta=theta)


def map_restate(*a):
    return map_parts(*a)[0]


def map_loop(K, k, theta_max, M, f, cx, cy, H, W):
    """The same by a literal per-pixel transcription (numpy's float64 scalars: IEEE doubles, and a division by zero is no exception)."""
    M = [D(v) for v in np.asarray(M, D).reshape(9)]
    k1, k2, k3, k4 = (D(v) for v in _k4(k))
    fx, fy, cxr, cyr, f, cx, cy, theta_max = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy, theta_max))
    out = np.full((H, W, 2), QNAN, F)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                xr, yr = (D(x) - cx) / f, (D(y) - cy) / f
                X = (M[0] * xr + M[1] * yr) + M[2]
                Y = (M[3] * xr + M[4] * yr) + M[5]
                Z = (M[6] * xr + M[7] * yr) + M[8]
                if not Z > 0.0:
                    continue
                a, b = X / Z, Y / Z
                r = np.sqrt(a * a + b * b)
                theta = fe_atan_scalar(r)
                if not theta <= theta_max:
                    continue
                t2 = theta * theta
                P = ONE + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
                theta_d = theta * P
                s = theta_d / r if r > 0.0 else ONE
                u, v = F(fx * (a * s) + cxr), F(fy * (b * s) + cyr)
                if u == u and v == v:
                    out[y, x] = (u, v)
    return out


def inv_parts(K, k, theta_max, R, f, cx, cy, Hs, Ws, steps=api.FISHEYE_STEPS, tol=TOL):
    """-> (inv Hs x Ws x 2 f32, dict(fold: a Q that is not finite or <= 0 in some step, converged, in_range, Z, theta, theta_d))"""
    R = np.asarray(R, D).reshape(9)
    k = [D(v) for v in _k4(k)]
    q = [D(3.0) * k[0], D(5.0) * k[1], D(7.0) * k[2], D(9.0) * k[3]]
    fx, fy, cxr, cyr, f, cx, cy, tol, theta_max = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy, tol, theta_max))
    vs, us = np.mgrid[0:Hs, 0:Ws]
    with np.errstate(all="ignore"):
        xd, yd = (us.astype(D) - cxr) / fx, (vs.astype(D) - cyr) / fy
        theta_d = np.sqrt(xd * xd + yd * yd)
        theta = theta_d
        fold = np.zeros((Hs, Ws), bool)
        for _ in range(steps):
            t2 = theta * theta
            P = _poly(k, t2)
            Q = ONE + t2 * (q[0] + t2 * (q[1] + t2 * (q[2] + t2 * q[3])))
            fold |= ~(np.isfinite(Q) & (Q > 0.0))
            theta = theta - (theta * P - theta_d) / Q
        e = theta * _poly(k, theta * theta) - theta_d
        converged = (np.abs(fx * e) <= tol) & (np.abs(fy * e) <= tol)
        in_range = (theta >= 0.0) & (theta <= theta_max)
        sn, cs = fe_sincos(np.where(in_range, theta, 0.0))
        g = np.where(theta_d > 0.0, sn / theta_d, ONE)
        rx, ry, rz = xd * g, yd * g, cs
        X = (R[0] * rx + R[1] * ry) + R[2] * rz
        Y = (R[3] * rx + R[4] * ry) + R[5] * rz
        Z = (R[6] * rx + R[7] * ry) + R[8] * rz
        xs, ys = (f * (X / Z) + cx).astype(F), (f * (Y / Z) + cy).astype(F)
        ok = ~fold & converged & in_range & (Z > 0.0) & ~np.isnan(xs) & ~np.isnan(ys)
    out = np.full((Hs, Ws, 2), QNAN, F)
    out[ok, 0], out[ok, 1] = xs[ok], ys[ok]
    return out, dict(fold=fold, converged=converged & ~fold, in_range=in_range, Z=Z, theta=theta, theta_d=theta_d)


def inv_restate(*a, **kw):
    return inv_parts(*a, **kw)[0]


def inv_loop(K, k, theta_max, R, f, cx, cy, Hs, Ws, steps=api.FISHEYE_STEPS, tol=TOL):
    """The same by a literal per-pixel transcription."""
    R = [D(v) for v in np.asarray(R, D).reshape(9)]
    k1, k2, k3, k4 = (D(v) for v in _k4(k))
    fx, fy, cxr, cyr, f, cx, cy, tol, theta_max = (D(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], f, cx, cy, tol, theta_max))
    out = np.full((Hs, Ws, 2), QNAN, F)

    def pixel(u, v):
        xd, yd = (D(u) - cxr) / fx, (D(v) - cyr) / fy
        theta_d = np.sqrt(xd * xd + yd * yd)
        theta = theta_d
        for _ in range(steps):
            t2 = theta * theta
            P = ONE + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
            Q = ONE + t2 * (D(3.0) * k1 + t2 * (D(5.0) * k2 + t2 * (D(7.0) * k3 + t2 * (D(9.0) * k4))))
            if not (np.isfinite(Q) and Q > 0.0):
                return None
            theta = theta - (theta * P - theta_d) / Q
        t2 = theta * theta
        e = theta * (ONE + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - theta_d
        if not (abs(fx * e) <= tol and abs(fy * e) <= tol):
            return None
        if not (theta >= 0.0 and theta <= theta_max):
            return None
        sn, cs = fe_sincos_scalar(theta)
        g = sn / theta_d if theta_d > 0.0 else ONE
        rx, ry, rz = xd * g, yd * g, cs
        X = (R[0] * rx + R[1] * ry) + R[2] * rz
        Y = (R[3] * rx + R[4] * ry) + R[5] * rz
        Z = (R[6] * rx + R[7] * ry) + R[8] * rz
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


# ------------------------------------------------------------------------------------------------ inputs
K_ZERO = ()
K_FOUR = (-0.035, 0.006, -0.0025, 0.0004)          # the issue's four-coefficient lens: Q > 0 out to 95 degrees and beyond
K_FOLD = (0.1, -0.3, 0.05, 0.0)                    # folds back at 59.79 degrees
LENSES = dict(zero=(K_ZERO, None), four=(K_FOUR, None), capped=(K_FOUR, 100.0), fold=(K_FOLD, None))          # name -> (k, fov)
ROTATIONS = ("identity", "sixty")
VIEWS = [(lens, "identity") for lens in LENSES] + [(lens, "sixty") for lens in ("zero", "four", "fold")]


def theta_max_of(lens):
    k, fov = LENSES[lens]
    return lio.fisheye_theta_max(k, fov)


@functools.lru_cache(maxsize=None)
def view(shape, lens, rotation):
    """-> (K, k, theta_max, M, f, cx, cy) of a fisheye view for a grid of `shape`, M rectified -> raw.  Raw focal lengths 0.39 and 0.38 of the
    longer side n: half a row, (n - 1) / 2 raw pixels, reaches theta_d = 1.26 rad, 72 degrees.  Rectified focal length 0.16 n: half a row reaches
    |xr| = 3.08, 72 degrees.  "identity": whole-numbered centres, so that the principal ray meets a pixel centre and r = 0 exactly there;
    "sixty": 60 degrees about the y axis and centres off the grid."""
    H, W = shape
    n = float(max(H, W))
    if rotation == "identity":
        K, M, cx, cy = rc.pinhole(0.39 * n, 0.38 * n, float(W // 2), float(H // 2)), np.eye(3), float(W // 2), float(H // 2)
    else:
        K, M, cx, cy = rc.pinhole(0.39 * n, 0.38 * n, 0.5 * (W - 1) + 1.3, 0.5 * (H - 1) - 0.7), rc.rot(0.0, 60.0, 0.0), 0.5 * (W - 1) - 0.4, 0.5 * (H - 1) + 0.2
    return K, LENSES[lens][0], theta_max_of(lens), M, 0.16 * n, cx, cy


def inv_view(shape, lens, rotation):
    """The same view as inverse-map arguments: (K, k, theta_max, R = M^T, f, cx, cy)."""
    K, k, tm, M, f, cx, cy = view(shape, lens, rotation)
    return K, k, tm, np.ascontiguousarray(np.asarray(M).T), f, cx, cy


# ------------------------------------------------------------------------------------------------ 1 - 4. host tests
def case_theta_max():
    """io.fisheye_theta_max: the fold of the folding lens, pi / 2 without one, the cap of fov; the refusal of a fifth coefficient."""
    fold = lio.fisheye_theta_max(K_FOLD)
    assert abs(math.degrees(fold) - 59.79) <= 0.005, math.degrees(fold)
    k1, k2, k3, k4 = K_FOLD
    Q = lambda th: 1 + 3 * k1 * th ** 2 + 5 * k2 * th ** 4 + 7 * k3 * th ** 6 + 9 * k4 * th ** 8
    assert Q(fold) > 0.0 and Q(fold / (1.0 - 1e-6) * (1.0 + 1e-6)) < 0.0 and all(Q(t) > 0.0 for t in np.linspace(0.0, fold, 1000))
    assert lio.fisheye_theta_max(()) == lio.fisheye_theta_max(None) == lio.fisheye_theta_max(K_FOUR) == 0.5 * math.pi
    assert all(Q4 > 0 for Q4 in (1 + 3 * K_FOUR[0] * t ** 2 + 5 * K_FOUR[1] * t ** 4 + 7 * K_FOUR[2] * t ** 6 + 9 * K_FOUR[3] * t ** 8 for t in np.linspace(0, math.radians(95), 500)))
    assert lio.fisheye_theta_max(K_FOUR, fov=100.0) == math.radians(100.0) / 2 and lio.fisheye_theta_max(K_FOLD, fov=100.0) == math.radians(50.0)
    assert lio.fisheye_theta_max(K_FOLD, fov=170.0) == fold and lio.fisheye_theta_max((), fov=220.0) == 0.5 * math.pi
    assert lio.fisheye_theta_max((0.0, 0.0, -0.2)) < 0.5 * math.pi          # a leading zero coefficient: a cubic in theta^2
    try:
        lio.fisheye_theta_max(np.zeros(5))
        raise AssertionError("five coefficients were accepted")
    except ValueError:
        pass
    return fold


PINHOLE_KEYS = ["K0", "K1", "R0", "R1", "baseline", "calib", "cx0", "cx1", "cy", "dist0", "dist1", "doffs", "f"]


def _same_transform(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if key == "calib":
            assert bytes(a[key]) == bytes(b[key])
        elif isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
        else:
            assert type(a[key]) is type(b[key]) and a[key] == b[key], key


def case_transform():
    """io.stereo_rectify(model=): the pinhole dict is what it was; the fisheye dict has the same rotations and intrinsics, four coefficients
    and the three new keys; the refusals."""
    s = rc.cones_setup()
    args = (s["K0"], rc.CONES_RIG["dist0"], s["K1"], rc.CONES_RIG["dist1"], s["R"], s["T"])
    kw = dict(f=s["f"], principal=s["principal"])
    plain = lio.stereo_rectify(*args, **kw)
    assert sorted(plain) == PINHOLE_KEYS and plain["dist0"].shape == (8,)
    _same_transform(plain, lio.stereo_rectify(*args, model="pinhole", **kw))
    _same_transform(plain, lio.stereo_rectify(*args, model="pinhole", fov=90.0, **kw))          # fov belongs to the fisheye model
    fish = lio.stereo_rectify(s["K0"], K_FOUR[:2], s["K1"], K_FOLD, s["R"], s["T"], model="fisheye", **kw)
    assert sorted(fish) == sorted(PINHOLE_KEYS + ["model", "theta_max0", "theta_max1"]) and fish["model"] == "fisheye"
    assert same(fish["dist0"], np.array(K_FOUR[:2] + (0.0, 0.0))) and same(fish["dist1"], np.array(K_FOLD))
    assert fish["theta_max0"] == 0.5 * math.pi and fish["theta_max1"] == lio.fisheye_theta_max(K_FOLD)
    _same_transform({k: v for k, v in plain.items() if not k.startswith("dist")}, {k: v for k, v in fish.items() if k in plain and not k.startswith("dist")})
    capped = lio.stereo_rectify(s["K0"], None, s["K1"], K_FOLD, s["R"], s["T"], model="fisheye", fov=100.0)
    assert capped["theta_max0"] == capped["theta_max1"] == math.radians(50.0) and same(capped["dist0"], np.zeros(4))
    bad = [dict(model="equisolid"), dict(model=None), dict(model="fisheye", dist0=np.zeros(5)), dict(model="fisheye", dist1=rc.DIST8)]
    for b in bad:
        a = list(args)
        a[1], a[3] = b.pop("dist0", a[1][:4]), b.pop("dist1", a[3][:4])
        try:
            lio.stereo_rectify(*a, **b)
            raise AssertionError(f"accepted: {b}")
        except ValueError:
            pass
    from localexpstereo_amd import stereo
    try:
        stereo.Rectifier(*args, raw_size=(4, 4), model="mei", device="cpu")
        raise AssertionError("an unknown model was accepted")
    except ValueError:
        pass
    for call in (lambda: api.fisheye(np.eye(3), np.zeros(5)), lambda: api.fisheye(np.array([[1.0, 0.1, 0], [0, 1, 0], [0, 0, 1]]))):
        try:
            call()
            raise AssertionError("accepted")
        except ValueError:
            pass
    cam = api.fisheye(rc.pinhole(3.0, 4.0, 1.0, 2.0), (0.5,), 1.25)
    assert (cam.fx, cam.fy, cam.cx, cam.cy, list(cam.k), cam.theta_max) == (3.0, 4.0, 1.0, 2.0, [0.5, 0.0, 0.0, 0.0], 1.25) and api.fisheye(cam) is cam
    assert api.fisheye(np.eye(3)).theta_max == 0.5 * math.pi and api.FISHEYE_STEPS == 10
    return len(bad)


def case_restatement_matches_loop(shape=(5, 7)):
    n = 0
    for lens, rotation in VIEWS:
        a, b = map_restate(*view(shape, lens, rotation), *shape), map_loop(*view(shape, lens, rotation), *shape)
        assert same(a, b), (lens, rotation, first_diff(a, b))
        for steps in STEPS:
            a, b = inv_restate(*inv_view(shape, lens, rotation), *shape, steps=steps), inv_loop(*inv_view(shape, lens, rotation), *shape, steps=steps)
            assert same(a, b), (lens, rotation, steps, first_diff(a, b))
            n += 1
        n += 1
    return n


def case_populations():
    """Each kind of pixel the device cases need occurs in their inputs; every population is non-empty."""
    seen = {}

    def add(key, m):
        seen[key] = seen.get(key, 0) + int(np.count_nonzero(m))

    for shape in SHAPES[2:]:
        H, W = shape
        for lens, rotation in VIEWS:
            args = view(shape, lens, rotation)
            mp, p = map_parts(*args, H, W)
            nan = np.isnan(mp[..., 0])
            assert same(nan, np.isnan(mp[..., 1]))
            front = p["Z"] > 0.0
            with np.errstate(all="ignore"):
                t = np.where(p["r"] > 1.0, 1.0 / p["r"], p["r"])
            add("map: stored", ~nan)
            add("map: r = 0", front & (p["r"] == 0.0))
            add(f"map: theta > theta_max ({lens})", front & (p["theta"] > args[2]))
            add(f"map: Z <= 0 ({rotation})", ~front)
            add("map: big", front & (p["r"] > 1.0))
            add("map: mid", front & (t > T8))
            add("map: mid and big", front & (t > T8) & (p["r"] > 1.0))
            add("map: neither", front & ~(t > T8) & ~(p["r"] > 1.0))
            assert same(nan, ~front | ~(p["theta"] <= args[2])), (shape, lens, rotation)
            if rotation == "identity":
                assert not nan[H // 2, W // 2] and mp[H // 2, W // 2].tolist() == [W // 2, H // 2] and p["r"][H // 2, W // 2] == 0.0          # the principal point itself
                assert float(np.abs((np.arange(W) - args[5]) / args[4]).max()) >= 3.0                                                 # |xr| up to 3
            for steps in STEPS:
                inv, q = inv_parts(*inv_view(shape, lens, rotation), H, W, steps=steps)
                nan = np.isnan(inv[..., 0])
                assert same(nan, np.isnan(inv[..., 1]))
                live = q["converged"] & q["in_range"]
                qq = np.floor(q["theta"] / PI2 + 0.5)
                add("inverse: stored", ~nan)
                add("inverse: theta_d = 0", ~nan & (q["theta_d"] == 0.0))
                add(f"inverse: Q <= 0 ({lens})", q["fold"])
                add(f"inverse: residual fails at {steps} steps", ~q["fold"] & ~q["converged"])
                add(f"inverse: theta > theta_max ({lens})", q["converged"] & ~q["in_range"])
                add(f"inverse: Z <= 0 ({rotation})", live & ~(q["Z"] > 0.0))
                add("inverse: q = 0", ~nan & (qq == 0))
                add("inverse: q = 1", ~nan & (qq == 1))
                assert same(nan, ~(live & (q["Z"] > 0.0))), (shape, lens, rotation, steps)
                if rotation == "identity":
                    assert inv[H // 2, W // 2].tolist() == [W // 2, H // 2]
                if lens != "fold":
                    assert not q["fold"].any(), (lens, steps)
        # the widest rays: at least 70 degrees on either side of the axis, in both directions
        assert math.degrees(math.atan((W // 2) / view(shape, "zero", "identity")[4])) >= 70.0 and math.degrees((W // 2) / view(shape, "zero", "identity")[0][0, 0]) >= 70.0
    need = ["map: stored", "map: r = 0", "map: theta > theta_max (fold)", "map: theta > theta_max (capped)", "map: Z <= 0 (sixty)", "map: big", "map: mid",
            "map: mid and big", "map: neither", "inverse: stored", "inverse: theta_d = 0", "inverse: Q <= 0 (fold)", "inverse: residual fails at 1 steps",
            "inverse: theta > theta_max (capped)", "inverse: Z <= 0 (sixty)", "inverse: q = 0", "inverse: q = 1"]
    for key in need:
        assert seen.get(key, 0) > 0, (key, seen)
    assert seen["map: Z <= 0 (identity)"] == 0 and seen["inverse: residual fails at 10 steps"] <= seen["inverse: residual fails at 1 steps"]
    return seen


# ------------------------------------------------------------------------------------------------ device harness
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def dev_map(lib, K, k, theta_max, M, f, cx, cy, H, W):
    out = pc.Guarded(lib, H * W * 2)
    api.rectify_map_fisheye(api.fisheye(K, k, theta_max), M, f, cx, cy, out.ptr, H, W, lib=lib)
    return out.check().view(F).reshape(H, W, 2)


def dev_inv(lib, K, k, theta_max, R, f, cx, cy, Hs, Ws, steps=api.FISHEYE_STEPS, tol=TOL):
    out = pc.Guarded(lib, Hs * Ws * 2)
    api.unrectify_map_fisheye(api.fisheye(K, k, theta_max), R, f, cx, cy, out.ptr, Hs, Ws, steps=steps, tol=tol, lib=lib)
    return out.check().view(F).reshape(Hs, Ws, 2)


# ------------------------------------------------------------------------------------------------ 5, 6. the two kernels
def case_map_kernel(lib, shape):
    H, W = shape
    n = 0
    for lens, rotation in VIEWS:
        args = view(shape, lens, rotation)
        got, want = dev_map(lib, *args, H, W), map_restate(*args, H, W)
        assert same(got, want), f"fisheye map {H}x{W} {lens} {rotation}: {first_diff(got, want)}"
        n += 1
    return n


def case_unmap_kernel(lib, shape):
    Hs, Ws = shape
    n = 0
    for (lens, rotation), steps in itertools.product(VIEWS, STEPS):
        args = inv_view(shape, lens, rotation)
        got, want = dev_inv(lib, *args, Hs, Ws, steps=steps), inv_restate(*args, Hs, Ws, steps=steps)
        assert same(got, want), f"fisheye inverse map {Hs}x{Ws} {lens} {rotation} steps {steps}: {first_diff(got, want)}"
        n += 1
    args = inv_view(shape, "four", "sixty")                                         # a tight residual bound, and a theta_max beyond 90 degrees
    for tol, tm in ((1e-9, args[2]), (TOL, math.radians(95.0)), (TOL, math.pi)):
        a = args[:2] + (tm,) + args[3:]
        got, want = dev_inv(lib, *a, Hs, Ws, tol=tol), inv_restate(*a, Hs, Ws, tol=tol)
        assert same(got, want), f"fisheye inverse map {Hs}x{Ws} tol {tol} theta_max {tm}: {first_diff(got, want)}"
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ 7. round trip
ROUND_SHAPE = (64, 257)
ROUND_TOLS = (TOL, 1e-9)


def round_view():
    """The four-coefficient lens with a field of +-60 degrees along a raw row of 257 pixels (fx = 128 / theta_d(60 degrees)), looking into a
    rectified frame rotated by about a degree."""
    th = math.radians(60.0)
    th_d = th * (1 + sum(c * th ** (2 * i + 2) for i, c in enumerate(K_FOUR)))
    return rc.pinhole(128.0 / th_d, 124.0, 128.3, 31.6), K_FOUR, lio.fisheye_theta_max(K_FOUR), rc.rot(1.0, -0.8, 1.2), 60.0, 128.0, 32.0


def round_trip_figures(inv, tol):
    """-> dict(kept: the share of raw pixels the inverse keeps, err: the largest |forward(xs, ys) - (u, v)| over them, px, f32: the f32 term,
    bound = tol + f32).  The f32 term: (xs, ys) are stored rounded to f32, each off by at most half an ulp of the largest rectified coordinate;
    through the forward model a coordinate moves by at most the absolute row sum of the Jacobian d(u, v) / d(xs, ys) times that, and the
    Jacobian comes from central differences of the plain-form model (step 1e-3 px: truncation of order 1e-6 relative, rounding 1e-10)."""
    K, k, tm, R, f, cx, cy = round_view()
    ok = ~np.isnan(inv[..., 0])
    vs, us = np.nonzero(ok)
    xs, ys = inv[ok][:, 0].astype(D), inv[ok][:, 1].astype(D)
    err = float(np.abs(forward(K, k, R, f, cx, cy, xs, ys) - np.stack([us, vs], 1)).max())
    h = 1e-3
    jx = (forward(K, k, R, f, cx, cy, xs + h, ys) - forward(K, k, R, f, cx, cy, xs - h, ys)) / (2 * h)
    jy = (forward(K, k, R, f, cx, cy, xs, ys + h) - forward(K, k, R, f, cx, cy, xs, ys - h)) / (2 * h)
    stretch = float((np.abs(jx) + np.abs(jy)).max())
    half_ulp = 0.5 * float(np.spacing(F(max(np.abs(xs).max(), np.abs(ys).max()))))
    return dict(kept=float(ok.mean()), err=err, f32=stretch * half_ulp, bound=float(tol) + stretch * half_ulp, stretch=stretch)


def case_round_trip(lib=None, restated=False):
    """For every raw pixel the inverse keeps, the plain-form model at its f32 (xs, ys) returns to (u, v) within tol plus the f32 term, and at
    least 90 % of the raw pixels are kept.  restated: of the numpy restatement alone.
    Measured (numpy restatement, 10 steps; the device returns the same bytes): every pixel kept; error 1.604e-5 px at tol 1e-3 and at tol 1e-9,
    against an f32 term of 1.642e-5 px (a stretch of 2.15 raw pixels per rectified pixel, half an ulp of 7.6e-6 px at a coordinate near 240):
    the Newton residual itself is of order 1e-14 px, and the error is the f32 rounding of (xs, ys) alone."""
    Hs, Ws = ROUND_SHAPE
    K, k, tm, R, f, cx, cy = round_view()
    out = {}
    for tol in ROUND_TOLS:
        want = inv_restate(K, k, tm, R, f, cx, cy, Hs, Ws, tol=tol)
        inv = want if restated else dev_inv(lib, K, k, tm, R, f, cx, cy, Hs, Ws, tol=tol)
        fig = round_trip_figures(inv, tol)
        print(f"fisheye round trip, {'numpy restatement' if restated else 'device'}, tol {tol}:", fig)
        assert fig["kept"] >= 0.9 and fig["err"] <= fig["bound"], fig
        assert restated or same(inv, want)
        out[tol] = fig
    return out


# ------------------------------------------------------------------------------------------------ 8. refusals
def case_refusals(lib):
    L = api.load(lib)
    vp = C.c_void_p
    H, W = 3, 5
    buf = pc.Guarded(lib, H * W * 2)
    mp = buf.ptr
    eye = (C.c_double * 9)(*np.eye(3).reshape(9))
    ARG, UNSUP = api.LES_HIP_ERR_ARG, api.LES_HIP_ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")
    cam = api.fisheye(rc.pinhole(10.0, 10.0, 2.0, 1.0), K_FOUR, 1.5)

    def fmap(cam_=cam, M=eye, f=10.0, d_map=mp, H_=H, W_=W):
        return L.les_hip_rectify_map_fisheye(C.byref(cam_) if cam_ is not None else None, M, f, 2.0, 1.0, vp(d_map) if d_map else None, H_, W_, 0, None)

    def umap(cam_=cam, R=eye, f=10.0, steps=10, tol=1e-3, d_map=mp, H_=H, W_=W):
        return L.les_hip_unrectify_map_fisheye(C.byref(cam_) if cam_ is not None else None, R, f, 2.0, 1.0, steps, tol, vp(d_map) if d_map else None, H_, W_, 0, None)

    def lens(fx=10.0, fy=10.0, k=K_FOUR, theta_max=1.5):
        return api.fisheye(rc.pinhole(fx, fy, 2.0, 1.0), k, theta_max)

    cams = [lens(fx=0.0), lens(fy=-1.0), lens(fx=nan), lens(fy=inf)]                                                          # the pinhole entries' refusals
    cams += [lens(k=(nan,)), lens(k=(0.0, inf)), lens(k=(0.0, 0.0, -inf)), lens(k=(0.0, 0.0, 0.0, nan))]                       # a k that is not finite
    cams += [lens(theta_max=t) for t in (nan, 0.0, -0.0, -1.0, float(np.nextafter(math.pi, 4.0)), 4.0, inf, -inf)]              # theta_max outside (0, pi]
    refused = []
    for call in (fmap, umap):
        refused += [call(cam_=None), call(None if call is fmap else cam, None), call(d_map=None), call(H_=0), call(W_=0), call(H_=-2), call(W_=-1), call(f=0.0),
                    call(f=nan), call(f=inf), call(f=-1.0), call(d_map=mp + 4)]
        refused += [call(cam_=c) for c in cams]
    refused += [umap(steps=0), umap(steps=-1), umap(steps=65), umap(tol=0.0), umap(tol=-1e-3), umap(tol=nan)]
    assert refused == [ARG] * len(refused), refused
    assert L.les_hip_last_error() != b""
    big = [fmap(H_=65536), umap(H_=65536)]                                                                                     # the launch grid
    assert big == [UNSUP] * len(big), big
    assert (buf.check() == buf.g).all(), "a refused call wrote"
    for call in (lambda: api.rectify_map_fisheye(lens(theta_max=4.0), np.eye(3), 10.0, 2.0, 1.0, mp, H, W, lib=lib),
                 lambda: api.unrectify_map_fisheye(cam, np.eye(3), 10.0, 2.0, 1.0, mp, H, W, steps=0, lib=lib)):
        try:
            call()
            raise AssertionError("accepted")
        except api.LesHipError as ex:
            assert f"error {ARG}" in str(ex)
    assert (buf.check() == buf.g).all(), "a refused call wrote"
    # theta_max = pi itself is inside, and a good call still works afterwards
    assert fmap(cam_=lens(theta_max=math.pi)) == api.LES_HIP_OK and not (buf.check() == buf.g).any()
    buf2 = pc.Guarded(lib, H * W * 2)
    assert umap(d_map=buf2.ptr) == api.LES_HIP_OK and not (buf2.check() == buf2.g).all()
    return len(refused) + len(big)


# ------------------------------------------------------------------------------------------------ 9 - 11. the cones crop through a fisheye rig
RAW_SIZE = rc.RAW_SIZE                   # 108 x 136 raw frames
CONES_F = 76.0                           # the focal length the 96 x 120 crop is given: its corner, 76.1 px from the centre, lies 45.04 degrees off the axis
CONES_RIG = dict(angles=(1.0, -0.8, 1.2), T=(-0.16, 0.004, -0.003), k0=K_FOUR, k1=(-0.03, 0.008, -0.003, 0.0005))
RENDER_STEPS = 30
CONES_FOCAL = ((98.0, 99.0), (97.0, 100.0))           # (fx, fy) of the two raw cameras


@functools.lru_cache(maxsize=None)
def cones_setup():
    """rectify_cases.cones_setup for a fisheye rig: the cones crop as the rectified truth at f = 76 px, two fisheye cameras of different
    four-coefficient lenses, about 1 degree of rig rotation; the raw frames are rendered in numpy: every raw pixel -> its ray by an fp64
    Newton inversion with 30 steps -> the rectified frame -> the truth image, bilinear.  Raw focal lengths of about 98 px (x) and 100 px (y):
    the crop's half width, 38 degrees off the axis, lands 64 px from the centre of a raw row of 136 pixels, and its half height, 32 degrees, 55 px
    from the centre of a raw column of 108: every column of the rectified frame has raw pixels, a row or two at the top and at the bottom have
    none.  (Columns without raw pixels would lie in the matcher's search range as black pixels -- what MidV3(valid=True) is for, not this test.)"""
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    assert math.degrees(math.atan(math.hypot(0.5 * (W - 1), 0.5 * (H - 1)) / CONES_F)) >= 45.0 and CONES_F <= 77.0
    f, principal = CONES_F, (0.5 * (W - 1), 0.5 * (W - 1), 0.5 * (H - 1))
    Hs, Ws = RAW_SIZE
    K0 = rc.pinhole(*CONES_FOCAL[0], 0.5 * (Ws - 1) + 0.8, 0.5 * (Hs - 1) - 0.6)
    K1 = rc.pinhole(*CONES_FOCAL[1], 0.5 * (Ws - 1) - 1.1, 0.5 * (Hs - 1) + 0.7)
    R, T = rc.rot(*CONES_RIG["angles"]), np.array(CONES_RIG["T"])
    tr = lio.stereo_rectify(K0, CONES_RIG["k0"], K1, CONES_RIG["k1"], R, T, f=f, principal=principal, model="fisheye")
    raws = []
    for m, (K, k, im) in enumerate(((K0, CONES_RIG["k0"], imL), (K1, CONES_RIG["k1"], imR))):
        vs, us = np.mgrid[0:Hs, 0:Ws].astype(D)
        Q = unproject(K, k, us, vs, RENDER_STEPS) @ tr[f"R{m}"].T
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


def cones_rectifier(lib, **kw):
    from localexpstereo_amd import stereo
    s = cones_setup()
    return stereo.Rectifier(s["K0"], CONES_RIG["k0"], s["K1"], CONES_RIG["k1"], s["R"], s["T"], raw_size=RAW_SIZE, size=s["gt"].shape, f=s["f"],
                            principal=s["principal"], device=_dev(lib), lib=lib, model="fisheye", **kw)


def cones_maps():
    """The numpy restatements of the rig's forward and inverse maps, per view."""
    s = cones_setup()
    tr = s["transform"]
    H, W = s["gt"].shape
    Hs, Ws = RAW_SIZE
    fwd = [map_restate(tr[f"K{m}"], tr[f"dist{m}"], tr[f"theta_max{m}"], tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], H, W) for m in (0, 1)]
    inv = [inv_restate(tr[f"K{m}"], tr[f"dist{m}"], tr[f"theta_max{m}"], tr[f"R{m}"], tr["f"], tr[f"cx{m}"], tr["cy"], Hs, Ws) for m in (0, 1)]
    return fwd, inv


@functools.lru_cache(maxsize=None)
def cones_restated():
    """The numpy restatement of the whole chain on the raw fisheye pair -> (imL, imR, validL, validR)"""
    s = cones_setup()
    out = [rc.remap_restate(raw, mp, 1) for raw, mp in zip((s["rawL"], s["rawR"]), cones_maps()[0])]
    return out[0][0], out[1][0], out[0][1] != 0, out[1][1] != 0


def raw_crop(raw):
    (Hs, Ws), (H, W) = RAW_SIZE, cones_setup()["gt"].shape
    return np.ascontiguousarray(raw[(Hs - H) // 2:(Hs - H) // 2 + H, (Ws - W) // 2:(Ws - W) // 2 + W])


def cones_figures(imL, imR, validL, validR):
    s = cones_setup()
    both = validL & validR
    return dict(valid_both=float(both.mean()), rect_L=rc.mad(imL, s["imL"], both), rect_R=rc.mad(imR, s["imR"], both),
                raw_L=rc.mad(raw_crop(s["rawL"]), s["imL"], both), raw_R=rc.mad(raw_crop(s["rawR"]), s["imR"], both))


def case_cones_restated():
    """The caps hold for the numpy restatement alone: at least 90 % of the pixels valid in both views, the rectified pair at most half as far
    from the original as the raw pair's centre crop."""
    fig = cones_figures(*cones_restated())
    print("cones through the fisheye rig, numpy restatement:", fig)
    assert fig["valid_both"] >= 0.9, fig
    assert fig["rect_L"] <= 0.5 * fig["raw_L"] and fig["rect_R"] <= 0.5 * fig["raw_R"], fig
    return fig


def case_cones(lib):
    """The raw fisheye pair through stereo.Rectifier(model="fisheye") against the original pair and against the numpy restatement of the whole
    chain; crop(); unrectify of a fronto-parallel label map; to_raw.
    Measured (the device returns the restatement's bytes, so there is one set of figures): 98.1 % of the pixels valid in both views; mean
    absolute difference to the original pair 4.56 (left) and 4.41 (right) grey levels, against 24.55 and 22.75 for the raw pair's centre crop."""
    from localexpstereo_amd import stereo
    s = cones_setup()
    tr = s["transform"]
    H, W = s["gt"].shape
    Hs, Ws = RAW_SIZE
    rect = cones_rectifier(lib)
    assert rect.model == "fisheye" and rect.steps == api.FISHEYE_STEPS and rect.transform["model"] == "fisheye"
    fwd, inv = cones_maps()
    for m in (0, 1):
        assert same(rect.maps[m].cpu().numpy(), fwd[m]), f"map {m}: {first_diff(rect.maps[m].cpu().numpy(), fwd[m])}"
        assert same(rect.inverse_maps[m].cpu().numpy(), inv[m]), f"inverse map {m}: {first_diff(rect.inverse_maps[m].cpu().numpy(), inv[m])}"
    got = rect.rectify(s["rawL"], s["rawR"])
    want = cones_restated()
    for key, w in zip(("imL", "imR", "validL", "validR"), want):
        assert same(got[key], w), f"{key}: {first_diff(got[key], w)}"
    fig, fig_np = cones_figures(got["imL"], got["imR"], got["validL"], got["validR"]), cones_figures(*want)
    print("cones through the fisheye rig, device:", fig)
    assert fig == fig_np and fig["valid_both"] >= 0.9, (fig, fig_np)
    assert fig["rect_L"] <= 0.5 * fig["raw_L"] and fig["rect_R"] <= 0.5 * fig["raw_R"], fig
    # crop() returns exactly the crop, and rebuilds the inverse maps from the shifted intrinsics
    best = rect.valid_rect()
    assert best == stereo.largest_rect(want[2] & want[3]) and best[2] * best[3] >= 0.8 * H * W and best[2:] != (H, W), best
    for r in ((3, 10, 20, 100), None):
        c = rect.crop(r)
        y0, x0, h, w = best if r is None else r
        out = c.rectify(s["rawL"], s["rawR"])
        for key in ("imL", "imR", "validL", "validR"):
            assert same(out[key], np.ascontiguousarray(got[key][y0:y0 + h, x0:x0 + w])), (r, key)
        assert r is not None or (out["validL"].all() and out["validR"].all())
        tc = c.transform
        assert c.model == "fisheye" and c.size == (h, w) and (tc["cx0"], tc["cx1"], tc["cy"]) == (tr["cx0"] - x0, tr["cx1"] - x0, tr["cy"] - y0)
        for m in (0, 1):
            w_inv = inv_restate(tc[f"K{m}"], tc[f"dist{m}"], tc[f"theta_max{m}"], tc[f"R{m}"], tc["f"], tc[f"cx{m}"], tc["cy"], Hs, Ws)
            assert same(c.inverse_maps[m].cpu().numpy(), w_inv), (r, m)
    # a fronto-parallel label map: every valid point, rotated into the rectified frame, has the one Z = f baseline / (d + doffs)
    n = 0
    for m, d in ((0, 20.0), (1, 7.5)):
        lab = np.zeros((H, W, 4), F)
        lab[..., 2] = d
        out = rect.unrectify(lab, viewMode=m)
        ok = out["valid"]
        inside = uc.lab_parts(lab, None, inv[m], tr[f"R{m}"].T, tr["f"], tr[f"cx{m}"], tr["cy"], tr["doffs"], tr["baseline"])[1]["inside"]
        assert same(ok, inside) and ok.sum() >= 0.5 * Hs * Ws, (m, int(ok.sum()))
        Z = out["points"][ok].astype(D) @ tr[f"R{m}"][2]
        assert np.allclose(Z, s["f"] * tr["baseline"] / (d + tr["doffs"]), rtol=1e-5, atol=0.0), (m, float(Z.min()), float(Z.max()))
        assert np.isnan(out["points"][~ok]).all()
        n += int(ok.sum())
    # to_raw(rectify(raw)) is valid wherever the inverse map lies inside the frame
    for m, name in ((0, "L"), (1, "R")):
        back, valid = rect.to_raw(got["im" + name], viewMode=m, interp="linear")
        xs, ys = inv[m][..., 0].astype(D), inv[m][..., 1].astype(D)
        with np.errstate(invalid="ignore"):
            inside = (xs >= 0.0) & (xs <= W - 1.0) & (ys >= 0.0) & (ys <= H - 1.0)
        assert same(valid, inside) and inside.any() and not inside.all()
        seen = inside & rc.valid_of(np.stack([np.clip(xs, 0, W - 1), np.clip(ys, 0, H - 1)], -1).astype(F), H, W)
        print(f"to_raw(rectify(raw)) view {m}: mean absolute difference to the raw frame over {int(seen.sum())} pixels:", rc.mad(back, s["raw" + name], seen))
    return dict(fig, points=n)


# Measured on the CPU simulator build with the numpy restatement of the rectification fed into rectify_cases.wta_bad1 (case_matcher(sim_lib,
# rectified=cones_restated())): bad-1.0 over 11 245 pixels: original pair 11.57 %, rectified pair 15.90 %, raw pair 98.16 %.  The margin is
# that excess plus one percentage point: two resamplings blur -- the second one stretches the raw frame's border by 1 / cos^2(38 degrees) =
# 1.6 --, and the rate moves by single pixels on a crop this small.  (The volumes are exact: the MI355X gives the same figures.)
MATCHER_EXCESS = 0.043309
MATCHER_MARGIN = MATCHER_EXCESS + 0.01


def case_matcher(lib, rectified=None):
    """rectify_cases.case_matcher on the fisheye rig: bad-1.0 of the one-view wta against the ground truth over the known pixels valid in both
    views, on the original pair, the fisheye-rectified pair and the raw pair (its centre crop).  rectified: (imL, imR, validL, validR) to use
    in the place of the Rectifier's output (the measurement of the margin feeds the numpy restatement).
    Measured (simulator build, numpy restatement of the rectification; 11 245 pixels): original 11.57 %, rectified 15.90 %, raw 98.16 %; the
    rectified pair may exceed the original by MATCHER_MARGIN = 4.33 + 1 points, and the raw pair must exceed the rectified one by more."""
    s = cones_setup()
    if rectified is None:
        r = cones_rectifier(lib).rectify(s["rawL"], s["rawR"])
        rectified = (r["imL"], r["imR"], r["validL"], r["validR"])
    imL, imR, validL, validR = rectified
    gt = s["gt"]
    mask = (gt > 0) & np.isfinite(gt) & validL & validR
    out = dict(pixels=int(mask.sum()), original=rc.wta_bad1(lib, s["imL"], s["imR"], gt, mask), rectified=rc.wta_bad1(lib, imL, imR, gt, mask),
               raw=rc.wta_bad1(lib, raw_crop(s["rawL"]), raw_crop(s["rawR"]), gt, mask))
    print("one-view wta on the cones crop through the fisheye rig, bad-1.0:", out, "margin", MATCHER_MARGIN)
    assert out["pixels"] >= 8000, out
    assert out["rectified"] <= out["original"] + MATCHER_MARGIN, out
    assert out["raw"] > out["rectified"] + MATCHER_MARGIN, out
    return out


# ------------------------------------------------------------------------------------------------ 12. the pinhole model is untouched
def case_pinhole_untouched(lib):
    """With `model` left at its default the cones rig of rectify_cases gives what it gave: stereo_rectify's dict, Rectifier.maps and
    .inverse_maps as the pinhole restatements of rectify_cases / unrectify_cases, rectify's bytes."""
    s = rc.cones_setup()
    rect = rc.cones_rectifier(lib)
    assert rect.model == "pinhole" and rect.steps == api.UNRECTIFY_STEPS
    assert sorted(rect.transform) == PINHOLE_KEYS
    _same_transform(rect.transform, s["transform"])
    H, W = s["gt"].shape
    for m, args in enumerate(uc.cones_views()):
        K, dist, R, f, cx, cy = args
        assert same(rect.maps[m].cpu().numpy(), rc.map_restate(K, dist, R.T, f, cx, cy, H, W)), m
        assert same(rect.inverse_maps[m].cpu().numpy(), uc.inv_restate(*args, *rc.RAW_SIZE)), m
    got = rect.rectify(s["rawL"], s["rawR"])
    for key, w in zip(("imL", "imR", "validL", "validR"), rc.cones_restated()):
        assert same(got[key], w), key
    from localexpstereo_amd import stereo
    named = stereo.Rectifier(s["K0"], rc.CONES_RIG["dist0"], s["K1"], rc.CONES_RIG["dist1"], s["R"], s["T"], raw_size=rc.RAW_SIZE, size=s["gt"].shape, f=s["f"],
                             principal=s["principal"], device=_dev(lib), lib=lib, model="pinhole", fov=120.0)
    for m in (0, 1):
        assert same(named.maps[m].cpu().numpy(), rect.maps[m].cpu().numpy()) and same(named.inverse_maps[m].cpu().numpy(), rect.inverse_maps[m].cpu().numpy())
    return True
