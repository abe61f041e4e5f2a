"""Cases of the 3D reconstruction (csrc/les_reproject.h: les_hip_reproject, les_hip_mesh, les_hip_mesh_tile, FastGCStereo.reconstruct), shared by the
simulator tests (-m "not gpu") and the MI355X tests (-m gpu) of test_reproject.py.  `lib` = the simulator build's path, None = the HIP build.

The definition, restated in numpy.  Calibration (f, cx, cy, doffs, baseline) in float32; view m has cx_m = cx + (m ? doffs : 0).  Per pixel (x, y)
with label (a, b, c, .): d = (a x + b y) + c in float32, un-fused; then in float64 from the float32 inputs, in this order, rounded to float32 once:
D = d + doffs; valid iff d finite, D > 0, the drop mask is zero, and Z <= z_max when z_max > 0; Z = (f baseline) / D; X = ((x - cx_m) Z) / f;
Y = ((y - cy) Z) / f; n = (a f, b f, ((a cx_m + b cy) + c) + doffs); normal = -n / sqrt((nx nx + ny ny) + nz nz).  Invalid pixels: NaN
(0x7fc00000) in both maps, 0 in the valid map; valid: 255.
Mesh: p, q connected iff both valid and |l_p(p) - l_q(p)| + |l_p(q) - l_q(q)| <= max_jump in float32; quad (x, y) -> T0 = (p00, p01, p10),
T1 = (p10, p01, p11), each iff its three edges are connected; vertex k = the k-th valid pixel in row-major order; triangles in row-major quad
order, T0 first.  Everything is compared bit for bit."""
import functools
import math
import os
import tempfile

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import io as lio
from tests import post_cases as pcs

F32, F64 = np.float32, np.float64
QNAN = np.array([0x7fc00000], np.uint32).view(F32)[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ restatement
def reproject_ref(lab, calib, mode, drop=None, z_max=None, exact=False):
    """(points, normals, valid) as les_hip_reproject writes them.  calib: (f, cx, cy, doffs, baseline).  exact: the float64 values before the
    final rounding, and the un-normalised n, as (P, n, valid) -- for the identities."""
    lab = np.asarray(lab, F32)
    H, W = lab.shape[:2]
    f, cx, cy, doffs, bl = (F64(F32(v)) for v in calib)
    cxm = cx + doffs if mode else cx
    ys, xs = np.mgrid[0:H, 0:W].astype(F64)
    d = pcs.disparities(lab)
    with np.errstate(all="ignore"):
        D = d.astype(F64) + doffs
        valid = np.isfinite(d) & (D > 0)
        if drop is not None:
            valid &= np.asarray(drop) == 0
        Z = (f * bl) / D
        if z_max is not None and z_max > 0:
            valid &= Z <= F64(F32(z_max))
        X = ((xs - cxm) * Z) / f
        Y = ((ys - cy) * Z) / f
        a, b, c = (lab[..., k].astype(F64) for k in range(3))
        nx, ny, nz = a * f, b * f, ((a * cxm + b * cy) + c) + doffs
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        P, n = np.stack([X, Y, Z], -1), np.stack([nx, ny, nz], -1)
        if exact:
            return P, n, valid
        points, normals = P.astype(F32), np.stack([-nx / length, -ny / length, -nz / length], -1).astype(F32)
    points[~valid] = QNAN
    normals[~valid] = QNAN
    return points, normals, np.where(valid, 255, 0).astype(np.uint8)


def reproject_loop(lab, calib, mode, drop=None, z_max=None):
    """The definition read literally, one pixel at a time with Python floats (IEEE doubles), for tiny maps."""
    lab = np.asarray(lab, F32)
    H, W = lab.shape[:2]
    f, cx, cy, doffs, bl = (float(F32(v)) for v in calib)
    cxm = cx + doffs if mode else cx
    points, normals, valid = np.full((H, W, 3), QNAN, F32), np.full((H, W, 3), QNAN, F32), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            a, b, c = lab[y, x, :3]
            with np.errstate(all="ignore"):
                d = (a * F32(x) + b * F32(y)) + c
            assert d.dtype == F32
            D = float(d) + doffs
            if not math.isfinite(float(d)) or not D > 0 or (drop is not None and drop[y, x] != 0):
                continue
            Z = (f * bl) / D
            if z_max is not None and z_max > 0 and not Z <= float(F32(z_max)):
                continue
            X, Y = ((float(x) - cxm) * Z) / f, ((float(y) - cy) * Z) / f
            a, b, c = float(a), float(b), float(c)
            nx, ny, nz = a * f, b * f, ((a * cxm + b * cy) + c) + doffs
            length = math.sqrt((nx * nx + ny * ny) + nz * nz)
            points[y, x] = (X, Y, Z)
            normals[y, x] = (-nx / length, -ny / length, -nz / length) if length > 0 else (QNAN,) * 3
            valid[y, x] = 255
    return points, normals, valid


def _z(L, x, y):
    return (L[..., 0] * x + L[..., 1] * y) + L[..., 2]


def _psi(Lp, xp, yp, Lq, xq, yq):
    with np.errstate(all="ignore"):
        return np.abs(_z(Lp, xp, yp) - _z(Lq, xp, yp)) + np.abs(_z(Lp, xq, yq) - _z(Lq, xq, yq))


def mesh_ref(lab, valid, max_jump):
    """(vertex_index H x W int32, vertex_pixel nv int32, triangles nt x 3 int32) as les_hip_mesh writes them."""
    lab = np.asarray(lab, F32)
    H, W = lab.shape[:2]
    v = np.asarray(valid) != 0
    vi = np.where(v, np.cumsum(v.ravel()).reshape(H, W) - 1, -1).astype(np.int32)
    vpix = np.flatnonzero(v.ravel()).astype(np.int32)
    if H < 2 or W < 2:
        return vi, vpix, np.zeros((0, 3), np.int32)
    ys, xs = np.mgrid[0:H, 0:W].astype(F32)
    cut = {"00": (slice(0, H - 1), slice(0, W - 1)), "10": (slice(0, H - 1), slice(1, W)), "01": (slice(1, H), slice(0, W - 1)), "11": (slice(1, H), slice(1, W))}
    t = F32(max_jump)

    def conn(p, q):
        sp, sq = cut[p], cut[q]
        with np.errstate(all="ignore"):
            return v[sp] & v[sq] & (_psi(lab[sp], xs[sp], ys[sp], lab[sq], xs[sq], ys[sq]) <= t)
    diag = conn("10", "01")
    t0 = conn("00", "01") & conn("00", "10") & diag
    t1 = conn("10", "11") & conn("01", "11") & diag
    corners = np.stack([np.stack([vi[cut["00"]], vi[cut["01"]], vi[cut["10"]]], -1), np.stack([vi[cut["10"]], vi[cut["01"]], vi[cut["11"]]], -1)], 2)
    return vi, vpix, np.ascontiguousarray(corners[np.stack([t0, t1], -1)], np.int32).reshape(-1, 3)


def mesh_loop(lab, valid, max_jump):
    """The definition read literally, one quad at a time, for tiny maps."""
    lab = np.asarray(lab, F32)
    H, W = lab.shape[:2]
    t = F32(max_jump)
    vi, k = np.full((H, W), -1, np.int32), 0
    for y in range(H):
        for x in range(W):
            if valid[y, x]:
                vi[y, x], k = k, k + 1

    def connected(p, q):
        (xp, yp), (xq, yq) = p, q
        if not (valid[yp, xp] and valid[yq, xq]):
            return False
        lp, lq = lab[yp, xp], lab[yq, xq]
        return bool(_psi(lp, F32(xp), F32(yp), lq, F32(xq), F32(yq)) <= t)
    tri = []
    for y in range(H - 1):
        for x in range(W - 1):
            p00, p10, p01, p11 = (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
            if connected(p00, p01) and connected(p00, p10) and connected(p10, p01):
                tri.append([vi[q[1], q[0]] for q in (p00, p01, p10)])
            if connected(p10, p11) and connected(p01, p11) and connected(p10, p01):
                tri.append([vi[q[1], q[0]] for q in (p10, p01, p11)])
    return vi, np.array([y * W + x for y in range(H) for x in range(W) if valid[y, x]], np.int32), np.array(tri, np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ inputs
def calib_for(H, W):
    """A Middlebury-like calibration whose principal point is near the middle of the H x W image."""
    return (1234.5, 0.5 * W + 0.37, 0.5 * H - 0.21, 31.111, 193.001)


def _cells(H, W, rng, ch, cw, slope):
    """Slanted planes, one per ch x cw cell, disparities around 20 .. 60 at the cell."""
    lab = np.zeros((H, W, 4), F32)
    for y0 in range(0, H, ch):
        for x0 in range(0, W, cw):
            a, b = rng.uniform(-slope, slope, 2)
            lab[y0:y0 + ch, x0:x0 + cw, :3] = (a, b, rng.uniform(20, 60) - a * x0 - b * y0)
    return lab


def in_one_plane(H, W, rng):
    lab = np.zeros((H, W, 4), F32)
    lab[..., :3] = (0.0078125, -0.00390625, 40.0)      # (positive disparities at every shape of the tests)
    return dict(lab=lab, max_jump=1.0, facing=True, full=True)


def in_random_planes(H, W, rng):
    lab = np.zeros((H, W, 4), F32)
    lab[..., 0], lab[..., 1] = rng.uniform(-0.9, 0.9, (H, W)), rng.uniform(-0.9, 0.9, (H, W))
    ys, xs = np.mgrid[0:H, 0:W]
    lab[..., 2] = rng.uniform(5, 80, (H, W)) - lab[..., 0] * xs - lab[..., 1] * ys
    lab[..., 3] = rng.uniform(-1, 1, (H, W))
    return dict(lab=lab, max_jump=25.0)


def in_step(H, W, rng):
    """Two fronto-parallel halves 10 apart: at max_jump 1 the column of quads across the step is torn."""
    lab = np.zeros((H, W, 4), F32)
    lab[..., 2] = 20.0
    lab[:, (W + 1) // 2:, 2] = 30.0
    return dict(lab=lab, max_jump=1.0, facing=True, step=True)


def in_half_nan(H, W, rng):
    lab = _cells(H, W, rng, 5, 7, 0.3)
    bad = rng.random((H, W)) < 0.5
    lab[bad, 2] = np.where(rng.random(int(bad.sum())) < 0.5, np.nan, np.inf).astype(F32)
    lab[rng.random((H, W)) < 0.05, 0] = -np.inf
    return dict(lab=lab, max_jump=2.0)


def in_negative_bands(H, W, rng):
    """Bands of rows (columns where there is one row) with D < 0, D == 0 exactly, and D the smallest positive float32 step above 0."""
    lab = np.zeros((H, W, 4), F32)
    lab[..., 2] = 25.0
    doffs = F32(calib_for(H, W)[3])
    vals = [F32(-40.0), -doffs, np.nextafter(-doffs, F32(0)), F32(-31.0)]
    for k, val in enumerate(vals):
        if H > 1:
            lab[(k + 1) % H::len(vals) + 2, :, 2] = val
        else:
            lab[:, (k + 1) % W::len(vals) + 2, 2] = val
    return dict(lab=lab, max_jump=1.0)


def in_drop_mask(H, W, rng):
    lab = _cells(H, W, rng, 4, 6, 0.5)
    drop = np.where(rng.random((H, W)) < 0.3, rng.integers(1, 256, (H, W)), 0).astype(np.uint8)
    return dict(lab=lab, drop=drop, max_jump=3.0)


def in_z_max(H, W, rng):
    """Disparities on both sides of the one whose depth is z_max, and pixels AT it: Z <= z_max keeps them."""
    lab = np.zeros((H, W, 4), F32)
    lab[..., 2] = rng.choice(np.array([8.889, 68.889, 18.889, 28.889], F32), (H, W))
    f, _, _, doffs, bl = (F64(F32(v)) for v in calib_for(H, W))
    z_at = F32((f * bl) / (F64(F32(18.889)) + doffs))                       # rounded to float32: above or below the exact depth, the restatement decides
    return dict(lab=lab, z_max=float(z_at), max_jump=100.0)


def in_jump_zero(H, W, rng):
    """max_jump 0: only pixels of one and the same plane are joined (psi is exactly 0 there)."""
    lab = _cells(H, W, rng, 3, 5, 0.25)
    return dict(lab=lab, max_jump=0.0)


def in_jump_inf(H, W, rng):
    """max_jump +inf: every pair of valid neighbours is joined (a NaN psi is impossible here: the planes are finite and small)."""
    d = in_random_planes(H, W, rng)
    d["lab"][rng.random((H, W)) < 0.2, 2] = np.nan
    d["max_jump"] = float("inf")
    return d


def in_checkerboard(H, W, rng):
    """One plane, every other pixel dropped: ceil(H W / 2) vertices and no triangle."""
    d = in_one_plane(H, W, rng)
    ys, xs = np.mgrid[0:H, 0:W]
    d.update(drop=np.where((ys + xs) % 2 == 1, 255, 0).astype(np.uint8), facing=False, full=False, checker=True)
    return d


INPUTS = dict(one_plane=in_one_plane, random_planes=in_random_planes, step=in_step, half_nan=in_half_nan, negative_bands=in_negative_bands,
              drop_mask=in_drop_mask, z_max=in_z_max, jump_zero=in_jump_zero, jump_inf=in_jump_inf, checkerboard=in_checkerboard)
BIG_INPUTS = ("one_plane", "half_nan")      # at the shape whose tile count exceeds the scan's width


def make_input(name, H, W):
    d = INPUTS[name](H, W, np.random.default_rng(2000 + 31 * H + W + sum(map(ord, name))))
    d["lab"] = np.ascontiguousarray(d["lab"], F32)
    d.setdefault("drop", None)
    d.setdefault("z_max", None)
    d["calib"] = calib_for(H, W)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, H, W):
    """The input and its restatement -- per view (points, normals, valid), and the mesh -- computed once, shared by the simulator and the MI355X
    tests; read-only."""
    d = make_input(name, H, W)
    d["views"] = [reproject_ref(d["lab"], d["calib"], m, d["drop"], d["z_max"]) for m in (0, 1)]
    assert np.array_equal(d["views"][0][2], d["views"][1][2])                # (validity does not depend on the view)
    d["mesh"] = mesh_ref(d["lab"], d["views"][0][2], d["max_jump"])
    for a in [d["lab"], d["drop"], *d["mesh"], *d["views"][0], *d["views"][1]]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def tile(lib):
    L = api.load(lib)
    a, b = api.C.c_int(0), api.C.c_int(0)
    assert L.les_hip_mesh_tile(api.C.byref(a), api.C.byref(b)) == 0
    assert a.value > 0 and a.value % 64 == 0 and b.value > 0
    return a.value, b.value


SHAPE_IDS = ("pixel", "row", "column", "quad", "tile", "tile_plus_1", "straddle")


def shapes(lib):
    """The smallest shapes at which each piece can go wrong, from the compiled-in tile T: one pixel; one row and one column (no quads; more than
    one tile); one quad; H W = T; H W = T + 1 (two tiles, the second holds one pixel); three tiles at an odd width that divides nothing: quads
    straddle both tile borders and the width is no multiple of 4."""
    T, _ = tile(lib)
    h = next(k for k in range(2, T + 2) if (T + 1) % k == 0)                # (T + 1 = h * w; T + 1 prime: one column)
    return [(1, 1), (1, T + 5), (T + 5, 1), (2, 2), (T // 32, 32), (h, (T + 1) // h), ((2 * T) // 37 + 3, 37)]


def big_shape(lib):
    """More tiles than the scan takes per turn: its loop runs twice."""
    T, S = tile(lib)
    return (S + 1, T + 3)


# ------------------------------------------------------------------------------------------------ the restatement itself (CPU only)
def case_restatement():
    """reproject_ref == reproject_loop and mesh_ref == mesh_loop, bit for bit, on maps of at most 9 x 12 of every input kind, both views."""
    assert {"les_hip_reproject", "les_hip_mesh", "les_hip_mesh_tile"} <= set(api.SYMBOLS)      # the entries this restates
    n = 0
    for H, W in ((1, 1), (1, 9), (7, 1), (2, 2), (6, 7), (9, 12)):
        for name in INPUTS:
            d = make_input(name, H, W)
            for m in (0, 1):
                got, want = reproject_ref(d["lab"], d["calib"], m, d["drop"], d["z_max"]), reproject_loop(d["lab"], d["calib"], m, d["drop"], d["z_max"])
                for g, w, what in zip(got, want, ("points", "normals", "valid")):
                    assert np.array_equal(_bits(g), _bits(w)), (name, H, W, m, what)
            for g, w, what in zip(mesh_ref(d["lab"], got[2], d["max_jump"]), mesh_loop(d["lab"], got[2], d["max_jump"]), ("vertex_index", "vertex_pixel", "triangles")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, H, W, what)
            n += 1
    return n


def case_plane_identity():
    """For random planes and Middlebury-like calibrations, n . P = f baseline up to what the float32 evaluation of d explains.

    Exactly, n . P = Z (a x + b y + c + doffs) = f baseline (d* + doffs) / (d + doffs), d* the exact disparity and d its float32 evaluation, so
    |n . P - f baseline| = |d(n . P)/dd| |d* - d| with d(n . P)/dd = f baseline / D.  d = fl(fl(fl(a x) + fl(b y)) + c) passes four roundings
    to nearest, each at most half an ulp of its own result: |d* - d| <= (ulp(a x) + ulp(b y) + ulp(a x + b y) + ulp(d)) / 2 (float32 ulps of the
    computed values).  On top, the float64 arithmetic of the restatement and of this test: every term of n . P passes at most 13 roundings of
    relative size 2^-53 (D 1, f baseline 1, the division 1, cx_m 1, x - cx_m 1, its product and division 2, a f 1, the term's product 1, the
    two sums 2; n_z: 5 instead), each relative to a partial result no larger than M = |a f X| + |b f Y| + (|a cx_m| + |b cy| + |c| + |doffs|) Z."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for trial in range(40):
        H, W = int(rng.integers(2, 9)), int(rng.integers(2, 12))
        calib = (rng.uniform(500, 8000), rng.uniform(0, 3000), rng.uniform(0, 2000), rng.choice([0.0, rng.uniform(0, 300)]), rng.uniform(50, 600))
        lab = np.zeros((H, W, 4), F32)
        lab[..., 0], lab[..., 1], lab[..., 2] = rng.uniform(-2, 2, (H, W)), rng.uniform(-2, 2, (H, W)), rng.uniform(-50, 300, (H, W))
        f, cx, cy, doffs, bl = (F64(F32(v)) for v in calib)
        ys, xs = np.mgrid[0:H, 0:W].astype(F32)
        ax, by = lab[..., 0] * xs, lab[..., 1] * ys
        d = (ax + by) + lab[..., 2]
        dd = 0.5 * (np.spacing(np.abs(ax)).astype(F64) + np.spacing(np.abs(by)) + np.spacing(np.abs(ax + by)) + np.spacing(np.abs(d)))
        for m in (0, 1):
            P, n, valid = reproject_ref(lab, calib, m, exact=True)
            assert valid.any()
            cxm = cx + doffs if m else cx
            a, b, c = (lab[..., k].astype(F64) for k in range(3))
            t0, t1, t2 = n[..., 0] * P[..., 0], n[..., 1] * P[..., 1], n[..., 2] * P[..., 2]
            M = np.abs(t0) + np.abs(t1) + (np.abs(a * cxm) + np.abs(b * cy) + np.abs(c) + np.abs(doffs)) * P[..., 2]
            err = np.abs(((t0 + t1) + t2) - f * bl)[valid]
            allowed = ((f * bl) / (d.astype(F64) + doffs) * dd + 13 * 2.0 ** -53 * M)[valid]
            assert (err <= allowed).all(), (trial, m, float((err / allowed).max()))
            worst = max(worst, float((err / allowed).max()))
    return worst


def case_normal_direction():
    """On a one-plane map the unit normal is the direction of the cross product of the steps to the neighbouring points, taken so that it faces the
    camera: (P(x, y + 1) - P) x (P(x + 1, y) - P), the order of T0.  The planes have dyadic coefficients, so d is exact in float32 and the points
    lie on the plane up to the float64 roundings alone (any other plane adds the rounding of d, which case_plane_identity bounds).  The points are
    the float64 ones; their coordinates carry at most 7 roundings
    of relative size u = 2^-53, so a step e is off by at most 14 u max|P|, the direction of e1 x e2 by at most
    phi = (14 u Pmax / |e1| + 14 u Pmax / |e2|) / sin(angle(e1, e2)) + 8 u (the cross product's and the normalisation's own roundings), and
    1 - cos is at most phi^2 / 2 + 4 u (the dot product's roundings)."""
    u, worst = 2.0 ** -53, 0.0
    for calib, plane in (((3997.684, 1176.728, 1011.728, 131.111, 193.001), (0.03125, -0.015625, 60.0)), ((1234.5, 6.0, 4.0, 0.0, 160.0), (0.375, 0.25, 15.0)),
                         ((2945.377, 1284.862, 954.52, 146.53, 178.089), (-0.75, 0.5, 40.0))):
        lab = np.zeros((8, 11, 4), F32)
        lab[..., :3] = plane
        for m in (0, 1):
            P, n, valid = reproject_ref(lab, calib, m, exact=True)
            assert valid.all()
            unit = -n / np.sqrt((n * n).sum(-1, keepdims=True))
            e1, e2 = P[1:, :-1] - P[:-1, :-1], P[:-1, 1:] - P[:-1, :-1]
            g = np.cross(e1, e2)
            l1, l2, lg = (np.sqrt((v * v).sum(-1)) for v in (e1, e2, g))
            cos = (g * unit[:-1, :-1]).sum(-1) / lg
            phi = (14 * u * np.abs(P).max() / l1 + 14 * u * np.abs(P).max() / l2) / (lg / (l1 * l2)) + 8 * u
            assert (cos > 0).all() and (1.0 - cos <= phi * phi / 2 + 4 * u).all(), (calib, plane, m, float((1.0 - cos).max()))
            worst = max(worst, float((1.0 - cos).max()))
            assert ((unit * P).sum(-1) < 0).all()                              # it faces the camera: towards the origin, n . P = -f baseline / |n|
    return worst


def case_ply_round_trip():
    """write_ply -> read_ply returns every array bit for bit (NaN payloads, signed zeros, every byte value), with and without the optional parts."""
    rng = np.random.default_rng(11)
    n, k = 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for nv, nt in ((0, 0), (1, 0), (257, 0), (300, 411)):
            v = rng.integers(0, 2 ** 32, (nv, 3), dtype=np.uint64).astype(np.uint32).view(F32)            # any bit pattern, NaNs included
            nrm = rng.integers(0, 2 ** 32, (nv, 3), dtype=np.uint64).astype(np.uint32).view(F32)
            if nv:
                v[0] = (-0.0, np.inf, QNAN)
            col = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
            tri = rng.integers(0, max(nv, 1), (nt, 3)).astype(np.int32)
            for with_n, with_c, with_t in ((False, False, False), (True, False, False), (False, True, True), (True, True, True)):
                path = os.path.join(tmp, f"m{k}.ply")
                k += 1
                lio.write_ply(path, v, nrm if with_n else None, col if with_c else None, tri if with_t else None)
                got = lio.read_ply(path)
                for name, want in (("vertices", v), ("normals", nrm if with_n else None), ("colors", col if with_c else None), ("triangles", tri if with_t else None)):
                    if want is None:
                        assert got[name] is None, name
                    else:
                        assert got[name].dtype == want.dtype and got[name].shape == want.shape and np.array_equal(_bits(got[name]), _bits(want)), (name, nv, nt)
                n += 1
    return n


def check_closed_form(d, H, W, nv, nt):
    """The counts known in closed form."""
    if d.get("full"):
        assert (nv, nt) == (H * W, 2 * (H - 1) * (W - 1)), (nv, nt)
    if d.get("step"):
        assert (nv, nt) == (H * W, 2 * (H - 1) * (W - 2) if W >= 2 else 0), (nv, nt)
    if d.get("checker"):
        assert (nv, nt) == ((H * W + 1) // 2, 0), (nv, nt)


def case_mesh_counts():
    """The restatement's counts in closed form: one plane, the step, the checkerboard, all NaN."""
    n = 0
    for H, W in ((1, 1), (1, 6), (5, 1), (2, 2), (7, 9), (12, 5)):
        for name in ("one_plane", "step", "checkerboard"):
            d = reference(name, H, W)
            check_closed_form(d, H, W, len(d["mesh"][1]), len(d["mesh"][2]))
            n += 1
        lab = np.full((H, W, 4), np.nan, F32)
        valid = reproject_ref(lab, calib_for(H, W), 0)[2]
        vi, vpix, tri = mesh_ref(lab, valid, float("inf"))
        assert (vi == -1).all() and len(vpix) == 0 and len(tri) == 0
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ device plumbing
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def context(lib, H, W, im=None):
    if im is None:
        im = np.full((H, W, 3), 90, np.uint8)
    return pcs.context(lib, im, im, 2)


def device_run(e, lib, d, mode):
    """reproject and mesh through the tensor forms -> host arrays (points, normals, valid, vertex_index, vertex_pixel, triangles)."""
    import torch
    dev = _dev(lib)
    lab = torch.from_numpy(np.array(d["lab"], F32)).to(dev)
    drop = torch.from_numpy(np.array(d["drop"])).to(dev) if d["drop"] is not None else None
    points, normals, valid = e.reproject(lab, api.Calib(*d["calib"]), mode=mode, drop=drop, z_max=d["z_max"], device=dev)
    e.synchronize()
    vi, vpix, tri = e.mesh(lab, valid, d["max_jump"], mode=mode, device=dev)
    assert np.array_equal(_bits(lab.cpu().numpy()), _bits(d["lab"])), "the labels were written"
    return tuple(t.cpu().numpy() for t in (points, normals, valid, vi, vpix, tri))


def device_ptr_forms(e, lib, d, H, W, want):
    """The _ptr forms: NULL points / normals leave the other outputs as they are; capacity beyond the counts stays untouched; a second call on the
    kept workspace gives the same bytes."""
    import torch
    dev = _dev(lib)
    lab = torch.from_numpy(np.array(d["lab"], F32)).to(dev)
    drop = torch.from_numpy(np.array(d["drop"])).to(dev) if d["drop"] is not None else None
    calib = api.Calib(*d["calib"])
    for with_points in (True, False):
        out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device=dev)
        valid = torch.full((H, W), 0x5A, dtype=torch.uint8, device=dev)
        e.reproject_ptr(0, lab.data_ptr(), drop.data_ptr() if drop is not None else None, calib, d["z_max"], out.data_ptr() if with_points else None,
                        None if with_points else out.data_ptr(), valid.data_ptr())
        e.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want[0] if with_points else want[1])) and np.array_equal(valid.cpu().numpy(), want[2])
    valid = torch.from_numpy(np.array(want[2])).to(dev)
    ntri = max(1, 2 * (H - 1) * (W - 1))
    for turn in range(2):
        vi = torch.full((H, W), -7, dtype=torch.int32, device=dev)
        vpix = torch.full((H * W,), -7, dtype=torch.int32, device=dev)
        tri = torch.full((ntri, 3), -7, dtype=torch.int32, device=dev)
        counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
        e.mesh_ptr(0, lab.data_ptr(), valid.data_ptr(), d["max_jump"], vi.data_ptr(), vpix.data_ptr(), tri.data_ptr(), counts.data_ptr())
        e.synchronize()
        nv, nt = (int(c) for c in counts.cpu())
        assert (nv, nt) == (len(want[4]), len(want[5])), (nv, nt)
        assert np.array_equal(vi.cpu().numpy(), want[3]) and np.array_equal(vpix.cpu().numpy()[:nv], want[4]) and np.array_equal(tri.cpu().numpy()[:nt], want[5])
        assert (vpix.cpu().numpy()[nv:] == -7).all() and (tri.cpu().numpy()[nt:] == -7).all(), "written beyond the counts"


def check_properties(d, got):
    """Properties of a device result that hold whatever the restatement says."""
    points, normals, valid, vi, vpix, tri = got
    nv = len(vpix)
    assert (np.diff(vpix.astype(np.int64)) > 0).all(), "vertex_pixel is not strictly increasing"
    assert nv == int((valid != 0).sum()) and np.array_equal(vi.ravel()[vpix], np.arange(nv, dtype=np.int32))
    if len(tri):
        assert tri.min() >= 0 and tri.max() < nv, "a vertex number outside the vertices"
    if d.get("facing") and len(tri):
        P, N = points.reshape(-1, 3)[vpix].astype(F64), normals.reshape(-1, 3)[vpix].astype(F64)
        g = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
        assert ((g * (N[tri[:, 0]] + N[tri[:, 1]] + N[tri[:, 2]])).sum(-1) > 0).all(), "a triangle faces away from its vertex normals"


def case_device(lib, name, H, W, ptr_forms=True):
    """Both views' points, normals and valid map, vertex index, vertex pixel, triangles and counts == the restatement's, bit for bit."""
    d = reference(name, H, W)
    e = context(lib, H, W)
    try:
        got = [device_run(e, lib, d, m) for m in (0, 1)]
        if ptr_forms:
            device_ptr_forms(e, lib, d, H, W, d["views"][0] + d["mesh"])
    finally:
        e.close()
    for m in (0, 1):
        want = d["views"][m] + d["mesh"]
        for g, w, what in zip(got[m], want, ("points", "normals", "valid", "vertex_index", "vertex_pixel", "triangles")):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
            differ = _bits(g) != _bits(w)
            if what == "normals" and differ.any():         # (printed before the assertion: how many values, by how many float32 ulps)
                steps = np.abs(_bits(g).astype(np.int64) - _bits(w).astype(np.int64))[differ]
                print(f"{name} {H} x {W} view {m}: {int(differ.sum())} normal components differ, by at most {int(steps.max())} ulp")
            assert not differ.any(), f"{name} {H} x {W} view {m}: {int(differ.sum())} values of {what} differ"
        check_properties(d, got[m])
    nv, nt = len(got[0][4]), len(got[0][5])
    check_closed_form(d, H, W, nv, nt)
    return dict(vertices=nv, triangles=nt)


def _refused(call, code):
    try:
        call()
    except api.LesHipError as ex:
        assert f"error {code}" in str(ex), str(ex)
        return 1
    raise AssertionError("a bad argument was accepted")


def case_refusals(lib):
    """Every refusal of les_hip_reproject and les_hip_mesh; a refused call writes nothing; max_jump +inf is accepted."""
    import torch
    H, W, dev = 6, 9, _dev(lib)
    A = api.LES_HIP_ERR_ARG
    lab = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    lab[..., 2] = 10.0
    out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device=dev)
    valid = torch.full((H, W), 0x5A, dtype=torch.uint8, device=dev)
    ints = torch.full((2 * H * W, 3), -7, dtype=torch.int32, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    good = api.Calib(*calib_for(H, W))
    n = 0
    e = context(lib, H, W)
    try:
        rp = lambda mode=0, labels=lab.data_ptr(), calib=good, v=valid.data_ptr(): e.reproject_ptr(mode, labels, None, calib, None, out.data_ptr(), None, v)
        n += _refused(lambda: rp(labels=None), A)
        n += _refused(lambda: rp(calib=None), A)
        n += _refused(lambda: rp(v=None), A)
        for mode in (-1, 2):
            n += _refused(lambda: rp(mode=mode), A)
        for f, bl in ((0.0, 100.0), (-1.0, 100.0), (float("nan"), 100.0), (float("inf"), 100.0), (1000.0, 0.0), (1000.0, -2.0), (1000.0, float("nan")), (1000.0, float("inf"))):
            n += _refused(lambda: rp(calib=api.Calib(f, 4.0, 3.0, 0.0, bl)), A)
        args = [lab.data_ptr(), valid.data_ptr(), 1.0, ints.data_ptr(), ints.data_ptr(), ints.data_ptr(), counts.data_ptr()]
        for k in (0, 1, 3, 4, 5, 6):
            n += _refused(lambda: e.mesh_ptr(0, *(None if j == k else a for j, a in enumerate(args))), A)
        for jump in (-1.0, float("nan"), -float("inf"), -1e-30):
            n += _refused(lambda: e.mesh_ptr(0, *(jump if j == 2 else a for j, a in enumerate(args))), A)
        for mode in (-1, 2):
            n += _refused(lambda: e.mesh_ptr(mode, *args), A)
        e.synchronize()
        assert (out.cpu().numpy() == 7.0).all() and (valid.cpu().numpy() == 0x5A).all() and (ints.cpu().numpy() == -7).all() and (counts.cpu().numpy() == -7).all()
        points, normals, ok = e.reproject(lab, good, device=dev)
        e.synchronize()
        vi, vpix, tri = e.mesh(lab, ok, float("inf"), device=dev)
        assert len(vpix) == H * W and len(tri) == 2 * (H - 1) * (W - 1)
    finally:
        e.close()
    # a view that was not supplied at creation
    im = np.full((H, W, 3), 90, np.uint8)
    vol = np.zeros((2, H, W), F32)
    e = api.HipCostVolumeEnergy(im, None, vol, None, windR=2, eps=1.0, th_col=0.5, lib=lib, filter="")
    try:
        n += _refused(lambda: e.reproject_ptr(1, lab.data_ptr(), None, good, None, out.data_ptr(), None, valid.data_ptr()), A)
        n += _refused(lambda: e.mesh_ptr(1, *args), A)
        e.reproject_ptr(0, lab.data_ptr(), None, good, None, out.data_ptr(), None, valid.data_ptr())
        e.synchronize()
        assert (valid.cpu().numpy() == 255).all()
    finally:
        e.close()
    return n


# ------------------------------------------------------------------------------------------------ the driver
DRIVER_CALIB = dict(f=3740.0, cx=225.0, cy=187.5, doffs=0.0, baseline=160.0)     # Middlebury 2003's focal length and baseline; the crop's centre
DRIVER_TAU = 0.05


def _same(a, b):
    return a is b or (a is not None and b is not None and np.array_equal(_bits(a), _bits(b)))


def case_driver(lib, device):
    """reconstruct on the one-view wta result of the cones crop: the dict's shapes, colors == the image at vertex_pixel, no vertex below
    min_confidence; and the labellings wta, sgm and run return are byte-identical before and after reconstruct calls."""
    from tests import sgm_cases as sg
    st, e, keep = sg.driver(lib, device, "none", evaluate_on_device=True)
    try:
        H, W = e.H, e.W

        def labellings():
            res = [st.wta((0,)), st.sgm((0,))]
            st.log = []
            res.append(st.run(0, (0,), 0, labeling="wta"))
            return res
        before = labellings()
        lab = before[0][0]
        conf = st.confidence(lab)
        plain = st.reconstruct(lab, DRIVER_CALIB)
        picky = st.reconstruct(lab, lio.calib3d(DRIVER_CALIB), conf=conf, min_confidence=DRIVER_TAU, speckle=(50, 1.0), z_max=1.0e5)
        right = st.reconstruct(lab, DRIVER_CALIB, viewMode=1, max_jump=float("inf"))     # (any map will do: the right view's frame and image)
        after = labellings()
        for a, b in zip(before, after):
            assert _same(a[0], b[0]) and _same(a[1], b[1]), "a labelling changed after reconstruct"
        rgb = e.image(0)[..., ::-1].reshape(-1, 3)
        out = {}
        for name, r in (("plain", plain), ("picky", picky), ("right", right)):
            nv, nt = len(r["vertices"]), len(r["triangles"])
            assert r["points"].shape == r["normals"].shape == (H, W, 3) and r["valid"].shape == (H, W) and r["valid"].dtype == bool
            assert r["vertices"].shape == r["vertex_normals"].shape == (nv, 3) and r["colors"].shape == (nv, 3) and r["colors"].dtype == np.uint8
            assert r["triangles"].shape == (nt, 3) and r["triangles"].dtype == np.int32 and r["vertex_pixel"].shape == (nv,)
            assert nv == int(r["valid"].sum()) and np.array_equal(r["vertex_pixel"], np.flatnonzero(r["valid"].ravel()))
            assert np.array_equal(r["colors"], (e.image(1) if name == "right" else e.image(0))[..., ::-1].reshape(-1, 3)[r["vertex_pixel"]])
            assert np.array_equal(_bits(r["vertices"]), _bits(r["points"].reshape(-1, 3)[r["vertex_pixel"]]))
            assert np.array_equal(_bits(r["vertex_normals"]), _bits(r["normals"].reshape(-1, 3)[r["vertex_pixel"]]))
            assert not np.isnan(r["vertices"]).any() and np.isnan(r["points"][~r["valid"]]).all()
            assert nt == 0 or (r["triangles"].min() >= 0 and r["triangles"].max() < nv)
            out[name] = dict(vertices=nv, triangles=nt)
        assert np.array_equal(rgb[plain["vertex_pixel"]], plain["colors"])
        # the whole call == the restatement with the driver's default max_jump (th_smooth)
        calib = tuple(DRIVER_CALIB[k] for k in ("f", "cx", "cy", "doffs", "baseline"))
        want = reproject_ref(lab, calib, 0)
        assert np.array_equal(_bits(plain["points"]), _bits(want[0])) and np.array_equal(plain["valid"], want[2] != 0)
        assert np.array_equal(plain["triangles"], mesh_ref(lab, want[2], st.p["th_smooth"])[2])
        assert plain["valid"].all() and out["plain"]["vertices"] == H * W
        # min_confidence: no vertex below the threshold, and it dropped some
        assert not (conf.ravel()[picky["vertex_pixel"]] < DRIVER_TAU).any()
        assert 0 < out["picky"]["vertices"] < out["plain"]["vertices"]
        assert out["right"]["triangles"] == 2 * (H - 1) * (W - 1)
        # the mesh goes through a PLY file with its counts
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cones.ply")
            lio.write_ply(path, picky["vertices"], picky["vertex_normals"], picky["colors"], picky["triangles"])
            back = lio.read_ply(path)
            assert back["vertices"].shape == (out["picky"]["vertices"], 3) and back["triangles"].shape == (out["picky"]["triangles"], 3)
            assert np.array_equal(back["triangles"], picky["triangles"]) and np.array_equal(back["colors"], picky["colors"])
    finally:
        e.close()
        del keep
    return out


def case_midv2_ply(lib, device, monkeypatch, layers=None, **opts):
    """A PLY written from a MidV2 run on the cones crop (1 + 1 iterations) opens in read_ply with the expected counts: one vertex per valid pixel and
    the restatement's triangles at the run's own th_smooth.  MidV2 closes its energy, so the map is reconstructed on a fresh context over the same
    images.  layers, opts: as crossview_cases.case_driver_midv2 (the simulator leg: coarse layers, filter radius 6, host cuts)."""
    from localexpstereo_amd import stereo
    from tests import crossview_cases as cv
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    data = cv.cones_data()
    run, lab, raw = stereo.MidV2(data, iterations=1, pmIterations=1, device=device, lib=lib, **opts)
    H, W = lab.shape[:2]
    calib = tuple(DRIVER_CALIB[k] for k in ("f", "cx", "cy", "doffs", "baseline"))
    want_valid = reproject_ref(lab, calib, 0)[2]
    want_tri = mesh_ref(lab, want_valid, run.p["th_smooth"])[2]
    e = pcs.context(lib, data["imL"], data["imR"], 2)
    try:
        st = stereo.FastGCStereo(e, data["imL"], data["imR"], dict(lambda_=run.p["lambda_"], th_smooth=run.p["th_smooth"], windR=2), device=device, seed=1)
        r = st.reconstruct(lab, DRIVER_CALIB)
    finally:
        e.close()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cones_midv2.ply")
        lio.write_ply(path, r["vertices"], r["vertex_normals"], r["colors"], r["triangles"])
        back = lio.read_ply(path)
    nv, nt = int((want_valid != 0).sum()), len(want_tri)
    assert nv > 0 and nt > 0
    assert back["vertices"].shape == back["normals"].shape == (nv, 3) and back["colors"].shape == (nv, 3) and back["triangles"].shape == (nt, 3)
    assert np.array_equal(back["triangles"], want_tri) and np.array_equal(_bits(back["vertices"]), _bits(r["vertices"]))
    assert np.array_equal(back["colors"], np.ascontiguousarray(data["imL"])[..., ::-1].reshape(-1, 3)[r["vertex_pixel"]])
    return dict(pixels=H * W, vertices=nv, triangles=nt)
