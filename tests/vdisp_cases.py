"""Vertical disparity (Plane::v) in the image-based energy: NaiveStereoEnergy samples the other view at (x - sign d(x, y), y + v)
(LES/StereoEnergy.h:704-729), shared by the simulator tests (-m "not gpu") and the MI355X tests (-m gpu) of tests/test_vdisp.py.

The source coordinate is defined once (src_coords) and used by both restatements: raw_np (numpy, vectorised) and raw_loop (a literal
per-pixel loop of the getAffineTransform + warpAffine reading, [recollection] of OpenCV 3.1: coordinates quantised to 1/32 pixel,
replicated border, bilinear weights as products of the two axes' f32 fractions, the four taps summed in f32).  At v == 0 (-0.0
included) the reference adds nothing and the one-row reading of the oracle's naive_raw applies.  The guided filter of a restated raw
patch comes from the oracle (Oracle.filter_subregion), the bilateral one from tests/bilateral_cases.py."""
import math

import numpy as np

from localexpstereo_amd import api
from oracle import oracle as om
from tests import bilateral_cases as bc
from tests import interp_cases as ic
from tests import parity_cases as pc
from tests.util import load_cones_crop

F32 = np.float32
SENT = np.float32(1e6)


# ------------------------------------------------------------------------------------------------ restatements
def features(im, alpha=0.9):
    """NaiveStereoEnergy's feature image {(1-alpha) B, G, R, alpha Gx} (LES/StereoEnergy.h:644-664), H x W x 4 f32."""
    im = np.asarray(im, np.uint8)
    H, W = im.shape[:2]
    f = np.empty((H, W, 4), F32)
    k = 1.0 - float(F32(alpha))
    for c in range(3):
        f[..., c] = (im[..., c].astype(np.float64) * k).astype(F32)
    gray = (im[..., 0].astype(F32) * F32(0.114) + im[..., 1].astype(F32) * F32(0.587)) + im[..., 2].astype(F32) * F32(0.299)
    xs = np.arange(W)
    gx = F32(0.5) * (gray[:, np.minimum(xs + 1, W - 1)] - gray[:, np.maximum(xs - 1, 0)])
    f[..., 3] = gx * F32(alpha)
    return f


def src_coords(X, Y, plane, sign):
    """THE source coordinate of pixel (X, Y): xs = X - sign * z(X, Y) (z = (a X + b Y) + c in f32, the subtraction in double) and
    ys = (float)Y + v (the reference's float add), as doubles."""
    a, b, c, v = (F32(t) for t in plane)
    X = np.asarray(X)
    Y = np.asarray(Y)
    with np.errstate(all="ignore"):
        z = (a * X.astype(F32) + b * Y.astype(F32)) + c
        xs = X.astype(np.float64) - float(sign) * z.astype(np.float64)
        ys = (Y.astype(F32) + v).astype(np.float64)
    return xs, ys


def _axis(s, n):
    with np.errstate(all="ignore"):
        q = np.floor(s * 32.0 + 0.5) / 32.0
        fl = np.floor(q)
        f = (q - fl).astype(F32)
        k = np.fmin(np.fmax(fl, -2.0), n + 1.0).astype(np.int64)
    return np.clip(k, 0, n - 1), np.clip(k + 1, 0, n - 1), f


def raw_np(fs, fo, fr, plane, sign, thc, thg):
    """Raw cost of `plane` over filterRect fr = (x, y, w, h): f32 [h][w].  fs / fo: this view's / the other view's feature image."""
    x0, y0, w, h = (int(t) for t in fr)
    H, W = fs.shape[:2]
    Y, X = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    xs, ys = src_coords(X, Y, plane, sign)
    xa, xb, wx = _axis(xs, W)
    own = fs[Y, X]
    with np.errstate(all="ignore"):
        if F32(plane[3]) != 0:
            ya, yb, wy = _axis(ys, H)
            fx0, fy0 = F32(1) - wx, F32(1) - wy
            w00, w01, w10, w11 = fy0 * fx0, fy0 * wx, wy * fx0, wy * wx
            t00, t01, t10, t11 = fo[ya, xa], fo[ya, xb], fo[yb, xa], fo[yb, xb]
            s = ((t00 * w00[..., None] + t01 * w01[..., None]) + t10 * w10[..., None]) + t11 * w11[..., None]
        else:
            w0 = F32(1) - wx
            s = w0[..., None] * fo[Y, xa] + wx[..., None] * fo[Y, xb]
        d = np.abs(own - s)
        col = (d[..., 0] + d[..., 1]) + d[..., 2]
        grad = d[..., 3]
        thc, thg = F32(thc), F32(thg)
        return (np.where(col < thc, col, thc) + np.where(grad < thg, grad, thg)).astype(F32)


def _q32(s):
    q = math.floor(s * 32.0 + 0.5) / 32.0 if math.isfinite(s) else s
    return q


def raw_loop(fs, fo, fr, plane, sign, thc, thg):
    """raw_np as a literal per-pixel loop of the warpAffine reading: three source points (the filterRect's corners, y += v when
    v != 0) define the map; at pixel (X, Y) it gives (X - sign z(X, Y), Y + v); each coordinate is rounded to 1/32, split into an
    integer and a fraction, the taps clamped into the image, the bilinear weights formed as products and the taps summed in order."""
    x0, y0, w, h = (int(t) for t in fr)
    H, W = fs.shape[:2]
    v = F32(plane[3])
    out = np.zeros((h, w), F32)
    for yy in range(h):
        for xx in range(w):
            X, Y = x0 + xx, y0 + yy
            xs, ys = (float(t) for t in src_coords(X, Y, plane, sign))
            taps = []
            for s, n in ((xs, W), (ys, H)):
                q = _q32(s)
                fl = math.floor(q) if math.isfinite(q) else q
                f = F32(q - fl) if math.isfinite(q) else F32("nan")
                k = -2 if math.isnan(fl) else int(min(max(fl, -2.0), n + 1.0))
                taps.append((min(max(k, 0), n - 1), min(max(k + 1, 0), n - 1), f))
            (xa, xb, fx), (ya, yb, fy) = taps
            own = fs[Y, X]
            with np.errstate(all="ignore"):
                if v != 0:
                    wts = (((F32(1) - fy) * (F32(1) - fx)), ((F32(1) - fy) * fx), (fy * (F32(1) - fx)), (fy * fx))
                    pts = (fo[ya, xa], fo[ya, xb], fo[yb, xa], fo[yb, xb])
                    smp = [F32(0)] * 4
                    for ch in range(4):
                        acc = pts[0][ch] * wts[0]
                        for t in range(1, 4):
                            acc = F32(acc + pts[t][ch] * wts[t])
                        smp[ch] = acc
                else:
                    smp = [F32((F32(1) - fx) * fo[Y, xa][ch] + fx * fo[Y, xb][ch]) for ch in range(4)]
                col = F32(F32(abs(own[0] - smp[0]) + abs(own[1] - smp[1])) + abs(own[2] - smp[2]))
                grad = F32(abs(own[3] - smp[3]))
                out[yy, xx] = F32((col if col < F32(thc) else F32(thc)) + (grad if grad < F32(thg) else F32(thg)))
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def restatement_planes(H, W):
    nan, inf = float("nan"), float("inf")
    vs = [1 / 64, -1 / 64, 3 / 64, -3 / 64, 0.5 + 1 / 64, 1 / 32 - 1e-7, 1.0, -2.0, 3.0, 0.37, -0.37, H + 5.0, -(H + 7.0), 1e9]
    planes = [(0.02, -0.01, 6.5, v) for v in vs]
    planes += [(0.0, 0.0, 3.0 + 1 / 64, 0.25), (0.1, 0.05, -30.0, 1.5), (nan, 0.0, 2.0, 1.0), (0.0, 0.0, inf, 1.0), (0.0, 0.0, 2.0, nan),
               (0.0, 0.0, 2.0, inf), (0.0, 0.0, 2.0, -inf), (0.0, 0.0, 5.0, 0.0), (0.01, 0.0, 5.0, -0.0), (nan, nan, nan, 0.0)]
    return planes


def case_restatement_matches_loop():
    imL, imR = load_cones_crop()
    f = (features(imL), features(imR))
    H, W = imL.shape[:2]
    thc, thg = F32(10.0) * (F32(1) - F32(0.9)), F32(2.0) * F32(0.9)
    for mode in (0, 1):
        sign = -1.0 if mode else 1.0
        for i, pl in enumerate(restatement_planes(H, W)):
            fr = ((i * 7) % (W - 12), (i * 5) % (H - 9), 12, 9) if i % 3 else (0, H - 9, 12, 9)
            a = raw_np(f[mode], f[1 - mode], fr, pl, sign, thc, thg)
            b = raw_loop(f[mode], f[1 - mode], fr, pl, sign, thc, thg)
            assert np.array_equal(bits(a), bits(b)), (mode, pl)


def case_v0_is_the_oracle():
    """At v = 0 and v = -0.0 the restated raw cost is the oracle's (naive_raw) bit for bit: fed through the oracle's own guided filter it
    gives exactly the oracle's unfiltered-check output."""
    imL, imR = load_cones_crop()
    o = om.Oracle.naive(imL, imR, 31.0, windR=20)
    f = (features(imL), features(imR))
    H, W = imL.shape[:2]
    thc, thg = F32(10.0) * (F32(1) - F32(0.9)), F32(2.0) * F32(0.9)
    calls = [(0, (19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 14.25)), (1, (0, 0, W, H), (0, 0, W, H), (-0.02, 0.01, 17.3)),
             (1, (30, 0, 90, 60), (50, 0, 50, 40), (0.3, 0.2, -20.0)), (0, (10, 8, 80, 70), (30, 28, 40, 30), (0.0, 0.0, float("inf")))]
    for mode, fr, tr, abc in calls:
        raws = [raw_np(f[mode], f[1 - mode], fr, abc + (v,), -1.0 if mode else 1.0, thc, thg) for v in (0.0, -0.0)]
        assert np.array_equal(bits(raws[0]), bits(raws[1]))
        q = o.filter_subregion(fr, raws[0], mode)
        ref = o.unary(fr, tr, abc + (0.0,), mode=mode, check=False)
        sy, sx = tr[1] - fr[1], tr[0] - fr[0]
        got = q[sy:sy + tr[3], sx:sx + tr[2]]
        want = ref[tr[1]:tr[1] + tr[3], tr[0]:tr[0] + tr[2]]
        assert np.array_equal(bits(got), bits(want)), (mode, fr)


# ------------------------------------------------------------------------------------------------ device
class VPair:
    """An image-based library context of filter `filter` plus the oracle (guided filter, validity) over the cones crop (or the pair
    `ims`).  Duck-types interp_cases.InterpPair so that its call / batch runners and comparison apply."""

    def __init__(self, lib, filter="GF", windR=20, sig2=10.0, max_disp=31.0, ims=None):
        self.imL, self.imR = load_cones_crop() if ims is None else ims
        self.H, self.W = self.imL.shape[:2]
        self.D = int(max_disp) + 1
        self.filter = filter
        self.R = windR if filter in ("BF", "BL") else 0
        self.sig2 = sig2
        self.f = (features(self.imL), features(self.imR))
        self.thc, self.thg = F32(10.0) * (F32(1) - F32(0.9)), F32(2.0) * F32(0.9)
        self.o = om.Oracle.naive(self.imL, self.imR, max_disp, windR=windR)
        self.e = api.HipCostVolumeEnergy.naive(self.imL, self.imR, windR=windR, eps=sig2 if filter in ("BF", "BL") else 1e-4, max_disp=max_disp,
                                               lib=lib, filter=filter)

    def close(self):
        self.e.close()

    def raw(self, fr, plane, mode):
        return raw_np(self.f[mode], self.f[1 - mode], fr, plane, -1.0 if mode else 1.0, self.thc, self.thg)

    expected = ic.InterpPair.expected


def mixed_calls(H, W):
    """Single calls of both views with v = 0 and v != 0 (fractional, integer, beyond the image, NaN) and special planes."""
    calls = []
    base = [((0, 0, 62, 62), (0, 0, 42, 42), (0.0, 0.0, 12.0)), ((19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 14.25)),
            ((W - 62, H - 62, 62, 62), (W - 42, H - 42, 42, 42), (-0.11, 0.07, 9.5)), ((0, 0, W, H), (0, 0, W, H), (0.01, 0.02, 10.125)),
            ((30, 0, 90, 60), (50, 0, 50, 40), (0.3, 0.2, -20.0)), ((40, 40, 41, 41), (60, 60, 1, 1), (0.02, 0.01, 5.0))]
    vs = [0.37, -1.0, 0.0, 2.5 + 1 / 64, -0.0, H + 3.0]
    for i, (fr, tr, abc) in enumerate(base):
        calls.append((i % 2, fr, tr, abc + (vs[i],)))
    calls += [(0, (10, 8, 80, 70), (30, 28, 40, 30), (float("nan"), 0.0, 1.0, 0.5)), (1, (10, 8, 80, 70), (30, 28, 40, 30), (0.0, 0.0, float("inf"), -0.5)),
              (0, (10, 8, 80, 70), (30, 28, 40, 30), (0.0, 0.0, 4.0, float("nan"))), (1, (0, 0, W, H), (0, 0, W, H), (0.0, 0.0, 6.0, 1.0))]
    return calls


def case_single_calls(pr, scratch=True):
    s = pr.e.scratch() if scratch else None
    try:
        worst = 0.0
        for check in (True, False):
            worst = max(worst, ic.run_calls(pr, mixed_calls(pr.H, pr.W), check, scratch=s))
        return worst
    finally:
        if s is not None:
            pr.e.scratch_free(s)


def mixed_planes(n, D, H, W, seed, slant=0.2):
    p = pc.random_planes(n, D, H, W, seed, slant=slant)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-2.5, 2.5, n).astype(F32)
    v[::3] = 0.0
    v[1::5] = -0.0
    p[:, 3] = v
    return p


def case_cell_batches(pr, units=(9, 25), mode=0, seed=3, windR=20, kind=None):
    worst = 0.0
    for unit in units:
        layer = om.Layer(pr.W, pr.H, windR, unit)
        for si in (0, len(layer.sets) // 2):
            cells = layer.sets[si]
            planes = mixed_planes(len(cells), pr.D, pr.H, pr.W, seed + unit + si)
            for check in (True, False):
                _, w = ic.check_batch(pr, layer.filter[cells], layer.shared[cells], planes, mode, check, kind=kind)
                worst = max(worst, w)
    return worst


def case_slot_and_slab_batches(pr, mode=1, seed=7, kind=None):
    """Slot batches (several calls per cell, one slab per call group) and whole-image slabs."""
    layer = om.Layer(pr.W, pr.H, 20, 14)
    cells = layer.sets[0]
    slots = 3
    frs = np.tile(layer.filter[cells], slots)
    trs = np.tile(layer.shared[cells], slots)
    planes = mixed_planes(len(frs), pr.D, pr.H, pr.W, seed)
    _, w1 = ic.check_batch(pr, frs, trs, planes, mode, True, out_slabs=len(cells), kind=kind)
    fr = np.array([(0, 0, pr.W, pr.H)] * 4, np.int32).view(api.RECT_DT).reshape(-1)
    planes = mixed_planes(4, pr.D, pr.H, pr.W, seed + 1)
    _, w2 = ic.check_batch(pr, fr, fr, planes, 1 - mode, False, out_slabs=1, kind=kind)
    return max(w1, w2)


def case_negative_zero(pr, mode=0, seed=13):
    """v = -0.0 returns the bits of v = 0 on single calls and batches, with the same kernel kind."""
    H, W = pr.H, pr.W
    for fr, tr, abc in (((19, 22, 82, 74), (39, 42, 42, 34), (0.05, -0.03, 14.25)), ((0, 0, W, H), (0, 0, W, H), (0.01, 0.02, 10.125))):
        outs = [pr.e.ComputeUnaryPotential(fr, tr, np.zeros((H, W), F32), abc + (v,), mode=mode, check=True) for v in (0.0, -0.0)]
        assert np.array_equal(bits(outs[0]), bits(outs[1]))
    layer = om.Layer(W, H, 20, 9)
    cells = layer.sets[0]
    planes = pc.random_planes(len(cells), pr.D, H, W, seed, slant=0.2)
    planes[:, 3] = 0.0
    b = api.Batch(pr.e, layer.filter[cells], layer.shared[cells])
    k = b.kernel_kind(mode)
    b.destroy()
    got0 = ic.run_batch(pr, layer.filter[cells], layer.shared[cells], planes, mode, True, kind=k)
    planes[:, 3] = -0.0
    got1 = ic.run_batch(pr, layer.filter[cells], layer.shared[cells], planes, mode, True, kind=k)
    assert np.array_equal(bits(got0), bits(got1))


# ------------------------------------------------------------------------------------------------ proposers
class Mwc:
    """cv::RNG's multiply-with-carry ([recollection] of OpenCV 3.1), as csrc/les_propose.h."""

    def __init__(self, state):
        self.state = int(state)

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform_int(self, a, b):
        return a if a == b else self.next() % (b - a) + a

    def uniform_float(self, a, b):
        f = F32(self.next()) * F32(2.3283064365386962890625e-10)
        return F32(f * (F32(b) - F32(a)) + F32(a))


def expected_v(kind, labels, W, u, seed, m, mind, maxd, maxv):
    """The v a proposal draws and the generator state after the proposal (INIT: createRandomLabel; RANDOM: RandomProposer)."""
    r = Mwc(seed)
    k = r.uniform_int(0, int(u["h"]) * int(u["w"]))
    px, py = k % int(u["w"]), k // int(u["w"])
    maxv = F32(maxv)
    if kind == api.PROPOSE_INIT:
        r.uniform_float(mind, maxd)
        v = r.uniform_float(-maxv, maxv) if maxv != 0 else F32(0)
    else:
        lab = labels[int(u["y"]) + py, int(u["x"]) + px]
        r.next()                                                   # zs
        v = F32(lab["v"])
        if maxv != 0:
            dv = F32(float(maxv) * 2.0 ** -(m + 1))
            v = r.uniform_float(max(-maxv, F32(v - dv)), min(maxv, F32(v + dv)))
    for _ in range(4):                                             # the two doubles of the random unit vector
        r.next()
    return v, r.state


def case_proposers(lib, unit=14, seed=11):
    """Device INIT and RANDOM with a vertical range: v and the generator states as restated; v inside its range; with range 0 the planes
    and states of a context that never set one."""
    pr = VPair(lib)
    e2 = api.HipCostVolumeEnergy.naive(pr.imL, pr.imR, windR=20, max_disp=31.0, lib=lib)
    H, W, D = pr.H, pr.W, pr.D
    layer = om.Layer(W, H, 20, unit)
    cells = layer.sets[len(layer.sets) // 2]
    units = layer.unit[cells]
    n = len(cells)
    labels = pc._label_map(H, W, D, seed, noise=0.3)
    labels["v"] = np.random.default_rng(seed).uniform(-0.7, 0.7, (H, W)).astype(F32)      # inside every range below (a source outside
    # its range can propose outside it, as the reference does)
    bufs = []
    try:
        for e in (pr.e, e2):
            b = api.Batch(e, layer.filter[cells], layer.shared[cells])
            b.set_units(units)
            bufs.append((e, b, api.DeviceBuffer(e, labels.nbytes), api.DeviceBuffer(e, 8 * n), api.DeviceBuffer(e, 16 * n)))

        def run(i, kind, m, seeds):
            e, b, d_lab, d_rng, d_pl = bufs[i]
            d_lab.upload(labels)
            d_rng.upload(seeds)
            b.propose(kind, d_lab.ptr, d_rng.ptr, d_pl.ptr, m=m)
            e.synchronize()
            return d_pl.download((n,), api.PLANE_DT), d_rng.download((n,), np.uint64)

        for kind, m, maxv in ((api.PROPOSE_INIT, 0, 2.0), (api.PROPOSE_RANDOM, 0, 2.0), (api.PROPOSE_RANDOM, 3, 2.0), (api.PROPOSE_RANDOM, 1, 0.75)):
            seeds = pc._seeds(n, seed + 7 * kind + m)
            # range 0: the streams of a context that never set one
            pr.e.set_max_vdisparity(0.0)
            pr.e.set_random_vdisparity(0.0)
            g0, s0 = run(0, kind, m, seeds)
            h0, t0 = run(1, kind, m, seeds)
            assert g0.tobytes() == h0.tobytes() and np.array_equal(s0, t0)
            if kind == api.PROPOSE_INIT:
                pr.e.set_max_vdisparity(maxv)
            else:
                pr.e.set_random_vdisparity(maxv)
            got, st = run(0, kind, m, seeds)
            for i, u in enumerate(units):
                v, state = expected_v(kind, labels, W, u, int(seeds[i]), m, 0.0, float(D - 1), maxv)
                assert st[i] == state, (kind, m, i)
                assert bits(np.array([got["v"][i]]))[0] == bits(np.array([v]))[0], (kind, m, i, got["v"][i], v)
                assert -maxv <= got["v"][i] <= maxv
        pr.e.set_max_vdisparity(0.0)
        pr.e.set_random_vdisparity(0.0)
        # expansion keeps v; the setters refuse bad ranges
        g, _ = run(0, api.PROPOSE_EXPANSION, 0, pc._seeds(n, seed))
        assert np.all(np.isin(g["v"], labels["v"]))
        for bad in (-1.0, float("nan"), float("inf")):
            for f in (pr.e.set_max_vdisparity, pr.e.set_random_vdisparity):
                try:
                    f(bad)
                except api.LesHipError:
                    continue
                raise AssertionError(f"range {bad} accepted")
    finally:
        for e, b, *ds in bufs:
            for d in ds:
                d.free()
            b.destroy()
        e2.close()
        pr.close()
