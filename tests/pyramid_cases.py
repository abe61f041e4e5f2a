"""The half-resolution solve's way down and way up (csrc/les_pyramid.h): the definitions restated in numpy, and the cases tests/test_pyramid.py runs
on the CPU simulator build (lib = its path, tensors on "cpu") and on the MI355X (lib = None: the product library, tensors on "cuda").

All three operations are exact (integers, or f32 in a fixed order with power-of-two multipliers), so device results are compared BYTE for byte with
the restatement.  The one exception is the payload of a NaN the volume pool produces: which NaN an f32 add or multiply returns is the processor's
choice (x86 and gfx950 differ in the sign of the NaN made by inf - inf), so the NaN case compares where the NaNs lie, and every other entry's bytes."""
import ctypes as C

import numpy as np

from localexpstereo_amd import api

F = np.float32
SEGMENT = 256                   # INPUT pixels of a row segment of les_pool_volume_kernel: 2 kPyrTX (a wave's 64 lanes x 4 consecutive input pixels)
CHUNK = 32                      # INPUT slices a workgroup owes: 2 kPyrKC
GUARD = 64                      # guard words (bytes for u8 buffers) on either side of a device buffer
GUARD_BITS = 0x7FC0BEEF          # (as int32) a quiet NaN with a payload: no result equals it
GUARD_BYTE = 0xA5


def hs(n):
    return (int(n) + 1) // 2


# ------------------------------------------------------------------------------------------------ the restatement
def _pairs(n):
    """Source indices (2i, min(2i + 1, n - 1)) of the hs(n) pooled ones."""
    i = 2 * np.arange(hs(n))
    return i, np.minimum(i + 1, n - 1)


def pool_image(im):
    im = np.asarray(im, np.uint8)
    H, W = im.shape[:2]
    (y0, y1), (x0, x1) = _pairs(H), _pairs(W)
    p = im.astype(np.int64)
    s = p[np.ix_(y0, x0)] + p[np.ix_(y0, x1)] + p[np.ix_(y1, x0)] + p[np.ix_(y1, x1)]
    return ((s + 2) >> 2).astype(np.uint8)


def pool_image_loop(im):
    H, W = im.shape[:2]
    out = np.zeros((hs(H), hs(W), 3), np.uint8)
    for y in range(hs(H)):
        for x in range(hs(W)):
            for c in range(3):
                s = sum(int(im[min(2 * y + dy, H - 1), min(2 * x + dx, W - 1), c]) for dy in (0, 1) for dx in (0, 1))
                out[y, x, c] = (s + 2) >> 2
    return out


def pool_volume(v):
    v = np.ascontiguousarray(v, F)
    D, H, W = v.shape
    k = np.arange(hs(D))
    sm, sc, sp = np.maximum(2 * k - 1, 0), 2 * k, np.minimum(2 * k + 1, D - 1)
    (y0, y1), (x0, x1) = _pairs(H), _pairs(W)
    q, h = F(0.25), F(0.5)

    def t(ys, xs):
        ix = lambda s: v[np.ix_(s, ys, xs)]
        return (q * ix(sm) + h * ix(sc)) + q * ix(sp)

    with np.errstate(invalid="ignore", over="ignore"):
        r = (((t(y0, x0) + t(y0, x1)) + t(y1, x0)) + t(y1, x1)) * q
    assert r.dtype == F
    return r


def pool_volume_loop(v):
    D, H, W = v.shape
    out = np.zeros((hs(D), hs(H), hs(W)), F)
    q, h = F(0.25), F(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(hs(D)):
            for y in range(hs(H)):
                for x in range(hs(W)):
                    t = []
                    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        yy, xx = min(2 * y + dy, H - 1), min(2 * x + dx, W - 1)
                        t.append(F(F(q * v[max(2 * k - 1, 0), yy, xx]) + F(h * v[2 * k, yy, xx])) + F(q * v[min(2 * k + 1, D - 1), yy, xx]))
                    out[k, y, x] = F(F(F(t[0] + t[1]) + t[2]) + t[3]) * q
    return out


def _valid(a, b, c, v, X, Y, mind, maxd):
    """label_valid of csrc/les_kernels.h (LES/StereoEnergy.h:560-610) on arrays, in its f32 order.  -> (valid, ds)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ds = ((X.astype(F) * a + Y.astype(F) * b) + F(1) * c) + F(0) * v
        a5, b5 = a * F(5), b * F(5)
        ok = (ds >= mind) & (ds <= maxd)
        for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            d = (ds + a5 if sa > 0 else ds - a5)
            d = d + b5 if sb > 0 else d - b5
            ok &= (d >= mind) & (d <= maxd)
    return ok, ds


def upsample(src, im_full, im_half, mind, maxd):
    """-> (H x W x 4 planes, H x W kinds)"""
    src = np.ascontiguousarray(src, F)
    H, W = im_full.shape[:2]
    Hh, Wh = im_half.shape[:2]
    assert (Hh, Wh) == (hs(H), hs(W)) and src.shape == (Hh, Wh, 4)
    Y, X = np.mgrid[0:H, 0:W]
    xh, yh = X >> 1, Y >> 1
    xn = np.clip(xh + np.where(X & 1, 1, -1), 0, Wh - 1)
    yn = np.clip(yh + np.where(Y & 1, 1, -1), 0, Hh - 1)
    cands = [(xh, yh), (xn, yh), (xh, yn), (xn, yn)]
    full = im_full.astype(np.int64)
    sad = np.stack([np.abs(full - im_half[cy, cx].astype(np.int64)).sum(-1) for cx, cy in cands])
    win = sad.argmin(0)                                            # (the first of equal minima)
    cx = np.choose(win, [c[0] for c in cands])
    cy = np.choose(win, [c[1] for c in cands])
    l = src[cy, cx]
    a, b, c, v = (l[..., i] for i in range(4))
    mind, maxd = F(mind), F(maxd)
    with np.errstate(invalid="ignore", over="ignore"):
        c2 = (F(2) * c - F(0.5) * a) - F(0.5) * b
        v2 = F(2) * v
    ok, ds = _valid(a, b, c2, v2, X, Y, mind, maxd)
    fin = np.isfinite(ds)
    out = np.stack([a, b, c2, v2], -1).astype(F)
    kind = np.where(ok, 0, np.where(fin, 1, 2)).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        clamped = np.where(ds < mind, mind, np.where(ds > maxd, maxd, ds)).astype(F)
    out[kind == 1] = 0
    out[kind == 1, 2] = clamped[kind == 1]
    out[kind == 2] = 0
    out[kind == 2, 2] = mind
    return out, kind


def upsample_loop(src, im_full, im_half, mind, maxd):
    H, W = im_full.shape[:2]
    Hh, Wh = im_half.shape[:2]
    out, kind = np.zeros((H, W, 4), F), np.zeros((H, W), np.uint8)
    mind, maxd = F(mind), F(maxd)
    with np.errstate(invalid="ignore", over="ignore"):
        for Y in range(H):
            for X in range(W):
                xh, yh = X >> 1, Y >> 1
                xn = min(max(xh + (1 if X & 1 else -1), 0), Wh - 1)
                yn = min(max(yh + (1 if Y & 1 else -1), 0), Hh - 1)
                best, win = None, None
                for cx, cy in ((xh, yh), (xn, yh), (xh, yn), (xn, yn)):
                    s = sum(abs(int(im_full[Y, X, c]) - int(im_half[cy, cx, c])) for c in range(3))
                    if best is None or s < best:
                        best, win = s, (cy, cx)
                a, b, c, v = (F(t) for t in src[win])
                c2 = F(F(F(2) * c - F(0.5) * a) - F(0.5) * b)
                v2 = F(F(2) * v)
                ds = F(F(F(F(X) * a + F(Y) * b) + F(1) * c2) + F(0) * v2)
                a5, b5 = F(a * F(5)), F(b * F(5))
                five = [ds, F(F(ds + a5) + b5), F(F(ds + a5) - b5), F(F(ds - a5) + b5), F(F(ds - a5) - b5)]
                if all(d >= mind and d <= maxd for d in five):
                    out[Y, X], kind[Y, X] = (a, b, c2, v2), 0
                elif np.isfinite(ds):
                    out[Y, X], kind[Y, X] = (0, 0, min(max(ds, mind), maxd), 0), 1
                else:
                    out[Y, X], kind[Y, X] = (0, 0, mind, 0), 2
    return out, kind


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
def case_restatement():
    rng = np.random.default_rng(1)
    n = 0
    for H, W in ((1, 1), (2, 2), (5, 7), (4, 6)):
        im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert same_bytes(pool_image(im), pool_image_loop(im))
        n += 1
    assert (pool_image(np.full((3, 5, 3), 255, np.uint8)) == 255).all()
    for D, H, W in ((1, 1, 1), (2, 2, 2), (5, 5, 7), (4, 3, 6)):
        v = rng.random((D, H, W), dtype=F)
        v[rng.random(v.shape) < 0.05] = np.nan
        v[rng.random(v.shape) < 0.03] = np.inf
        a, b = pool_volume(v), pool_volume_loop(v)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same_bytes(np.where(np.isnan(a), F(0), a), np.where(np.isnan(b), F(0), b))
        n += 1
    for (Hh, Wh), (H, W) in (((1, 1), (1, 1)), ((3, 4), (5, 7)), ((4, 4), (8, 8))):
        for mind in (0.0, -2.0):
            im_full, src = upsample_inputs(H, W, mind, mind + 15.0, 50 + H, "random")
            a, ka = upsample(src, im_full, pool_image(im_full), mind, mind + 15.0)
            b, kb = upsample_loop(src, im_full, pool_image(im_full), mind, mind + 15.0)
            assert same_bytes(a, b) and same_bytes(ka, kb)
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ device plumbing
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def _up(a, lib):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(_dev(lib))


class Guarded:
    """A device buffer of n elements (int32 words or bytes) between guard elements, `lead` before and GUARD after; check() asserts the guards."""

    def __init__(self, lib, n, words=True, lead=GUARD, fill=None):
        import torch
        self.n, self.lead, self.words = n, lead, words
        self.g = GUARD_BITS if words else GUARD_BYTE
        self.buf = torch.full((lead + n + GUARD,), self.g, dtype=torch.int32 if words else torch.uint8, device=_dev(lib))
        if fill is not None:
            src = np.ascontiguousarray(fill)
            self.buf[lead:lead + n] = _up(src.view(np.int32 if words else np.uint8).reshape(-1), lib)
        self.ptr = self.buf.data_ptr() + (4 if words else 1) * lead

    def check(self):
        o = self.buf.cpu().numpy()
        assert (o[:self.lead] == self.g).all() and (o[self.lead + self.n:] == self.g).all(), "guard elements overwritten"
        return o[self.lead:self.lead + self.n].copy()


def dev_pool_image(lib, im):
    H, W = im.shape[:2]
    src = Guarded(lib, im.size, words=False, fill=im)
    dst = Guarded(lib, hs(H) * hs(W) * 3, words=False)
    api.pool_image(src.ptr, dst.ptr, H, W, lib=lib)
    out = dst.check().reshape(hs(H), hs(W), 3)
    assert same_bytes(src.check().reshape(im.shape), im)
    return out


def dev_pool_volume(lib, v, lead=GUARD, out_lead=GUARD):
    D, H, W = v.shape
    src = Guarded(lib, v.size, lead=lead, fill=v)
    dst = Guarded(lib, hs(D) * hs(H) * hs(W), lead=out_lead)
    api.pool_volume(src.ptr, dst.ptr, D, H, W, lib=lib)
    out = dst.check().view(F).reshape(hs(D), hs(H), hs(W))
    assert same_bytes(src.check().view(F).reshape(v.shape), v)
    return out


# ------------------------------------------------------------------------------------------------ 2. image pool
IMAGE_SHAPES = [(1, 1), (2, 2), (5, 7), (8, 130)]


def case_pool_image(lib, H, W):
    rng = np.random.default_rng(200 + 3 * H + W)
    im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = dev_pool_image(lib, im)
    assert same_bytes(got, pool_image(im))
    white = np.full((H, W, 3), 255, np.uint8)
    assert (dev_pool_image(lib, white) == 255).all()                # the rounding: (4 * 255 + 2) >> 2
    odd = np.full((H, W, 3), 1, np.uint8)
    odd[0, 0] = 2                                                   # (1 + 1 + 1 + 2 + 2) >> 2 = 1; a pixel of three 0s and a 2: (2 + 2) >> 2 = 1
    assert same_bytes(dev_pool_image(lib, odd), pool_image(odd))
    return int(got.sum())


# ------------------------------------------------------------------------------------------------ 3. volume pool
# (D, H, W): 1 x 1 x 1; even; odd everywhere; two row segments with a tail on the dword path (W % 4 != 0); three segments, the last of one output
# pixel; the carried slice across a chunk boundary and a segment boundary; three chunks on the vector path (W % 4 == 0).  Then, beyond the issue's
# list, the vector path across a segment boundary and across a chunk boundary with an odd height.
VOLUME_SHAPES = [(1, 1, 1), (2, 2, 2), (5, 5, 7), (9, 6, 258), (3, 3, 2 * SEGMENT + 2), (CHUNK + 1, 2, SEGMENT + 3), (2 * CHUNK + 1, 3, 40),
                 (5, 4, 2 * SEGMENT + 8), (CHUNK + 3, 5, SEGMENT + 8)]
UNALIGNED = (2 * CHUNK + 1, 3, 40)


def case_pool_volume(lib, D, H, W, lead=GUARD, out_lead=GUARD):
    rng = np.random.default_rng(300 + D + 3 * H + 7 * W)
    v = rng.random((D, H, W), dtype=F)
    got = dev_pool_volume(lib, v, lead=lead, out_lead=out_lead)
    ref = pool_volume(v)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    return float(got.mean())


def case_pool_volume_nonfinite(lib, D=7, H=5, W=9):
    """NaN, +inf and -inf at a clamped edge (the last slice, row and column: all three odd sizes clamp there) and in the interior."""
    rng = np.random.default_rng(9)
    v = rng.random((D, H, W), dtype=F)
    v[D - 1, H - 1, W - 1] = np.nan
    v[0, 0, W - 1] = np.inf
    v[D - 1, 0, 0] = -np.inf
    v[3, 2, 4] = np.nan
    v[2, 1, 1] = np.inf
    v[4, 3, 6] = -np.inf
    v[1, 3, 2], v[1, 3, 3] = np.inf, -np.inf                        # meet in one output: inf - inf
    got, ref = dev_pool_volume(lib, v), pool_volume(v)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref).sum() >= 3 and np.isposinf(ref).sum() >= 2 and np.isneginf(ref).sum() >= 2
    m = ~np.isnan(ref)
    assert same_bytes(got[m], ref[m])
    return int(np.isnan(ref).sum()), int(np.isinf(ref).sum())


def case_pool_errors(lib):
    import torch
    L = api.load(lib)
    vp = C.c_void_p
    a = torch.zeros(64, dtype=torch.float32, device=_dev(lib))
    b = torch.full((64,), 7.0, dtype=torch.float32, device=_dev(lib))
    pa, pb = a.data_ptr(), b.data_ptr()
    refused = [L.les_hip_pool_volume(None, vp(pb), 2, 2, 2, 0, None), L.les_hip_pool_volume(vp(pa), None, 2, 2, 2, 0, None),
               L.les_hip_pool_volume(vp(pa), vp(pb), 0, 2, 2, 0, None), L.les_hip_pool_volume(vp(pa), vp(pb), 2, -1, 2, 0, None),
               L.les_hip_pool_volume(vp(pa), vp(pb), 2, 2, 0, 0, None), L.les_hip_pool_image(None, vp(pb), 2, 2, 0, None),
               L.les_hip_pool_image(vp(pa), None, 2, 2, 0, None), L.les_hip_pool_image(vp(pa), vp(pb), 0, 2, 0, None), L.les_hip_pool_image(vp(pa), vp(pb), 2, 0, 0, None)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    assert L.les_hip_pool_volume(vp(pa), vp(pb), 65536, 256, 256, 0, None) == api.LES_HIP_ERR_UNSUPPORTED
    assert (b.cpu().numpy() == 7.0).all()
    try:
        api.pool_volume(pa, pb, 0, 2, 2, lib=lib)
        raise AssertionError("accepted")
    except api.LesHipError as ex:
        assert "error 1" in str(ex)
    return len(refused)


# ------------------------------------------------------------------------------------------------ 4. upsample
UPSAMPLE_SHAPES = [((1, 1), (1, 1)), ((3, 4), (5, 7)), ((4, 4), (8, 8)), ((17, 33), (33, 66))]       # (Hh, Wh) -> (H, W)
MIN_DISPS = (0.0, -2.0)
NDISP = 16


def upsample_inputs(H, W, mind, maxd, seed, guide):
    """-> (the full image, the half map of planes).  guide: "random"; "const" (ties everywhere: the first candidate wins); "edge" (two colours
    meeting at an ODD column: the half pixel that straddles the edge is a mixture, so both of its full columns must take a neighbour).  The
    planes: valid ones, and planted at random places planes that leave the range only at the full-resolution corners (steep), that leave it at
    the centre (kind 1), 1e30 (kind 1) and NaN / inf (kind 2)."""
    rng = np.random.default_rng(seed)
    Hh, Wh = hs(H), hs(W)
    if guide == "const":
        im = np.full((H, W, 3), 77, np.uint8)
    elif guide == "edge":
        e = min(2 * (W // 4) + 1, W - 1) | 1 if W > 1 else 0
        im = np.zeros((H, W, 3), np.uint8)
        im[:, :e], im[:, e:] = (10, 200, 30), (240, 20, 90)
    else:
        im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    src = np.zeros((Hh, Wh, 4), F)
    src[..., 0] = rng.uniform(-0.02, 0.02, (Hh, Wh))
    src[..., 1] = rng.uniform(-0.02, 0.02, (Hh, Wh))
    src[..., 2] = rng.uniform(0.5 * mind + 1.5, 0.5 * maxd - 1.5, (Hh, Wh))       # half disparities well inside the halved range
    src[..., 3] = rng.uniform(-0.5, 0.5, (Hh, Wh))
    pick = rng.random((Hh, Wh))
    steep = pick < 0.12                                             # centre inside the range, a corner ds +- 5a +- 5b outside
    yy, xx = np.mgrid[0:Hh, 0:Wh]
    src[steep, 0] = 2.0
    src[steep, 2] = (0.25 * (mind + maxd) - 2.0 * xx[steep]).astype(F)
    out_c = (pick >= 0.12) & (pick < 0.24)
    src[out_c, 0:2] = 0
    src[out_c, 2] = np.where(rng.random(out_c.sum()) < 0.5, 0.5 * maxd + 3.0, 0.5 * mind - 3.0)
    huge = (pick >= 0.24) & (pick < 0.30)
    src[huge, 2] = 1e30
    nonfin = (pick >= 0.30) & (pick < 0.40)
    src[nonfin, 2] = np.where(rng.random(nonfin.sum()) < 0.5, np.nan, np.inf)
    nanv = (pick >= 0.40) & (pick < 0.44)
    src[nanv, 3] = np.nan                                           # 0 * NaN: ds is NaN
    return im, src


def _volume_context(lib, im, mind, D=NDISP, seed=5, **kw):
    """A cheap full context over `im` (both views) for the upsample cases: unfiltered aggregation, a random volume."""
    H, W = im.shape[:2]
    vol = np.random.default_rng(seed).random((D, H, W), dtype=F)
    return api.HipCostVolumeEnergy(im, im, vol, vol, windR=2, eps=1e-4, th_col=0.5, max_disp=mind + D - 1, min_disp=mind, lib=lib, filter="", **kw)


def case_upsample(lib, half_shape, full_shape, mind, guide, mode=0):
    import torch
    H, W = full_shape
    maxd = mind + NDISP - 1
    im, src = upsample_inputs(H, W, mind, maxd, 400 + 5 * H + W + int(mind) + len(guide), guide)
    full = _volume_context(lib, im, mind)
    half = full.half()
    try:
        assert (half.H, half.W, half.D) == tuple(half_shape) + (hs(NDISP),) and half.params.min_disparity == 0.5 * mind
        im_half = pool_image(im)
        assert same_bytes(half.image(mode), im_half) and same_bytes(half.imL, im_half) and same_bytes(full.image(mode), im)
        s = Guarded(lib, src.size, fill=src)
        o = Guarded(lib, H * W * 4)
        k = Guarded(lib, H * W, words=False)
        L = full.L
        full._chk(L.les_hip_upsample_labels(full.h, half.h, mode, C.c_void_p(s.ptr), C.c_void_p(o.ptr), C.c_void_p(k.ptr)))
        full.synchronize()
        got, kind = o.check().view(F).reshape(H, W, 4), k.check().reshape(H, W)
        assert same_bytes(s.check().view(F).reshape(src.shape), src)
        ref, rkind = upsample(src, im, im_half, mind, maxd)
        assert same_bytes(kind, rkind), np.argwhere(kind != rkind)[:5].tolist()
        bad = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
        assert len(bad) == 0, (len(bad), bad[:5].tolist())
        counts = np.bincount(kind.ravel(), minlength=3)
        # every output is a valid label of the full context
        ok, _ = _valid(got[..., 0], got[..., 1], got[..., 2], got[..., 3], *np.mgrid[0:H, 0:W][::-1], F(mind), F(maxd))
        assert ok.all()
        # the Python layer: the same bytes from a host array, with and without the kind map; without it nothing else changes
        t, tk = full.upsample_labels(half, src, mode=mode, with_kind=True, device=_dev(lib))
        t2 = full.upsample_labels(half, torch.from_numpy(src.copy()).to(_dev(lib)), mode=mode, device=_dev(lib))
        full.synchronize()
        assert same_bytes(t.cpu().numpy(), ref) and same_bytes(tk.cpu().numpy(), rkind) and same_bytes(t2.cpu().numpy(), ref)
        Y, X = np.mgrid[0:H, 0:W]
        keep = rkind == 0
        if guide == "const":                                        # ties: the first candidate everywhere (the kept planes' slopes are all distinct)
            assert same_bytes(ref[keep][:, :2], src[Y >> 1, X >> 1][keep][:, :2])
        if guide == "edge" and W > 2:                               # both columns of the half pixel that straddles the edge took their outer neighbour's plane
            e = next(x for x in range(1, W) if im[0, x, 0] != im[0, x - 1, 0])
            assert e % 2 == 1
            for col, nb in ((e - 1, e // 2 - 1), (e, e // 2 + 1)):
                if 0 <= nb < hs(W):
                    k = keep[:, col]
                    assert same_bytes(ref[:, col][k][:, :2], src[np.arange(H) >> 1, nb][k][:, :2])
        return counts.tolist()
    finally:
        half.close()
        full.close()


def case_upsample_errors(lib):
    import torch
    im = np.random.default_rng(3).integers(0, 256, (6, 8, 3), dtype=np.uint8)
    full = _volume_context(lib, im, 0.0)
    half = full.half()
    other = _volume_context(lib, im[:5], 0.0)
    try:
        L, vp = full.L, C.c_void_p
        s = torch.zeros((3, 4, 4), dtype=torch.float32, device=_dev(lib))
        o = torch.full((6, 8, 4), 3.0, dtype=torch.float32, device=_dev(lib))
        refused = [L.les_hip_upsample_labels(None, half.h, 0, vp(s.data_ptr()), vp(o.data_ptr()), None),
                   L.les_hip_upsample_labels(full.h, None, 0, vp(s.data_ptr()), vp(o.data_ptr()), None),
                   L.les_hip_upsample_labels(full.h, half.h, 0, None, vp(o.data_ptr()), None),
                   L.les_hip_upsample_labels(full.h, half.h, 0, vp(s.data_ptr()), None, None),
                   L.les_hip_upsample_labels(full.h, half.h, 2, vp(s.data_ptr()), vp(o.data_ptr()), None),
                   L.les_hip_upsample_labels(full.h, other.h, 0, vp(s.data_ptr()), vp(o.data_ptr()), None),
                   L.les_hip_upsample_labels(full.h, half.h, 0, vp(o.data_ptr()), vp(o.data_ptr()), None)]
        assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
        full.synchronize()
        assert (o.cpu().numpy() == 3.0).all()
        try:
            full.upsample_labels(half, np.zeros((6, 8, 4), F), device=_dev(lib))
            raise AssertionError("a full-size map was accepted")
        except ValueError:
            pass
        return len(refused)
    finally:
        other.close()
        half.close()
        full.close()


# ------------------------------------------------------------------------------------------------ 5. the half context
HALF_SHAPE = (10, 22, 31)       # (D, H, W)
HALF_WINDR = 8                  # guided-filter radius 4 -> 2 in the half context
FILTERS = ("GF", "BF", "")
NPLANES = 8


def _half_inputs(seed=11):
    D, H, W = HALF_SHAPE
    rng = np.random.default_rng(seed)
    imL = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    imR = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    # smooth-ish images as well, so that the guided filter is not all noise
    imL[:, : W // 2] = (imL[:, : W // 2] // 4 + 60).astype(np.uint8)
    volL, volR = rng.random((D, H, W), dtype=F) * F(0.6), rng.random((D, H, W), dtype=F) * F(0.6)
    return imL, imR, volL, volR


def _eps(filt):
    return 10.0 if filt == "BF" else 1e-4


def _evaluate(e, lib, mind):
    """The unary costs of NPLANES planted planes over the cells of a layer, both views, and the WTA labels: bytes that depend on every table the
    context holds (volume, tiled copy, guide statistics, weight table, interpolation, disparity range)."""
    from localexpstereo_amd import pm
    units, shared, filt, sets = pm.layer_geometry(e.W, e.H, e.params.windR, 5)
    rng = np.random.default_rng(17)
    maxd = e.max_disp
    outs = []
    for mode in (0, 1):
        for i in range(NPLANES):
            cells = sets[i % len(sets)]
            n = len(cells)
            pl = np.zeros((n, 4), F)
            pl[:, 0] = rng.uniform(-0.15, 0.15, n)
            pl[:, 1] = rng.uniform(-0.15, 0.15, n)
            pl[:, 2] = rng.uniform(e.params.min_disparity + 1, maxd - 1, n) - pl[:, 0] * (shared[cells]["x"] + 2) - pl[:, 1] * (shared[cells]["y"] + 2)
            pl[:, 3] = rng.uniform(-0.5, 0.5, n)
            outs.append(e.unary_batch(filt[cells], shared[cells], pl, mode=mode, check=bool(i & 1)))
        lab, cost = e.wta_labels(mode, device=_dev(lib))
        e.synchronize()
        outs += [lab.cpu().numpy(), cost.cpu().numpy()]
    return outs


def case_create_half(lib, naive, filt, interp, mind):
    D, H, W = HALF_SHAPE
    imL, imR, volL, volR = _half_inputs()
    maxd = mind + D - 1
    if naive:
        full = api.HipCostVolumeEnergy.naive(imL, imR, windR=HALF_WINDR, eps=_eps(filt), max_disp=maxd, min_disp=mind, lib=lib, filter=filt, max_vdisp=1.0)
        full.set_random_vdisparity(0.5)
    else:
        full = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=HALF_WINDR, eps=_eps(filt), th_col=0.5, max_disp=maxd, min_disp=mind, lib=lib, filter=filt,
                                       interpolate=interp)
    half = ref = None
    try:
        half = full.half()
        full.close()                                                # the half context owns everything it needs
        hl, hr = pool_image(imL), pool_image(imR)
        assert (half.H, half.W) == (hs(H), hs(W)) and half.D == (1 if naive else hs(D)) and half.params.windR == HALF_WINDR // 2
        assert half.max_disp == 0.5 * maxd and half.params.min_disparity == 0.5 * mind and half.interpolate == interp and half.filter == full.filter
        assert same_bytes(half.imL, hl) and same_bytes(half.imR, hr)
        if naive:
            ref = api.HipCostVolumeEnergy.naive(hl, hr, windR=HALF_WINDR // 2, eps=_eps(filt), max_disp=0.5 * maxd, min_disp=0.5 * mind, lib=lib, filter=filt, max_vdisp=0.5)
            ref.set_random_vdisparity(0.25)
            assert half.max_vdisp == 0.5 and half.random_vdisp == 0.25
        else:
            ref = api.HipCostVolumeEnergy(hl, hr, pool_volume(volL), pool_volume(volR), windR=HALF_WINDR // 2, eps=_eps(filt), th_col=0.5, max_disp=0.5 * maxd,
                                          min_disp=0.5 * mind, lib=lib, filter=filt, interpolate=interp)
        assert half.num_fronto_planes == ref.num_fronto_planes
        a, b = _evaluate(half, lib, 0.5 * mind), _evaluate(ref, lib, 0.5 * mind)
        assert len(a) == len(b) == 2 * (NPLANES + 2)
        for i, (x, y) in enumerate(zip(a, b)):
            assert same_bytes(x, y), i
        finite = sum(int(np.isfinite(x).sum()) for x in a)
        assert finite > 0
        return finite
    finally:
        for e in (ref, half, full):
            if e is not None:
                e.close()


def case_create_half_errors(lib):
    D, H, W = HALF_SHAPE
    imL, imR, volL, volR = _half_inputs()
    L = api.load(lib)
    h = C.c_void_p()
    odd = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=HALF_WINDR, th_col=0.5, max_disp=D - 4, min_disp=-3.0, lib=lib)
    frac = api.HipCostVolumeEnergy(imL, imR, volL, volR, windR=HALF_WINDR, th_col=0.5, max_disp=D - 1, min_disp=-0.5, lib=lib)
    try:
        assert L.les_hip_create_half(C.byref(h), odd.h) == api.LES_HIP_ERR_UNSUPPORTED and not h.value
        assert b"even integer" in L.les_hip_last_error()
        assert L.les_hip_create_half(C.byref(h), frac.h) == api.LES_HIP_ERR_UNSUPPORTED and not h.value
        assert L.les_hip_create_half(None, odd.h) == api.LES_HIP_ERR_ARG
        assert L.les_hip_create_half(C.byref(h), None) == api.LES_HIP_ERR_ARG and not h.value
        assert b"null argument" in L.les_hip_last_error()
        try:
            odd.half()
            raise AssertionError("min_disp = -3 was accepted")
        except api.LesHipError as ex:
            assert "error 3" in str(ex)
        im = np.empty((H, W, 3), np.uint8)
        assert L.les_hip_get_image(None, 0, im.ctypes.data_as(C.c_void_p)) == api.LES_HIP_ERR_ARG
        assert L.les_hip_get_image(odd.h, 2, im.ctypes.data_as(C.c_void_p)) == api.LES_HIP_ERR_ARG
        assert L.les_hip_get_image(odd.h, 0, None) == api.LES_HIP_ERR_ARG
        one = api.HipCostVolumeEnergy(imL, None, volL, None, windR=HALF_WINDR, th_col=0.5, lib=lib)       # a single view: its half has that view alone
        try:
            assert L.les_hip_get_image(one.h, 1, im.ctypes.data_as(C.c_void_p)) == api.LES_HIP_ERR_ARG
            hh = one.half()
            try:
                assert same_bytes(hh.imL, pool_image(imL)) and hh.imR is None
            finally:
                hh.close()
        finally:
            one.close()
    finally:
        odd.close()
        frac.close()


# ------------------------------------------------------------------------------------------------ 6. the driver
SEED = 3                        # the drivers' seed: chosen on the simulator build, where the "half" start row lies far below the random one (see case_driver)


def _valid_labels(lab, mind, maxd):
    H, W = lab.shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    return _valid(lab[..., 0], lab[..., 1], lab[..., 2], lab[..., 3], X, Y, F(mind), F(maxd))[0]


def case_driver(lib, device, monkeypatch, which, layers=None, two_levels=False, **opts):
    """MidV3 / MidV2 (init="half") on the cones crop: 1 full-resolution graph-cut iteration over a nested run of 1 PatchMatch + 1 graph-cut
    iteration.  layers: None = the front end's own, else what replaces stereo._layers (the simulator run, as costvol_cases.case_driver and for
    its reason); opts: further arguments of the front end."""
    from localexpstereo_amd import stereo
    from tests import costvol_cases as cc
    from tests import crossview_cases as cv
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    coarse = dict(iterations=1, pmInit=1)
    if two_levels:
        coarse = dict(iterations=1, pmInit=0, labeling="half", coarse_params=dict(iterations=1, pmInit=1))
    kw = dict(device=device, lib=lib, seed=SEED, evaluate_on_device=True, **opts)
    if which == "MidV3":
        imL, imR, gt = cc.cones_pair()
        data = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
        run = lambda **k: stereo.MidV3(data, None, None, **dict(kw, **k))
    else:
        data = cv.cones_data()
        run = lambda **k: stereo.MidV2(data, **dict(kw, **k))
    H, W = data["imL"].shape[:2]
    st, lab, raw = run(iterations=1, pmIterations=0, init="half", coarse_params=coarse)
    assert lab.shape == (H, W, 4) and np.isfinite(lab).all() and same_bytes(lab, raw)
    assert _valid_labels(lab, 0.0, 63.0).all()
    energies = [r["energy"] for r in st.log]
    assert len(energies) == 2 and all(np.isfinite(energies))
    for a, b in zip(energies, energies[1:]):                        # never rises from the start row on (a set may move it by the rounding of its capacities)
        assert b <= a + 1e-6 * abs(a), energies
    cs = st.coarse_stats
    assert cs["shape"][:2] == (hs(H), hs(W)) and cs["iterations"] == 1 and cs["seconds"] > 0 and len(cs["log"]) >= 2 and st.coarse_seconds >= cs["seconds"]
    assert sum(cs["kind_pixels"][0]) == H * W and cs["kind_pixels"][0][2] == 0 and cs["lambda_"] == 2 * st.p["lambda_"] and cs["th_smooth"] == 0.5 * st.p["th_smooth"]
    assert all(u >= 3 for u in cs["units"]) and len(set(cs["units"])) == len(cs["units"])
    if two_levels:
        assert cs["labeling"] == "half" and cs["coarse_stats"]["shape"][:2] == (hs(hs(H)), hs(hs(W))) and cs["coarse_stats"]["labeling"] is None
        return energies
    assert cs["coarse_stats"] == {}
    # two runs give the same bytes
    st_b, lab_b, _ = run(iterations=1, pmIterations=0, init="half", coarse_params=coarse)
    assert same_bytes(lab, lab_b) and [r["energy"] for r in st_b.log] == energies
    # the start row lies below the start row of the default run with the same seed (the random start)
    st_r, _, _ = run(iterations=0, pmIterations=0)
    print(f"{which} on the cones crop, seed {SEED}: \"half\" start row energy {energies[0]:.1f} all {st.log[0]['all']:.2f} % -> {energies[-1]:.1f} / {st.log[-1]['all']:.2f} % after 1 "
          f"iteration; random start row {st_r.log[0]['energy']:.1f} / {st_r.log[0]['all']:.2f} %; kinds [kept, clamped, non-finite] {cs['kind_pixels'][0]}; "
          f"coarse {cs['seconds']:.2f} s of {st.coarse_seconds:.2f} s, whole run {st.seconds:.2f} s")
    assert energies[0] < st_r.log[0]["energy"], (energies[0], st_r.log[0]["energy"])
    # two views: both start from their own coarse map
    st_d, lab_d, raw_d = run(iterations=1, pmIterations=0, init="half", coarse_params=coarse, doDual=True)
    assert np.isfinite(lab_d).all() and sorted(st_d.raw_labelings) == [0, 1] and sorted(st_d.coarse_stats["kind_pixels"]) == [0, 1]
    assert _valid_labels(st_d.raw_labelings[1], 0.0, 63.0).all()
    return energies


def case_driver_refusals(lib, device):
    from localexpstereo_amd import stereo
    from tests import crossview_cases as cv
    st, e = cv.driver(lib, device, "none", world=2)
    try:
        try:
            st.run(1, (0,), 0, labeling="half")
            raise AssertionError("world = 2 was accepted")
        except NotImplementedError:
            pass
    finally:
        e.close()
    st, e = cv.driver(lib, device, "none")
    try:
        st.coarse_params = dict(iterations=1, pmInit=0, depth=2)
        try:
            st.run(0, (0,), 0, labeling="half")
            raise AssertionError("an unknown key of coarse_params was accepted")
        except TypeError:
            pass
        try:
            st.run(0, (0,), 0, labeling="half+planes")
            raise AssertionError("an unknown start was accepted")
        except ValueError:
            pass
    finally:
        e.close()
    assert stereo._parse_start("half") == ("half", False)
