"""Cases of tests/test_crossview.py: cross-view fusion (csrc/les_crossview.h: les_hip_warp_labels; stereo.FastGCStereo.cross_fuse and cross_view=)
on the CPU simulator build and on the MI355X.

The definition, restated from csrc/les_crossview.h.  src: the H x W planes (a, b, c, v) of view s, fallback: those of the target view 1 - s,
sign = +1 for s = 0 and -1 for s = 1.  For a source pixel (xs, y), every operation rounded to f32, in this order:
    d = (a xs + b y) + c        t = (xs - d sign) + 0.5
    the candidate exists iff -1e9 < t < 1e9 and rx = floor(t) lies in [0, W); it is dropped unless q = 1 - sign a >= 0.125 and b, c, v are finite
    its plane in the target view: (a / q, b / q, c / q, -v), on row y
Of the candidates that land on one (rx, y) the largest d wins (-0 = +0), among equal d the largest xs.  A target pixel with a winner gets its plane
and hit = 1, every other one fallback's plane bit for bit and hit = 0.

"-0 = +0" cannot be observed on a landing inside the image: two candidates of one target pixel with equal d have t = xs - sign d + 0.5 one pixel or
more apart unless xs is the same, so a tie in d between distinct sources needs |d| of 2^24 or more, which lands outside every image the kernel serves
(W <= 8192).  No population below pins that rule or the xs tie-break; they are part of the definition so that it is total.

The simulator legs of the driver cases (6) run MidV2 / MidV3 with stereo._layers replaced by sim_layers (two coarse layers) and a filter radius of 6,
the GPU legs run them unchanged: the drivers' own 15 proposals on 1 ... 25 pixel cells take tens of minutes on the fibre simulator.  The cross_view
path both legs go through is the same.

References, none of them the code under test: the vectorised numpy restatement below, itself held to a literal per-pixel loop.  Tolerances: out and
hit are compared bit for bit.  Landing bound: |d'(rx, y) - d| <= 0.5 |a'| + 1e-4, from rx <= t < rx + 1 with t = xs - sign d + 0.5 (the landing
column is at most half a pixel from the exact landing point, and the target plane's slope along x is a'); 1e-4 covers the f32 rounding of d, of
the three quotients and of t at disparities below 256.  Energies: a fusion may raise a view's energy only through the float rounding of the
capacities, fusion_cases.RISE |E|."""
import functools

import numpy as np

from localexpstereo_amd import api
from tests import eval_cases as ec
from tests import fusion_cases as fc

F = np.float32
SHAPES = ((1, 1), (3, 5), (2, 63), (2, 64), (3, 65), (2, 257), (4, 300), (2, 1025))       # (H, W): a row shorter than a wave, the wave and workgroup boundaries, the strided loop, several strides


def sign_of(src_mode):
    return F(1) if src_mode == 0 else F(-1)


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def warp_restate(src, fallback, src_mode):
    """-> (out H x W x 4, hit H x W u8, win H x W: the winning source column, -1 where none)"""
    H, W = src.shape[:2]
    s = sign_of(src_mode)
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    a, b, c, v = (src[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        d = ((a * xf + b * yf) + c).astype(F)
        t = ((xf - d * s) + F(0.5)).astype(F)
        ok = (t > F(-1.0e9)) & (t < F(1.0e9))
        rx = np.floor(np.where(ok, t, F(0))).astype(np.int64)
        ok &= (rx >= 0) & (rx < W)
        q = (F(1) - s * a).astype(F)
        ok &= (q >= F(0.125)) & np.isfinite(b) & np.isfinite(c) & np.isfinite(v)
        plane = np.stack([a / q, b / q, c / q, -v], -1).astype(F)
    out, hit, win = fallback.copy(), np.zeros((H, W), np.uint8), np.full((H, W), -1, np.int64)
    yy, xx = ys[ok], xs[ok]
    if len(yy):
        tgt = yy * W + rx[ok]
        dk = d[ok] + F(0)                                              # -0 -> +0
        order = np.lexsort((xx, dk, tgt))                              # by target pixel, then d, then xs: the winner is the last of its group
        last = np.ones(len(order), bool)
        last[:-1] = tgt[order][1:] != tgt[order][:-1]
        w = order[last]
        out[yy[w], rx[ok][w]] = plane[yy[w], xx[w]]
        hit[yy[w], rx[ok][w]] = 1
        win[yy[w], rx[ok][w]] = xx[w]
    return out, hit, win


def warp_loop(src, fallback, src_mode):
    """The same by a literal per-pixel transcription of the definition (scalar f32 operations)."""
    H, W = src.shape[:2]
    s = sign_of(src_mode)
    out, hit, win = fallback.copy(), np.zeros((H, W), np.uint8), np.full((H, W), -1, np.int64)
    with np.errstate(all="ignore"):
        for y in range(H):
            best = {}
            for xs in range(W):
                a, b, c, v = (F(k) for k in src[y, xs])
                d = F(F(F(a * F(xs)) + F(b * F(y))) + c)
                t = F(F(F(xs) - F(d * s)) + F(0.5))
                if not (t > F(-1.0e9) and t < F(1.0e9)):
                    continue
                rx = int(np.floor(t))
                if rx < 0 or rx >= W:
                    continue
                q = F(F(1) - F(s * a))
                if not (q >= F(0.125)) or not (np.isfinite(b) and np.isfinite(c) and np.isfinite(v)):
                    continue
                if rx not in best or d > best[rx][0] or (d == best[rx][0] and xs > best[rx][1]):
                    best[rx] = (d, xs, (F(a / q), F(b / q), F(c / q), F(-v)))
            for rx, (_, xs, plane) in best.items():
                out[y, rx], hit[y, rx], win[y, rx] = plane, 1, xs
    return out, hit, win


# ------------------------------------------------------------------------------------------------ label populations
def fallback_map(H, W, seed):
    lab = ec.cell_labels(H, W, seed, cell=4, maxd=30.0, slant=0.3)
    lab[..., 3] = np.random.default_rng(seed).uniform(-1, 1, (H, W)).astype(F)
    return np.ascontiguousarray(lab)


def pop_slanted(H, W, seed):
    """(a) random slanted planes, |a| <= 0.4, disparities below 256 / 8, and one nearer block: occlusion, holes, collisions."""
    lab = ec.cell_labels(H, W, seed, cell=5, maxd=min(30.0, 4.0 + W / 6.0), slant=0.4)
    lab[:, W // 3: W // 3 + max(1, W // 4), 2] += F(7.5)
    lab[..., 3] = np.random.default_rng(seed + 1).uniform(-1, 1, (H, W)).astype(F)
    return np.ascontiguousarray(lab)


def pop_collapse(H, W, seed, src_mode):
    """(b) a = +-0.8: on the rows where q = 0.2 about five sources land on one column (their c jittered per pixel); on the others q = 1.8 and the row spreads over 1.8 W columns."""
    rng = np.random.default_rng(seed)
    s = float(sign_of(src_mode))
    lab = np.zeros((H, W, 4), F)
    rows = np.arange(H) % 2 == 0
    lab[rows, :, 0], lab[~rows, :, 0] = F(0.8 * s), F(-0.8 * s)
    lab[rows, :, 2] = (-s * 0.3 * W + rng.uniform(-0.4, 0.4, (int(rows.sum()), W))).astype(F)          # t = 0.2 xs + 0.3 W + 0.5 -/+ jitter
    lab[~rows, :, 2] = rng.uniform(-0.4, 0.4, (int((~rows).sum()), W)).astype(F)
    lab[..., 3] = rng.uniform(-1, 1, (H, W)).astype(F)
    return lab


def specials(xs, W, s):
    """(c) the special planes of a source pixel at column xs (sign s) -> [(name, plane, kept: True / False / None = not stated)]."""
    s = float(s)
    ident = lambda **k: np.array([k.get("a", 0.0), k.get("b", 0.0), k.get("c", 0.0), k.get("v", 0.25)], F)
    a_edge = F(0.875)
    a_below = np.nextafter(a_edge, F(1))                               # q one step below 0.125
    assert F(1) - a_edge == F(0.125) and F(1) - a_below < F(0.125)
    on_self = lambda a: F(-(F(a) * F(xs)))                             # c with d = a xs + c = 0 exactly: the pixel lands on its own column
    out = [("q = 0.125", ident(a=s * a_edge, c=on_self(s * a_edge)), True), ("q just below 0.125", ident(a=s * a_below, c=on_self(s * a_below)), False),
           ("q = 0", ident(a=s * 1.0, c=on_self(s * 1.0)), False), ("q < 0", ident(a=s * 1.5, c=on_self(s * 1.5)), False),
           ("t = -0.5", ident(c=s * (xs + 1.0)), False), ("t = 0", ident(c=s * (xs + 0.5)), True), ("t = W - 1", ident(c=s * (xs + 0.5 - (W - 1))), True),
           ("t = W", ident(c=s * (xs + 0.5 - W)), False), ("t = -0.25", ident(c=s * (xs + 0.75)), False), ("d = 1e10", ident(c=1e10), False),
           ("v = 0.37", ident(v=0.37), True), ("v = -0.37", ident(v=-0.37), True), ("v = -0", ident(v=-0.0), True)]
    for k, comp in enumerate("abcv"):
        for name, val in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            p = ident()
            p[k] = val
            out.append((f"{comp} = {name}", p, False))
    return out


def pop_specials(H, W, seed, src_mode):
    """Maps of identity planes (a = b = c = 0: every pixel lands on itself) with the specials at random pixels, each special at least once:
    -> [(src, [(y, xs, name, kept)])]; as many maps as the shape needs to hold them all."""
    rng = np.random.default_rng(seed)
    s = sign_of(src_mode)
    n = len(specials(0, W, s))
    maps, k = [], 0
    while k < n:
        src = np.zeros((H, W, 4), F)
        src[..., 3] = F(0.25)
        where = []
        for p in rng.permutation(H * W)[: max(1, (H * W) // 2)]:          # at most every second pixel: the others stay identities
            if k == n:
                break
            y, xs = divmod(int(p), W)
            name, plane, kept = specials(xs, W, s)[k]
            src[y, xs] = plane
            where.append((y, xs, name, kept))
            k += 1
        maps.append((src, where))
    return maps


@functools.lru_cache(maxsize=None)
def cases(shape, src_mode):
    """Every (name, src, fallback, where) of a shape and source view, with its restated (out, hit, win): computed once, shared, left unchanged."""
    H, W = shape
    fb = fallback_map(H, W, 900 + W)
    out = [("slanted", pop_slanted(H, W, 100 + W + src_mode), fb, None), ("collapse", pop_collapse(H, W, 200 + W, src_mode), fb, None)]
    out += [(f"specials {i}", src, fb, where) for i, (src, where) in enumerate(pop_specials(H, W, 300 + W, src_mode))]
    res = []
    for name, src, fb, where in out:
        src.setflags(write=False)
        res.append((name, src, fb, where, warp_restate(src, fb, src_mode)))
    fb.setflags(write=False)
    return res


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the restatement itself (CPU only)
def case_restatement_matches_loop():
    checked = hits = 0
    for shape in SHAPES:
        for src_mode in (0, 1):
            for name, src, fb, where, (out, hit, win) in cases(shape, src_mode):
                lo, lh, lw = warp_loop(src, fb, src_mode)
                assert same(out, lo) and same(hit, lh) and same(win, lw), (shape, src_mode, name)
                for y, xs, what, kept in where or ():
                    # a kept special competes (it may still lose its column to a nearer pixel); a dropped one never wins
                    assert kept or not (win[y] == xs).any(), (shape, src_mode, what)
                    if what.startswith("v = ") and (win[y] == xs).any():
                        rx = int(np.nonzero(win[y] == xs)[0][0])
                        assert same(out[y, rx, 3], -src[y, xs, 3]) and np.signbit(out[y, rx, 3]) != np.signbit(src[y, xs, 3]), (shape, what)
                checked += 1
                hits += int(hit.sum())
    return checked, hits


def case_populations_do_what_they_say():
    """The populations hold what test 2 needs: occlusion, holes and collisions in (a); about five sources per column, won by the largest d and not the
    largest xs, in (b); in (c) every special placed, kept ones landing and dropped ones leaving the fallback in the output."""
    seen = set()
    for shape in SHAPES[3:]:
        H, W = shape
        for src_mode in (0, 1):
            s = sign_of(src_mode)
            for name, src, fb, where, (out, hit, win) in cases(shape, src_mode):
                ys, xs = np.mgrid[0:H, 0:W]
                if name == "slanted":
                    assert 0 < hit.sum() < H * W, (shape, name)                                  # holes
                    assert same(out[hit == 0], fb[hit == 0])
                    assert (np.abs(src[..., 0]) <= F(0.4)).all()
                    with np.errstate(all="ignore"):
                        d = (src[..., 0] * xs.astype(F) + src[..., 1] * ys.astype(F)) + src[..., 2]
                        rx = np.floor((xs.astype(F) - d * s) + F(0.5)).astype(np.int64)
                    assert ((rx >= 0) & (rx < W)).sum() > hit.sum(), (shape, name)               # collisions: more candidates in the image than pixels hit
                elif name == "collapse":
                    with np.errstate(all="ignore"):
                        d = (src[..., 0] * xs.astype(F) + src[..., 1] * ys.astype(F)) + src[..., 2]
                        rx = np.floor((xs.astype(F) - d * s) + F(0.5)).astype(np.int64)
                    row = 0
                    cols, counts = np.unique(rx[row][(rx[row] >= 0) & (rx[row] < W)], return_counts=True)
                    assert 4.0 <= counts.mean() <= 6.0, (shape, counts.mean())
                    not_last = 0
                    for cx in cols:
                        cand = np.nonzero(rx[row] == cx)[0]
                        assert win[row, cx] == cand[np.argmax(d[row, cand])]
                        not_last += int(win[row, cx] != cand.max())
                    # d decides, not xs.  Sources on one column have d = sign (xs - t) + 0.5 sign with t within one pixel: from the left view the
                    # largest d is the largest xs, from the right view the smallest
                    assert (not_last > 0) == (src_mode == 1), (shape, src_mode, not_last)
                else:
                    for y, x, what, kept in where:
                        seen.add(what)
                        if kept is False:
                            assert not (win[y] == x).any(), (shape, what)
                        if kept and what.startswith("t = "):
                            assert win[y, 0 if what == "t = 0" else W - 1] == x or hit[y, 0 if what == "t = 0" else W - 1], (shape, what)
                    assert (hit == 0).any() and same(out[hit == 0], fb[hit == 0])
    assert len(seen) == len(specials(0, 8, F(1))), seen
    return len(seen)


# ------------------------------------------------------------------------------------------------ device harness
class Dev:
    """An energy context of the shape (image-based cost, no aggregation: any image size) and device buffers for src, fallback, out, hit."""

    def __init__(self, lib, H, W):
        im = np.zeros((H, W, 3), np.uint8)
        self.e = api.HipCostVolumeEnergy.naive(im, im, windR=0, max_disp=63.0, lib=lib, filter="")
        self.H, self.W = H, W
        P = H * W
        self.src, self.fb, self.out = (api.DeviceBuffer(self.e, P * 16) for _ in range(3))
        self.hit = api.DeviceBuffer(self.e, max(16, P))

    def warp(self, src, fb, src_mode, in_place=False, with_hit=True):
        """-> (out, hit or None) of one call; in_place: d_out is the d_fallback buffer."""
        self.src.upload(src); self.fb.upload(fb)
        self.out.fill(0x5A); self.hit.fill(0x5A)
        dst = self.fb if in_place else self.out
        self.e.warp_labels(src_mode, self.src.ptr, self.fb.ptr, dst.ptr, self.hit.ptr if with_hit else None)
        self.e.synchronize()
        hit = self.hit.download((self.H, self.W), np.uint8)
        if not with_hit:
            assert (hit == 0x5A).all()
        return dst.download((self.H, self.W, 4), F), hit if with_hit else None

    def close(self):
        for b in (self.src, self.fb, self.out, self.hit):
            b.free()
        self.e.close()


# ------------------------------------------------------------------------------------------------ 2. kernel against the restatement
def case_kernel_bit_for_bit(lib, shape):
    H, W = shape
    d = Dev(lib, H, W)
    n = 0
    try:
        for src_mode in (0, 1):
            for name, src, fb, where, (want, want_hit, _) in cases(shape, src_mode):
                got, hit = d.warp(src, fb, src_mode)
                diff = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
                assert not diff.any(), f"{H}x{W}, view {src_mode}, {name}: {int(diff.sum())} planes differ from the restatement, first at {np.argwhere(diff)[0]}"
                assert same(hit, want_hit), (shape, src_mode, name)
                # (d) d_out is the d_fallback buffer, and no hit map
                got2, _ = d.warp(src, fb, src_mode, in_place=True, with_hit=False)
                assert same(got2, want), (shape, src_mode, name, "in place")
                n += 1
        # d_out may not be d_src
        try:
            d.e.warp_labels(0, d.src.ptr, d.fb.ptr, d.src.ptr)
            raise AssertionError("d_out == d_src was accepted")
        except api.LesHipError as ex:
            assert "error 1" in str(ex)
    finally:
        d.close()
    return n


WIDEST = (1, api.WARP_MAX_WIDTH)        # the widest row the kernel serves: 64 KB of dynamic LDS, 32 strides of the workgroup


# ------------------------------------------------------------------------------------------------ 3. landing bound
def case_landing_bound(lib, shape):
    """On population (a), from the KERNEL's output: at every hit pixel the transformed plane at the landing column is within 0.5 |a'| + 1e-4 of the
    winning source pixel's d.  -> (hit pixels, worst ratio to the bound)"""
    H, W = shape
    d = Dev(lib, H, W)
    worst, n = 0.0, 0
    try:
        for src_mode in (0, 1):
            name, src, fb, _, (_, _, win) = cases(shape, src_mode)[0]
            assert name == "slanted"
            got, hit = d.warp(src, fb, src_mode)
            ys, xs = np.nonzero(hit)
            if not len(ys):
                continue
            w = win[ys, xs]
            assert (w >= 0).all()
            l = src[ys, w]
            dsrc = ((l[:, 0] * w.astype(F) + l[:, 1] * ys.astype(F)) + l[:, 2]).astype(F)
            assert np.abs(dsrc).max() < 256
            o = got[ys, xs].astype(np.float64)
            dt = o[:, 0] * xs + o[:, 1] * ys + o[:, 2]
            bound = 0.5 * np.abs(o[:, 0]) + 1e-4
            err = np.abs(dt - dsrc.astype(np.float64))
            print(f"landing bound {H}x{W} view {src_mode}: {len(ys)} hit pixels, worst |d' - d| {err.max():.6f}, worst ratio to the bound {(err / bound).max():.4f}")
            assert (err <= bound).all(), (shape, src_mode, float((err / bound).max()))
            worst, n = max(worst, float((err / bound).max())), n + len(ys)
    finally:
        d.close()
    return n, worst


# ------------------------------------------------------------------------------------------------ 4. independence, the width limit
def case_independence(lib, device):
    """The same inputs on a second stream and beside another enqueued kernel (a 64 MB streaming copy on the context's stream) give the same bits."""
    shape = (4, 300)
    H, W = shape
    d = Dev(lib, H, W)
    try:
        name, src, fb, _, (want, want_hit, _) = cases(shape, 0)[0]
        got, hit = d.warp(src, fb, 0)
        assert same(got, want) and same(hit, want_hit)
        n = 1 << 24
        big = [api.DeviceBuffer(d.e, 4 * n) for _ in range(2)]
        big[0].fill(1)
        side = None
        if device == "cuda":
            import torch
            side = torch.cuda.Stream()
            d.e.set_thread_stream(side.cuda_stream)
        try:
            got2, hit2 = d.warp(src, fb, 0)                                                          # a second stream
            assert same(got2, want) and same(hit2, want_hit)
            d.src.upload(src); d.fb.upload(fb); d.out.fill(0x5A); d.hit.fill(0x5A)
            d.e._chk(d.e.L.les_hip_calib_copy(api.C.c_void_p(big[0].ptr), api.C.c_void_p(big[1].ptr), n, 0, None))      # default stream: runs beside
            d.e.warp_labels(0, d.src.ptr, d.fb.ptr, d.out.ptr, d.hit.ptr)
            d.e.synchronize()
            assert same(d.out.download((H, W, 4), F), want) and same(d.hit.download((H, W), np.uint8), want_hit)
        finally:
            if side is not None:
                d.e.set_thread_stream(0, bind=False)
                import torch
                torch.cuda.synchronize()
            for b in big:
                b.free()
    finally:
        d.close()


def case_width_limit(lib):
    """A row wider than the stated limit: LES_HIP_ERR_UNSUPPORTED and nothing launched (the output keeps its guard bytes); the limit is at least
    8192."""
    assert api.WARP_MAX_WIDTH >= 8192
    H, W = 1, api.WARP_MAX_WIDTH + 1
    d = Dev(lib, H, W)
    try:
        src = np.zeros((H, W, 4), F)
        d.src.upload(src); d.fb.upload(src); d.out.fill(0x5A); d.hit.fill(0x5A)
        try:
            d.e.warp_labels(0, d.src.ptr, d.fb.ptr, d.out.ptr, d.hit.ptr)
            raise AssertionError("a row above the limit was accepted")
        except api.LesHipError as ex:
            assert f"error {api.LES_HIP_ERR_UNSUPPORTED}" in str(ex), str(ex)
        d.e.synchronize()
        assert (d.out.download((H * W * 16,), np.uint8) == 0x5A).all() and (d.hit.download((H * W,), np.uint8) == 0x5A).all()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 5. cross_fuse on the cones crop
UNITS = (16, 60)
TABLE = [[(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANSAC, 1)], [(api.PROPOSE_EXPANSION, 1)]]


WINDR = 6                      # filter radius of the cross_fuse case (the energy's definition does not matter to it; 20 costs the simulator minutes)


def driver(lib, device, device_cuts, world=1, **opts):
    """stereo.FastGCStereo on the cones crop as tests/eval_cases.py pads it (image-based energy, both views), two layers."""
    from localexpstereo_amd import stereo
    imL, imR, gt = ec.cones_images()
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=WINDR, max_disp=63.0, lib=lib)
    st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=1.0, windR=WINDR), device=device, seed=3, device_cuts=device_cuts, world=world, **opts)
    st.setEvaluator(ec.lio.Evaluator(gt, gt > 0, 1.0), precision=0.25)
    st.concurrent_views = False
    for u, t in zip(UNITS, TABLE):
        st.addLayer(u, t)
    return st, e


def energy_of(st, e, device, labels, mode):
    """The energy of a labelling of view `mode` with its own dense costs."""
    from localexpstereo_amd import pm
    r = pm.PMRunner(e, UNITS, TABLE, seed=1, device=device, mode=mode)
    try:
        r.init_from_labels(labels)
        return sum(r.energy(st._pairwise()))
    finally:
        r.close()


def warp_on_device(e, src, fb, src_mode):
    H, W = src.shape[:2]
    bufs = [api.DeviceBuffer(e, H * W * 16) for _ in range(3)]
    try:
        bufs[0].upload(src); bufs[1].upload(fb)
        e.warp_labels(src_mode, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
        e.synchronize()
        return bufs[2].download((H, W, 4), F)
    finally:
        for b in bufs:
            b.free()


def case_cross_fuse(lib, device, device_cuts):
    """Both views come from a two-view run of one PatchMatch and one graph-cut iteration (its labellings before the post-processing)."""
    st, e = driver(lib, device, device_cuts)
    out = {}
    try:
        st.run(1, (0, 1), 1)
        maps = {m: st.raw_labelings[m] for m in (0, 1)}
        got = st.cross_fuse(maps)
        stats = st.cross_stats
        hand = {}
        for m in (0, 1):
            warped = warp_on_device(e, maps[1 - m], maps[m], 1 - m)
            assert same(warped, warp_restate(maps[1 - m], maps[m], 1 - m)[0])
            own = (got[m].view(np.uint32) == maps[m].view(np.uint32)).all(-1)
            other = (got[m].view(np.uint32) == warped.view(np.uint32)).all(-1)
            assert (own | other).all(), (m, int((~(own | other)).sum()))
            E0, E1 = energy_of(st, e, device, maps[m], m), energy_of(st, e, device, got[m], m)
            assert E1 <= E0 + fc.RISE * abs(E0), (m, E0, E1)
            assert ec.same_float(stats[m]["energy_before"], E0), (stats[m]["energy_before"], E0)
            assert stats[m]["hit_pixels"] == int(warp_restate(maps[1 - m], maps[m], 1 - m)[1].sum())
            out[f"view{m}"] = dict(pixels_taken=int((~own).sum()), hit_pixels=stats[m]["hit_pixels"], E_before=E0, E_after=E1, fall=E0 - E1)
            # the two fuse calls written out by hand
            hand[m] = st.fuse(maps[m], [warped], viewMode=m)
            assert same(hand[m], got[m]), m
        print("cross_fuse on the cones crop:", out)
        # a repeat is bit-identical; the order of the views cannot matter (both warps read the inputs: the hand-written calls above ran one by one)
        again = st.cross_fuse({1: maps[1], 0: maps[0]})
        assert same(again[0], got[0]) and same(again[1], got[1])
        try:
            st.cross_fuse({0: maps[0]})
            raise AssertionError("one view was accepted")
        except ValueError:
            pass
        st2, e2 = driver(lib, device, device_cuts, world=2)
        try:
            st2.cross_fuse(maps)
            raise AssertionError("world = 2 was accepted")
        except NotImplementedError:
            pass
        finally:
            e2.close()
    finally:
        e.close()
    return out


# ------------------------------------------------------------------------------------------------ 6. the driver
def cones_data():
    imL, imR, gt = ec.cones_images()
    return dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=0.25)


def check_cross_rows(st, pmInit, maxIteration, cross_view):
    """The inner-loop log of a cross_view run: per view and graph-cut iteration that ends with a cross-view step, the rows of the fusion's sets follow
    those of the cuts, and no view's energy after the step is above the energy before it (within RISE).  -> worst relative change over a step"""
    worst = -np.inf
    steps = [it for it in range(1, maxIteration + 1) if it % cross_view == 0 or it == maxIteration]
    assert [s["iteration"] for s in st.cross_view_stats] == steps
    for m in (0, 1):
        rows = [r for r in st.inner_log if r["mode"] == m]
        per_it = {it: [r for r in rows if r["iteration"] == it] for it in range(1, pmInit + maxIteration + 1)}
        nsets = len(per_it[1])
        for it in range(1, pmInit + maxIteration + 1):
            is_step = it - pmInit in steps
            assert len(per_it[it]) == (2 if is_step else 1) * nsets, (m, it, len(per_it[it]), nsets)
            if is_step:
                before, after = per_it[it][nsets - 1]["energy"], per_it[it][-1]["energy"]
                assert after <= before + fc.RISE * abs(before), (m, it, before, after)
                worst = max(worst, (after - before) / abs(before))
                if m == 0:          # the iteration's row of the main log is made after the step
                    main = [r for r in st.log if r["index"] == it][0]
                    assert ec.same_float(main["energy"], after), (main["energy"], after)
    return worst


def sim_layers(st, sizes):
    """The simulator runs' layers in the place of stereo._layers: two layers of few, large cells and three proposals in all (MidV2's 5 / 15 / 25 and
    MidV3's 1 / 3 / 10 pixel cells with 15 proposals take tens of minutes on the fibre simulator)."""
    st.addLayer(24, [(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANSAC, 1)])
    st.addLayer(92, [(api.PROPOSE_EXPANSION, 1)])


def case_driver_midv2(lib, device, monkeypatch, layers=None, **opts):
    """MidV2 on the cones crop, two views, 1 + 2 iterations.  layers: None = MidV2's own, else what replaces stereo._layers; opts: further arguments
    of MidV2 (the simulator run: sim_layers and a filter radius of 6; the GPU test runs MidV2 unchanged)."""
    from localexpstereo_amd import stereo
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    data = cones_data()
    kw = dict(iterations=2, pmIterations=1, doDual=True, device=device, lib=lib, **opts)
    st_a, lab_a, raw_a = stereo.MidV2(data, **kw)
    st_b, lab_b, raw_b = stereo.MidV2(data, cross_view=0, **kw)
    assert same(lab_a, lab_b) and same(raw_a, raw_b) and not st_b.cross_view_stats
    st_c, lab_c, raw_c = stereo.MidV2(data, cross_view=1, inner_loop_log=True, **kw)
    assert lab_c.shape == lab_a.shape and np.isfinite(lab_c).all()
    worst = check_cross_rows(st_c, 1, 2, 1)
    taken = [s["views"][m]["pixels_taken"] for s in st_c.cross_view_stats for m in (0, 1)]
    print(f"MidV2 cones crop, cross_view=1: worst relative energy change over a cross-view step {worst:.3e}, pixels taken per step and view {taken}; "
          f"final energy {st_c.log[-2]['energy']:.2f} against {st_a.log[-2]['energy']:.2f} without")
    try:
        stereo.MidV2(data, iterations=1, pmIterations=1, doDual=False, cross_view=1, device=device, lib=lib, **opts)
        raise AssertionError("cross_view with one view was accepted")
    except ValueError:
        pass
    return worst


def case_driver_midv3(lib, device, monkeypatch, layers=None, **opts):
    """MidV3 from the pair alone (volumes built on the device), two views, 1 + 1 iterations, cross_view=1.  layers, opts: as case_driver_midv2."""
    from localexpstereo_amd import stereo
    from tests import costvol_cases as cc
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    imL, imR, gt = cc.cones_pair()
    data = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
    st, lab, raw = stereo.MidV3(data, None, None, iterations=1, pmIterations=1, doDual=True, device=device, lib=lib, cross_view=1, inner_loop_log=True, **opts)
    assert lab.shape == gt.shape + (4,) and np.isfinite(lab).all()
    worst = check_cross_rows(st, 1, 1, 1)
    print(f"MidV3 from the pair, cross_view=1: worst relative energy change over a cross-view step {worst:.3e}")
    return worst
