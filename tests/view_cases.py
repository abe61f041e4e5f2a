"""Cases of tests/test_view.py: view synthesis and the photometric check (csrc/les_view.h: les_hip_render_view, les_hip_blend_views,
les_hip_photo_error; api.HipCostVolumeEnergy.render_view / .blend_views / .photo_error; stereo.FastGCStereo.synthesize / .photo_error /
max_photo_error=; io.photometric) on the CPU simulator build and on the MI355X.

The definitions, restated from csrc/les_view.h.  Every operation rounded to f32, in this order; sign = +1 for source view 0, -1 for view 1.
  render    source pixel (xs, y), label (a, b, c, v):  d = (a xs + b y) + c,  tt = (xs - (d t) sign) + 0.5;  the candidate exists iff
            -1e9 < tt < 1e9 and rx = floor(tt) lies in [0, W).  Per target column the largest d wins (-0 = +0), among equal d the largest xs:
            disp[rx] = its d, hit = 1.  A column 0 < rx < W - 1 without a winner whose neighbours both have hit == 1 and |disp[rx-1] - disp[rx+1]| <= 1
            gets disp = (disp[rx-1] + disp[rx+1]) * 0.5, hit = 2.  Every hit column:  xsrc = rx + (disp t) sign clamped to [0, W - 1],  x0 = floor(xsrc),
            x1 = min(x0 + 1, W - 1),  w = xsrc - x0,  per channel val = ((1 - w) c0) + (w c1),  out = (u8)(int)(val + 0.5).  A hole: colour 0, disp NaN, hit 0.
            (The clamp is xsrc > 0 ? (xsrc < W - 1 ? xsrc : W - 1) : 0: a NaN -- a crack at t = 0 between two disparities whose sum overflows -- samples column 0.)
  blend     per pixel, a side counts where its hit != 0: both and |dL - dR| <= tol: colour (u8)(int)((((1 - t) cL) + (t cR)) + 0.5), disp
            ((1 - t) dL) + (t dR), src 3; both otherwise: the larger disp, a tie to the left, src 1 / 2; one: it, src 1 / 2; none: src 0, colour 0,
            disp NaN.  fill: a hole takes colour and disp of l, the nearest column to the left that was no hole, or r, the nearest to the right: the
            smaller disp, equal to l, the one there is when one is missing; src 4.  A row of holes stays.
  photo     d as above; vis 0 when the t = 1 candidate does not exist; 2 when it is not the winner of its column; else xo = xs - d sign, vis 0
            unless 0 <= xo <= W - 1, else vis 1 and err = ((|val_b - b| + |val_g - g|) + |val_r - r|) / 3 with val the OTHER image sampled at xo as
            above, unrounded, against the pixel's own bytes.  err NaN where vis != 1.

References, none of them the code under test: the vectorised numpy restatements below, themselves held to literal per-pixel loops.  Tolerances:
none -- every output is compared bit for bit (u8 colours, f32 disp / err with their NaN pattern 0x7fc00000, hit / src / vis).  The cones figures
are strict inequalities between the restatement's own numbers, which the device matches bit for bit.

Shapes: the label warp's (crossview_cases.SHAPES: a row shorter than a wave, the wave and workgroup boundaries, the strided loop, several strides;
the blend's scan chunks are 1 ... 5 columns there) and the widest row, (2, 8192), 32 columns per scan chunk."""
import functools

import numpy as np

from localexpstereo_amd import api
from tests import costvol_cases as cc
from tests import crossview_cases as cv
from tests import eval_cases as ec

F = np.float32
SHAPES = cv.SHAPES
WIDEST = (2, api.WARP_MAX_WIDTH)
TS = (0.0, 0.25, 0.5, 1.0)
QNAN = np.uint32(0x7FC00000).view(F)
sign_of, same = cv.sign_of, cv.same


def nan_map(H, W):
    return np.full((H, W), QNAN, F)


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def disparity(lab):
    H, W = lab.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        return ((lab[..., 0] * xs.astype(F) + lab[..., 1] * ys.astype(F)) + lab[..., 2]).astype(F)


def splat(lab, src_mode, t):
    """Phase A -> (d H x W, ok: the candidate exists, rx: its landing column, win H x W: the winning source column per target column, -1 none)"""
    H, W = lab.shape[:2]
    s, t = sign_of(src_mode), F(t)
    ys, xs = np.mgrid[0:H, 0:W]
    d = disparity(lab)
    with np.errstate(all="ignore"):
        tt = ((xs.astype(F) - (d * t) * s) + F(0.5)).astype(F)
        ok = (tt > F(-1.0e9)) & (tt < F(1.0e9))
        rx = np.floor(np.where(ok, tt, F(0))).astype(np.int64)
    ok &= (rx >= 0) & (rx < W)
    win = np.full((H, W), -1, np.int64)
    yy, xx = ys[ok], xs[ok]
    if len(yy):
        tgt = yy * W + rx[ok]
        order = np.lexsort((xx, d[ok] + F(0), tgt))              # by target pixel, then d (-0 -> +0), then xs: the winner is the last of its group
        last = np.ones(len(order), bool)
        last[:-1] = tgt[order][1:] != tgt[order][:-1]
        w = order[last]
        win[yy[w], rx[ok][w]] = xx[w]
    return d, ok, rx, win


def sample(img, rows, xsrc):
    """img rows sampled linearly at xsrc in [0, W - 1] (arrays of one shape) -> val, float32 [..., 3], unrounded"""
    W = img.shape[1]
    x0f = np.floor(xsrc).astype(F)
    x0 = x0f.astype(np.int64)
    x1 = np.minimum(x0 + 1, W - 1)
    w = (xsrc - x0f).astype(F)[..., None]
    c0, c1 = img[rows, x0].astype(F), img[rows, x1].astype(F)
    return (((F(1) - w) * c0).astype(F) + (w * c1).astype(F)).astype(F)


def round_u8(val):
    return (val + F(0.5)).astype(F).astype(np.int32).astype(np.uint8)


def render_restate(lab, img, src_mode, t):
    """-> (bgr H x W x 3 u8, disp H x W f32, hit H x W u8)"""
    H, W = lab.shape[:2]
    s, t = sign_of(src_mode), F(t)
    d, _, _, win = splat(lab, src_mode, t)
    ys, xs = np.mgrid[0:H, 0:W]
    won = win >= 0
    disp, hit = nan_map(H, W), won.astype(np.uint8)
    disp[won] = d[ys[won], win[won]]
    if W >= 3:
        dl, dr = disp[:, :-2], disp[:, 2:]
        with np.errstate(all="ignore"):
            crack = ~won[:, 1:-1] & won[:, :-2] & won[:, 2:] & (np.abs(dl - dr) <= F(1))
            mid = ((dl + dr).astype(F) * F(0.5)).astype(F)
        disp[:, 1:-1][crack] = mid[crack]
        hit[:, 1:-1][crack] = 2
    bgr = np.zeros((H, W, 3), np.uint8)
    h = hit != 0
    with np.errstate(all="ignore"):
        xsrc = (xs[h].astype(F) + (disp[h] * t) * s).astype(F)
    xsrc = np.where(xsrc > F(0), np.where(xsrc < F(W - 1), xsrc, F(W - 1)), F(0)).astype(F)              # (a NaN becomes 0)
    bgr[h] = round_u8(sample(img, ys[h], xsrc))
    return bgr, disp, hit


def render_loop(lab, img, src_mode, t):
    """The same by a literal per-pixel transcription of the definition (scalar f32 operations)."""
    H, W = lab.shape[:2]
    s, t = sign_of(src_mode), F(t)
    bgr, disp, hit = np.zeros((H, W, 3), np.uint8), nan_map(H, W), np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(H):
            best = {}
            for xs in range(W):
                a, b, c, _ = (F(k) for k in lab[y, xs])
                d = F(F(F(a * F(xs)) + F(b * F(y))) + c)
                tt = F(F(F(xs) - F(F(d * t) * s)) + F(0.5))
                if not (tt > F(-1.0e9) and tt < F(1.0e9)):
                    continue
                rx = int(np.floor(tt))
                if rx < 0 or rx >= W:
                    continue
                if rx not in best or d > best[rx][0] or (d == best[rx][0] and xs > best[rx][1]):
                    best[rx] = (d, xs)
            for rx, (d, _) in best.items():
                disp[y, rx], hit[y, rx] = d, 1
            for rx in range(1, W - 1):
                if rx not in best and rx - 1 in best and rx + 1 in best and abs(F(best[rx - 1][0] - best[rx + 1][0])) <= F(1):
                    disp[y, rx], hit[y, rx] = F(F(best[rx - 1][0] + best[rx + 1][0]) * F(0.5)), 2
            for rx in range(W):
                if not hit[y, rx]:
                    continue
                xsrc = F(F(rx) + F(F(disp[y, rx] * t) * s))
                xsrc = (xsrc if xsrc < F(W - 1) else F(W - 1)) if xsrc > F(0) else F(0)
                x0 = int(np.floor(xsrc))
                x1 = min(x0 + 1, W - 1)
                w = F(xsrc - F(x0))
                for k in range(3):
                    val = F(F(F(F(1) - w) * F(img[y, x0, k])) + F(w * F(img[y, x1, k])))
                    bgr[y, rx, k] = int(F(val + F(0.5)))
    return bgr, disp, hit


def blend_restate(t, tol, fill, left, right, shape):
    """left / right: (bgr, disp, hit) or None -> (bgr, disp, src)"""
    H, W = shape
    t, tol = F(t), F(tol)
    none = (np.zeros((H, W, 3), np.uint8), np.zeros((H, W), F), np.zeros((H, W), np.uint8))
    (bl, dl, hl), (br, dr, hr) = (left or none), (right or none)
    hl, hr = hl != 0, hr != 0
    with np.errstate(all="ignore"):
        agree = hl & hr & (np.abs(dl - dr) <= tol)
        right_wins = hr & (~hl | (~agree & (dr > dl)))
        left_wins = hl & ~agree & ~right_wins
        mix_c = round_u8((((F(1) - t) * bl.astype(F)).astype(F) + (t * br.astype(F)).astype(F)).astype(F))
        mix_d = (((F(1) - t) * dl).astype(F) + (t * dr).astype(F)).astype(F)
    src = np.where(agree, 3, np.where(left_wins, 1, np.where(right_wins, 2, 0))).astype(np.uint8)
    bgr, disp = np.zeros((H, W, 3), np.uint8), nan_map(H, W)
    bgr[agree], disp[agree] = mix_c[agree], mix_d[agree]
    bgr[left_wins], disp[left_wins] = bl[left_wins], dl[left_wins]
    bgr[right_wins], disp[right_wins] = br[right_wins], dr[right_wins]
    if fill:
        cols = np.broadcast_to(np.arange(W), (H, W))
        some = src != 0
        l = np.maximum.accumulate(np.where(some, cols, -1), axis=1)
        r = np.minimum.accumulate(np.where(some, cols, W)[:, ::-1], axis=1)[:, ::-1]
        ys = np.broadcast_to(np.arange(H)[:, None], (H, W))
        hole = ~some & ((l >= 0) | (r < W))
        lc, rc = np.clip(l, 0, W - 1), np.clip(r, 0, W - 1)
        with np.errstate(all="ignore"):
            take_r = (l < 0) | ((r < W) & (disp[ys, rc] < disp[ys, lc]))
        pick = np.where(take_r, rc, lc)
        fb, fd = bgr[ys, pick], disp[ys, pick]
        bgr, disp, src = bgr.copy(), disp.copy(), src.copy()
        bgr[hole], disp[hole], src[hole] = fb[hole], fd[hole], 4
    return bgr, disp, src


def blend_loop(t, tol, fill, left, right, shape):
    H, W = shape
    t, tol = F(t), F(tol)
    bgr, disp, src = np.zeros((H, W, 3), np.uint8), nan_map(H, W), np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                hl, hr = left is not None and left[2][y, x] != 0, right is not None and right[2][y, x] != 0
                if hl and hr:
                    dl, dr = left[1][y, x], right[1][y, x]
                    if abs(F(dl - dr)) <= tol:
                        for k in range(3):
                            bgr[y, x, k] = int(F(F(F(F(F(1) - t) * F(left[0][y, x, k])) + F(t * F(right[0][y, x, k]))) + F(0.5)))
                        disp[y, x], src[y, x] = F(F(F(F(1) - t) * dl) + F(t * dr)), 3
                        continue
                    hl, hr = not dr > dl, dr > dl
                if hl:
                    bgr[y, x], disp[y, x], src[y, x] = left[0][y, x], left[1][y, x], 1
                elif hr:
                    bgr[y, x], disp[y, x], src[y, x] = right[0][y, x], right[1][y, x], 2
            if fill:
                before = src[y].copy()
                for x in range(W):
                    if before[x]:
                        continue
                    l = next((q for q in range(x - 1, -1, -1) if before[q]), None)
                    r = next((q for q in range(x + 1, W) if before[q]), None)
                    if l is None and r is None:
                        continue
                    p = l if r is None else (r if l is None else (r if disp[y, r] < disp[y, l] else l))
                    bgr[y, x], disp[y, x], src[y, x] = bgr[y, p], disp[y, p], 4
    return bgr, disp, src


def photo_restate(lab, own, other, mode):
    """-> (err H x W f32, vis H x W u8)"""
    H, W = lab.shape[:2]
    s = sign_of(mode)
    d, ok, rx, win = splat(lab, mode, 1.0)
    ys, xs = np.mgrid[0:H, 0:W]
    winner = ok & (win[ys, np.clip(rx, 0, W - 1)] == xs)
    with np.errstate(all="ignore"):
        xo = (xs.astype(F) - d * s).astype(F)
        inside = (xo >= F(0)) & (xo <= F(W - 1))
    vis = np.where(ok & ~winner, 2, np.where(winner & inside, 1, 0)).astype(np.uint8)
    err = nan_map(H, W)
    m = vis == 1
    a = np.abs(sample(other, ys[m], xo[m]) - own[m].astype(F)).astype(F)
    err[m] = (((a[:, 0] + a[:, 1]).astype(F) + a[:, 2]).astype(F) / F(3)).astype(F)
    return err, vis


def photo_loop(lab, own, other, mode):
    H, W = lab.shape[:2]
    s = sign_of(mode)
    err, vis = nan_map(H, W), np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(H):
            cand, best = {}, {}
            for xs in range(W):
                a, b, c, _ = (F(k) for k in lab[y, xs])
                d = F(F(F(a * F(xs)) + F(b * F(y))) + c)
                tt = F(F(F(xs) - F(F(d * F(1)) * s)) + F(0.5))
                if not (tt > F(-1.0e9) and tt < F(1.0e9)):
                    continue
                rx = int(np.floor(tt))
                if rx < 0 or rx >= W:
                    continue
                cand[xs] = (rx, d)
                if rx not in best or d > best[rx][0] or (d == best[rx][0] and xs > best[rx][1]):
                    best[rx] = (d, xs)
            for xs, (rx, d) in cand.items():
                if best[rx][1] != xs:
                    vis[y, xs] = 2
                    continue
                xo = F(F(xs) - F(d * s))
                if not (xo >= F(0) and xo <= F(W - 1)):
                    continue
                x0 = int(np.floor(xo))
                x1 = min(x0 + 1, W - 1)
                w = F(xo - F(x0))
                a = [abs(F(F(F(F(F(1) - w) * F(other[y, x0, k])) + F(w * F(other[y, x1, k]))) - F(own[y, xs, k]))) for k in range(3)]
                err[y, xs], vis[y, xs] = F(F(F(a[0] + a[1]) + a[2]) / F(3)), 1
    return err, vis


# ------------------------------------------------------------------------------------------------ populations and images
def pop_stretch(H, W, seed, src_mode):
    """sign a = -0.5: at t = 1 the row stretches 1.5 x (every second gap is a one-column crack between disparities 0.5 apart); odd rows are tilted
    along y as well."""
    rng = np.random.default_rng(seed)
    s = float(sign_of(src_mode))
    lab = np.zeros((H, W, 4), F)
    lab[..., 0] = F(-0.5 * s)
    lab[1::2, :, 1] = F(0.125)
    lab[..., 2] = (s * 0.25 * W + rng.uniform(-0.05, 0.05, (H, W))).astype(F)
    lab[..., 3] = rng.uniform(-1, 1, (H, W)).astype(F)
    return lab


def pop_nonfinite(H, W, seed, src_mode):
    """The slanted population with NaN, +inf and -inf in every component at random pixels, and its last row without any finite c."""
    rng = np.random.default_rng(seed)
    lab = cv.pop_slanted(H, W, seed + 7).copy()
    n = max(1, (H * W) // 12)
    for k in range(4):
        for val in (np.nan, np.inf, -np.inf):
            p = rng.integers(0, H * W, n)
            lab.reshape(-1, 4)[p, k] = val
    lab[H - 1, :, 2] = np.nan
    if W >= 5 and H > 1:             # a crack whose disparity overflows: at t = 0 its source position is inf * 0
        lab[0, 1:4] = 0
        lab[0, 1:4, 2] = (F(3e38), np.nan, F(3e38))
    return lab


def pop_scene(H, W, src_mode):
    """One fronto-parallel scene in both views: a background at disparity 2 and a nearer block at 6 (left view: columns W/3 ... W/3 + W/4; the right
    view sees it 6 columns further left).  The two renders of any t agree where both see a surface."""
    lab = np.zeros((H, W, 4), F)
    lab[..., 2] = F(2)
    x0, x1 = W // 3, W // 3 + max(1, W // 4)
    if src_mode == 1:
        x0, x1 = max(0, x0 - 6), max(0, x1 - 6)
    lab[:, x0:x1, 2] = F(6)
    return lab


POPS = ("slanted", "stretch", "collapse", "nonfinite", "scene")
WARPABLE = ("slanted", "stretch", "scene")          # every candidate passes the label warp's extra drops: q >= 0.125 and b, c, v finite


@functools.lru_cache(maxsize=None)
def labels(name, shape, src_mode):
    H, W = shape
    lab = {"slanted": lambda: cv.pop_slanted(H, W, 100 + W + src_mode), "stretch": lambda: pop_stretch(H, W, 400 + W, src_mode),
           "collapse": lambda: cv.pop_collapse(H, W, 200 + W, src_mode), "nonfinite": lambda: pop_nonfinite(H, W, 500 + W + src_mode, src_mode),
           "scene": lambda: pop_scene(H, W, src_mode)}[name]()
    lab = np.ascontiguousarray(lab, F)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def images(shape, kind):
    """kind "random": random bytes; "edges": columns of 0 and 255 next to each other (shifted per channel and row), so that both ends of the rounding
    are reached.  -> (imL, imR)"""
    H, W = shape
    if kind == "random":
        out = ec.random_images(H, W, 700 + W)
    else:
        ys, xs = np.mgrid[0:H, 0:W]
        out = tuple(np.stack([(((xs + ys + k + m) // (1 + k)) % 2 * 255) for k in range(3)], -1).astype(np.uint8) for m in (0, 1))
    for im in out:
        im.setflags(write=False)
    return tuple(np.ascontiguousarray(im) for im in out)


IMAGES = ("random", "edges")


@functools.lru_cache(maxsize=None)
def render_want(name, shape, src_mode, t, kind):
    out = render_restate(labels(name, shape, src_mode), images(shape, kind)[src_mode], src_mode, t)
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def photo_want(name, shape, mode, kind):
    im = images(shape, kind)
    return photo_restate(labels(name, shape, mode), im[mode], im[1 - mode], mode)


BLENDS = (("scene", 1.0, 1), ("scene", 1.0, 0), ("slanted", 1.0, 1), ("slanted", 0.0, 1), ("nonfinite", 1.0, 1), ("nonfinite", 1.0, 0), ("stretch", 0.5, 0))       # (population of both views, tol, fill)


def blend_inputs(name, shape, t, kind="random"):
    """The restated renders of both views for the camera at t -> (left, right)"""
    return render_want(name, shape, 0, t, kind), render_want(name, shape, 1, float(F(1) - F(t)), kind)


def same_maps(got, want):
    return all(same(g, w) for g, w in zip(got, want))


def first_diff(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if not same(g, w):
            gb, wb = (np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.uint32) for a in (g, w))
            return f"output {k}: {int((gb != wb).sum())} elements differ, first at {np.argwhere(gb != wb)[0]}"
    return "equal"


# ------------------------------------------------------------------------------------------------ 1. the restatements themselves (CPU only)
def case_restatement_matches_loop():
    """Every population, both views and both images against the per-pixel loops: all of TS on rows up to 300 pixels, t = 0.5 on the longer ones."""
    n = 0
    for shape in SHAPES:
        for src_mode in (0, 1):
            for i, name in enumerate(POPS):
                kind = IMAGES[(i + src_mode) % 2]
                lab, im = labels(name, shape, src_mode), images(shape, kind)
                for t in (TS if shape[1] <= 300 else (0.5,)):
                    assert same_maps(render_want(name, shape, src_mode, t, kind), render_loop(lab, im[src_mode], src_mode, t)), (shape, src_mode, name, t)
                    n += 1
                assert same_maps(photo_want(name, shape, src_mode, kind), photo_loop(lab, im[src_mode], im[1 - src_mode], src_mode)), (shape, src_mode, name)
        for name, tol, fill in BLENDS:
            for t in ((0.25, 1.0) if shape[1] <= 300 else (0.5,)):
                left, right = blend_inputs(name, shape, t)
                for l, r in ((left, right), (left, None), (None, right)):
                    assert same_maps(blend_restate(t, tol, fill, l, r, shape), blend_loop(t, tol, fill, l, r, shape)), (shape, name, t, tol, fill)
                    n += 1
    return n


def case_populations_do_what_they_say():
    """The populations hold what the device cases need: occlusion, holes and collisions in "slanted"; single-column cracks in "stretch"; about five
    sources per column in "collapse"; dropped candidates in "nonfinite"; every value of hit, vis and src."""
    seen_src, seen_vis = set(), set()
    for shape in SHAPES[3:]:
        H, W = shape
        for src_mode in (0, 1):
            for name in POPS:
                lab = labels(name, shape, src_mode)
                d, ok, rx, win = splat(lab, src_mode, 1.0)
                _, _, hit = render_want(name, shape, src_mode, 1.0, "random")
                err, vis = photo_want(name, shape, src_mode, "random")
                seen_vis |= set(np.unique(vis).tolist())
                assert np.isnan(err[vis != 1]).all() and np.isfinite(err[vis == 1]).all()
                if name == "slanted":
                    assert (hit == 0).any() and (hit == 1).any(), (shape, name)                          # holes
                    assert ok.sum() > (win >= 0).sum(), (shape, name)                                     # collisions
                    assert (vis == 2).any(), (shape, name)                                                # occlusion
                elif name == "stretch":
                    assert (hit == 2).sum() >= W // 8, (shape, name, int((hit == 2).sum()))               # cracks, a third of the landed span
                    cols = np.nonzero(hit[0] == 2)[0]
                    assert (hit[0, cols - 1] == 1).all() and (hit[0, cols + 1] == 1).all()
                elif name == "collapse":
                    cols, counts = np.unique(rx[0][ok[0]], return_counts=True)
                    assert 4.0 <= counts.mean() <= 6.0, (shape, counts.mean())
                    assert (hit[1] == 2).any(), shape                                                     # the 1.8 x rows crack too
                elif name == "nonfinite":
                    assert (~np.isfinite(d)).any() and not ok[~np.isfinite(d)].any() and not ok[H - 1].any(), shape
                    _, disp0, hit0 = render_want(name, shape, src_mode, 0.0, "random")
                    assert hit0[0, 2] == 2 and np.isinf(disp0[0, 2]), shape                               # the overflowing crack
                    for k in range(4):
                        assert np.isnan(lab[..., k]).any() and np.isinf(lab[..., k]).any(), (shape, k)
        for name, tol, fill in BLENDS:
            for t in (0.25, 0.5):
                left, right = blend_inputs(name, shape, t)
                _, disp, src = blend_restate(t, tol, fill, left, right, shape)
                seen_src |= {(int(v), fill) for v in np.unique(src)}
                assert np.isnan(disp[src == 0]).all()
                if name == "nonfinite" and H > 1:
                    assert (src[H - 1] == 0).all(), shape                                                 # a row without a pixel stays a hole when filling
    assert seen_vis == {0, 1, 2}, seen_vis
    assert {(v, 0) for v in (0, 1, 2, 3)} <= seen_src and {(v, 1) for v in (0, 1, 2, 3, 4)} <= seen_src, seen_src
    # the rounding reaches both ends on the edges image: a rendered 0 and a rendered 255 next to interpolated values
    bgr, _, hit = render_want("slanted", (4, 300), 0, 0.5, "edges")
    vals = set(np.unique(bgr[hit != 0]).tolist())
    assert {0, 255} <= vals and len(vals) > 2, sorted(vals)[:8]
    return sorted(seen_src)


def case_photometric_summary():
    from localexpstereo_amd import io as lio
    err = np.array([[1.0, np.nan, 30.0], [np.nan, 5.0, np.nan]], F)
    vis = np.array([[1, 2, 1], [0, 1, 2]], np.uint8)
    got = lio.photometric(err, vis, thresh=10.0)
    assert got == dict(mean=12.0, bad=1.0 / 3.0, visible=0.5, occluded=2.0 / 6.0), got
    none = lio.photometric(np.full((1, 2), np.nan, F), np.zeros((1, 2), np.uint8))
    assert np.isnan(none["mean"]) and np.isnan(none["bad"]) and none["visible"] == 0.0
    return got


# ------------------------------------------------------------------------------------------------ device harness
GUARD = 0x5A


class Dev:
    """An energy context over the two images (image-based cost, no aggregation: any image size) and the device buffers of the three calls."""

    def __init__(self, lib, imL, imR):
        self.e = api.HipCostVolumeEnergy.naive(imL, imR, windR=0, max_disp=63.0, lib=lib, filter="")
        self.H, self.W = H, W = imL.shape[:2]
        P = H * W
        new = lambda n: api.DeviceBuffer(self.e, max(16, n))
        self.lab, self.img = new(P * 16), new(P * 3)
        self.sides = [(new(P * 3), new(P * 4), new(P)) for _ in range(2)]
        self.out = (new(P * 3), new(P * 4), new(P))
        self.all = [self.lab, self.img, *self.sides[0], *self.sides[1], *self.out]

    def _read(self, bufs, second=np.float32):
        H, W = self.H, self.W
        return bufs[0].download((H, W, 3), np.uint8), bufs[1].download((H, W), second), bufs[2].download((H, W), np.uint8)

    def render(self, lab, src_mode, t, image=None, into=None):
        """-> (bgr, disp, hit) of one call; image None: the context's; into: which buffers (default: the output's)"""
        bufs = into or self.out
        self.lab.upload(lab)
        if image is not None:
            self.img.upload(image)
        for b in bufs:
            b.fill(GUARD)
        self.e.render_view_ptr(src_mode, self.lab.ptr, self.img.ptr if image is not None else None, t, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
        self.e.synchronize()
        return self._read(bufs)

    def blend(self, t, tol, fill, left, right):
        for side, bufs in zip((left, right), self.sides):
            if side is not None:
                for a, b in zip(side, bufs):
                    b.upload(a)
        for b in self.out:
            b.fill(GUARD)
        ptrs = [tuple(b.ptr for b in bufs) if side is not None else None for side, bufs in zip((left, right), self.sides)]
        self.e.blend_views_ptr(t, tol, fill, ptrs[0], ptrs[1], *(b.ptr for b in self.out))
        self.e.synchronize()
        return self._read(self.out)

    def photo(self, lab, mode):
        self.lab.upload(lab)
        self.out[1].fill(GUARD); self.out[2].fill(GUARD)
        self.e.photo_error_ptr(mode, self.lab.ptr, self.out[1].ptr, self.out[2].ptr)
        self.e.synchronize()
        return self.out[1].download((self.H, self.W), F), self.out[2].download((self.H, self.W), np.uint8)

    def untouched(self):
        return all((b.download((b.nbytes,), np.uint8) == GUARD).all() for b in self.out)

    def close(self):
        for b in self.all:
            b.free()
        self.e.close()


def refused(code, fn, *args):
    try:
        fn(*args)
    except api.LesHipError as ex:
        assert f"error {code}" in str(ex), str(ex)
        return True
    raise AssertionError(f"accepted: {args}")


# ------------------------------------------------------------------------------------------------ 2. kernels against the restatement
def case_kernels_bit_for_bit(lib, shape, pops=POPS, ts=TS, kinds=IMAGES):
    """All three kernels on one shape: every population, source view, t and image against the restatement, bit for bit; t = 0 returns the source
    image; at t = 1 hit == 1 exactly where the label warp hits.  -> calls compared"""
    H, W = shape
    n = 0
    for kind in kinds:
        im = images(shape, kind)
        d = Dev(lib, *im)
        try:
            for src_mode in (0, 1):
                for name in pops:
                    lab = labels(name, shape, src_mode)
                    for t in ts:
                        want = render_want(name, shape, src_mode, t, kind)
                        got = d.render(lab, src_mode, t)                                           # the context's image
                        assert same_maps(got, want), f"render {H}x{W} view {src_mode} {name} t={t} {kind}: {first_diff(got, want)}"
                        n += 1
                    got = d.render(lab, src_mode, 0.5, image=im[1 - src_mode])                    # a caller's image (the other view's bytes)
                    want = render_restate(lab, im[1 - src_mode], src_mode, 0.5)
                    assert same_maps(got, want), f"render, own image {H}x{W} view {src_mode} {name}: {first_diff(got, want)}"
                    if 0.0 in ts:
                        bgr, disp, hit = render_want(name, shape, src_mode, 0.0, kind)
                        fin = np.isfinite(disparity(lab))
                        assert same(bgr[fin], im[src_mode][fin]) and (hit[fin] == 1).all() and same(disp[fin], disparity(lab)[fin]), (shape, name)
                    if 1.0 in ts and name in WARPABLE:
                        whit = cv.warp_restate(lab, lab, src_mode)[1]
                        assert same(render_want(name, shape, src_mode, 1.0, kind)[2] == 1, whit == 1), (shape, src_mode, name)
                    got = d.photo(lab, src_mode)
                    want = photo_want(name, shape, src_mode, kind)
                    assert same_maps(got, want), f"photo error {H}x{W} view {src_mode} {name} {kind}: {first_diff(got, want)}"
                    n += 1
            if kind == kinds[0]:
                for name, tol, fill in BLENDS:
                    if name not in pops:
                        continue
                    for t in (0.25, 1.0):
                        left, right = blend_inputs(name, shape, t, kind)
                        for l, r in ((left, right), (left, None), (None, right)):
                            got, want = d.blend(t, tol, fill, l, r), blend_restate(t, tol, fill, l, r, shape)
                            assert same_maps(got, want), f"blend {H}x{W} {name} t={t} tol={tol} fill={fill} sides {l is not None, r is not None}: {first_diff(got, want)}"
                            n += 1
        finally:
            d.close()
    return n


def case_widest_row(lib):
    """The stated limit is served: (2, 8192), 65536 bytes of dynamic LDS in the render and the photo error, 32 columns per scan chunk in the blend."""
    return case_kernels_bit_for_bit(lib, WIDEST, pops=("slanted", "stretch"), ts=(0.5, 1.0), kinds=("random",))


def case_warp_hits(lib, shape=(4, 300)):
    """At t = 1, from the KERNELS' outputs: hit == 1 exactly where les_hip_warp_labels reports hit, on the populations all of whose candidates
    pass the label warp's extra drops."""
    im = images(shape, "random")
    d, w = Dev(lib, *im), cv.Dev(lib, *shape)
    n = 0
    try:
        for src_mode in (0, 1):
            for name in WARPABLE:
                lab = labels(name, shape, src_mode)
                _, _, hit = d.render(lab, src_mode, 1.0)
                _, whit = w.warp(lab, lab, src_mode)
                assert same(hit == 1, whit == 1), (src_mode, name)
                n += int(whit.sum())
    finally:
        d.close(); w.close()
    return n


# ------------------------------------------------------------------------------------------------ 3. independence, refusals
def case_independence(lib, shape=(4, 300)):
    """The outputs of a row do not change when the other rows' inputs change."""
    H, W = shape
    rng = np.random.default_rng(5)
    im = images(shape, "random")
    row = 2
    others = np.arange(H) != row
    im2 = [a.copy() for a in im]
    for a in im2:
        a[others] = rng.integers(0, 256, a[others].shape, dtype=np.uint8)
    d, d2 = Dev(lib, *im), Dev(lib, *im2)
    try:
        for src_mode in (0, 1):
            lab = labels("slanted", shape, src_mode)
            lab2 = lab.copy()
            lab2[others] = labels("collapse", shape, src_mode)[others]
            for a, b in zip(d.render(lab, src_mode, 0.5), d2.render(lab2, src_mode, 0.5)):
                assert same(a[row], b[row]) and not same(a, b)
            for a, b in zip(d.photo(lab, src_mode), d2.photo(lab2, src_mode)):
                assert same(a[row], b[row]) and not same(a, b)
        left, right = blend_inputs("slanted", shape, 0.25)
        l2, r2 = ([a.copy() for a in side] for side in blend_inputs("collapse", shape, 0.25))
        for a, b in zip(l2 + r2, left + right):
            a[row] = b[row]
        for a, b in zip(d.blend(0.25, 1.0, 1, left, right), d.blend(0.25, 1.0, 1, l2, r2)):
            assert same(a[row], b[row]) and not same(a, b)
    finally:
        d.close(); d2.close()


def case_refusals(lib):
    """What the three calls refuse, and that a refused call launches nothing (the outputs keep their guard bytes)."""
    shape = (3, 65)
    im = images(shape, "random")
    lab = labels("slanted", shape, 0)
    ARG, UNSUP = api.LES_HIP_ERR_ARG, api.LES_HIP_ERR_UNSUPPORTED
    d = Dev(lib, *im)
    try:
        d.lab.upload(lab); d.img.upload(im[0])
        for b in d.out + d.sides[0] + d.sides[1]:
            b.fill(GUARD)
        o, (l, r), e = [b.ptr for b in d.out], [tuple(b.ptr for b in s) for s in d.sides], d.e
        for t in (-0.1, 1.5, float("nan")):
            refused(ARG, e.render_view_ptr, 0, d.lab.ptr, None, t, *o)
            refused(ARG, e.blend_views_ptr, t, 1.0, 1, l, r, *o)
        refused(ARG, e.render_view_ptr, 2, d.lab.ptr, None, 0.5, *o)
        refused(ARG, e.render_view_ptr, 0, None, None, 0.5, *o)
        for k in range(3):
            refused(ARG, e.render_view_ptr, 0, d.lab.ptr, None, 0.5, *(None if j == k else p for j, p in enumerate(o)))
            refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, l, r, *(None if j == k else p for j, p in enumerate(o)))
            refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, tuple(None if j == k else p for j, p in enumerate(l)), r, *o)      # a partly given triple
        refused(ARG, e.render_view_ptr, 0, d.lab.ptr, o[0], 0.5, *o)                               # d_out_bgr is the image that is read
        for tol in (-1.0, float("nan")):
            refused(ARG, e.blend_views_ptr, 0.5, tol, 1, l, r, *o)
        refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, None, None, *o)
        refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, l, r, l[0], o[1], o[2])                       # an output that is one of the renders
        refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, l, r, o[0], r[1], o[2])
        refused(ARG, e.blend_views_ptr, 0.5, 1.0, 1, l, r, o[0], o[1], l[2])
        refused(ARG, e.photo_error_ptr, 2, d.lab.ptr, o[1], o[2])
        refused(ARG, e.photo_error_ptr, 0, None, o[1], o[2])
        refused(ARG, e.photo_error_ptr, 0, d.lab.ptr, None, o[2])
        refused(ARG, e.photo_error_ptr, 0, d.lab.ptr, o[1], None)
        e.synchronize()
        assert d.untouched()
    finally:
        d.close()
    # a context created with one image
    H, W = shape
    one = api.HipCostVolumeEnergy(im[0], None, np.zeros((2, H, W), F), None, windR=0, max_disp=1.0, lib=lib, filter="")
    bufs = [api.DeviceBuffer(one, H * W * 16) for _ in range(3)]
    try:
        for b in bufs:
            b.fill(GUARD)
        refused(ARG, one.photo_error_ptr, 0, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
        refused(ARG, one.render_view_ptr, 1, bufs[0].ptr, None, 0.5, bufs[1].ptr, bufs[2].ptr, bufs[2].ptr)      # the view that is missing, and no image given
        one.synchronize()
        assert all((b.download((b.nbytes,), np.uint8) == GUARD).all() for b in bufs)
    finally:
        for b in bufs:
            b.free()
        one.close()
    # one past the width limit
    assert api.WARP_MAX_WIDTH >= 8192
    W = api.WARP_MAX_WIDTH + 1
    z = np.zeros((1, W, 3), np.uint8)
    d = Dev(lib, z, z)
    try:
        d.lab.upload(np.zeros((1, W, 4), F))
        for b in d.out + d.sides[0] + d.sides[1]:
            b.fill(GUARD)
        o, (l, r) = [b.ptr for b in d.out], [tuple(b.ptr for b in s) for s in d.sides]
        refused(UNSUP, d.e.render_view_ptr, 0, d.lab.ptr, None, 0.5, *o)
        refused(UNSUP, d.e.blend_views_ptr, 0.5, 1.0, 1, l, r, *o)
        refused(UNSUP, d.e.photo_error_ptr, 0, d.lab.ptr, o[1], o[2])
        d.e.synchronize()
        assert d.untouched()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 4. the cones crop
def cones_labels(shift=0.0):
    """The fixture's ground truth as the left view's label map (96 x 120): fronto-parallel planes at gt + shift, c = NaN where gt == 0."""
    imL, imR, gt = cc.cones_pair()
    lab = np.zeros(gt.shape + (4,), F)
    lab[..., 2] = np.where(gt > 0, gt + F(shift), QNAN).astype(F)
    return imL, imR, lab


def case_cones(lib):
    """The two claims of the feature on real images, from the DEVICE's outputs (which are the restatement's, bit for bit): the render at t = 1 is
    closer to the real right image than the unwarped left one; the photometric error of the ground truth is below that of shifted maps."""
    from localexpstereo_amd import io as lio
    imL, imR, lab = cones_labels()
    d = Dev(lib, imL, imR)
    out = {}
    try:
        got = d.render(lab, 0, 1.0)
        assert same_maps(got, render_restate(lab, imL, 0, 1.0))
        seen = got[2] != 0
        mad = lambda a, b: float(np.abs(a[seen].astype(np.float64) - b[seen].astype(np.float64)).mean())
        out.update(rendered=int(seen.sum()), render_vs_imR=mad(got[0], imR), imL_vs_imR=mad(imL, imR))
        means = {}
        for shift in (0.0, 1.0, -3.0):
            l = cones_labels(shift)[2]
            ev = d.photo(l, 0)
            assert same_maps(ev, photo_restate(l, imL, imR, 0))
            means[shift] = lio.photometric(*ev)
        out.update(photo_gt=means[0.0], photo_plus1=means[1.0]["mean"], photo_minus3=means[-3.0]["mean"])
        print("cones crop:", out)
        assert seen.sum() > 5000 and out["render_vs_imR"] < out["imL_vs_imR"], out
        assert means[0.0]["mean"] < means[1.0]["mean"] and means[0.0]["mean"] < means[-3.0]["mean"], out
    finally:
        d.close()
    return out


# ------------------------------------------------------------------------------------------------ 5. the driver
TAU = 10.0                    # max_photo_error of the driver case, grey levels (io.photometric's default threshold)


def case_driver(lib, device):
    """stereo.FastGCStereo on the cones crop as crossview_cases pads it (96 x 184, image-based energy; the simulator leg: filter radius 6, the
    MI355X: MidV2's 20): synthesize against the hand-chained calls and the restatement; photo_error; max_photo_error= on the one-view wta()."""
    from localexpstereo_amd import stereo
    data = cv.cones_data()
    imL, imR = data["imL"], data["imR"]
    windR = 6 if lib is not None else 20
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=windR, max_disp=float(data["ndisp"] - 1), lib=lib)
    out = {}
    try:
        params = dict(lambda_=1.0, windR=windR)
        st = stereo.FastGCStereo(e, imL, imR, params, device=device, seed=3)
        gt = np.where(np.isfinite(data["dispGT"]), data["dispGT"], QNAN).astype(F)
        L = np.zeros(gt.shape + (4,), F)
        L[..., 2] = gt
        R = cv.warp_restate(L, np.full(L.shape, QNAN, F), 0)[0]                                    # the same scene as the right view's labels; NaN where nothing landed
        for t in (0.5, 0.25):
            got = st.synthesize({0: L, 1: R}, t=t)
            left, right = e.render_view(L, 0, t, device=device), e.render_view(R, 1, 1.0 - t, device=device)
            hand = tuple(o.cpu().numpy() for o in e.blend_views(t, left, right, tol=1.0, fill=True, device=device))
            assert same_maps(got, hand), t
            want = blend_restate(t, 1.0, 1, render_restate(L, imL, 0, t), render_restate(R, imR, 1, float(F(1) - F(t))), gt.shape)
            assert same_maps(got, want), first_diff(got, want)
            assert got[0].dtype == np.uint8 and got[0].shape == gt.shape + (3,) and got[1].dtype == F and got[2].dtype == np.uint8
            out[f"src_counts_t{t}"] = np.bincount(got[2].ravel(), minlength=5).tolist()
        for m, lab, im in ((0, L, imL), (1, R, imR)):                                               # one map: a one-sided render plus fill
            got = st.synthesize(lab, t=0.5, viewMode=m, fill=(m == 0))
            side = render_restate(lab, im, m, 0.5)
            assert same_maps(got, blend_restate(0.5, 1.0, int(m == 0), side if m == 0 else None, side if m == 1 else None, gt.shape)), m
        try:
            st.synthesize({2: L})
            raise AssertionError("view 2 was accepted")
        except ValueError:
            pass
        ev = st.photo_error(L)
        assert same_maps(ev, photo_restate(L, imL, imR, 0)) and same_maps(st.photo_error(R, viewMode=1), photo_restate(R, imR, imL, 1))
        # max_photo_error: the one-view result by hand
        plain = st.wta((0,))
        assert same(plain[0], plain[1])
        st2 = stereo.FastGCStereo(e, imL, imR, params, device=device, seed=3, max_photo_error=TAU)
        lab, raw = st2.wta((0,))
        assert same(raw, plain[1])
        err, vis = st2.photo_error(raw)
        mask = (vis == 1) & (err > F(TAU))
        assert mask.any() and not mask.all()
        want = e.post_process_host(raw, None, 1.5, st2.p["omega"], fail=(mask, None))[0]
        assert same(lab, want) and not same(lab, raw)
        changed = (np.ascontiguousarray(lab).view(np.uint32) != np.ascontiguousarray(raw).view(np.uint32)).any(-1)
        assert not changed[~mask].any(), "a pixel outside the mask changed"
        assert same(st2.wta((0,), post_process=False)[0], raw)
        out.update(masked=int(mask.sum()), changed=int(changed.sum()))
        for tau in (-1.0, float("nan")):
            try:
                stereo.FastGCStereo(e, imL, imR, {}, device=device, max_photo_error=tau)
                raise AssertionError(f"max_photo_error {tau} was accepted")
            except ValueError:
                pass
        sw = stereo.FastGCStereo(e, imL, imR, {}, device=device, world=2, max_photo_error=TAU)
        for fn in (lambda: sw.synthesize(L), lambda: sw.photo_error(L), lambda: sw.run(1, (0,), 0)):
            try:
                fn()
                raise AssertionError("world = 2 was accepted")
            except NotImplementedError:
                pass
    finally:
        e.close()
    print("driver on the cones crop:", out)
    return out
