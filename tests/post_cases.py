"""Cases of the dual-view post-processing (left-right consistency check, horizontal nearest-valid fill, colour-weighted
median; csrc/les_post.h), shared by the simulator tests (-m "not gpu") and the MI355X tests (-m gpu) in test_post_process.py.
The library (`lib` = the HIP build on the GPU box, the CPU SIMT-simulator build of the same sources in the build container) is
compared bit for bit with the oracle (oracle/les_oracle.cpp) and with an independent numpy restatement of
PMStereoBase::doConsistencyCheck / postProcess (LES/PMStereoBase.h:111-250) and StereoEnergy::computePatchWeight
(LES/StereoEnergy.h:251-257).

The median's order is total: (disparity at p, window scan index), -0 == +0, every NaN after +inf (NaNs tie).

Weights: the restatement's exp (float64, rounded once to float32) and the host's std::exp(float) may differ by one ulp, so the
restatement equals the library except at near-ties (a prefix sum within 1e-6 sumw of the centre); there either neighbour of
the crossing is accepted and the pixels are counted.  Every plane carries a unique tag in its 4th component (Plane::v, never read), so a bit comparison
shows which window pixel was picked.
"""
import numpy as np

from localexpstereo_amd import api, synth
from oracle import oracle as om

F32 = np.float32
NEAR_TIE_RTOL = 1e-6


# ------------------------------------------------------------------------------------------------ restatement
def disparities(lab):
    """computeDisparities: (a x + b y) + c in float32, not fused."""
    H, W = lab.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(F32)
    with np.errstate(all="ignore"):
        return (lab[..., 0] * xs + lab[..., 1] * ys) + lab[..., 2]


def lr_check_ref(dispL, dispR, thr):
    """doConsistencyCheck (LES/PMStereoBase.h:111-144): 255 inconsistent, 128 maps outside the other view, 0 consistent.
    v = (x - ds sign) + 0.5 in float32; outside unless -1e9 < v < 1e9; then int() truncation toward zero."""
    disp = (np.asarray(dispL, F32), np.asarray(dispR, F32))
    H, W = disp[0].shape
    xs = np.arange(W, dtype=F32)[None, :]
    out = []
    for i in range(2):
        ds, sign = disp[i], F32(-1.0 if i else 1.0)
        with np.errstate(all="ignore"):
            v = (xs - ds * sign) + F32(0.5)
            inside = (v > F32(-1e9)) & (v < F32(1e9))
            rx = np.trunc(np.where(inside, v, F32(-1.0))).astype(np.int64)
        ok = inside & (rx >= 0) & (rx < W)
        dsr = np.take_along_axis(disp[1 - i], np.clip(rx, 0, W - 1), axis=1)
        with np.errstate(all="ignore"):
            bad = np.abs(dsr - ds) > F32(thr)
        f = np.full((H, W), 128, np.uint8)
        f[ok] = np.where(bad[ok], 255, 0)
        out.append(f)
    return out[0], out[1]


def dilate3(m):
    """cv::dilate with the default 3x3 kernel; pixels outside the image do not contribute."""
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), m.dtype)
    p[1:-1, 1:-1] = m
    return np.max([p[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)


def fill_ref(lab, failb, fail2):
    """Horizontal nearest-valid fill (:166-201): the first pixels left / right of p outside the dilated mask donate;
    both present -> the left one if zl < zr at p, else the right one; none -> unchanged."""
    H, W = failb.shape
    out = lab.copy()
    idx = np.broadcast_to(np.arange(W), (H, W))
    ok = fail2 != 255
    left = np.maximum.accumulate(np.where(ok, idx, -1), axis=1)
    right = np.minimum.accumulate(np.where(ok, idx, W)[:, ::-1], axis=1)[:, ::-1]
    ys, xs = np.nonzero(failb)
    xl, xr = left[ys, xs], right[ys, xs]
    hl, hr = xl >= 0, xr < W
    pl, pr = lab[ys, np.clip(xl, 0, W - 1)], lab[ys, np.clip(xr, 0, W - 1)]
    fx, fy = xs.astype(F32), ys.astype(F32)
    with np.errstate(all="ignore"):
        zl = (pl[:, 0] * fx + pl[:, 1] * fy) + pl[:, 2]
        zr = (pr[:, 0] * fx + pr[:, 1] * fy) + pr[:, 2]
    use_left = hl & (~hr | (zl < zr))
    take = hl | hr
    new = np.where(use_left[:, None], pl, pr)
    out[ys[take], xs[take]] = new[take]
    stats = dict(no_donor=int((~take).sum()), one_side=int((hl ^ hr).sum()), fill_ties=int((hl & hr & (zl == zr)).sum()))
    return out, stats


def weight_table(omega):
    """computePatchWeight: float32(exp(-float32(|dI|_1) / float32(omega))); |dI|_1 of 8-bit colours is an integer 0 .. 765.  The
    exponential is taken in float64 and rounded once to float32 (numpy's own float32 exp is off by one ulp in about a third of
    the entries)."""
    arg = -np.arange(766, dtype=F32) / F32(omega)
    with np.errstate(under="ignore"):
        return np.exp(arg.astype(np.float64)).astype(F32)


def median_ref(copy, failb, im, windR, omega, chunk_elems=1 << 21):
    """Colour-weighted median (:207-250) over the post-fill copy, vectorised over the failed pixels.  Sort key = (disparity at p
    with -0 == +0 and NaN last, window scan index); sumw and the running sum are sequential float64 sums (np.cumsum); the first
    element whose running sum is > sumw / 2 is picked.  Returns (labels, near) with near = {(y, x): acceptable labels}."""
    H, W = failb.shape
    out = copy.copy()
    wtab = weight_table(omega)
    imi = np.asarray(im).astype(np.int32)
    ys, xs = np.nonzero(failb)
    dy, dx = np.mgrid[-windR:windR + 1, -windR:windR + 1]
    dy, dx = dy.ravel(), dx.ravel()
    A = dy.size
    near = {}
    stats = dict(failed=int(ys.size), nan_windows=0, inf_windows=0, tie_picks=0, median_moved=0)
    step = max(1, chunk_elems // A)
    for s in range(0, ys.size, step):
        py, px = ys[s:s + step], xs[s:s + step]
        n = py.size
        qy, qx = py[:, None] + dy[None], px[:, None] + dx[None]
        valid = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
        ad = np.abs(imi[qy, qx] - imi[py, px][:, None, :]).sum(-1)
        w = np.where(valid, wtab[ad], F32(0)).astype(np.float64)
        L = copy[qy, qx]
        fx, fy = px.astype(F32)[:, None], py.astype(F32)[:, None]
        with np.errstate(all="ignore"):
            z = (L[..., 0] * fx + L[..., 1] * fy) + L[..., 2]
        isn = np.isnan(z)
        zc = np.where(isn, F32(0), z) + F32(0)                  # -0 + 0 = +0
        scan = np.broadcast_to(np.arange(A), (n, A))
        order = np.lexsort((scan, zc, isn, ~valid), axis=-1)
        ws = np.take_along_axis(w, order, 1)
        sumw = np.cumsum(w, axis=1)[:, -1]
        cum = np.cumsum(ws, axis=1)
        center = sumw / 2.0
        above = cum > center[:, None]
        has = above.any(1)
        j = above.argmax(1)
        r = np.arange(n)
        pick = order[r, j]
        sel = L[r, pick]
        out[py[has], px[has]] = sel[has]
        stats["median_moved"] += int((sel[has].view(np.uint32) != copy[py[has], px[has]].view(np.uint32)).any(-1).sum())
        stats["nan_windows"] += int((isn & valid).any(1).sum())
        stats["inf_windows"] += int((np.isinf(z) & valid).any(1).sum())
        # exact disparity tie between distinct labels at the pick (the scan-order tie-break decides)
        Ls = np.take_along_axis(L, order[..., None], 1)
        zs = np.take_along_axis(zc, order, 1)
        ns = np.take_along_axis(isn, order, 1)
        vs = np.take_along_axis(valid, order, 1)
        for dj in (-1, 1):
            k = np.clip(j + dj, 0, A - 1)
            t = has & (k != j) & vs[r, k] & (zs[r, k] == zs[r, j]) & (ns[r, k] == ns[r, j]) & (Ls[r, k].view(np.uint32) != Ls[r, j].view(np.uint32)).any(-1)
            stats["tie_picks"] += int(t.sum())
        # near-ties: every element that would be the crossing if the prefix sums moved by up to tol
        tol = NEAR_TIE_RTOL * sumw
        prev = np.concatenate([np.full((n, 1), -np.inf), cum[:, :-1]], axis=1)
        cand = (cum > (center - tol)[:, None]) & (prev <= (center + tol)[:, None]) & vs
        for i in np.nonzero(cand.sum(1) > 1)[0]:
            near[(int(py[i]), int(px[i]))] = Ls[i][cand[i]]
    stats["near_ties"] = len(near)
    return out, near, stats


def post_process_ref(LL, LR, imL, imR, windR, thr, omega):
    """postProcess (LES/PMStereoBase.h:146-250) on two H x W x 4 float32 label maps: ([outL, outR], [near-ties], stats)."""
    labs = [np.array(LL, F32), np.array(LR, F32)]
    fl, fr = lr_check_ref(disparities(labs[0]), disparities(labs[1]), thr)
    outs, nears, stats = [], [], []
    for lab, f, im in zip(labs, (fl, fr), (imL, imR)):
        failb = np.where(f > 0, 255, 0).astype(np.uint8)
        filled, fst = fill_ref(lab, failb, dilate3(failb))
        out, near, mst = median_ref(filled, failb, im, windR, omega)
        outs.append(out)
        nears.append(near)
        stats.append({**fst, **mst, "fail255": int((f == 255).sum()), "fail128": int((f == 128).sum()),
                      "changed": int((out.view(np.uint32) != lab.view(np.uint32)).any(-1).sum())})
    return outs, nears, stats


def post_process_loop(LL, LR, imL, imR, windR, thr, omega):
    """Literal per-pixel transcription of postProcess (LES/PMStereoBase.h:146-250) for tiny images."""
    labs = [np.array(LL, F32), np.array(LR, F32)]
    H, W = labs[0].shape[:2]

    def getz(l, x, y):
        with np.errstate(all="ignore"):
            return (l[0] * F32(x) + l[1] * F32(y)) + l[2]

    disp = [np.array([[getz(lab[y, x], x, y) for x in range(W)] for y in range(H)], F32) for lab in labs]
    fail = [np.zeros((H, W), np.uint8) for _ in range(2)]
    for i in range(2):
        sign = F32(-1.0 if i else 1.0)
        for y in range(H):
            for x in range(W):
                ds = disp[i][y, x]
                with np.errstate(all="ignore"):
                    v = (F32(x) - ds * sign) + F32(0.5)
                if not (F32(-1e9) < v < F32(1e9)):
                    fail[i][y, x] = 128
                    continue
                rx = int(v)
                if 0 <= rx < W:
                    with np.errstate(all="ignore"):
                        fail[i][y, x] = 255 if abs(disp[1 - i][y, rx] - ds) > F32(thr) else 0
                else:
                    fail[i][y, x] = 128
    for i in range(2):
        fail[i] = np.where(fail[i] > 0, 255, 0).astype(np.uint8)
    fail2 = [np.zeros((H, W), np.uint8) for _ in range(2)]
    for i in range(2):
        for y in range(H):
            for x in range(W):
                fail2[i][y, x] = max(fail[i][yy, xx] for yy in range(max(y - 1, 0), min(y + 2, H)) for xx in range(max(x - 1, 0), min(x + 2, W)))
    for i in range(2):
        for y in range(H):
            for x in range(W):
                if fail[i][y, x] == 0:
                    continue
                pl = pr = None
                xx = x
                while xx >= 0 and fail2[i][y, xx] == 255:
                    xx -= 1
                if xx >= 0:
                    pl = labs[i][y, xx].copy()
                xx = x
                while xx < W and fail2[i][y, xx] == 255:
                    xx += 1
                if xx < W:
                    pr = labs[i][y, xx].copy()
                if pl is None and pr is None:
                    continue
                elif pl is None:
                    labs[i][y, x] = pr
                elif pr is None:
                    labs[i][y, x] = pl
                elif getz(pl, x, y) < getz(pr, x, y):
                    labs[i][y, x] = pl
                else:
                    labs[i][y, x] = pr
    ims = (np.asarray(imL).astype(np.int64), np.asarray(imR).astype(np.int64))
    for i in range(2):
        copy = labs[i].copy()
        for y in range(H):
            for x in range(W):
                if fail[i][y, x] == 0:
                    continue
                median = []
                sumw = 0.0
                for yy in range(max(y - windR, 0), min(y + windR + 1, H)):
                    for xx in range(max(x - windR, 0), min(x + windR + 1, W)):
                        absdiff = F32(abs(ims[i][y, x] - ims[i][yy, xx]).sum())
                        with np.errstate(under="ignore"):
                            w = F32(np.exp(np.float64(-absdiff / F32(omega))))
                        sumw += float(w)
                        z = getz(copy[yy, xx], x, y)
                        median.append((copy[yy, xx], float(w), (1, 0.0) if np.isnan(z) else (0, float(z) + 0.0)))
                median.sort(key=lambda t: t[2])                  # stable: equal keys keep the scan order
                center = sumw / 2.0
                sumw = 0.0
                for l, w, _ in median:
                    sumw += w
                    if sumw > center:
                        labs[i][y, x] = l
                        break
    return labs


# ------------------------------------------------------------------------------------------------ scenes
def tag(LL, LR):
    """A unique tag per label in Plane::v (1 .. 2 H W, exact in float32)."""
    H, W = LL.shape[:2]
    LL[..., 3] = 1 + np.arange(H * W, dtype=F32).reshape(H, W)
    LR[..., 3] = 1 + H * W + np.arange(H * W, dtype=F32).reshape(H, W)
    return LL, LR


def image(H, W, seed, colours=0):
    """Guide image; colours > 0: only that many distinct colours (repeated colours: exact weight ties)."""
    im = synth.make_guide(H, W, seed)
    if colours:
        rng = np.random.default_rng(seed)
        pal = rng.integers(0, 256, (colours, 3)).astype(np.uint8)
        im = pal[(im[..., 1].astype(np.int64) * colours) // 256]
    return np.ascontiguousarray(im)


def scene_surfaces(H, W, seed, D=16):
    """The three-surface scene of case_post_process: consistent surfaces in both views, blocks of wrong labels, isolated
    outliers, huge disparities in the first columns (outside) and a NaN plane."""
    rng = np.random.default_rng(seed)
    xs = np.mgrid[0:H, 0:W][1].astype(F32)

    def view(sign):
        lab = np.zeros((H, W, 4), F32)
        for k, (a, b, c) in enumerate([(0.01, 0.0, 4.0), (0.0, 0.02, 8.0), (-0.01, 0.01, 14.0)]):
            band = (xs + (0 if sign > 0 else c)) // (W / 3.0)
            m = band == k if k < 2 else band >= 2
            lab[m] = (a, b, c + (a * c if sign < 0 else 0.0), 0.0)
        return lab

    LL, LR = view(+1.0), view(-1.0)
    for lab in (LL, LR):
        for _ in range(max(1, H * W // 1500)):
            x0, y0 = int(rng.integers(0, max(1, W - 4))), int(rng.integers(0, max(1, H - 4)))
            w, h = int(rng.integers(1, 14)), int(rng.integers(1, 10))
            lab[y0:y0 + h, x0:x0 + w] = (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0, D), 0.0)
        noisy = rng.random((H, W)) < 0.02
        lab[noisy, 2] += rng.uniform(3, 9, int(noisy.sum())).astype(F32)
    LL[:, :min(3, W)] = (0.0, 0.0, 1e12, 0.0)
    LL[H // 2, W // 2] = (np.nan, 0.0, 1.0, 0.0)
    return tag(LL, LR)


def scene_corners(H, W):
    """Fronto-parallel disparity 0 in both views except wrong labels in the four corners (the median's window clipped on two
    sides, the fill with a donor on one side only)."""
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    for y in (0, H - 1):
        for x in (0, W - 1):
            LL[y, x] = (0.0, 0.0, 7.0 if x else -7.0, 0.0)
            LR[y, x] = (0.0, 0.0, 5.0 if x else -5.0, 0.0)
    return tag(LL, LR)


def scene_crossing(H, W, seed):
    """Exact disparity ties between distinct planes: five slopes through (x0, y, 2) for every crossing column x0, each pixel labelled
    by a random plane of its nearest crossing column; the right view is consistent only in a band, so the crossing columns fail and
    the median sorts several planes of equal disparity at p."""
    rng = np.random.default_rng(seed)
    slopes = np.array([-0.5, -0.25, 0.0, 0.25, 0.5], F32)
    cols = np.arange(2, W, 6)
    LL = np.zeros((H, W, 4), F32)
    xs = np.arange(W)
    near = cols[np.abs(xs[:, None] - cols[None]).argmin(1)]
    k = rng.integers(0, slopes.size, (H, W))
    a = slopes[k]
    LL[..., 0] = a
    LL[..., 2] = F32(2.0) - a * near[None, :].astype(F32)
    LR = np.zeros((H, W, 4), F32)
    LR[..., 2] = 2.0
    LR[:, ::3, 2] = 9.0
    return tag(LL, LR)


def scene_signed_zero(H=12, W=16):
    """Uniform image; even columns hold planes of disparity -0, odd columns +0; one inconsistent pixel per view."""
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    for lab in (LL, LR):
        lab[:, 0::2, :3] = -0.0
    LL[H // 2, W // 2, :3] = (0.0, 0.0, 5.0)
    LR[H // 2 - 1, W // 2 - 1, :3] = (0.0, 0.0, 5.0)
    return tag(LL, LR)


def scene_nonfinite(H=14, W=20, nan_sign=1.0, extra=False):
    """A row of NaN labels (no donor: the whole row fails, NaN reaches the windows of the median); extra: also a row of
    alternating +-NaN, +-inf and 1e12 planes, a row whose failures touch the left border and one touching the right border (a
    donor on one side only), and a run between two donors of equal disparity at p (fill tie zl == zr)."""
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    LL[..., 2] = LR[..., 2] = 1.0
    LL[H // 2, :, 2] = np.copysign(np.nan, nan_sign)
    if extra:
        vals = [np.nan, -np.nan, np.inf, -np.inf, 1e12, -1e12]
        LR[2, :, 2] = [np.copysign(np.nan, 1.0) if i % 6 == 0 else np.copysign(np.nan, -1.0) if i % 6 == 1 else vals[i % 6] for i in range(W)]
        LL[H - 3, :4, 2] = 6.0                                   # left border: right donor only
        LL[H - 2, W - 4:, 2] = 6.0                               # right border: left donor only
        LR[H - 4, W // 2 - 2:W // 2 + 2, 2] = 6.0                # both donors are the plane z = 1 (distinct tags): zl == zr
        LR[H - 4, W // 2 - 4, :3] = (0.0, 0.0, 1.0)
    return tag(LL, LR)


def scene_random_nonfinite(H, W, seed):
    """Random fronto-parallel labels with NaN of both signs, +-inf and huge values sprinkled in both views."""
    rng = np.random.default_rng(seed)
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    LL[..., 2] = 3.0
    LR[..., 2] = 3.0
    for lab in (LL, LR):
        m = rng.random((H, W))
        lab[m < 0.1, 2] = rng.uniform(-5, 20, int((m < 0.1).sum()))
        lab[(m >= 0.1) & (m < 0.13), 2] = np.nan
        lab[(m >= 0.13) & (m < 0.16), 2] = -np.nan
        lab[(m >= 0.16) & (m < 0.18), 2] = np.inf
        lab[(m >= 0.18) & (m < 0.2), 2] = -np.inf
    return tag(LL, LR)


# ------------------------------------------------------------------------------------------------ contexts and cases
def context(lib, imL, imR, windR, filter=""):
    """A context of any filter: post-processing reads only windR and the two images."""
    H, W = imL.shape[:2]
    vol = np.zeros((2, H, W), F32)
    eps = {"GF": 1e-4, "BF": 10.0, "": 1.0}[filter]
    return api.HipCostVolumeEnergy(imL, imR, vol, vol, windR=windR, eps=eps, th_col=0.5, lib=lib, filter=filter)


def compare_restatement(got, ref, near, name):
    """got == ref bit for bit, except at near-ties where got must be one of the acceptable labels.  Returns the number of
    near-tie pixels at which the two picks differ."""
    gb, rb = got.view(np.uint32), ref.view(np.uint32)
    diff = np.nonzero((gb != rb).any(-1))
    moved = 0
    for y, x in zip(*diff):
        acc = near.get((int(y), int(x)))
        assert acc is not None, f"view {name}: ({y}, {x}) differs from the restatement: got {got[y, x]}, want {ref[y, x]}"
        assert (acc.view(np.uint32) == gb[y, x]).all(-1).any(), f"view {name}: ({y}, {x}) is a near-tie, but {got[y, x]} is no neighbour of the crossing"
        moved += 1
    return moved


def case_post_process(lib, scene, imL, imR, windR, thr=1.5, omega=10.0, filter="", repeat=False):
    """les_hip_post_process == oracle bit for bit, == restatement except at near-ties; the consistency masks of
    les_hip_consistency_check == lr_check_ref.  Returns the restatement's statistics per view (plus the near-ties met)."""
    LL, LR = scene
    e = context(lib, imL, imR, windR, filter)
    try:
        got = e.post_process_host(LL, LR, threshold=thr, omega=omega)
        if repeat:
            again = e.post_process_host(LL, LR, threshold=thr, omega=omega)
            for g, a in zip(got, again):
                assert np.array_equal(g.view(np.uint32), a.view(np.uint32)), "a repeated post-processing differs"
        masks = consistency_masks(e, LL, LR, thr)
    finally:
        e.close()
    ora = om.post_process(LL, LR, imL, imR, windR=windR, threshold=thr, omega=omega)
    ref, nears, stats = post_process_ref(LL, LR, imL, imR, windR, thr, omega)
    fl, fr = lr_check_ref(disparities(LL), disparities(LR), thr)
    assert np.array_equal(masks[0], fl) and np.array_equal(masks[1], fr), "consistency masks differ from the restatement"
    for v, name in enumerate("LR"):
        same = (got[v].view(np.uint32) == ora[v].view(np.uint32)).all(-1)
        assert same.all(), f"view {name}: {int((~same).sum())} pixels differ from the oracle (windR {windR}, omega {omega}, thr {thr})"
        stats[v]["near_tie_moves"] = compare_restatement(got[v], ref[v], nears[v], name)
        assert stats[v]["near_tie_moves"] <= 0.001 * max(stats[v]["failed"], 1), stats[v]
    return stats


def consistency_masks(e, LL, LR, thr):
    H, W = e.H, e.W
    bufs = [api.DeviceBuffer(e, H * W * 16) for _ in range(2)] + [api.DeviceBuffer(e, H * W) for _ in range(2)]
    try:
        bufs[0].upload(np.ascontiguousarray(LL, F32))
        bufs[1].upload(np.ascontiguousarray(LR, F32))
        e.consistency_check(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, thr)
        return bufs[2].download((H, W), np.uint8), bufs[3].download((H, W), np.uint8)
    finally:
        for b in bufs:
            b.free()


def check_edges(H=6, W=24):
    """Disparity maps (fronto-parallel planes: disparity = c exactly) for the consistency check's edges, with the expected
    mask value of each probed pixel: (LL, LR, [(view, y, x, thr, expected)])."""
    dl, dr = np.full((H, W), 2.0, F32), np.full((H, W), 2.0, F32)
    probes = []
    # view L, row 0/1: |dsr - ds| exactly at the threshold (consistent) and one ulp above (inconsistent), thresholds 1.5 and 1.0
    for y, thr in ((0, 1.5), (1, 1.0)):
        dl[y, 10], dr[y, 8] = 2.0, F32(2.0 + thr)
        dl[y, 14], dr[y, 12] = 2.0, np.nextafter(F32(2.0 + thr), F32(np.inf))
        probes += [(0, y, 10, thr, 0), (0, y, 14, thr, 255)]
    # view R mirrors it: v = x + ds + 0.5
    for y, thr in ((0, 1.5), (1, 1.0)):
        dr[y, 16], dl[y, 18] = 2.0, F32(2.0 + thr)
        dr[y, 4], dl[y, 6] = 2.0, np.nextafter(F32(2.0 + thr), F32(np.inf))
        probes += [(1, y, 16, thr, 0), (1, y, 4, thr, 255)]
    # view L row 2: v in (-1, 0) truncates to 0 (inside); v = -1 is outside; v = W - 0.5 -> W - 1 (inside); v = W is outside
    dl[2, 0], dr[2, 0] = 0.9, 0.9
    dl[2, 1] = 2.5
    dl[2, W - 1] = 0.0
    dl[2, W - 2] = -1.5
    dr[2, W - 1] = 0.0
    probes += [(0, 2, 0, 1.5, 0), (0, 2, 1, 1.5, 128), (0, 2, W - 1, 1.5, 0), (0, 2, W - 2, 1.5, 128)]
    # row 3, both views: NaN, +-inf and +-1e12 disparities are outside
    for x, d in zip(range(3, 15, 2), (np.nan, -np.nan, np.inf, -np.inf, 1e12, -1e12)):
        dl[3, x] = d
        dr[3, x + 1] = d
        probes += [(0, 3, x, 1.5, 128), (1, 3, x + 1, 1.5, 128)]
    # row 4: the other view's disparity at rx is NaN / inf: |dsr - ds| > thr is false for NaN (consistent), true for inf
    dr[4, 8], dr[4, 10] = np.nan, np.inf
    probes += [(0, 4, 10, 1.5, 0), (0, 4, 12, 1.5, 255)]
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    LL[..., 2], LR[..., 2] = dl, dr
    return tag(LL, LR) + (probes,)


def case_consistency_edges(lib):
    """les_hip_consistency_check == lr_check_ref bit for bit at the edges of check_edges, both views, thresholds 1.5 and 1.0;
    every probed pixel has the value the reference's arithmetic gives it."""
    LL, LR, probes = check_edges()
    H, W = LL.shape[:2]
    assert np.array_equal(disparities(LL), LL[..., 2], equal_nan=True)
    im = image(H, W, 3)
    e = context(lib, im, im, 2)
    try:
        for thr in (1.5, 1.0):
            got = consistency_masks(e, LL, LR, thr)
            ref = lr_check_ref(disparities(LL), disparities(LR), thr)
            ora = om.consistency_check(disparities(LL), disparities(LR), thr)
            for v in range(2):
                assert np.array_equal(got[v], ref[v]), f"view {v}, thr {thr}: {np.argwhere(got[v] != ref[v])[:8]}"
                assert np.array_equal(got[v], ora[v])
            for v, y, x, t, want in probes:
                if t == thr:
                    assert ref[v][y, x] == want, (v, y, x, thr, ref[v][y, x], want)
    finally:
        e.close()
    return len(probes)
