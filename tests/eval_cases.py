"""Cases of tests/test_device_eval.py: the device-side Evaluator (csrc/les_eval.h: les_hip_evaluate, les_hip_batch_region_energy) on the CPU
simulator build and on the MI355X.

References, none of them the code under test: a numpy float32 restatement of the per-pixel terms (below, itself checked against a literal
per-pixel Python loop), the host graph-cut context (gc.GraphCut.data_cost / smoothness_cost, les_gc_expansion_moves(check=True)), io.Evaluator.

Tolerance of a sum (derived, not measured): N finite non-negative f32 terms added in fp64 in any order differ from the exact sum S by at most
(N - 1) 2^-53 S to first order.  sum_bound(N, S) = N 2^-52 S is used between the device and math.fsum of the terms, twice that between the
device and the host (each is within the bound of the exact sum)."""
import contextlib
import math
import os

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import gc as lgc
from localexpstereo_amd import io as lio

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
FORWARD = ((+1, 0), (0, +1), (-1, +1), (+1, +1))       # GE, EG, LG, GG: the order the host sums them in
PW = dict(lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01)


def sum_bound(n_terms, s):
    return n_terms * 2.0 ** -52 * abs(s)


# ------------------------------------------------------------------------------------------------ restatement
def coeff_table(omega, epsilon):
    """initSmoothnessCoeff (LES/StereoEnergy.h:131-163) as the library tabulates it: max(epsilon, expf(-(float)k / omega)), k = |dI|_1 of 8-bit
    colours.  exp is evaluated in double on the f32 quotient and rounded once to f32 (case_table_matches_host checks every entry against the
    host context's own table)."""
    return np.array([max(F(epsilon), F(math.exp(float(F(-F(k) / F(omega)))))) for k in range(766)], F)


def absdiff(img):
    """|dI|_1 towards the four forward neighbours: dict direction -> H x W ints (0 where the pair leaves the image) and the inside masks."""
    H, W = img.shape[:2]
    im = img.astype(np.int64)
    ad, inside = {}, {}
    for dx, dy in FORWARD:
        a = np.zeros((H, W), np.int64)
        m = np.zeros((H, W), bool)
        ys, xs = np.mgrid[0:H, 0:W]
        ok = (xs + dx >= 0) & (xs + dx < W) & (ys + dy < H)
        a[ok] = np.abs(im[ys[ok], xs[ok]] - im[ys[ok] + dy, xs[ok] + dx]).sum(-1)
        m[ok] = True
        ad[(dx, dy)], inside[(dx, dy)] = a, m
    return ad, inside


def getz(lab, x, y):
    """Plane::GetZ in f32: (a x + b y) + c, every operation rounded to f32 (no fused multiply-add)."""
    return (lab[..., 0] * x.astype(F) + lab[..., 1] * y.astype(F)) + lab[..., 2]


def pair_terms(img, labels, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01):
    """computeSmoothnessTerm (LES/StereoEnergy.h:225-230) of every forward pair inside the image, f32: dict direction -> (terms H x W, inside mask).
    term = coeff * min(|z_p(p) - z_q(p)| + |z_p(q) - z_q(q)|, th) * lambda with std::min(d, th) = (th < d) ? th : d (a NaN d stays NaN)."""
    labels = np.asarray(labels, F)
    H, W = labels.shape[:2]
    tab = coeff_table(omega, epsilon)
    ad, inside = absdiff(img)
    ys, xs = np.mgrid[0:H, 0:W]
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for dx, dy in FORWARD:
            m = inside[(dx, dy)]
            yq, xq = np.where(m, ys + dy, ys), np.where(m, xs + dx, xs)
            lp, lq = labels, labels[yq, xq]
            d = np.abs(getz(lp, xs, ys) - getz(lq, xs, ys)) + np.abs(getz(lp, xq, yq) - getz(lq, xq, yq))
            d = d.astype(F)
            mn = np.where(F(th_smooth) < d, F(th_smooth), d).astype(F)
            t = ((tab[ad[(dx, dy)]] * mn).astype(F) * F(lambda_)).astype(F)
            out[(dx, dy)] = (np.where(m, t, F(0)), m)
    return out


def pair_terms_loop(img, labels, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01):
    """The same, as a literal per-pixel loop over numpy f32 scalars (small maps only)."""
    H, W = labels.shape[:2]
    tab = coeff_table(omega, epsilon)
    out = {d: (np.zeros((H, W), F), np.zeros((H, W), bool)) for d in FORWARD}

    def z(l, x, y):
        return F(F(F(l[0] * F(x)) + F(l[1] * F(y))) + l[2])
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(H):
            for x in range(W):
                for dx, dy in FORWARD:
                    xq, yq = x + dx, y + dy
                    if xq < 0 or xq >= W or yq >= H:
                        continue
                    k = sum(abs(int(img[y, x, c]) - int(img[yq, xq, c])) for c in range(3))
                    lp, lq = labels[y, x], labels[yq, xq]
                    d = F(abs(F(z(lp, x, y) - z(lq, x, y))) + abs(F(z(lp, xq, yq) - z(lq, xq, yq))))
                    mn = F(th_smooth) if F(th_smooth) < d else d
                    out[(dx, dy)][0][y, x] = F(F(tab[k] * mn) * F(lambda_))
                    out[(dx, dy)][1][y, x] = True
    return out


def smooth_terms(img, labels, **pw):
    """All forward pair terms inside the image as one flat f32 array."""
    t = pair_terms(img, labels, **pw)
    return np.concatenate([t[d][0][t[d][1]] for d in FORWARD])


def disparities(labels):
    H, W = labels.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    return getz(np.asarray(labels, F), xs, ys).astype(F)


def quantize(d, precision):
    """Evaluator::quantize (LES/Evaluator.h:106-111) as stereo.FastGCStereo._row does it."""
    if precision > 0:
        with np.errstate(invalid="ignore"):
            return (np.rint(d / F(precision)) * F(precision)).astype(F)
    return d


def fsum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return float("nan") if np.isnan(a).any() else math.fsum(a.tolist())


def bits(x):
    return np.float64(x).view(np.uint64)


def same_float(a, b):
    return bits(a) == bits(b) or (a != a and b != b)


# ------------------------------------------------------------------------------------------------ fixtures
def random_images(H, W, seed, smooth_colours=False):
    rng = np.random.default_rng(seed)
    if smooth_colours:          # neighbours a few grey levels apart: exp(-|dI| / omega) well above epsilon
        base = rng.integers(100, 110, (H, W, 3))
        return base.astype(np.uint8), (base + rng.integers(0, 3, (H, W, 3))).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def cones_images():
    """The cones crop as case_stereo_driver pads it (both views 96 x 184), its ground truth and mask."""
    z = np.load(os.path.join(GOLDEN, "cones_crop.npz"))
    imL, imRw, gt = z["imL"], np.ascontiguousarray(z["imR_wide"]), z["gt"]
    imLw = np.ascontiguousarray(np.concatenate([np.repeat(imL[:, :1], 64, axis=1), imL], axis=1))
    gtw = np.concatenate([np.zeros((gt.shape[0], 64), F), gt], axis=1).astype(F)
    return imLw, imRw, gtw


def cell_labels(H, W, seed, cell=5, maxd=40.0, slant=0.3):
    """Random slanted planes, one per cell x cell block."""
    rng = np.random.default_rng(seed)
    hb, wb = -(-H // cell), -(-W // cell)
    pl = np.stack([rng.uniform(-slant, slant, (hb, wb)), rng.uniform(-slant, slant, (hb, wb)), rng.uniform(0, maxd, (hb, wb)), np.zeros((hb, wb))], -1)
    lab = np.repeat(np.repeat(pl, cell, 0), cell, 1)[:H, :W].astype(F)
    # the plane passes through its drawn disparity at the block's centre
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (xs // cell) * cell + cell // 2, (ys // cell) * cell + cell // 2
    lab[..., 2] = (lab[..., 2] - lab[..., 0] * cx - lab[..., 1] * cy).astype(F)
    return np.ascontiguousarray(lab)


def sentinel_costs(H, W, seed, frac=0.03):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 0.5, (H, W)).astype(F)
    c[rng.random((H, W)) < frac] = F(1e6)
    return c


class Dev:
    """An energy context (image-based cost, no aggregation: any image size) with device label / cost maps."""

    def __init__(self, lib, imL, imR, max_disp=63.0):
        self.e = api.HipCostVolumeEnergy.naive(imL, imR, windR=0, max_disp=max_disp, lib=lib, filter="")
        self.imL, self.imR = np.ascontiguousarray(imL), np.ascontiguousarray(imR)
        self.H, self.W = self.e.H, self.e.W
        self.labels = api.DeviceBuffer(self.e, self.H * self.W * 16)
        self.cost = api.DeviceBuffer(self.e, self.H * self.W * 4)

    def img(self, mode):
        return self.imL if mode == 0 else self.imR

    def upload(self, labels, cost):
        self.labels.upload(np.ascontiguousarray(labels, F))
        self.cost.upload(np.ascontiguousarray(cost, F))

    def evaluate_once(self, labels, cost, mode=0, pw=PW, **ev_args):
        self.upload(labels, cost)
        ev = api.DeviceEvaluator(self.e, max_rows=1, **ev_args)
        try:
            ev.evaluate(self.labels.ptr, self.cost.ptr, mode=mode, index=7, **pw)
            return ev.rows()[0]
        finally:
            ev.close()

    def close(self):
        self.labels.free(); self.cost.free()
        self.e.close()


def host_energy(imL, imR, labels, cost, mode, pw=PW):
    g = lgc.GraphCut(imL, imR, **pw)
    try:
        g.labels[mode][...] = labels
        g.costs[mode][...] = cost
        return g.data_cost(mode), g.smoothness_cost(mode)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ the restatement itself
def case_restatement_matches_loop():
    for (H, W), seed in (((1, 2), 1), ((2, 1), 2), ((2, 2), 3), ((5, 7), 4), ((6, 4), 5)):
        imL, _ = random_images(H, W, seed, smooth_colours=seed % 2 == 0)
        lab = cell_labels(H, W, seed, cell=2, maxd=6.0, slant=0.4 if seed % 2 else 0.02)
        for pw in (PW, dict(lambda_=0.7, th_smooth=0.25, omega=4.0, epsilon=0.2)):
            a, b = pair_terms(imL, lab, **pw), pair_terms_loop(imL, lab, **pw)
            for d in FORWARD:
                assert np.array_equal(a[d][1], b[d][1])
                assert np.array_equal(a[d][0].view(np.uint32), b[d][0].view(np.uint32)), (H, W, d)
    # the pair counts: 1 x 2 and 2 x 1 hold one pair, 2 x 2 six, every direction among them
    assert len(smooth_terms(np.zeros((1, 2, 3), np.uint8), np.zeros((1, 2, 4), F))) == 1
    assert len(smooth_terms(np.zeros((2, 1, 3), np.uint8), np.zeros((2, 1, 4), F))) == 1
    t = pair_terms(np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 4), F))
    assert [int(t[d][1].sum()) for d in FORWARD] == [2, 2, 1, 1]


def case_table_matches_host():
    """Every entry of the restated coefficient table against the host context's own (host/StereoEnergy.h: std::exp in float): a 1 x 2 image whose
    two pixels are k grey levels apart, labels 0.25 apart at both pixels (d = 0.5, below th 1), lambda 1: the one term is table[k] / 2, exactly."""
    for omega, epsilon in ((10.0, 0.01), (4.0, 0.2)):
        tab = coeff_table(omega, epsilon)
        lab = np.zeros((1, 2, 4), F)
        lab[0, 1, 2] = 0.25
        for k in range(766):
            im = np.zeros((1, 2, 3), np.uint8)
            im[0, 1] = (min(k, 255), min(max(k - 255, 0), 255), max(k - 510, 0))
            _, s = host_energy(im, None, lab, np.zeros((1, 2), F), 0, dict(lambda_=1.0, th_smooth=1.0, omega=omega, epsilon=epsilon))
            assert s == float(tab[k]) * 0.5, (omega, epsilon, k, s, tab[k])


# ------------------------------------------------------------------------------------------------ 1. terms, bit for bit
def case_terms_bit_for_bit(lib):
    checked = dict(trunc=0, no_trunc=0, floor=0, no_floor=0)
    for H, W in ((1, 2), (2, 1), (2, 2)):
        for seed in range(8):
            big_colour, trunc = bool(seed & 1), bool(seed & 2)
            imL, imR = random_images(H, W, 100 + seed, smooth_colours=not big_colour)
            lab = cell_labels(H, W, 200 + seed, cell=1, maxd=30.0 if trunc else 0.4, slant=0.3 if trunc else 0.05)
            if H * W == 4 and not trunc:
                lab[..., :2] = 0            # fronto-parallel planes with dyadic offsets: the six terms stay within a few binades of each other
                lab[..., 2] = np.array([[0.25, 0.5], [0.75, 0.125]], F)
            cost = np.random.default_rng(seed).uniform(0, 1, (H, W)).astype(F)
            d = Dev(lib, imL, imR)
            try:
                for mode in (0, 1):
                    pw = dict(PW, lambda_=1.0 if seed < 4 else 0.7)
                    terms = smooth_terms(d.img(mode), lab, **pw)
                    assert len(terms) == (1 if H * W == 2 else 6)
                    nz = terms[terms != 0].astype(np.float64)
                    if len(nz) > 1:          # the fp64 sum of six f32 terms is exact in any order while their exponents are at most 26 apart
                        assert np.log2(nz.max() / nz.min()) <= 26, terms
                    row = d.evaluate_once(lab, cost, mode, pw)
                    want = fsum(terms)
                    assert same_float(row["smooth"], want), (H, W, seed, mode, row["smooth"], want)
                    if H * W == 2:
                        assert row["smooth"] == float(terms[0])
                    assert same_float(row["data"], fsum(cost)) and row["index"] == 7 and row["mode"] == mode
                    hd, hs = host_energy(imL, imR, lab, cost, mode, pw)
                    assert same_float(row["smooth"], hs) and same_float(row["data"], hd)
                    # which branches this case took
                    ad, inside = absdiff(d.img(mode))
                    tab = coeff_table(pw["omega"], pw["epsilon"])
                    ks = np.concatenate([ad[k][inside[k]] for k in FORWARD])
                    checked["floor" if (tab[ks] == F(pw["epsilon"])).any() else "no_floor"] += 1
                    full = pair_terms(d.img(mode), lab, **dict(pw, th_smooth=1e30))
                    untr = np.concatenate([full[k][0][full[k][1]] for k in FORWARD])
                    checked["trunc" if (untr != terms).any() else "no_trunc"] += 1
            finally:
                d.close()
    assert all(v > 0 for v in checked.values()), checked      # truncation at th_smooth active and not, the epsilon floor active and not
    return checked


# ------------------------------------------------------------------------------------------------ 2. sums
def sum_scenes():
    yield "37x53", random_images(37, 53, 11) + (None,)
    yield "64x64", random_images(64, 64, 12, smooth_colours=True) + (None,)
    yield "cones", cones_images()


def case_sums(lib):
    worst = 0.0
    for name, (imL, imR, _) in sum_scenes():
        H, W = imL.shape[:2]
        d = Dev(lib, imL, imR)
        try:
            for mode in (0, 1):
                lab = cell_labels(H, W, 31 + mode)
                cost = sentinel_costs(H, W, 41 + mode)
                row = d.evaluate_once(lab, cost, mode)
                terms = smooth_terms(d.img(mode), lab, **PW)
                n_data, n_smooth = H * W, len(terms)
                assert n_smooth <= 4 * H * W and n_smooth == 4 * H * W - 3 * W - 3 * H + 2       # image borders contribute nothing
                S_d, S_s = fsum(cost), fsum(terms)
                assert abs(row["data"] - S_d) <= sum_bound(n_data, S_d), (name, mode, row["data"], S_d)
                assert abs(row["smooth"] - S_s) <= sum_bound(n_smooth, S_s), (name, mode, row["smooth"], S_s)
                hd, hs = host_energy(imL, imR, lab, cost, mode)
                assert abs(row["data"] - hd) <= 2 * sum_bound(n_data, S_d) and abs(row["smooth"] - hs) <= 2 * sum_bound(n_smooth, S_s)
                assert row["energy"] == row["data"] + row["smooth"]
                worst = max(worst, abs(row["smooth"] - S_s) / S_s)
                assert (cost == F(1e6)).any() and S_s > 0
        finally:
            d.close()
    return worst


def case_nonfinite(lib):
    """NaN and inf planes / costs: the same rows are NaN as on the host."""
    imL, imR = random_images(37, 53, 13)
    H, W = 37, 53
    d = Dev(lib, imL, imR)
    try:
        base_lab, base_cost = cell_labels(H, W, 5), sentinel_costs(H, W, 6)
        variants = []
        for what in ("nan_plane", "inf_plane", "inf_offset_pair", "nan_cost", "inf_cost"):
            lab, cost = base_lab.copy(), base_cost.copy()
            if what == "nan_plane":
                lab[10, 20, 0] = np.nan
            if what == "inf_plane":
                lab[0, 0, 2] = np.inf               # |inf - finite| = inf: truncated to th, the sum stays finite
            if what == "inf_offset_pair":
                lab[5, 5, 2] = lab[5, 6, 2] = np.inf    # inf - inf = NaN
            if what == "nan_cost":
                cost[36, 52] = np.nan
            if what == "inf_cost":
                cost[3, 3] = np.inf
            variants.append((what, lab, cost))
        for what, lab, cost in variants:
            for mode in (0, 1):
                row = d.evaluate_once(lab, cost, mode)
                hd, hs = host_energy(imL, imR, lab, cost, mode)
                assert (row["data"] != row["data"]) == (hd != hd) and (row["smooth"] != row["smooth"]) == (hs != hs), (what, row, hd, hs)
                assert np.isinf(row["data"]) == np.isinf(hd) and np.isinf(row["smooth"]) == np.isinf(hs), (what, row, hd, hs)
                s_terms = smooth_terms(d.img(mode), lab, **PW)
                assert (row["smooth"] != row["smooth"]) == bool(np.isnan(s_terms).any())
                if what in ("nan_plane", "inf_offset_pair"):
                    assert row["smooth"] != row["smooth"] and row["data"] == row["data"]
                if what == "nan_cost":
                    assert row["data"] != row["data"] and row["smooth"] == row["smooth"]
                if what == "inf_plane":
                    assert np.isfinite(row["smooth"])
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 3. rates
def case_rates(lib):
    imL, imR, gt = cones_images()
    H, W = gt.shape
    rng = np.random.default_rng(3)
    nonocc = rng.random((H, W)) < 0.8
    thr = 0.5
    d = Dev(lib, imL, imR)
    seen = dict(boundary=0, ties=0)
    try:
        for precision in (-1.0, 0.25):
            gt2 = gt.copy()
            gt2[5, 70:90] = 0.0                     # invalid: 0
            gt2[6, 70:90] = np.inf                  # invalid: not finite
            gt2[7, 70:75] = -3.0
            # fronto-parallel labels: the disparity is the offset, exactly
            lab = np.zeros((H, W, 4), F)
            disp = (gt2 + rng.uniform(-1.0, 1.0, (H, W)).astype(F)).astype(F)
            disp[~np.isfinite(disp)] = 7.0
            # exactly at |d - gt| == threshold (quarter-pel ground truth: gt +- 0.5 is exact in f32)
            disp[20, 64:124] = gt2[20, 64:124] + F(thr)
            disp[21, 64:124] = gt2[21, 64:124] - F(thr)
            disp[22, 64:124] = np.nextafter(gt2[22, 64:124] + F(thr), F(np.inf))        # one ulp outside
            # quantisation ties: d / precision at k + 0.5 (round-half-even)
            disp[30, 64:124] = (np.arange(60, dtype=F) + F(0.5)) * F(0.25)
            disp[31, 64:124] = -(np.arange(60, dtype=F) + F(0.5)) * F(0.25)
            disp[40, 100:110] = np.nan
            lab[..., 2] = disp
            # a slanted block as well (GetZ with a, b != 0)
            blk = cell_labels(H, W, 9)[50:80, 70:150]
            lab[50:80, 70:150] = blk
            dd = disparities(lab)
            assert np.array_equal(dd[20, 64:124], disp[20, 64:124]) and np.isnan(dd[40, 100:110]).all()
            ref = lio.Evaluator(gt2, nonocc, thr)
            q = quantize(dd, precision)
            want_all, want_non = ref.evaluate(q)
            with np.errstate(invalid="ignore"):
                good = np.abs(q - gt2) <= F(thr)
            row = d.evaluate_once(lab, np.zeros((H, W), F), 0, dispGT=gt2, nonocc=nonocc, error_threshold=thr, precision=precision)
            assert row["n_valid"] == int(ref.valid.sum()) and row["n_nonocc"] == int(nonocc.sum())
            assert row["good_valid"] == int((good & ref.valid).sum()) and row["good_nonocc"] == int((good & nonocc).sum()), (precision, row)
            assert row["all"] == want_all and row["nonocc"] == want_non
            if precision < 0:
                assert good[20, 64:124][ref.valid[20, 64:124]].all() and good[21, 64:124][ref.valid[21, 64:124]].all() and not good[22, 64:124].any()
                seen["boundary"] += int(ref.valid[20, 64:124].sum())
            else:
                k = dd[30, 64:124] / F(0.25)
                assert np.array_equal(k - np.floor(k), np.full(60, 0.5, F))
                assert np.array_equal(q[30, 64:124] / F(0.25) % 2, np.zeros(60, F))            # ties went to the even multiple
                seen["ties"] += 60
            assert not good[40, 100:110].any() and not ref.valid[5, 70:90].any() and not ref.valid[6, 70:90].any()
        # no ground truth: the counts are 0
        row = d.evaluate_once(lab, np.zeros((H, W), F), 0)
        assert (row["good_valid"], row["good_nonocc"], row["n_valid"], row["n_nonocc"]) == (0, 0, 0, 0) and "all" not in row
    finally:
        d.close()
    assert seen["boundary"] > 0 and seen["ties"] > 0
    return seen


# ------------------------------------------------------------------------------------------------ 4. determinism and stream order
def case_determinism_and_stream_order(lib, device):
    import torch
    imL, imR, gt = cones_images()
    H, W = gt.shape
    e = api.HipCostVolumeEnergy.naive(imL, imR, windR=0, max_disp=63.0, lib=lib, filter="")
    dev = torch.device(device)
    if dev.type == "cuda":
        e.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    lab_a, lab_b = cell_labels(H, W, 1), cell_labels(H, W, 2)
    cost = sentinel_costs(H, W, 3)
    t_a, t_b = torch.from_numpy(lab_a).to(dev), torch.from_numpy(lab_b).to(dev)
    t_lab, t_cost = t_a.clone(), torch.from_numpy(cost).to(dev)
    key = lambda r: tuple(int(bits(r[k])) for k in ("data", "smooth")) + tuple(r[k] for k in ("good_valid", "good_nonocc", "n_valid", "n_nonocc"))
    ev = api.DeviceEvaluator(e, dispGT=gt, nonocc=gt > 0, error_threshold=1.0, precision=0.25, max_rows=5)
    try:
        ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=0, **PW)
        ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=1, **PW)
        if dev.type == "cuda":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream(dev))
            e.synchronize()
            e.set_thread_stream(side.cuda_stream)
            try:
                ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=2, **PW)
                side.synchronize()
            finally:
                e.set_thread_stream(0, bind=False)
        else:
            e.set_thread_stream(0)                  # (the simulator has one "stream": the binding itself is exercised)
            try:
                ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=2, **PW)
            finally:
                e.set_thread_stream(0, bind=False)
        # an evaluation, the label map overwritten on the same stream, another evaluation -- then one read
        t_lab.copy_(t_b)
        ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=3, **PW)
        t_lab.copy_(t_a)
        ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=4, **PW)
        try:
            ev.evaluate(t_lab.data_ptr(), t_cost.data_ptr(), mode=0, index=5, **PW)
            raise AssertionError("a full log must be an error")
        except api.LesHipError as ex:
            assert "full" in str(ex)
        rows = ev.rows()
        assert [r["index"] for r in rows] == [0, 1, 2, 3, 4]
        assert key(rows[0]) == key(rows[1]) == key(rows[2]) == key(rows[4])
        assert key(rows[3]) != key(rows[0])
        want_a, want_b = fsum(smooth_terms(imL, lab_a, **PW)), fsum(smooth_terms(imL, lab_b, **PW))
        n = 4 * H * W
        assert abs(rows[0]["smooth"] - want_a) <= sum_bound(n, want_a) and abs(rows[3]["smooth"] - want_b) <= sum_bound(n, want_b)
        assert abs(want_a - want_b) > 4 * sum_bound(n, want_a)
        assert [key(r) for r in ev.rows()] == [key(r) for r in rows]          # the refused call left the rows intact
    finally:
        ev.close()
        e.close()


# ------------------------------------------------------------------------------------------------ 5 / 6. region energy and the self-check
class ConesRun:
    """The cones crop under the cost-volume energy (units as case_quality_cones_gc), after init + one PatchMatch iteration, graph-cut context begun."""

    def __init__(self, lib, device, units=(5, 15, 25), seed=11, device_cuts="all", pm_iterations=1):
        import torch
        from localexpstereo_amd import pm
        from tests import parity_cases as pc
        self.torch = torch
        imL, vol, gt = pc.cones_ad_volume()
        self.imL = imL
        self.e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=20, eps=1e-4, th_col=0.12, max_disp=63.0, lib=lib)
        table = [[(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANSAC, 1), (api.PROPOSE_RANDOM, 7)],
                 [(api.PROPOSE_EXPANSION, 2), (api.PROPOSE_RANSAC, 1)], [(api.PROPOSE_EXPANSION, 2), (api.PROPOSE_RANSAC, 1)]][: len(units)]
        self.r = pm.PMRunner(self.e, units, table, seed=seed, device=device)
        self.g = lgc.GraphCut(imL, None, lambda_=1.0)
        self.r.init_labels()
        for it in range(pm_iterations):
            self.r.iteration(it)
        self.r.device_cuts = device_cuts
        self.r.begin_gc(self.g)

    def dev_f64(self, n):
        return self.torch.zeros(max(1, n), dtype=self.torch.float64, device=self.r.device)

    def close(self):
        self.r.close(); self.e.close(); self.g.close()


def region_terms(t, cost, rect):
    """fusedEnergy (host/ExpansionMove.h:243-266) of the current maps for one cell as a flat list of terms (for math.fsum and the term count): the
    costs of the region + the forward pairs with an endpoint in it.  t: pair_terms(...) of the maps."""
    x0, y0, w, h = (int(rect[k]) for k in ("x", "y", "w", "h"))
    H, W = cost.shape
    inr = np.zeros((H, W), bool)
    inr[y0:y0 + h, x0:x0 + w] = True
    terms = [cost[inr].astype(np.float64)]
    ys, xs = np.mgrid[0:H, 0:W]
    for dx, dy in FORWARD:
        v, m = t[(dx, dy)]
        yq, xq = np.where(m, ys + dy, ys), np.where(m, xs + dx, xs)
        terms.append(v[m & (inr | inr[yq, xq])].astype(np.float64))
    return np.concatenate(terms)


def case_runner_energy(lib, device, units=(12,)):
    """pm.PMRunner.energy == computeCurrentEnergy of the host context for the same maps: the initial labelling (1e6 sentinels among its costs) and
    the maps after one and two PatchMatch iterations -- the rows for which the host route of the log has no smoothness number."""
    cr = ConesRun(lib, device, units=units, pm_iterations=0)
    try:
        r, g = cr.r, cr.g
        n = r.H * r.W
        for step in range(3):
            if step:
                r.iteration(step - 1)
            data, smooth = r.energy(g.params)
            r.sync_gc_state()
            hd, hs = g.data_cost(0), g.smoothness_cost(0)
            assert abs(data - hd) <= 2 * sum_bound(n, hd) and abs(smooth - hs) <= 2 * sum_bound(4 * n, hs), (data, hd, smooth, hs)
            assert np.isfinite(smooth) and smooth > 0
    finally:
        cr.close()


def case_region_energy(lib, device, units=(5, 15, 25), sets_per_layer=1, locksteps=2):
    """les_hip_batch_region_energy for the lock-steps of one set of each layer of the cones crop, per cell:
    (a) against math.fsum of the restated terms of the same maps, within the sum bound (N = the cell's term count);
    (b) against the host path: the lock-step is moved by the host route (les_gc_expansion_moves(check=True), its own gap <= 1e-5 asserted), and the
    device value of the moved maps is held to the host's fusedEnergy of the same maps (les_gc_region_energy) within twice the sum bound, and to the
    host solver's flow on the same graphs (flow0 + flow) within the check's 1e-5;
    (c) a cell evaluated alone gives the bits it gives among the others.  Cells at the image border and 1 x 1 target rects included."""
    torch = __import__("torch")
    cr = ConesRun(lib, device, units=units)
    r, g, p = cr.r, cr.g, cr.g.params
    checked, border, tiny = 0, 0, 0
    try:
        H, W = r.H, r.W
        for li, layer in enumerate(r.shards):
            for sh in [s for s in layer if s.n][:sets_per_layer]:
                r._gc_buffers(sh)
                for kind, m in list(r._proposals(li, 0))[:locksteps]:
                    r._propose(sh, kind, m)
                    # the device's graphs (bit-identical to the host construction: tests/parity_cases.py: case_expansion_graph) for the host's solver
                    flow0 = sh.batch.expansion_graph(sh.planes.data_ptr(), r.labels.data_ptr(), r.cur.data_ptr(), r.prop.data_ptr(), sh.payload.data_ptr(), mode=0,
                                                     want_flow0=True, **p)
                    r.sync_gc_state()
                    prop = r.prop.cpu().numpy()
                    planes = sh.planes[: sh.n].cpu().numpy()
                    gap = g.expansion_moves(sh.regions, planes, prop, mode=0, check=True)      # the host route: its moves, its flow == fusedEnergy check
                    assert gap <= 1e-5
                    hm, hf = np.zeros(max(1, sh.graph_nodes), np.uint8), np.zeros(sh.n, np.float64)
                    lgc.solve_prebuilt(sh.regions, sh.payload[: sh.graph_nodes * 5].cpu().numpy(), sh.graph_off, hm, flows_out=hf)
                    r.labels.copy_(torch.from_numpy(g.labels[0])); r.cur.copy_(torch.from_numpy(g.costs[0]))      # the host-moved maps
                    out = cr.dev_f64(sh.n)
                    r._region_energy(sh, out)
                    r._sync()
                    dev_e = out[: sh.n].cpu().numpy()
                    lab1, cur1 = g.labels[0].copy(), g.costs[0].copy()
                    t = pair_terms(cr.imL, lab1, **p)
                    host_e = g.region_energy(sh.regions, mode=0)
                    for i in range(sh.n):
                        terms = region_terms(t, cur1, sh.regions[i])
                        S = fsum(terms)
                        assert abs(dev_e[i] - S) <= sum_bound(len(terms), S), (li, i, dev_e[i], S)
                        assert abs(dev_e[i] - host_e[i]) <= 2 * sum_bound(len(terms), S), (li, i, dev_e[i], host_e[i])
                        assert abs(flow0[i] + hf[i] - dev_e[i]) <= 1e-5 * max(1.0, abs(dev_e[i])) + 2 * sum_bound(len(terms), S), (li, i, flow0[i] + hf[i], dev_e[i])
                        rc = sh.regions[i]
                        border += int(rc["x"] == 0 or rc["y"] == 0 or rc["x"] + rc["w"] == W or rc["y"] + rc["h"] == H)
                        checked += 1
                    for i in sorted({0, sh.n // 2, sh.n - 1}):          # alone == with the others, bit for bit
                        b1 = api.Batch(r.e, sh.batch_filter[i:i + 1], sh.regions[i:i + 1])
                        one = cr.dev_f64(1)
                        b1.region_energy(r.labels.data_ptr(), r.cur.data_ptr(), one.data_ptr(), mode=0, **p)
                        r._sync()
                        assert bits(float(one[0])) == bits(dev_e[i]), (li, i)
                        b1.destroy()
        # 1 x 1 target rects (image corners among them), a column and a row
        lab1, cur1 = r.labels.cpu().numpy(), r.cur.cpu().numpy()
        t = pair_terms(cr.imL, lab1, **p)
        rects = np.array([(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (17, 23, 1, 1), (40, 0, 1, 7), (0, 50, 9, 1)], np.int32)
        fr = np.array([(max(0, x - 20), max(0, y - 20), min(W, x + w + 20) - max(0, x - 20), min(H, y + h + 20) - max(0, y - 20)) for x, y, w, h in rects], np.int32)
        b = api.Batch(r.e, fr, rects)
        out = cr.dev_f64(len(rects))
        b.region_energy(r.labels.data_ptr(), r.cur.data_ptr(), out.data_ptr(), mode=0, **p)
        r._sync()
        r.sync_gc_state()
        host_e = g.region_energy(rects, mode=0)
        for i, rc in enumerate(api._rects(rects)):
            terms = region_terms(t, cur1, rc)
            S = fsum(terms)
            assert abs(float(out[i]) - S) <= sum_bound(len(terms), S), (i, float(out[i]), S)
            assert abs(float(out[i]) - host_e[i]) <= 2 * sum_bound(len(terms), S), (i, float(out[i]), host_e[i])
            tiny += 1
        b.destroy()
    finally:
        cr.close()
    assert checked > 0 and border > 0 and tiny == 7
    return checked, border


def case_check_can_fail(lib, device, seed=5):
    """One lock-step's graphs on the cones crop, cut on the device, applied: gap <= 1e-5.  Then, from the same starting maps, edited copies of the masks
    (host-side edits): a minimum cut is a lower bound for every labelling of the cell, so E_after >= flow0 + flow - 1e-5 max(1, |E_after|) for every
    edited mask, and for the complemented and the random masks E_after exceeds flow0 + flow by more than that bound: the check reports them."""
    torch = __import__("torch")
    cr = ConesRun(lib, device, units=(12,))
    r, p = cr.r, cr.g.params
    rng = np.random.default_rng(seed)
    try:
        sh = next(s for s in r.shards[0] if s.n >= 2)
        r._gc_buffers(sh)
        kind, m = list(r._proposals(0, 0))[0]
        r._propose(sh, kind, m)
        flow0 = sh.batch.expansion_graph(sh.planes.data_ptr(), r.labels.data_ptr(), r.cur.data_ptr(), r.prop.data_ptr(), sh.payload.data_ptr(), mode=0,
                                         want_flow0=True, **p)
        st, fl = r._status(sh.n), cr.dev_f64(sh.n)
        sh.batch.solve_graphs(sh.payload.data_ptr(), sh.masks.data_ptr(), st.data_ptr(), flows_dev=fl.data_ptr())
        r._sync()
        assert not st.cpu().numpy().any()
        cut = flow0 + fl[: sh.n].cpu().numpy()
        lab0, cur0 = r.labels.clone(), r.cur.clone()
        masks = sh.masks[: sh.graph_nodes].cpu().numpy().copy()
        out = cr.dev_f64(sh.n)

        def energy_with(mk):
            r.labels.copy_(lab0); r.cur.copy_(cur0)
            dm = torch.from_numpy(np.ascontiguousarray(mk)).to(r.device)
            r._apply(sh, dm.data_ptr())
            r._region_energy(sh, out)
            r._sync()
            return out[: sh.n].cpu().numpy().copy()

        e_cut = energy_with(masks)
        bound = 1e-5 * np.maximum(1.0, np.abs(e_cut))
        gap = np.abs(cut - e_cut) / np.maximum(1.0, np.abs(e_cut))
        assert gap.max() <= 1e-5, gap.max()
        off = np.asarray(sh.graph_off, np.int64)
        sizes = np.array([int(rc["w"]) * int(rc["h"]) for rc in sh.regions], np.int64)
        edits = []
        for k in range(16):                             # single interior bytes flipped
            i = int(rng.integers(sh.n))
            w, h = int(sh.regions[i]["w"]), int(sh.regions[i]["h"])
            x, y = int(rng.integers(1, max(2, w - 1))), int(rng.integers(1, max(2, h - 1)))
            mk = masks.copy()
            mk[off[i] + y * w + x] ^= 255
            edits.append(("flip", mk))
        for k in range(8):
            edits.append(("random", np.where(rng.random(len(masks)) < 0.5, 255, 0).astype(np.uint8)))
        edits.append(("complement", (255 - masks).astype(np.uint8)))
        reported = 0
        for what, mk in edits:
            e_after = energy_with(mk)
            b = 1e-5 * np.maximum(1.0, np.abs(e_after))
            changed = np.array([(mk[o:o + s] != masks[o:o + s]).any() for o, s in zip(off, sizes)])
            below = e_after < cut - b
            assert not below.any(), (what, np.nonzero(below)[0], e_after[below], cut[below])       # a minimum cut is a lower bound
            if what != "flip":
                assert changed.all()
                assert (e_after > cut + b).all(), (what, np.nonzero(~(e_after > cut + b))[0])       # ... and the check reports these
                reported += int(changed.sum())
        r.labels.copy_(lab0); r.cur.copy_(cur0)
    finally:
        cr.close()
    return float(gap.max()), reported


# ------------------------------------------------------------------------------------------------ 7. whole runs
def stereo_run(lib, device, units, pmInit, maxIteration, views=(0,), device_cuts=None, table=None, seed=3, energy="naive", **opts):
    """stereo.FastGCStereo on the cones crop.  energy "naive": config 1's image-based cost on the padded crop, both views available (as
    tests/parity_cases.py: case_stereo_driver); "volume": the absolute-difference cost volume of the left view (as case_quality_cones_gc)."""
    from localexpstereo_amd import stereo
    if energy == "naive":
        imL, imR, gt = cones_images()
        e = api.HipCostVolumeEnergy.naive(imL, imR, max_disp=63.0, lib=lib)
    else:
        from tests import parity_cases as pc
        imL, vol, gt = pc.cones_ad_volume()
        imR = None
        e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=20, eps=1e-4, th_col=0.12, max_disp=63.0, lib=lib)
    check = opts.pop("check_flow_energy", False)
    st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=1.0), device=device, seed=seed, device_cuts=device_cuts, **opts)
    st.setEvaluator(lio.Evaluator(gt, gt > 0, 1.0), precision=0.25)
    st.check_flow_energy = check
    st.concurrent_views = False
    ex, ra, rn = api.PROPOSE_EXPANSION, api.PROPOSE_RANSAC, api.PROPOSE_RANDOM
    tabs = [[(ex, 1), (ra, 1), (rn, 7)], [(ex, 2), (ra, 1)], [(ex, 2), (ra, 1)]] if table is None else table
    for u, t in zip(units, tabs):
        st.addLayer(u, t)
    lab, raw = st.run(maxIteration, views, pmInit)
    e.close()
    return st, lab, raw


@contextlib.contextmanager
def rows_checked_against_host(n_pixels):
    """While active, every row that stereo.FastGCStereo logs is held to the host context's value for the same maps (labels and costs copied down
    after the row was made: data within twice the sum bound of N = H W terms, smooth of N <= 4 H W): the initial, PatchMatch and post-processing
    rows too, for which the default log has no smoothness number to compare with.  Yields the list of row indices checked."""
    from localexpstereo_amd import stereo
    orig, seen = stereo.FastGCStereo._evaluate_body, []

    def body(self, index, mode, runner, g, t0):
        orig(self, index, mode, runner, g, t0)
        row = self.log[-1]
        runner._sync()
        hd, hs = host_energy(self.imL, self.imR, runner.labels.cpu().numpy(), runner.cur.cpu().numpy(), mode, self._pairwise())
        assert abs(row["data"] - hd) <= 2 * sum_bound(n_pixels, hd), (index, row["data"], hd)
        assert abs(row["smooth"] - hs) <= 2 * sum_bound(4 * n_pixels, hs), (index, row["smooth"], hs)
        seen.append(index)
    stereo.FastGCStereo._evaluate_body = body
    try:
        yield seen
    finally:
        stereo.FastGCStereo._evaluate_body = orig


def compare_logs(st_dev, st_host, pmInit, maxIteration, n_pixels):
    """evaluate_on_device=True against the default run of the same seed (the rows of both logs)."""
    assert [r["index"] for r in st_dev.log] == [r["index"] for r in st_host.log]
    for rd, rh in zip(st_dev.log, st_host.log):
        S = abs(rh["data"])
        assert abs(rd["data"] - rh["data"]) <= 2 * sum_bound(n_pixels, S), (rd, rh)
        assert np.isfinite(rd["smooth"]) and rd["energy"] == rd["data"] + rd["smooth"]
        is_gc = pmInit < rd["index"] <= pmInit + maxIteration
        if is_gc:
            assert abs(rd["smooth"] - rh["smooth"]) <= 2 * sum_bound(4 * n_pixels, abs(rh["smooth"])), (rd, rh)
        else:
            assert rh["smooth"] != rh["smooth"]                 # the host route has no number here
        assert rd["all"] == rh["all"] and rd["nonocc"] == rh["nonocc"], (rd, rh)
        assert "time" in rd


def check_inner_log(st, pmInit, maxIteration, views):
    """Shape of an inner-loop log and its agreement with the main rows; -> (worst rise of `data` over a PatchMatch set, worst relative rise of the
    energy over a graph-cut set)."""
    rows = st.inner_log
    assert rows and all(set(r) == {"iteration", "layer", "set", "mode", "data", "smooth", "energy", "all", "nonocc"} for r in rows)
    main = {r["index"]: r for r in st.log}
    worst_pm, worst_gc = 0.0, 0.0
    for m in views:
        mine = [r for r in rows if r["mode"] == m]
        assert [r["iteration"] for r in mine] == sorted(r["iteration"] for r in mine)
        for it in range(1, pmInit + maxIteration + 1):
            of_it = [r for r in mine if r["iteration"] == it]
            assert of_it and [(r["layer"], r["set"]) for r in of_it] == sorted((r["layer"], r["set"]) for r in of_it)
            if m == 0:      # the last inner row of an iteration is that iteration's main row
                last = of_it[-1]
                for k in ("data", "smooth", "energy", "all", "nonocc"):
                    assert same_float(last[k], main[it][k]), (it, k, last[k], main[it][k])
        prev = None
        for r in mine:
            if prev is not None:
                if r["iteration"] <= pmInit:
                    assert r["data"] <= prev["data"], (prev, r)         # WTA replaces a cost only by a smaller one
                    worst_pm = max(worst_pm, r["data"] - prev["data"])
                elif prev["iteration"] > pmInit:
                    worst_gc = max(worst_gc, (r["energy"] - prev["energy"]) / abs(prev["energy"]))
            prev = r
    return worst_pm, worst_gc


def whole_run_cases(lib, device, kw, n_pixels, views=(0,)):
    """Test 7 on one scene: `kw` are stereo_run's arguments.  -> dict of the measured rises."""
    pmInit, maxIteration = kw["pmInit"], kw["maxIteration"]
    st0, lab0, raw0 = stereo_run(lib, device, views=views, **kw)
    with rows_checked_against_host(n_pixels) as seen:
        st1, lab1, raw1 = stereo_run(lib, device, views=views, evaluate_on_device=True, **kw)
    assert seen == [r["index"] for r in st1.log]
    assert lab0.tobytes() == lab1.tobytes() and raw0.tobytes() == raw1.tobytes()           # evaluation does not perturb the run
    compare_logs(st1, st0, pmInit, maxIteration, n_pixels)
    st2, lab2, raw2 = stereo_run(lib, device, views=views, inner_loop_log=True, **kw)
    assert lab0.tobytes() == lab2.tobytes() and raw0.tobytes() == raw2.tobytes()
    assert not st0.inner_log and not st1.inner_log
    pm_rise, gc_rise = check_inner_log(st2, pmInit, maxIteration, views)
    st3, _, _ = stereo_run(lib, device, views=views, inner_loop_log=True, **dict(kw, device_cuts="none"))
    _, host_rise = check_inner_log(st3, pmInit, maxIteration, views)
    out = dict(pm_rise=pm_rise, gc_rise_device_cuts=gc_rise, gc_rise_host_cuts=host_rise)
    # a set may raise the energy only through float rounding of the capacities: at most 1e-6 E, or twice what the host-cut run shows
    assert gc_rise <= max(1e-6, 2 * host_rise), out
    return out


def _check_counters(st):
    """What a check_flow_energy="device" run books: the gap, every device solver's own worst gap, and how many of the lock-steps were held to the host
    solver's flow because the device solver's own flow value missed 1e-5 (those re-solves are NOT cuts of the run: host_cuts stays 0)."""
    sec = st.gc_seconds
    total = sum(v for k, v in sec.items() if k.startswith("locksteps_checked_") and k != "locksteps_checked_with_host_flow")
    fell_back = sec.get("locksteps_checked_with_host_flow", 0)
    assert total > 0 and 0 <= fell_back <= total, sec
    assert (fell_back > 0) == any(v > 1e-5 for k, v in sec.items() if k.startswith("own_max_gap_")), sec
    return dict(gc_max_gap=st.gc_max_gap, locksteps=total, locksteps_held_to_the_host_flow=fell_back, share_held_to_the_host_flow=round(fell_back / total, 3),
                **{k: v for k, v in sec.items() if k.startswith(("own_max_gap", "locksteps_checked_", "cells_", "tiled_handed", "check_host_flow"))})


def check_device_run(lib, device, kw, views=(0,)):
    """check_flow_energy="device": the run stays on the device path and equals the unchecked run; -> its counters."""
    st0, lab0, _ = stereo_run(lib, device, views=views, **kw)
    st, lab, _ = stereo_run(lib, device, views=views, check_flow_energy="device", **kw)
    sec = st.gc_seconds
    assert st.gc_max_gap <= 1e-5, (st.gc_max_gap, sec)
    assert st.gc_moves_raised == 0
    assert sec.get("cells_checked_on_device", 0) > 0 and sec.get("cells_cut_on_device", 0) == sec["cells_checked_on_device"], sec
    assert sec.get("host_graph_locksteps", 0) == 0 and sec.get("host_cuts", 0.0) == 0.0 and sec.get("cells_recut_on_host", 0) == 0, sec
    assert lab.tobytes() == lab0.tobytes()
    return _check_counters(st)


# ------------------------------------------------------------------------------------------------ whole runs through MidV2 / MidV3 (MI355X)
def _midv(kind, data, iterations, pmIterations, doDual=False, **opts):
    """kind "midv2": stereo.MidV2 on `data`; "objects": stereo.MidV3 on the synthetic scene of tools/e2e_bench.py at 1436 x 992 x 256."""
    import sys
    from localexpstereo_amd import stereo
    if kind == "midv2":
        return stereo.MidV2(data, iterations=iterations, pmIterations=pmIterations, doDual=doDual, **opts) + (data["imL"].shape[0] * data["imL"].shape[1],)
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import e2e_bench
    H, W, D = 992, 1436, 256
    imL, imR, gt, volL = e2e_bench.scene_inputs(kind, H, W, D, "cuda")
    d = dict(imL=imL, imR=imR, dispGT=gt, nonocc=np.ones((H, W), bool), ndisp=D, gt_prec=-1.0)
    return stereo.MidV3(d, volL, None, iterations=iterations, pmIterations=pmIterations, doDual=doDual, smooth_weight=0.5, mc_threshold=0.5,
                        error_threshold=1.0, device="cuda", **opts) + (H * W,)


def midv_whole_runs(kind, data, iterations, pmIterations, doDual=False):
    """Test 7 through the front ends (their keyword pass-through included).  -> the measured rises per set."""
    views = (0, 1) if doDual else (0,)
    st0, lab0, raw0, n = _midv(kind, data, iterations, pmIterations, doDual)
    with rows_checked_against_host(n) as seen:
        st1, lab1, raw1, _ = _midv(kind, data, iterations, pmIterations, doDual, evaluate_on_device=True)
    assert seen == [r["index"] for r in st1.log]
    assert lab0.tobytes() == lab1.tobytes() and raw0.tobytes() == raw1.tobytes()
    compare_logs(st1, st0, pmIterations, iterations, n)
    st2, lab2, raw2, _ = _midv(kind, data, iterations, pmIterations, doDual, inner_loop_log=True)
    assert lab0.tobytes() == lab2.tobytes() and raw0.tobytes() == raw2.tobytes()
    pm_rise, gc_rise = check_inner_log(st2, pmIterations, iterations, views)
    assert st2.gc_seconds.get("sets_without_round_trips", 0) == st0.gc_seconds.get("sets_without_round_trips", 0) > 0      # the log rode on the speculative sets
    st3, _, _, _ = _midv(kind, data, iterations, pmIterations, doDual, inner_loop_log=True, device_cuts="none")
    _, host_rise = check_inner_log(st3, pmIterations, iterations, views)
    out = dict(pm_rise=pm_rise, gc_rise_device_cuts=gc_rise, gc_rise_host_cuts=host_rise, final_energy=st2.log[-1]["energy"])
    assert gc_rise <= max(1e-6, 2 * host_rise), out
    return out


def midv_check_device(data, iterations, pmIterations, kind="midv2"):
    """check_flow_energy="device" with device_cuts="all" through the front end; -> the counters (every solver's own worst gap among them)."""
    st0, lab0, _, _ = _midv(kind, data, iterations, pmIterations, device_cuts="all")
    st, lab, _, _ = _midv(kind, data, iterations, pmIterations, device_cuts="all", check_flow_energy="device")
    sec = st.gc_seconds
    assert st.gc_max_gap <= 1e-5, (st.gc_max_gap, sec)
    assert st.gc_moves_raised == 0, sec
    assert sec.get("cells_checked_on_device", 0) > 0 and sec.get("cells_cut_on_device", 0) == sec["cells_checked_on_device"], sec
    assert sec.get("host_graph_locksteps", 0) == 0 and sec.get("host_cuts", 0.0) == 0.0 and sec.get("cells_recut_on_host", 0) == 0, sec
    assert lab.tobytes() == lab0.tobytes()
    return _check_counters(st)
