"""Cases of tests/test_fusion.py: fusion moves on the device (csrc/les_pairwise.h: les_hip_batch_fusion_graph, les_hip_batch_apply_masks_labels,
pm.PMRunner.fuse, stereo.FastGCStereo.fuse) on the CPU simulator build and on the MI355X.

The definition, restated from csrc/les_pairwise.h.  Maps L0 (current) and L1 (proposal), cur[p] / prop[p] their unary costs, mask 255 = the pixel
takes L1[p].  For a pixel ee and a forward neighbour le (GE, EG, LG, GG), T(a, b) = min(|a(ee) - b(ee)| + |a(le) - b(le)|, th) * w * lambda with
pw_dot's operation order: c00 = T(L0[ee], L0[le]), c01 = T(L0[ee], L1[le]), c10 = T(L1[ee], L0[le]), c11 = T(L1[ee], L1[le]).  Per node, one
t-link replays: add(cur, prop); for k = 0..7 with the neighbour pt outside the cell and inside the image add(term(L0[p], L0[pt]), term(L1[p],
L0[pt])); for each forward direction, as j of the preceding pixel add(c00 - c01, 0), then as i of its own pair cap = max(0, ((c10 + c01) -
c11) - c00) and add(c01, c11).  A pair with ((c10 + c01) - c11) - c00 < 0 is counted as non-submodular.

References, none of them the code under test: the numpy f32 restatement below (itself checked against a literal per-pair loop in the reference's
program order), an fp64 enumeration of all labellings of small grids, the host max-flow solver (gc.solve_prebuilt), the expansion-move entry
points (whose graphs tests/parity_cases.py holds to the host construction), les_hip_batch_region_energy (held to the host by tests/eval_cases.py).

Tolerances: payloads, masks applied and labels are compared bit for bit.  flow0: 1e-9 relative, as case_expansion_graph.  Cut values of cells of
at most 16 nodes: 1e-9 max(1, sum |terminal|), as case_device_maxflow_vs_brute_force.  Flow against energy: the reference's 1e-5 relative
(LES/FastGCStereo.h:406).  Energy never rises over a set by more than 1e-6 E (tests/eval_cases.py: whole_run_cases)."""
import functools
import os
from types import SimpleNamespace

import numpy as np

from localexpstereo_amd import api
from localexpstereo_amd import gc as lgc
from tests import eval_cases as ec

F = np.float32
FWD = ((+1, 0), (0, +1), (-1, +1), (+1, +1))                                          # GE, EG, LG, GG: the order the graph is linked in
NB = ((-1, 0), (+1, 0), (0, -1), (0, +1), (-1, -1), (+1, -1), (-1, +1), (+1, +1))     # LE GE EL EG LL GL LG GG (LES/StereoEnergy.h:99-110)
PW = dict(lambda_=0.7, th_smooth=1.0, omega=10.0, epsilon=0.01)


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def dot(l, x, y):
    """pw_dot / channelDot: ((a x + b y) + c * 1) + v * 0, every operation rounded to f32."""
    return ((l[..., 0] * x + l[..., 1] * y) + l[..., 2] * F(1)) + l[..., 3] * F(0)


def getz(l, x, y):
    """Plane::GetZ: (a x + b y) + c."""
    return (l[..., 0] * x + l[..., 1] * y) + l[..., 2]


def tmin(d, th):
    """std::min(d, th) = (th < d) ? th : d."""
    return np.where(F(th) < d, F(th), d).astype(F)


def shifted(a, dx, dy):
    """a at (y + dy, x + dx), indices clamped to the image, and the mask of the pixels whose neighbour is inside it."""
    H, W = a.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    yq, xq = ys + dy, xs + dx
    inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
    return a[np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)], inside


def coeff(img, tab, dx, dy):
    """pw_coeff of every pixel towards (dx, dy): tab[|dI|_1], 0 where the pair leaves the image."""
    q, inside = shifted(img.astype(np.int64), dx, dy)
    return np.where(inside, tab[np.abs(img.astype(np.int64) - q).sum(-1)], F(0)).astype(F)


def fusion_terms(img, L0, L1, pw):
    """c00, c01, c10, c11 of every pixel ee towards each forward direction (H x W f32 each; garbage where the pair leaves the image)."""
    H, W = L0.shape[:2]
    tab = ec.coeff_table(pw["omega"], pw["epsilon"])
    ys, xs = (g.astype(F) for g in np.mgrid[0:H, 0:W])
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for dx, dy in FWD:
            xq, yq = xs + F(dx), ys + F(dy)
            w = coeff(img, tab, dx, dy)
            n0, _ = shifted(L0, dx, dy)
            n1, _ = shifted(L1, dx, dy)
            e = [(dot(L0, xs, ys), dot(L0, xq, yq)), (dot(L1, xs, ys), dot(L1, xq, yq))]          # the pixel's own labels at ee and at le
            n = [(dot(n0, xs, ys), dot(n0, xq, yq)), (dot(n1, xs, ys), dot(n1, xq, yq))]          # the neighbour's labels at ee and at le
            T = lambda a, b: ((tmin(np.abs(a[0] - b[0]) + np.abs(a[1] - b[1]), pw["th_smooth"]) * w) * F(pw["lambda_"])).astype(F)
            out.append((T(e[0], n[0]), T(e[0], n[1]), T(e[1], n[0]), T(e[1], n[1])))
    return out


class TLinks:
    """MaxFlow add_tweights (TLink of csrc/les_pairwise.h) for an array of nodes, under a mask."""

    def __init__(self, shape):
        self.tr, self.flow = np.zeros(shape, F), np.zeros(shape, np.float64)

    def add(self, cap_source, cap_sink, mask):
        cs, ck = np.broadcast_to(np.asarray(cap_source, F), self.tr.shape), np.broadcast_to(np.asarray(cap_sink, F), self.tr.shape)
        d = self.tr
        with np.errstate(invalid="ignore", over="ignore"):
            cs2 = np.where(d > 0, cs + d, cs).astype(F)
            ck2 = np.where(d > 0, ck, ck - d).astype(F)
            self.flow = np.where(mask, self.flow + np.where(cs2 < ck2, cs2, ck2).astype(np.float64), self.flow)
            self.tr = np.where(mask, (cs2 - ck2).astype(F), self.tr)


def restate_cell(img, L0, L1, cur, prop, rect, pw, terms=None):
    """The fusion graph of one cell -> (payload h x w x 5 f32, flow0 fp64, non-submodular pairs)."""
    x0, y0, w, h = (int(v) for v in rect)
    H, W = L0.shape[:2]
    terms = fusion_terms(img, L0, L1, pw) if terms is None else terms
    tab = ec.coeff_table(pw["omega"], pw["epsilon"])
    Y, X = np.mgrid[y0:y0 + h, x0:x0 + w]
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    in_cell = lambda xx, yy: (xx >= x0) & (xx < x0 + w) & (yy >= y0) & (yy < y0 + h)
    t = TLinks((h, w))
    t.add(cur[sl], prop[sl], np.ones((h, w), bool))
    Xf, Yf = X.astype(F), Y.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        for dx, dy in NB:
            xt, yt = X + dx, Y + dy
            m = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H) & ~in_cell(xt, yt)
            if not m.any():
                continue
            lpt = L0[np.clip(yt, 0, H - 1), np.clip(xt, 0, W - 1)]
            co = coeff(img, tab, dx, dy)[sl]
            xtf, ytf = xt.astype(F), yt.astype(F)
            term = lambda ls: ((co * tmin(np.abs(getz(ls, Xf, Yf) - getz(lpt, Xf, Yf)) + np.abs(getz(ls, xtf, ytf) - getz(lpt, xtf, ytf)), pw["th_smooth"]))
                               * F(pw["lambda_"])).astype(F)
            t.add(term(L0[sl]), term(L1[sl]), m)
        cap = np.zeros((h, w, 4), F)
        count = 0
        for d, (dx, dy) in enumerate(FWD):
            c00, c01, c10, c11 = terms[d]
            xs, ys = X - dx, Y - dy                                           # as j of the preceding pixel
            m = in_cell(xs, ys)
            ysc, xsc = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
            t.add((c00[ysc, xsc] - c01[ysc, xsc]).astype(F), F(0), m)
            m = in_cell(X + dx, Y + dy)                                       # as i of its own pair
            bcd = (((c10[sl] + c01[sl]) - c11[sl]) - c00[sl]).astype(F)
            count += int(((bcd < 0) & m).sum())
            cap[..., d] = np.where(m & (F(0) < bcd), bcd, F(0))
            t.add(c01[sl], c11[sl], m)
    return np.concatenate([t.tr[..., None], cap], -1).astype(F), float(t.flow.sum()), count


# ------------------------------------------------------------------------------------------------ the literal per-pair loop
class _Scalar:
    def __init__(self):
        self.tr, self.flow = F(0), 0.0

    def add(self, cs, ck):
        cs, ck, d = F(cs), F(ck), self.tr
        if d > 0:
            cs = F(cs + d)
        else:
            ck = F(ck - d)
        self.flow += float(cs if cs < ck else ck)
        self.tr = F(cs - ck)


def _sdot(l, x, y):
    return F(F(F(F(l[0] * F(x)) + F(l[1] * F(y))) + F(l[2] * F(1))) + F(l[3] * F(0)))


def _sgetz(l, x, y):
    return F(F(F(l[0] * F(x)) + F(l[1] * F(y))) + l[2])


def _sT(a, b, ee, le, w, pw):
    d = F(abs(F(_sdot(a, *ee) - _sdot(b, *ee))) + abs(F(_sdot(a, *le) - _sdot(b, *le))))
    mn = F(pw["th_smooth"]) if F(pw["th_smooth"]) < d else d
    return F(F(mn * w) * F(pw["lambda_"]))


def restate_cell_loop(img, L0, L1, cur, prop, rect, pw):
    """The same graph by the reference's program (LES/FastGCStereo.h:257-363 with c11 kept): every node's unary and border t-links first, then
    the pairs direction by direction in raster order, each pair adding to its two nodes."""
    x0, y0, w, h = (int(v) for v in rect)
    H, W = L0.shape[:2]
    tab = ec.coeff_table(pw["omega"], pw["epsilon"])
    co = lambda x, y, dx, dy: tab[sum(abs(int(img[y, x, c]) - int(img[y + dy, x + dx, c])) for c in range(3))]
    node = [[_Scalar() for _ in range(w)] for _ in range(h)]
    cap = np.zeros((h, w, 4), F)
    count = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                X, Y = x0 + x, y0 + y
                node[y][x].add(cur[Y, X], prop[Y, X])
                for dx, dy in NB:
                    xt, yt = X + dx, Y + dy
                    if (x0 <= xt < x0 + w and y0 <= yt < y0 + h) or not (0 <= xt < W and 0 <= yt < H):
                        continue
                    c, lpt = co(X, Y, dx, dy), L0[yt, xt]
                    terms = []
                    for ls in (L0[Y, X], L1[Y, X]):
                        d = F(abs(F(_sgetz(ls, X, Y) - _sgetz(lpt, X, Y))) + abs(F(_sgetz(ls, xt, yt) - _sgetz(lpt, xt, yt))))
                        terms.append(F(F(c * (F(pw["th_smooth"]) if F(pw["th_smooth"]) < d else d)) * F(pw["lambda_"])))
                    node[y][x].add(terms[0], terms[1])
        for d, (dx, dy) in enumerate(FWD):
            for y in range(h):
                for x in range(w):
                    xn, yn = x + dx, y + dy
                    if not (0 <= xn < w and 0 <= yn < h):
                        continue
                    ee, le = (x0 + x, y0 + y), (x0 + xn, y0 + yn)
                    wgt = co(ee[0], ee[1], dx, dy)
                    a0, a1, b0, b1 = L0[ee[1], ee[0]], L1[ee[1], ee[0]], L0[le[1], le[0]], L1[le[1], le[0]]
                    c00, c01, c10, c11 = _sT(a0, b0, ee, le, wgt, pw), _sT(a0, b1, ee, le, wgt, pw), _sT(a1, b0, ee, le, wgt, pw), _sT(a1, b1, ee, le, wgt, pw)
                    bcd = F(F(F(c10 + c01) - c11) - c00)
                    count += int(bcd < 0)
                    cap[y, x, d] = bcd if F(0) < bcd else F(0)
                    node[y][x].add(c01, c11)
                    node[yn][xn].add(F(c00 - c01), F(0))
    tr = np.array([[n.tr for n in row] for row in node], F)
    return np.concatenate([tr[..., None], cap], -1).astype(F), float(sum(n.flow for row in node for n in row)), count


# ------------------------------------------------------------------------------------------------ fixtures
def label_map(H, W, seed, cell=5, maxd=2.5, slant=0.15):
    """Random slanted planes per block, a few disparities apart: pair differences on both sides of th_smooth."""
    lab = ec.cell_labels(H, W, seed, cell=cell, maxd=maxd, slant=slant)
    lab[..., 3] = np.random.default_rng(seed + 1000).uniform(-1, 1, (H, W)).astype(F)      # a vertical disparity: pw_dot multiplies it by 0
    return np.ascontiguousarray(lab)


IMG_H, IMG_W = 96, 128
# hand-made cells on the 128 x 96 image: 1 x 1, 1 x 7, 7 x 1, 2 x 2 and three more of at most 16 nodes, the four corners, the four edges, an interior
# 45 x 45 cell (the register kernel's), all disjoint; a 50 x 50 cell (2500 > 2304 nodes: the tiled solver); the whole image (48 graph chunks)
SMALL = [(56, 70, 1, 1), (58, 62, 1, 7), (10, 60, 7, 1), (30, 70, 2, 2), (20, 62, 3, 4), (40, 62, 4, 4), (24, 70, 3, 5),
         (0, 0, 5, 4), (122, 0, 6, 5), (0, 92, 7, 4), (123, 90, 5, 6), (40, 0, 9, 6), (0, 30, 6, 9), (121, 40, 7, 8), (50, 91, 8, 5), (8, 8, 45, 45)]
BATCHES = {"small": SMALL, "50x50": [(60, 10, 50, 50)], "whole": [(0, 0, IMG_W, IMG_H)]}


@functools.lru_cache(maxsize=None)
def scene():
    imL, imR = ec.random_images(IMG_H, IMG_W, 21, smooth_colours=True)
    rng = np.random.default_rng(22)
    return SimpleNamespace(imL=imL, imR=imR, L0=label_map(IMG_H, IMG_W, 31, cell=5), L1=label_map(IMG_H, IMG_W, 32, cell=7),
                           cur=rng.uniform(0, 0.5, (IMG_H, IMG_W)).astype(F), prop=rng.uniform(0, 0.5, (IMG_H, IMG_W)).astype(F))


@functools.lru_cache(maxsize=None)
def restated(mode, name):
    """The restated graphs of a batch of the scene, computed once: [(payload, flow0, count)] per cell."""
    s = scene()
    img = s.imL if mode == 0 else s.imR
    terms = fusion_terms(img, s.L0, s.L1, PW)
    return [restate_cell(img, s.L0, s.L1, s.cur, s.prop, r, PW, terms) for r in BATCHES[name]]


class Dev:
    """An energy context on the scene's images (image-based cost, no aggregation) and the four device maps."""

    def __init__(self, lib, s=None):
        s = scene() if s is None else s
        self.s = s
        self.e = api.HipCostVolumeEnergy.naive(s.imL, s.imR, windR=0, max_disp=63.0, lib=lib, filter="")
        H, W = self.e.H, self.e.W
        self.L0, self.L1 = api.DeviceBuffer(self.e, H * W * 16), api.DeviceBuffer(self.e, H * W * 16)
        self.cur, self.prop = api.DeviceBuffer(self.e, H * W * 4), api.DeviceBuffer(self.e, H * W * 4)
        self.extra = []
        self.reset()

    def reset(self, L1=None):
        self.L0.upload(self.s.L0); self.L1.upload(self.s.L1 if L1 is None else L1)
        self.cur.upload(self.s.cur); self.prop.upload(self.s.prop)

    def buf(self, nbytes):
        b = api.DeviceBuffer(self.e, max(16, nbytes))
        self.extra.append(b)
        return b

    def maps(self):
        H, W = self.e.H, self.e.W
        self.e.synchronize()
        return self.L0.download((H, W, 4), F), self.cur.download((H, W), F)

    def close(self):
        for b in [self.L0, self.L1, self.cur, self.prop] + self.extra:
            b.free()
        self.e.close()


def batch_of(d, name):
    trs = api._rects(np.array(BATCHES[name], np.int32))
    b = api.Batch(d.e, trs, trs)
    return b, trs, b.graph_offsets(), b.graph_nodes()


def fusion_graph(d, b, nn, mode, L1=None, pw=PW):
    """-> (payload nn x 5, flow0, counts) of the batch from the device."""
    pay, cnt = d.buf(nn * 20), d.buf(4 * b.n)
    cnt.fill(0x5A)                                                      # the entry point zeroes the counts itself
    f0 = b.fusion_graph((d.L1 if L1 is None else L1).ptr, d.L0.ptr, d.cur.ptr, d.prop.ptr, pay.ptr, mode=mode, want_flow0=True, nonsubmodular_dev=cnt.ptr, **pw)
    d.e.synchronize()
    return pay, pay.download((nn, 5), F), f0, cnt.download((b.n,), np.int32)


def host_cut(trs, payload, off, nn):
    masks, flows = np.zeros(max(1, nn), np.uint8), np.zeros(len(trs), np.float64)
    lgc.solve_prebuilt(trs, np.ascontiguousarray(payload.reshape(-1), F), off, masks, flows_out=flows)
    return masks[:nn], flows


# ------------------------------------------------------------------------------------------------ 1. the restatement itself (CPU only)
def case_restatement_matches_loop():
    checked = 0
    for (H, W), rects, seed in (((7, 8), [(2, 1, 4, 5), (0, 0, 3, 3), (5, 4, 3, 3), (0, 0, 8, 7), (3, 3, 1, 1), (1, 6, 5, 1)], 1),
                                ((6, 5), [(1, 1, 3, 4), (0, 0, 5, 6), (4, 0, 1, 6)], 2)):
        imL, _ = ec.random_images(H, W, seed, smooth_colours=True)
        L0, L1 = label_map(H, W, 40 + seed, cell=2), label_map(H, W, 50 + seed, cell=3)
        rng = np.random.default_rng(seed)
        cur, prop = rng.uniform(0, 0.5, (H, W)).astype(F), rng.uniform(0, 0.5, (H, W)).astype(F)
        for pw in (PW, dict(lambda_=1.0, th_smooth=0.4, omega=4.0, epsilon=0.2)):
            for r in rects:
                a, b = restate_cell(imL, L0, L1, cur, prop, r, pw), restate_cell_loop(imL, L0, L1, cur, prop, r, pw)
                assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (H, W, r)
                assert abs(a[1] - b[1]) <= 1e-12 * max(1.0, abs(b[1])) and a[2] == b[2], (r, a[1:], b[1:])
                checked += 1
    return checked


def case_enumeration(instances=40, H=3, W=4):
    """fp64, the whole H x W grid as one cell: the cut cost of the graph equals E' for all 2^(H W) labellings, E' >= E, and E' = E at all-keep and
    all-take, where E is the true energy of the mixed labelling and E' raises the "i takes, j keeps" cost of every non-submodular pair by its
    deficit.  Bound of the comparison: ~60 fp64 terms of order 1 summed in two orders differ by far less than 1e-12 max(1, E').
    -> (worst difference, share of non-submodular pairs)"""
    n = H * W
    codes = np.arange(1 << n, dtype=np.int64)
    take = ((codes[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)          # True = SOURCE = the pixel takes L1
    worst, nonsub, npairs = 0.0, 0, 0
    for inst in range(instances):
        rng = np.random.default_rng(100 + inst)
        L = [np.stack([rng.uniform(-0.3, 0.3, (H, W)), rng.uniform(-0.3, 0.3, (H, W)), rng.uniform(0, 2.5, (H, W))], -1) for _ in range(2)]
        u = [rng.uniform(0, 0.5, n), rng.uniform(0, 0.5, n)]
        tr, flow0 = np.zeros(n), 0.0

        def add(i, cs, ck):
            nonlocal flow0
            if tr[i] > 0:
                cs += tr[i]
            else:
                ck -= tr[i]
            flow0 += min(cs, ck)
            tr[i] = cs - ck
        for i in range(n):
            add(i, u[0][i], u[1][i])
        z = lambda l, x, y: l[0] * x + l[1] * y + l[2]
        pairs = []
        for dx, dy in FWD:
            for y in range(H):
                for x in range(W):
                    xn, yn = x + dx, y + dy
                    if not (0 <= xn < W and 0 <= yn < H):
                        continue
                    wgt = rng.uniform(0.05, 1.0)
                    T = lambda a, b: min(abs(z(a, x, y) - z(b, x, y)) + abs(z(a, xn, yn) - z(b, xn, yn)), 1.0) * wgt
                    c = [[T(L[s][y, x], L[t][yn, xn]) for t in (0, 1)] for s in (0, 1)]
                    bcd = c[1][0] + c[0][1] - c[1][1] - c[0][0]
                    i, j = y * W + x, yn * W + xn
                    pairs.append((i, j, c, max(0.0, bcd), max(0.0, -bcd)))
                    add(i, c[0][1], c[1][1])
                    add(j, c[0][0] - c[0][1], 0.0)
        cut = flow0 + np.where(take, np.maximum(-tr, 0)[None, :], np.maximum(tr, 0)[None, :]).sum(1)
        E = np.where(take, u[1][None, :], u[0][None, :]).sum(1)
        Ep = E.copy()
        for i, j, c, cap, deficit in pairs:
            ti, tj = take[:, i], take[:, j]
            cut += cap * (ti & ~tj)
            term = np.where(ti, np.where(tj, c[1][1], c[1][0]), np.where(tj, c[0][1], c[0][0]))
            E += term
            Ep += term + deficit * (ti & ~tj)
            nonsub += int(deficit > 0)
            npairs += 1
        assert np.all(np.abs(cut - Ep) <= 1e-12 * np.maximum(1.0, Ep)), (inst, np.abs(cut - Ep).max())
        assert np.all(Ep >= E) and Ep[0] == E[0] and Ep[-1] == E[-1], inst
        worst = max(worst, float(np.abs(cut - Ep).max()))
    assert nonsub > 0                                                        # the truncation path is exercised
    return worst, nonsub / npairs


# ------------------------------------------------------------------------------------------------ 2. payload, flow0, counts
def case_payload(lib):
    total = 0
    d = Dev(lib)
    try:
        for mode in (0, 1):
            for name in BATCHES:
                b, trs, off, nn = batch_of(d, name)
                _, got, f0, cnt = fusion_graph(d, b, nn, mode)
                for i, ((x, y, w, h), (pay, flow0, count)) in enumerate(zip(BATCHES[name], restated(mode, name))):
                    g = got[off[i]: off[i] + w * h].reshape(h, w, 5)
                    diff = g.view(np.uint32) != pay.view(np.uint32)
                    assert not diff.any(), f"view {mode}, {name}, cell {i} ({w}x{h}): {int(diff.sum())} payload values differ from the restatement"
                    assert abs(f0[i] - flow0) <= 1e-9 * max(1.0, abs(flow0)), (mode, name, i, f0[i], flow0)
                    assert cnt[i] == count, (mode, name, i, cnt[i], count)
                    total += count
                assert (got[:, 1:] > 0).mean() > 0.2 or name == "small"            # real pairwise structure
                b.destroy()
    finally:
        d.close()
    assert total > 0
    return total


# ------------------------------------------------------------------------------------------------ 3. the pin to the expansion chain
def exact_scene():
    """An instance on which the f32 arithmetic of the pair terms is exact: a one-colour image per view (every coefficient is exp(0) = 1), planes
    with slopes in eighths and offsets in quarters (every product, sum and difference below is a small multiple of 1/8), lambda 1."""
    rng = np.random.default_rng(7)
    dyadic = lambda shape: np.stack([rng.integers(-2, 3, shape) / 8.0, rng.integers(-2, 3, shape) / 8.0, rng.integers(0, 11, shape) / 4.0,
                                     rng.integers(-4, 5, shape) / 4.0], -1).astype(F)
    blocks = dyadic((-(-IMG_H // 5), -(-IMG_W // 5)))
    L0 = np.ascontiguousarray(np.repeat(np.repeat(blocks, 5, 0), 5, 1)[:IMG_H, :IMG_W])
    one = lambda v: np.full((IMG_H, IMG_W, 3), v, np.uint8)
    return SimpleNamespace(imL=one(90), imR=one(140), L0=L0, L1=L0.copy(), cur=scene().cur, prop=scene().prop, planes=dyadic)


def case_pin_to_expansion(lib):
    """L1 constant over every cell (each cell's plane written over its region): the fusion graph IS the expansion graph of those planes bit for
    bit, and the label-map apply gives the bits of the plane apply (random masks).

    The counts.  With one plane P as L1, c11 = 0 and T is a truncated metric on the evaluated planes, so c10 + c01 >= c00 and no pair is
    non-submodular -- in exact arithmetic.  In f32 the three terms are rounded on their own (two differences, a sum and two products each: five
    roundings a term), and where P lies between the two current labels at both pixels the inequality is an equality that rounding can miss by at
    most 16 ulp of c00.  So: on exact_scene (f32 arithmetic exact) every count is asserted to be 0; on the random scene every count equals the
    restated one, every pair counted is within 2^-20 c00 of zero, and it is a pair the expansion kernel clamps as well (its capacity is 0 in the
    identical payload).  Measured on the simulator build: 4 pairs of the 45 x 45 cell of view 0, deficits 7.5e-9 ... 3.0e-8 (about one ulp)."""
    rng = np.random.default_rng(5)
    rounding_pairs = 0
    for which, s, pw in (("random", scene(), PW), ("exact", exact_scene(), dict(PW, lambda_=1.0))):
        d = Dev(lib, s)
        try:
            for mode, name in ((0, "small"), (1, "small"), (0, "50x50"), (1, "whole")):
                rects = BATCHES[name]
                if which == "exact":
                    planes = s.planes(len(rects))
                else:
                    planes = np.stack([rng.uniform(-0.15, 0.15, len(rects)), rng.uniform(-0.15, 0.15, len(rects)), rng.uniform(0, 2.5, len(rects)),
                                       rng.uniform(-1, 1, len(rects))], -1).astype(F)
                L1 = s.L1.copy()
                for (x, y, w, h), pl in zip(rects, planes):
                    L1[y:y + h, x:x + w] = pl
                d.reset(L1)
                b, trs, off, nn = batch_of(d, name)
                _, got, f0, cnt = fusion_graph(d, b, nn, mode, pw=pw)
                dpl, pay2 = d.buf(16 * len(rects)), d.buf(nn * 20)
                dpl.upload(planes)
                f0e = b.expansion_graph(dpl.ptr, d.L0.ptr, d.cur.ptr, d.prop.ptr, pay2.ptr, mode=mode, want_flow0=True, **pw)
                d.e.synchronize()
                want = pay2.download((nn, 5), F)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (which, mode, name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                assert np.array_equal(f0, f0e), (which, mode, name)
                if which == "exact":
                    assert not cnt.any(), (mode, name, cnt)
                    assert (got[:, 1:] > 0).any()
                else:
                    terms = fusion_terms(s.imL if mode == 0 else s.imR, s.L0, L1, pw)
                    for i, (x, y, w, h) in enumerate(rects):
                        sl, n = (slice(y, y + h), slice(x, x + w)), 0
                        Y, X = np.mgrid[0:h, 0:w]
                        for k, (dx, dy) in enumerate(FWD):
                            c00, c01, c10, c11 = (t[sl] for t in terms[k])
                            pair = (X + dx >= 0) & (X + dx < w) & (Y + dy < h)          # both pixels in the cell
                            assert not c11[pair].any()
                            bcd = ((c10 + c01) - c11) - c00
                            m = (bcd < 0) & pair
                            assert (np.abs(bcd[m]) <= 2.0 ** -20 * c00[m]).all(), (mode, name, i, bcd[m], c00[m])
                            assert not got[off[i]: off[i] + w * h].reshape(h, w, 5)[..., 1 + k][m].any()
                            n += int(m.sum())
                        assert cnt[i] == n, (mode, name, i, cnt[i], n)
                        rounding_pairs += n
                masks = np.where(rng.random(nn) < 0.5, 255, 0).astype(np.uint8)
                dm = d.buf(nn)
                dm.upload(masks)
                b.apply_masks_labels(d.L1.ptr, dm.ptr, d.cur.ptr, d.prop.ptr, d.L0.ptr)
                lab_f, cur_f = d.maps()
                d.reset(L1)
                b.apply_masks(dpl.ptr, dm.ptr, d.cur.ptr, d.prop.ptr, d.L0.ptr)
                lab_e, cur_e = d.maps()
                assert np.array_equal(lab_f.view(np.uint32), lab_e.view(np.uint32)) and np.array_equal(cur_f.view(np.uint32), cur_e.view(np.uint32))
                assert (lab_f.view(np.uint32) != s.L0.view(np.uint32)).any()
                b.destroy()
        finally:
            d.close()
    return rounding_pairs


# ------------------------------------------------------------------------------------------------ 3b. one plane with non-finite coefficients
NONFINITE_PLANES = np.array([(np.inf, 0, 1, 0), (0, -np.inf, 1, 0), (np.nan, 0, 1, 0), (0, 0, np.nan, 0), (3e38, 3e38, 3e38, 0), (0, 0, np.inf, 0),
                             (0, 0, -3e38, np.inf), (1e30, -1e30, 0, np.nan)], F)
NONFINITE_RUNS = (("small", 0), ("small", 1), ("50x50", 0))
NONFINITE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expansion_nonfinite.npz")


def one_plane_nonfinite(lib):
    """Batch.expansion_graph of the scene with NONFINITE_PLANES cycled over the cells -> {"<batch>_<mode>_payload": nn x 5 f32, "..._flow0": n f64}."""
    out = {}
    d = Dev(lib)
    try:
        for name, mode in NONFINITE_RUNS:
            b, trs, off, nn = batch_of(d, name)
            planes = np.ascontiguousarray(NONFINITE_PLANES[np.arange(b.n) % len(NONFINITE_PLANES)])
            dpl, pay = d.buf(16 * b.n), d.buf(nn * 20)
            dpl.upload(planes)
            f0 = b.expansion_graph(dpl.ptr, d.L0.ptr, d.cur.ptr, d.prop.ptr, pay.ptr, mode=mode, want_flow0=True, **PW)
            d.e.synchronize()
            out[f"{name}_{mode}_payload"], out[f"{name}_{mode}_flow0"] = pay.download((nn, 5), F), f0
            b.destroy()
    finally:
        d.close()
    return out


def record_one_plane_nonfinite(lib):
    """Writes tests/golden/expansion_nonfinite.npz (outputs only, compressed).  Called by hand on the commit whose expansion graphs are to be
    kept -- never by a test."""
    np.savez_compressed(NONFINITE_GOLDEN, **one_plane_nonfinite(lib))


def case_one_plane_nonfinite(lib):
    """Expansion moves whose plane has an infinite, NaN or near-overflow coefficient.  With one plane P the pair term c11 = T(P, P) is 0 only for
    finite P (inf - inf = NaN), and the expansion graph never forms it: c01 and c10 are truncated to th_smooth and stay finite where a computed
    c11 would turn the node's words into NaN.  No restatement decides that, so the expected values are recorded ones: payload and flow0 of
    Batch.expansion_graph from the CPU simulator build of the commit before the expansion and fusion graph kernels became one template
    (tests/golden/expansion_nonfinite.npz, written by record_one_plane_nonfinite).  That commit's MI355X build gave the same words, so one
    recorded set serves both backends.  Every word is bit-equal or NaN on both sides (NaN payload bits are not promised); the 50 x 50 cell, whose
    plane is (inf, 0, 1, 0), has no NaN word and a finite non-zero one.  -> (words compared, NaN words)"""
    want = np.load(NONFINITE_GOLDEN)
    got = one_plane_nonfinite(lib)
    assert sorted(want.files) == sorted(got)
    words = nans = 0
    for key in want.files:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, key
        bits = np.uint32 if g.dtype == F else np.uint64
        same = (g.view(bits) == w.view(bits)) | (np.isnan(g) & np.isnan(w))
        assert same.all(), f"{key}: {int((~same).sum())} of {same.size} words differ from the recorded ones"
        words += same.size
        nans += int(np.isnan(w).sum())
    big = got["50x50_0_payload"]
    assert not np.isnan(big).any() and (np.isfinite(big) & (big != 0)).any()
    assert nans > 0                                                          # the small batch's NaN planes reach the payload
    return words, nans


# ------------------------------------------------------------------------------------------------ 4. cuts on fusion payloads (device solvers)
def enumerated_minimum(p5, w, h):
    """The smallest cut capacity (fp64) over all 2^(w h) labellings of one cell's payload (as case_device_maxflow_vs_brute_force enumerates them)."""
    n = w * h
    codes = np.arange(1 << n, dtype=np.int64)
    src = ((codes[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    q = p5.reshape(h, w, 5).astype(np.float64)
    tr = q[..., 0].reshape(-1)
    cap = np.where(src, np.maximum(-tr, 0)[None, :], np.maximum(tr, 0)[None, :]).sum(1)
    for k, (dx, dy) in enumerate(FWD):
        for y in range(h):
            for x in range(w):
                xx, yy = x + dx, y + dy
                if q[y, x, 1 + k] > 0 and 0 <= xx < w and 0 <= yy < h:
                    cap += q[y, x, 1 + k] * (src[:, y * w + x] & ~src[:, yy * w + xx])
    return float(cap.min())


def case_device_cuts(lib):
    """The device solvers on fusion payloads: status 0; cells of at most 16 nodes: the mask's cut under the restated graph is the enumerated
    minimum; cells of at most 2304 nodes: the host solver's mask node for node; the 50 x 50 and whole-image cells (tiled solver): the rule of
    case_tiled_maxflow_hard_cells -- the host solver's mask node for node, flows to 1e-6 sum |terminal| + 1e-5 |flow| + 1e-5."""
    from tests import parity_cases as pc
    d = Dev(lib)
    enumerated = 0
    try:
        for mode in (0, 1):
            for name in BATCHES:
                b, trs, off, nn = batch_of(d, name)
                pay, got, f0, cnt = fusion_graph(d, b, nn, mode)
                dm, ds, df = d.buf(nn), d.buf(4 * b.n), d.buf(8 * b.n)
                if b.max_cell_nodes <= api.Batch.MAXFLOW_MAX_NODES:
                    b.solve_graphs(pay.ptr, dm.ptr, ds.ptr, df.ptr)
                else:
                    ws = d.buf(b.tiled_workspace_bytes() + 256)
                    wp = (ws.ptr + 255) & ~255
                    b.solve_graphs_tiled(pay.ptr, dm.ptr, ds.ptr, wp, ws.nbytes - (wp - ws.ptr), df.ptr)
                d.e.synchronize()
                assert not ds.download((b.n,), np.int32).any(), (mode, name)
                dev_m, dev_f = dm.download((nn,), np.uint8), df.download((b.n,), np.float64)
                host_m, host_f = host_cut(trs, got, off, nn)
                for i, ((x, y, w, h), (rpay, _, _)) in enumerate(zip(BATCHES[name], restated(mode, name))):
                    n, src = w * h, dev_m[off[i]: off[i] + w * h] != 0
                    assert np.array_equal(src, host_m[off[i]: off[i] + n] != 0), f"view {mode}, {name}, cell {i} ({w}x{h}): {int((src != (host_m[off[i]: off[i] + n] != 0)).sum())} nodes differ from the host cut"
                    tsum = float(np.abs(rpay[..., 0]).astype(np.float64).sum())
                    assert abs(dev_f[i] - host_f[i]) <= 1e-6 * tsum + 1e-5 * abs(host_f[i]) + 1e-5, (mode, name, i, dev_f[i], host_f[i])
                    if n <= 16:
                        p5 = np.ascontiguousarray(rpay.reshape(-1, 5))
                        assert abs(pc._cut_capacity(p5, w, h, src) - enumerated_minimum(p5, w, h)) <= 1e-9 * max(1.0, tsum), (mode, name, i)
                        enumerated += 1
                b.destroy()
    finally:
        d.close()
    assert enumerated == 2 * 7
    return enumerated


# ------------------------------------------------------------------------------------------------ 5 / 6. apply; flow and energy
def case_apply_and_energy(lib):
    """The host solver's masks of the device payloads applied from the label map: labels == where(mask, L1, L0) and cur == where(mask, prop, cur)
    bit for bit, pixels outside every cell untouched; then the host solver's flow + flow0 against les_hip_batch_region_energy of the moved maps:
    equal within the reference's 1e-5 relative for cells without a truncated pair, flow >= energy - that tolerance for the others.
    -> (cells with count 0, cells with count > 0, pixels moved)"""
    s = scene()
    exact = bounded = moved = 0
    d = Dev(lib)
    try:
        for mode in (0, 1):
            for name in BATCHES:
                d.reset()
                b, trs, off, nn = batch_of(d, name)
                _, got, f0, cnt = fusion_graph(d, b, nn, mode)
                masks, flows = host_cut(trs, got, off, nn)
                dm, de = d.buf(nn), d.buf(8 * b.n)
                dm.upload(masks)
                b.apply_masks_labels(d.L1.ptr, dm.ptr, d.cur.ptr, d.prop.ptr, d.L0.ptr)
                b.region_energy(d.L0.ptr, d.cur.ptr, de.ptr, mode=mode, **PW)
                lab, cur = d.maps()
                energy = de.download((b.n,), np.float64)
                taken = np.zeros((IMG_H, IMG_W), bool)
                for i, (x, y, w, h) in enumerate(BATCHES[name]):
                    taken[y:y + h, x:x + w] = masks[off[i]: off[i] + w * h].reshape(h, w) != 0
                assert np.array_equal(lab.view(np.uint32), np.where(taken[..., None], s.L1, s.L0).view(np.uint32)), (mode, name)
                assert np.array_equal(cur.view(np.uint32), np.where(taken, s.prop, s.cur).view(np.uint32)), (mode, name)
                moved += int(taken.sum())
                for i in range(b.n):
                    tol = 1e-5 * max(1.0, abs(energy[i]))
                    cutv = f0[i] + flows[i]
                    if cnt[i] == 0:
                        assert abs(cutv - energy[i]) <= tol, (mode, name, i, cutv, energy[i])
                        exact += 1
                    else:
                        assert cutv >= energy[i] - tol, (mode, name, i, cutv, energy[i])
                        bounded += 1
                b.destroy()
    finally:
        d.close()
    assert exact > 0 and bounded > 0 and moved > 0
    return exact, bounded, moved


# ------------------------------------------------------------------------------------------------ 7 / 8. PMRunner.fuse, FastGCStereo.fuse on the cones crop
UNITS = (12, 40, 184)          # 36 x 36 cells (one workgroup each), 120-wide cells (tiled solver), and ONE cell: the whole 184 x 96 image
TABLE = [[(api.PROPOSE_EXPANSION, 1), (api.PROPOSE_RANSAC, 1), (api.PROPOSE_RANDOM, 7)], [(api.PROPOSE_EXPANSION, 2), (api.PROPOSE_RANSAC, 1)],
         [(api.PROPOSE_EXPANSION, 2), (api.PROPOSE_RANSAC, 1)]]
RISE = 1e-6                    # a set may raise the energy only through the float rounding of the capacities (tests/eval_cases.py: whole_run_cases)


class Cones:
    """The cones crop under the cost-volume energy (as tests/eval_cases.py: ConesRun); a and b: the labellings after init_labels and one PatchMatch
    iteration with seeds 11 and 12.  Every fusion starts from a labelling's dense costs (init_from_labels: the route of run(labeling=))."""

    def __init__(self, lib, device, device_cuts):
        from localexpstereo_amd import pm
        from tests import parity_cases as pc
        self.lib, self.device, self.device_cuts, self.pm = lib, device, device_cuts, pm
        self.imL, vol, self.gt = pc.cones_ad_volume()
        self.e = api.HipCostVolumeEnergy(self.imL, None, vol, None, windR=20, eps=1e-4, th_col=0.12, max_disp=63.0, lib=lib)
        self.g = lgc.GraphCut(self.imL, None, lambda_=1.0)
        self.params = self.g.params
        sols, runners = [], []
        for seed in (11, 12):
            r = pm.PMRunner(self.e, UNITS, TABLE, seed=seed, device=device)
            r.init_labels()
            r.iteration(0)
            r._sync()
            sols.append(r.labels.cpu().numpy().copy())
            runners.append(r)
        self.a, self.b = sols
        runners[1].close()
        self.r = runners[0]                      # every fusion below runs on this one
        self.r.device_cuts = device_cuts
        self.r.begin_gc(self.g)

    def start(self, labels):
        """The runner at `labels` with their dense costs, the inner-loop log armed -> (energy, cost map)."""
        r = self.r
        r.init_from_labels(labels)
        if r.inner_log is not None:
            r.inner_log.evaluator.close()
        r.inner_log = SimpleNamespace(evaluator=api.DeviceEvaluator(self.e, max_rows=len(r.sets) + 1), params=self.params, meta=[])
        r.inner_iteration = 0
        data, smooth = r.energy(self.params)
        return data + smooth, r.cur.cpu().numpy().copy()

    def fuse(self, labels_b, layers=None):
        """-> (stats, fused labels, cur, prop, energies after every set)"""
        r = self.r
        st = r.fuse(labels_b, layers=layers)
        rows = r.inner_log.evaluator.rows()
        return st, r.labels.cpu().numpy().copy(), r.cur.cpu().numpy().copy(), r.prop.cpu().numpy().copy(), [row["energy"] for row in rows]

    def close(self):
        if self.r.inner_log is not None:
            self.r.inner_log.evaluator.close()
        self.r.close(); self.e.close(); self.g.close()


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


def case_runner_fuse(lib, device, device_cuts):
    from localexpstereo_amd import stereo
    c = Cones(lib, device, device_cuts)
    out = {}
    try:
        a, b = c.a, c.b
        assert not _same(a, b)
        # E(a), E(b): each labelling with its own dense costs
        E_b, _ = c.start(b)
        E_a, cur_a = c.start(a)
        layers = [0, 1]
        st, fused, cur, prop_b, energies = c.fuse(b, layers)
        from_a, from_b = (fused.view(np.uint32) == a.view(np.uint32)).all(-1), (fused.view(np.uint32) == b.view(np.uint32)).all(-1)
        assert (from_a | from_b).all()
        taken = ~from_a
        assert taken.any() and (~from_b).any()                               # both occur
        assert _same(cur, np.where(taken, prop_b, cur_a))
        assert len(energies) == sum(1 for li, _ in c.r.sets if li in layers) and st["cells"] == sum(sh.n for li, sh in c.r.sets if li in layers) and st["pixels_taken"] >= int(taken.sum())
        assert 0 < st["nonsubmodular_pairs"] < st["pairs"]
        rises = np.diff([E_a] + energies)
        assert rises.max() <= RISE * abs(E_a), (rises.max(), E_a)
        E_ab = energies[-1]
        assert E_ab <= E_a + RISE * abs(E_a) and E_ab < E_a, (E_ab, E_a)
        out.update(E_a=E_a, E_b=E_b, E_ab=E_ab, worst_rise=float(rises.max()), taken=int(taken.sum()), nonsubmodular_share=st["nonsubmodular_pairs"] / st["pairs"])
        # the other way round
        c.start(b)
        _, fused_ba, _, _, energies = c.fuse(a, layers)
        assert np.diff([E_b] + energies).max() <= RISE * abs(E_b) and energies[-1] <= E_b + RISE * abs(E_b), (energies[-1], E_b)
        out["E_ba"] = energies[-1]
        # a labelling fused with itself: nothing moves
        c.start(a)
        st_aa, fused_aa, cur_aa, _, energies = c.fuse(a, layers)
        assert _same(fused_aa, a) and _same(cur_aa, cur_a) and st_aa["nonsubmodular_pairs"] == 0
        # one cell, the whole image: at or below both inputs
        c.start(a)
        st1, fused1, _, _, energies = c.fuse(b, [2])
        assert st1["cells"] == 1 and int(c.r.sets[-1][1].regions[0]["w"]) == c.r.W and int(c.r.sets[-1][1].regions[0]["h"]) == c.r.H
        assert energies[-1] <= min(E_a, E_b) + RISE * abs(min(E_a, E_b)), (energies[-1], E_a, E_b)
        out["E_one_cell"] = energies[-1]
        # several ranks: refused
        r2 = c.pm.PMRunner(c.e, (40,), TABLE[:1], seed=1, rank=0, world=2, device=device)
        try:
            r2.fuse(b)
            raise AssertionError("world = 2 was accepted")
        except NotImplementedError:
            pass
        finally:
            r2.close()
        # 8. the driver: the same labelling as the runner-level calls
        st8 = stereo.FastGCStereo(c.e, c.imL, None, dict(lambda_=1.0), device=device, seed=3, device_cuts=device_cuts, evaluate_on_device=True)
        st8.setEvaluator(ec.lio.Evaluator(c.gt, c.gt > 0, 1.0), precision=0.25)
        for u, t in zip(UNITS[:2], TABLE):
            st8.addLayer(u, t)
        got = st8.fuse(a, [b])
        assert _same(got, fused)
        assert [r["index"] for r in st8.log] == [0, 1] and ec.same_float(st8.log[0]["energy"], E_a) and ec.same_float(st8.log[1]["energy"], E_ab)
        assert len(st8.fuse_stats) == 1 and st8.fuse_stats[0]["pixels_taken"] == st["pixels_taken"]
    finally:
        c.close()
    return out
