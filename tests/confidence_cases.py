"""Cases of tests/test_confidence.py: the confidence of a label map under the aggregated cost volume (csrc/les_confidence.h: les_hip_slab_confidence,
les_hip_slab_confidence_finish, les_hip_confidence; les_hip_post_process_masked; stereo.FastGCStereo(confidence=, min_confidence=); io.sparsification)
on the CPU simulator build and on the MI355X.

The definition, restated from csrc/les_confidence.h.  A pixel has costs c_0 ... c_{K-1}, one per slab; slab k belongs to disparity d0 + k.  Its label
(a, b, c, v) gives d = (a x + b y) + c, un-fused, and u = d - d0.  Slab k is in band iff |float(k) - u| <= band (a NaN u never is).  From own = rival =
+inf, k_r = -1, for k = 0 ... K-1: in band, c_k < own takes own = c_k; else c_k < rival takes rival = c_k, k_r = k (NaN and +inf never win, the
lowest k wins ties, -0 = +0).  conf = 0 when own is still +inf; else 1 when k_r < 0; else m = (rival - own) / scale and conf = m clamped to [0, 1]
with a NaN m giving 0.  All in f32.

References, none of them the code under test: the vectorised numpy restatement below (np.argmin over the masked slabs with NaN read as +inf), itself
held to a literal per-pixel loop; for the whole call, the restatement applied to the slabs the project's own batch path writes
(wtavol_cases.batch_slabs) on the same context; for les_hip_post_process_masked, the entries that exist already (les_hip_post_process_speckle,
les_hip_speckle_mask).  Tolerances: conf, own, rival and k_r are compared as bytes everywhere; label maps as bytes.

The ranking condition (case_ranks_errors) is the issue's: on the cones crop, one-view wta, bad-1.0 over the valid ground truth,
sparsification(...)["auc"] <= 0.5 ["bad"], for the restatement on the project's slabs and for the device's map.

The simulator legs of the driver cases run with crossview_cases.sim_layers and a filter radius of 6, as the cross-view cases do and for their
reason; the drivers run on the cones crop (crossview_cases.cones_data: 96 x 184, image-based energy, ground truth present)."""
import functools

import numpy as np

from localexpstereo_amd import api, synth
from localexpstereo_amd import io as lio
from tests import crossview_cases as cv
from tests import post_cases as pcs
from tests import speckle_cases as sk
from tests import wtavol_cases as wv

F = np.float32
SHAPES = wv.SHAPES                               # (5, 7): a 3-pixel tail; (33, 130): every other slab unaligned; (48, 64): the all-vector kernel
KS = wv.KS                                       # (1, 2, 3, 5, 9)
BANDS = (F(0.5), F(1.0), F(2.0))
D0 = wv.D0                                       # 3.0
SCALE = F(0.75)                                  # of the reduction cases: base costs lie in [2, 3], planted minima at 1 (a margin above the scale) and 1.25
chunkings = wv.chunkings
same = wv.same


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def own_disparity(labels):
    """d = (a x + b y) + c in f32, un-fused (every product and sum rounded)."""
    labels = np.asarray(labels, F)
    H, W = labels.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    with np.errstate(all="ignore"):
        return ((labels[..., 0] * xs).astype(F) + (labels[..., 1] * ys).astype(F)).astype(F) + labels[..., 2]


def conf_restate(slabs, labels, d0, band, scale):
    """slabs [K][H][W] f32, labels H x W x 4 -> (conf, own, rival: H x W f32, k_r: H x W int32)"""
    slabs = np.asarray(slabs, F)
    K = slabs.shape[0]
    with np.errstate(all="ignore"):
        u = (own_disparity(labels) - F(d0)).astype(F)
        inband = np.abs((np.arange(K, dtype=F)[:, None, None] - u[None]).astype(F)) <= F(band)        # NaN: False
        c = np.where(np.isnan(slabs), F(np.inf), slabs)
        first = lambda a: np.take_along_axis(a, np.argmin(a, axis=0)[None], 0)[0]                     # the FIRST of the minima (its own sign of zero)
        own = first(np.where(inband, c, F(np.inf)))
        cr = np.where(inband, F(np.inf), c)
        kr = np.argmin(cr, axis=0)
        rival = np.take_along_axis(cr, kr[None], 0)[0]
        kr = np.where(rival == np.inf, -1, kr).astype(np.int32)
        m = ((rival - own).astype(F) / F(scale)).astype(F)
        conf = np.where(own == np.inf, F(0), np.where(kr < 0, F(1), np.where(m > 0, np.where(m < 1, m, F(1)), F(0)))).astype(F)
    return conf, own.astype(F), rival.astype(F), kr


def conf_loop(slabs, labels, d0, band, scale):
    """The same by a literal per-pixel transcription of the definition (scalar f32 operations)."""
    K, H, W = slabs.shape
    conf, own_, rival_, kr_ = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), np.int32)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                a, b, c, _ = (F(t) for t in labels[y, x])
                u = F(F(F(a * F(x)) + F(b * F(y))) + c) - F(d0)
                own, rival, kr = F(np.inf), F(np.inf), -1
                for k in range(K):
                    ck = slabs[k, y, x]
                    if abs(F(F(k) - u)) <= F(band):
                        if ck < own:
                            own = ck
                    elif ck < rival:
                        rival, kr = ck, k
                if not own < np.inf:
                    cf = F(0)
                elif kr < 0:
                    cf = F(1)
                else:
                    m = F(F(rival - own) / F(scale))
                    cf = (m if m < 1 else F(1)) if m > 0 else F(0)
                conf[y, x], own_[y, x], rival_[y, x], kr_[y, x] = cf, own, rival, kr
    return conf, own_, rival_, kr_


# ------------------------------------------------------------------------------------------------ populations
def specials(K, rng):
    """The special pixels of a K-slab volume -> [(name, u or a whole label, costs[K])]; a scalar u stands for the fronto-parallel label
    (0, 0, D0 + u, 0)."""
    out = []
    base = lambda: rng.uniform(2.0, 3.0, K).astype(F)
    for j in wv.positions(K):
        c = base(); c[j] = F(1.0)
        out.append((f"u integer {j}, minimum on it", F(j), c))
        if j + 1 < K:
            c = base(); c[j + 1] = F(1.0)
            out.append((f"u integer {j}, minimum on the band-1 edge above", F(j), c))
            c = base(); c[j] = c[j + 1] = F(1.0)
            out.append((f"u half-integer {j}.5", F(j) + F(0.5), c))
            c = base(); c[j], c[j + 1] = F(0.0), F(-0.0)
            out.append((f"own +0 on slab {j} before -0", F(j), c + F(0)))
            c = base(); c[j], c[j + 1] = F(-0.0), F(0.0)
            out.append((f"own -0 on slab {j} before +0", F(j), c))
        c = base(); c[j] = F(np.nan)
        out.append((f"NaN cost on the label's slab {j}", F(j), c))
        c = base(); c[j] = F(np.inf)
        out.append((f"+inf cost on the label's slab {j}", F(j), c))
        c = base(); c[max(j - 2, 0):j + 3] = F(np.nan)
        out.append((f"all NaN within 2 of slab {j}", F(j), c))
        c = base(); c[max(j - 1, 0):j + 2] = F(np.inf)
        out.append((f"all +inf within 1 of slab {j}", F(j), c))
    # rivals: the label sits on slab 0, the far slabs hold what is asked for
    if K >= 4:
        c = base(); c[0] = F(1.0); c[K - 1] = c[K - 2] = F(1.25)
        out.append(("tied rival on the last two slabs", F(0), c))
        c = base(); c[0] = F(1.0); c[K - 2], c[K - 1] = F(0.0), F(-0.0)
        out.append(("rival +0 before -0", F(0), c))
        c = base(); c[0] = F(1.0); c[K - 2], c[K - 1] = F(-0.0), F(0.0)
        out.append(("rival -0 before +0", F(0), c))
        c = base(); c[K - 1] = F(1.0)
        out.append(("own above the rival", F(0), c))
        c = base(); c[0] = F(1.0); c[K - 1] = F(1.25)
        out.append(("margin 0.25 below the scale", F(0), c))
        c = base(); c[0] = F(1.0); c[K - 1] = F(np.nan); c[K - 2] = F(np.inf)
        out.append(("NaN and +inf outside the band", F(0), c))
        c = base(); c[0] = F(1.0); c[3:] = F(np.nan)
        out.append(("only NaN beyond slab 2", F(0), c))
        c = base(); c[0] = c[K - 1] = F(-np.inf)
        out.append(("own and rival -inf", F(0), c))
    out.append(("u -2.5, below every band", F(-2.5), base()))
    out.append((f"u {K - 1} + 2.5, above every band", F(K - 1) + F(2.5), base()))
    c = base(); c[0] = F(1.0)
    out.append(("u -2, on the band-2 edge of slab 0", F(-2.0), c))
    for name, val in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        out.append((f"{name} label", F(val), base()))
    out.append(("NaN slope", np.array([np.nan, 0, D0, 0], F), base()))
    out.append(("all NaN", F(0), np.full(K, np.nan, F)))
    out.append(("all +inf", F(0), np.full(K, np.inf, F)))
    out.append(("constant", F(K // 2), np.full(K, 1.5, F)))
    return out


@functools.lru_cache(maxsize=None)
def volumes(shape, K):
    """Every (slabs [K][H][W], labels H x W x 4, where) of a shape and K, as many as the shape needs to hold all specials on at most every second
    pixel; where = [(y, x, name)].  Computed once, shared, left unchanged.  The background: random costs on a 1 / 8 grid (ties happen by chance),
    random slanted planes whose own disparities spread from 2.5 slabs below the volume to 2.5 above it."""
    H, W = shape
    rng = np.random.default_rng(7000 * K + W)
    sp = specials(K, rng)
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    out, k = [], 0
    while k < len(sp):
        slabs = (rng.integers(8, 64, (K, H, W)) / 8.0).astype(F)
        labels = np.zeros((H, W, 4), F)
        labels[..., 0], labels[..., 1] = rng.uniform(-0.3, 0.3, (H, W)), rng.uniform(-0.3, 0.3, (H, W))
        labels[..., 2] = (D0 + rng.uniform(-2.5, K + 1.5, (H, W))).astype(F) - labels[..., 0] * xs - labels[..., 1] * ys
        labels[..., 3] = rng.uniform(-1, 1, (H, W))
        where = []
        for p in rng.permutation(H * W)[: max(1, (H * W) // 2)]:
            if k == len(sp):
                break
            y, x = divmod(int(p), W)
            name, u, c = sp[k]
            slabs[:, y, x] = c
            labels[y, x] = u if np.ndim(u) else (0, 0, D0 + u, 0)
            where.append((y, x, name))
            k += 1
        # every volume holds a slanted plane whose a x + b y rounds differently fused and un-fused (by chance on the larger shapes; drawn until it
        # does on a free pixel of the small one)
        taken = {(y, x) for y, x, _ in where}
        y, x = next((y, x) for y in range(H - 1, 0, -1) for x in range(W - 1, 2, -1) if (y, x) not in taken and x & (x - 1))      # (a x is inexact)
        while not fused_differs(labels).any():
            labels[y, x, :2] = rng.uniform(-0.3, 0.3, 2)
        slabs.setflags(write=False); labels.setflags(write=False)
        out.append((slabs, labels, where))
    return out


@functools.lru_cache(maxsize=None)
def restated(shape, K, band):
    return [conf_restate(slabs, labels, D0, band, SCALE) for slabs, labels, _ in volumes(shape, K)]


# ------------------------------------------------------------------------------------------------ the restatement itself (CPU only)
def case_restatement_matches_loop():
    n = 0
    for shape in SHAPES[:1] + ((6, 10),):
        for K in KS:
            for band in BANDS + (F(0.0),):
                for slabs, labels, _ in volumes(shape, K):
                    a, b = conf_restate(slabs, labels, D0, band, SCALE), conf_loop(slabs, labels, D0, band, SCALE)
                    assert all(same(p, q) for p, q in zip(a, b)), (shape, K, float(band))
                    n += 1
    return n


def fused_differs(labels):
    """Pixels whose a x + b y rounds differently with the first product fused into the sum (fma(a, x, b y), in float64: the product a x is exact
    there) than un-fused."""
    H, W = labels.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    a, b = labels[..., 0], labels[..., 1]
    with np.errstate(all="ignore"):
        unfused = ((a * xs).astype(F) + (b * ys).astype(F)).astype(F)
        fused = (a.astype(np.float64) * xs + (b * ys).astype(F).astype(np.float64)).astype(F)
        return np.isfinite(unfused) & (unfused != fused)


def case_populations_hold_what_the_cases_need():
    """Every special case really occurs at every K that can hold it, and the restatement gives it what the issue's list says it must."""
    n = 0
    for shape in SHAPES:
        for K in KS:
            names, fused, partial = set(), 0, 0
            for band in BANDS:
                for (slabs, labels, where), (conf, own, rival, kr) in zip(volumes(shape, K), restated(shape, K, band)):
                    assert ((conf >= 0) & (conf <= 1)).all()
                    u = own_disparity(labels) - D0
                    with np.errstate(invalid="ignore"):
                        nband = (np.abs(np.arange(K, dtype=F)[:, None, None] - u[None]) <= band).sum(0)
                    fused += int(fused_differs(labels).sum())
                    partial += int(((conf > 0) & (conf < 1)).sum())
                    for y, x, name in where:
                        names.add(name)
                        cf, o, r, k = conf[y, x], own[y, x], rival[y, x], kr[y, x]
                        inside = lambda j, w: len(range(max(j - w, 0), min(j + w, K - 1) + 1))
                        if name.startswith("u integer") and name.endswith("minimum on it"):
                            j = int(name.split()[2].rstrip(","))
                            assert nband[y, x] == inside(j, int(band)) and o == 1, (shape, K, band, name)         # band 1: three slices (where they exist)
                            assert cf == 1                                                                       # a margin above the scale, or no rival at all
                            if nband[y, x] == K:
                                assert k == -1 and r == np.inf                                                   # the band covers every slab
                        if name.endswith("band-1 edge above"):
                            assert (o == 1) == (band >= 1) and (k == int(name.split()[2].rstrip(",")) + 1) == (band < 1), (shape, K, band, name)
                        if name.startswith("u half-integer"):                                                    # band 0.5: both slices sit ON the edge
                            assert o == 1 and (nband[y, x] == 2 if band < 1.5 else nband[y, x] >= 2), (shape, K, band, name)
                        if name.startswith("own +0") or name.startswith("own -0"):
                            assert o == 0 and np.signbit(o) == name.startswith("own -0"), (shape, K, band, name)
                        if name.startswith("rival +0") or name.startswith("rival -0"):
                            if K - 2 > band:
                                assert r == 0 and np.signbit(r) == name.startswith("rival -0") and k == K - 2 and cf == 0, (shape, K, band, name)
                        if name == "tied rival on the last two slabs" and K - 2 > band:
                            assert k == K - 2 and r == F(1.25) and cf == F(F(0.25) / SCALE)
                        if name == "own above the rival" and K - 1 > band:
                            assert o > r and cf == 0
                        if name == "margin 0.25 below the scale" and K - 1 > band:
                            assert 0 < cf < 1
                        if name == "own and rival -inf" and K - 1 > band:
                            assert o == -np.inf and r == -np.inf and cf == 0                                     # a NaN margin
                        if name.startswith(("u -2.5", "NaN label", "+inf label", "-inf label", "NaN slope")) or name in ("all NaN", "all +inf") or "above every band" in name:
                            assert cf == 0 and o == np.inf, (shape, K, band, name)
                        if name.startswith("u -2,"):
                            assert (cf > 0) == (band >= 2) and nband[y, x] == (1 if band >= 2 else 0)
                        if name.startswith("all NaN within 2"):
                            assert cf == 0 and o == np.inf
                        if name.startswith("all +inf within 1"):
                            assert band >= 2 or (cf == 0 and o == np.inf), (shape, K, band, name)
                        if name.startswith(("NaN cost on", "+inf cost on")) and band < 1:
                            assert cf == 0 and o == np.inf
                        if name == "constant":
                            assert cf == (1 if nband[y, x] == K else 0)
                        n += 1
            want = {nm for nm, *_ in specials(K, np.random.default_rng(0))}
            assert names == want, (shape, K, want - names)
            assert fused > 0, (shape, K, "no pixel whose a x + b y rounds differently fused and un-fused")
            assert partial > 0 or K == 1, (shape, K, "no confidence strictly between 0 and 1")
            if K <= 3:                                             # band 2 covers every slab of a label on slab 1 (slab 0 for K = 1)
                conf, _, _, kr = restated(shape, K, BANDS[2])[0]
                assert ((conf == 1) & (kr < 0)).any()
    return n


# ------------------------------------------------------------------------------------------------ device harness
class Dev:
    """An energy context of the shape (image-based cost, no aggregation: any image size; min_disparity D0) and device buffers for the labels, the
    slabs of one volume, the state and the four outputs."""

    def __init__(self, lib, H, W, kmax):
        im = np.zeros((H, W, 3), np.uint8)
        self.e = api.HipCostVolumeEnergy.naive(im, im, windR=0, max_disp=63.0, min_disp=float(D0), lib=lib, filter="")
        self.H, self.W, P = H, W, H * W
        assert self.e.slab_confidence_state_bytes() >= 16 * P
        self.slabs = api.DeviceBuffer(self.e, kmax * P * 4 + 16)
        self.state = api.DeviceBuffer(self.e, self.e.slab_confidence_state_bytes())
        self.labels = api.DeviceBuffer(self.e, P * 16)
        self.out = [api.DeviceBuffer(self.e, P * 4) for _ in range(4)]

    def feed(self, slabs, labels, chunk, band, offset_floats=0):
        """The step calls of one volume in chunks of `chunk` slabs (the state is filled with a guard byte first: k_first = 0 must initialise it;
        after the first chunk the label map is overwritten: it is read only then)."""
        K, P = slabs.shape[0], self.H * self.W
        base = self.slabs.ptr + 4 * offset_floats
        self.e._chk(self.e.L.les_hip_memcpy_h2d(self.e.h, api.C.c_void_p(base), api._ptr(np.ascontiguousarray(slabs)), slabs.nbytes))
        self.labels.upload(labels)
        self.state.fill(0x5A)
        for k0 in range(0, K, chunk):
            self.e.slab_confidence(self.labels.ptr if k0 == 0 else None, base + 4 * k0 * P, min(chunk, K - k0), k0, band, self.state.ptr)
            if k0 == 0:
                self.e.synchronize()
                self.labels.fill(0x5A)

    def finish(self, scale, parts=True):
        for b in self.out:
            b.fill(0x5A)
        self.e.slab_confidence_finish(self.state.ptr, scale, self.out[0].ptr, *(b.ptr if parts else None for b in self.out[1:]))
        self.e.synchronize()
        return tuple(b.download((self.H, self.W), dt) for b, dt in zip(self.out, (F, F, F, np.int32)))

    def close(self):
        for b in [self.slabs, self.state, self.labels] + self.out:
            b.free()
        self.e.close()


NAMES = ("conf", "own", "rival", "k_r")


def describe(got, want):
    for g, w, name in zip(got, want, NAMES):
        diff = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        if diff.any():
            y, x = np.argwhere(diff)[0]
            return f"{name}: {int(diff.sum())} pixels differ from the restatement, first at ({y}, {x}): {g[y, x]!r} against {w[y, x]!r}"
    return ""


# ------------------------------------------------------------------------------------------------ 1. kernels against the restatement, chunk independence
def case_kernel_bit_for_bit(lib, shape):
    """Every volume of the shape, K, band and chunking against the restatement, the four outputs as bits; all chunkings of one input give identical
    bits (also asserted directly); a slab base 4 bytes off the 16-byte grid gives the same; NULL optional outputs leave conf as it is."""
    H, W = shape
    d = Dev(lib, H, W, max(KS))
    n = 0
    try:
        for K in KS:
            for vi, (slabs, labels, _) in enumerate(volumes(shape, K)):
                for band in BANDS:
                    want = restated(shape, K, band)[vi]
                    first = None
                    for chunk in chunkings(K):
                        d.feed(slabs, labels, chunk, band)
                        got = d.finish(SCALE)
                        msg = describe(got, want)
                        assert not msg, f"{H}x{W}, K {K}, volume {vi}, band {band}, chunks of {chunk}: {msg}"
                        if first is not None:
                            assert all(same(g, f) for g, f in zip(got, first)), (shape, K, chunk, "chunk independence")
                        first = first or got
                        n += 1
                    d.feed(slabs, labels, 2, band, offset_floats=1)
                    got = d.finish(SCALE, parts=False)
                    assert same(got[0], first[0]), (shape, K, "unaligned slabs")
                    assert all((np.ascontiguousarray(g).view(np.uint8) == 0x5A).all() for g in got[1:]), "a NULL output was written"
    finally:
        d.close()
    return n


# ------------------------------------------------------------------------------------------------ 2. the whole call
def contexts(lib):
    """name -> (energy, views): the 64 x 48 x 16 synthetic volumes of the golden fixtures under the guided filter with windR 20 and min_disp 3, both
    views; a bilateral context over the same volumes; a cones crop with the image-based energy (16 disparities, radius 6), both views."""
    H, W, D = 48, 64, 16
    gl, gr = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    vl, vr = synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43)
    imL, imR, _ = wv.ec.cones_images()
    imL, imR = np.ascontiguousarray(imL[20:60, 64:134]), np.ascontiguousarray(imR[20:60, 64:134])
    yield "synthetic volume, guided filter, min_disp 3", api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=20, th_col=0.5, min_disp=3.0, lib=lib), (0, 1)
    yield "synthetic volume, bilateral", api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=4, eps=10.0, th_col=0.5, lib=lib, filter="BF"), (0, 1)
    yield "cones crop, image-based", api.HipCostVolumeEnergy.naive(imL, imR, windR=12, max_disp=15.0, lib=lib), (0, 1)


def mixed_labels(e, wta, seed):
    """A label map that exercises the whole call: the view's own WTA labels on every other row, random slanted planes from 2 slabs below the
    volume to 2 above it elsewhere."""
    rng = np.random.default_rng(seed)
    H, W, K = e.H, e.W, e.num_fronto_planes
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    lab = np.zeros((H, W, 4), F)
    lab[..., 0], lab[..., 1] = rng.uniform(-0.2, 0.2, (H, W)), rng.uniform(-0.2, 0.2, (H, W))
    lab[..., 2] = (F(e.params.min_disparity) + rng.uniform(-2.0, K + 1.0, (H, W))).astype(F) - lab[..., 0] * xs - lab[..., 1] * ys
    lab[::2] = wta[::2]
    return lab


def raw_scale_by_hand(e, name):
    """The default scale worked out from how include/localexp_hip.h states the raw cost: the volume energy truncates its costs at th_col; the
    image-based cost is (1 - alpha) min(|dI|, th_col) + alpha min(|dG|, th_grad) with the defaults alpha 0.9, th_col 10, th_grad 2."""
    return F(F(1 - F(0.9)) * F(10.0) + F(0.9) * F(2.0)) if "image-based" in name else F(0.5)


def case_whole_call(lib, device):
    import torch
    out = {}
    for name, e, views in contexts(lib):
        try:
            assert e.raw_cost_max() == raw_scale_by_hand(e, name), (name, e.raw_cost_max())
            K, d0 = e.num_fronto_planes, e.params.min_disparity
            assert K == (13 if "min_disp 3" in name else 16)
            for m in views:
                slabs = wv.batch_slabs(e, m)
                assert np.isfinite(slabs).all()
                w_lab, w_cost = (t.cpu().numpy() for t in e.wta_labels(m, device=device))
                lab = mixed_labels(e, w_lab, 5 + m)
                t_lab = torch.from_numpy(lab.copy()).to(device)
                got_by_chunk = {}
                for chunk, band in ((0, 1.0), (5, 1.0), (1, 0.5), (K, 2.0)):
                    want = conf_restate(slabs, lab, d0, band, e.raw_cost_max())
                    got = tuple(t.cpu().numpy() for t in e.confidence(t_lab, mode=m, band=band, chunk=chunk, parts=True, device=device))
                    e.synchronize()
                    msg = describe(got, want)
                    assert not msg, f"{name}, view {m}, chunk {chunk}, band {band}: {msg}"
                    got_by_chunk[(chunk, band)] = got
                assert all(same(a, b) for a, b in zip(got_by_chunk[(0, 1.0)], got_by_chunk[(5, 1.0)])), "two chunk values differ"
                # the form without parts, from a host array, with a scale of the caller's
                c2 = e.confidence(lab, mode=m, scale=0.25, device=device).cpu().numpy()
                assert same(c2, conf_restate(slabs, lab, d0, 1.0, 0.25)[0])
                # the two calls share a workspace: neither changes what the other returns
                w2 = tuple(t.cpu().numpy() for t in e.wta_labels(m, device=device))
                assert same(w2[0], w_lab) and same(w2[1], w_cost), "wta_labels differs after a confidence call"
                c3 = tuple(t.cpu().numpy() for t in e.confidence(t_lab, mode=m, parts=True, device=device))
                assert all(same(a, b) for a, b in zip(c3, got_by_chunk[(0, 1.0)])), "confidence differs after a wta_labels call"
                assert same(t_lab.cpu().numpy(), lab), "the labels were written"
                conf = got_by_chunk[(0, 1.0)][0]
                on_wta = conf[::2]
                out[f"{name}, view {m}"] = dict(mean_conf_wta_rows=float(on_wta.mean()), mean_conf_random_rows=float(conf[1::2].mean()),
                                                zero=int((conf == 0).sum()), one=int((conf == 1).sum()))
                assert (conf > 0).any() and (conf == 0).any()
                # a WTA label is the arg-min of the whole curve: its in-band minimum is the curve's, so own <= rival wherever a rival exists
                o, r, k = (a[::2] for a in got_by_chunk[(0, 1.0)][1:])
                assert (o[k >= 0] <= r[k >= 0]).all() and same(o, w_cost[::2]), name
        finally:
            e.close()
    return out


def _refused(call):
    try:
        call()
    except api.LesHipError as ex:
        assert f"error {api.LES_HIP_ERR_ARG}" in str(ex), str(ex)
        return 1
    raise AssertionError("a bad argument was accepted")


def case_argument_errors(lib, device):
    """Every refusal of les_hip_confidence and of the two reduction entries returns LES_HIP_ERR_ARG and leaves the outputs untouched."""
    H, W, D = 48, 64, 16
    gl, vl = synth.make_guide(H, W, 1234), synth.make_volume(D, H, W, 42)
    P, n = H * W, 0
    nan, inf = float("nan"), float("inf")
    for kw, bad_range in ((dict(), False), (dict(max_disp=2.0, min_disp=3.0), True)):
        e = api.HipCostVolumeEnergy(gl, None, vl, None, windR=20, th_col=0.5, lib=lib, **kw)           # the left view only
        lab, state = api.DeviceBuffer(e, P * 16), api.DeviceBuffer(e, e.slab_confidence_state_bytes())
        outs = [api.DeviceBuffer(e, P * 4) for _ in range(4)]
        try:
            lab.upload(np.zeros((H, W, 4), F))
            for b in outs + [state]:
                b.fill(0x5A)
            o = [b.ptr for b in outs]
            if bad_range:
                n += _refused(lambda: e.confidence_ptr(0, lab.ptr, 0, 1.0, 0.5, *o))
                n += _refused(lambda: e.wta_labels(0, 0, True, lab.ptr, o[0]))                           # the range les_hip_wta_labels refuses
            else:
                for args in ((0, 0, 0, 1.0, 0.5, *o), (0, lab.ptr, 0, 1.0, 0.5, 0, *o[1:]), (1, lab.ptr, 0, 1.0, 0.5, *o), (2, lab.ptr, 0, 1.0, 0.5, *o),
                             (-1, lab.ptr, 0, 1.0, 0.5, *o), (0, lab.ptr, 0, -0.5, 0.5, *o), (0, lab.ptr, 0, nan, 0.5, *o), (0, lab.ptr, 0, 1.0, 0.0, *o),
                             (0, lab.ptr, 0, 1.0, -1.0, *o), (0, lab.ptr, 0, 1.0, nan, *o), (0, lab.ptr, 0, 1.0, inf, *o)):
                    n += _refused(lambda: e.confidence_ptr(*args))
                for fn in (lambda: e.slab_confidence(0, o[1], 1, 0, 1.0, state.ptr), lambda: e.slab_confidence(lab.ptr, 0, 1, 0, 1.0, state.ptr),
                           lambda: e.slab_confidence(lab.ptr, o[1], 1, 0, 1.0, 0), lambda: e.slab_confidence(lab.ptr, o[1], -1, 0, 1.0, state.ptr),
                           lambda: e.slab_confidence(lab.ptr, o[1], 1, -1, 1.0, state.ptr), lambda: e.slab_confidence(lab.ptr, o[1], 1, 0, -1.0, state.ptr),
                           lambda: e.slab_confidence(lab.ptr, o[1], 1, 0, nan, state.ptr), lambda: e.slab_confidence(lab.ptr, o[1], 1, 0, 1.0, state.ptr + 4),
                           lambda: e.slab_confidence_finish(0, 0.5, *o), lambda: e.slab_confidence_finish(state.ptr, 0.5, 0, *o[1:]),
                           lambda: e.slab_confidence_finish(state.ptr, 0.0, *o), lambda: e.slab_confidence_finish(state.ptr, nan, *o),
                           lambda: e.slab_confidence_finish(state.ptr, inf, *o)):
                    n += _refused(fn)
            e.synchronize()
            for b in outs:
                assert (b.download((P * 4,), np.uint8) == 0x5A).all(), "a refused call wrote an output"
            assert (state.download((state.nbytes,), np.uint8) == 0x5A).all(), "a refused call wrote the state"
            assert not lab.download((P * 16,), np.uint8).any()
        finally:
            for b in outs + [lab, state]:
                b.free()
            e.close()
    return n


# ------------------------------------------------------------------------------------------------ 3. les_hip_post_process_masked
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case_post_masked(lib, views):
    """Held against existing entries only, on the island scene of speckle_cases (its islands agree across the views: only a mask finds them).
    (a) fail=(None, None) and all-zero masks equal les_hip_post_process_speckle; (b) the caller's masks set to speckle_mask(labels, s, t) with
    max_size 0 equal les_hip_post_process_speckle(..., s, t) without a caller's mask.  views (0, 1): the two-view form; (0,) / (1,): the one-view
    forms.  All as bytes."""
    H, W = sk.POST_SHAPE
    thr, omega = 1.5, 10.0
    s, t = sk.POST_SPECKLE
    scene = sk.island_scene(H, W, 17)
    ims = tuple(pcs.image(H, W, q) for q in sk.RANDOM_GUIDE_SEEDS)
    labs = tuple(scene[m] if m in views else None for m in (0, 1))
    dev = sk._dev(lib)
    e = pcs.context(lib, *ims, sk.POST_WINDR)
    try:
        want = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=(s, t))
        zeros = tuple(np.zeros((H, W), np.uint8) if l is not None else None for l in labs)
        a_null = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=(s, t), fail=(None, None))
        a_zero = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=(s, t), fail=zeros)
        masks = tuple(e.speckle_mask(l, s, t, device=dev).cpu().numpy() if l is not None else None for l in labs)
        b_mask = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=(0, t), fail=masks)
        b_bool = e.post_process_host(*labs, threshold=thr, omega=omega, fail=tuple(m > 0 if m is not None else None for m in masks))
        # a mask of the absent view is ignored
        b_extra = e.post_process_host(*labs, threshold=thr, omega=omega, fail=tuple(m if m is not None else np.ones((H, W), np.uint8) for m in masks)) if len(views) == 1 else b_mask
        base = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=(0, t))
    finally:
        e.close()
    out = {}
    for m in (0, 1):
        if m not in views:
            assert all(r[m] is None for r in (want, a_null, a_zero, b_mask, b_bool, b_extra))
            continue
        for got, what in ((a_null, "NULL masks"), (a_zero, "all-zero masks"), (b_mask, "speckle masks as the caller's"), (b_bool, "without speckle="),
                          (b_extra, "a mask for the absent view")):
            assert np.array_equal(_bits(got[m]), _bits(want[m])), f"view {m}, {what}: {int((_bits(got[m]) != _bits(want[m])).any(-1).sum())} pixels differ"
        assert masks[m].any() and (_bits(want[m]) != _bits(base[m])).any(), "the masks change nothing: the case is empty"
        out[m] = dict(mask_pixels=int((masks[m] > 0).sum()), changed=int((_bits(want[m]) != _bits(labs[m])).any(-1).sum()))
    return out


# ------------------------------------------------------------------------------------------------ 4. / 5. drivers
TAU = 0.05


def driver(lib, device, **opts):
    """stereo.FastGCStereo on the cones crop (crossview_cases.cones_data: image-based energy, both views, ground truth).  The simulator leg: filter
    radius 6, crossview_cases.sim_layers, host cuts; the MI355X: MidV2's radius 20 and layers 5 / 15 / 25, device cuts."""
    from localexpstereo_amd import stereo
    data = cv.cones_data()
    sim = lib is not None
    windR = 6 if sim else 20
    e = api.HipCostVolumeEnergy.naive(data["imL"], data["imR"], windR=windR, max_disp=float(data["ndisp"] - 1), lib=lib)
    st = stereo.FastGCStereo(e, data["imL"], data["imR"], dict(lambda_=1.0, windR=windR), device=device, seed=3, device_cuts="none" if sim else "all", **opts)
    st.setEvaluator(lio.Evaluator(data["dispGT"], data["nonocc"], 1.0), precision=data["gt_prec"])
    st.concurrent_views = False
    (cv.sim_layers if sim else stereo._layers)(st, (5, 15, 25))
    return st, e, data


def case_drivers(lib, device):
    from localexpstereo_amd import stereo
    out = {}
    plain = {}
    st, e, _ = driver(lib, device)
    try:
        plain["wta"] = st.wta((0,))
        assert st.confidences == {}
        plain["run"] = st.run(1, (0, 1), 1)
        raws = dict(st.raw_labelings)
    finally:
        e.close()
    st, e, _ = driver(lib, device, confidence=True)
    try:
        # confidence=True: the same labellings, and the maps of the raw labellings
        got = st.wta((0,))
        assert same(got[0], plain["wta"][0]) and same(got[1], plain["wta"][1]) and same(got[0], got[1])
        assert sorted(st.confidences) == [0] and st.confidences[0].dtype == F and st.confidences[0].shape == (e.H, e.W)
        conf_wta = st.confidences[0]
        assert same(conf_wta, e.confidence(st.raw_labelings[0], mode=0, device=device).cpu().numpy())
        assert same(conf_wta, st.confidence(st.raw_labelings[0]))
        parts = st.confidence(st.raw_labelings[0], viewMode=0, parts=True, band=2.0)
        assert len(parts) == 4 and parts[3].dtype == np.int32 and not same(parts[0], conf_wta)
        got = st.run(1, (0, 1), 1)
        assert same(got[0], plain["run"][0]) and same(got[1], plain["run"][1]) and sorted(st.confidences) == [0, 1]
        for m in (0, 1):
            assert same(st.raw_labelings[m], raws[m])
            assert same(st.confidences[m], e.confidence(st.raw_labelings[m], mode=m, device=device).cpu().numpy()), m
        out.update(wta_mean_conf=float(conf_wta.mean()), run_mean_conf=float(st.confidences[0].mean()))
        # min_confidence: the one-view result by hand
        st2 = stereo.FastGCStereo(e, st.imL, st.imR, dict(lambda_=1.0, windR=e.params.windR), device=device, seed=3, min_confidence=TAU)
        assert st2.with_confidence
        lab, raw = st2.wta((0,))
        assert same(raw, plain["wta"][1]) and same(st2.confidences[0], conf_wta)
        low = conf_wta < F(TAU)
        assert low.any() and not low.all()
        want = e.post_process_host(raw, None, 1.5, st2.p["omega"], fail=(low, None))[0]
        assert same(lab, want) and not same(lab, raw)
        changed = (_bits(lab) != _bits(raw)).any(-1)
        assert not changed[~low].any(), "a pixel outside the mask changed"
        # ... and with a speckle filter beside it
        st3 = stereo.FastGCStereo(e, st.imL, st.imR, dict(lambda_=1.0, windR=e.params.windR), device=device, seed=3, min_confidence=TAU, speckle=sk.DRIVER_SPECKLE)
        lab3, raw3 = st3.wta((0,))
        assert same(raw3, raw) and same(lab3, e.post_process_host(raw, None, 1.5, st3.p["omega"], speckle=sk.DRIVER_SPECKLE, fail=(low, None))[0])
        # two views: both masks
        lab4, raw4 = st2.wta((0, 1))
        lows = tuple(st2.confidences[m] < F(TAU) for m in (0, 1))
        want4 = e.post_process_host(st2.raw_labelings[0], st2.raw_labelings[1], 1.5, st2.p["omega"], fail=lows)
        assert same(lab4, want4[0]) and same(raw4, raw)
        assert same(st2.wta((0,), post_process=False)[0], raw)
        out.update(low_pixels=int(low.sum()), changed=int(changed.sum()))
        for tau in (0.0, -0.1, 1.5, float("nan")):
            try:
                stereo.FastGCStereo(e, st.imL, st.imR, {}, device=device, min_confidence=tau)
                raise AssertionError(f"min_confidence {tau} was accepted")
            except ValueError:
                pass
        assert stereo.FastGCStereo(e, st.imL, st.imR, {}, device=device, min_confidence=1.0).min_confidence == 1.0
        for kw in (dict(confidence=True), dict(min_confidence=TAU)):
            sw = stereo.FastGCStereo(e, st.imL, st.imR, {}, device=device, world=2, **kw)
            for fn in (lambda: sw.wta((0,)), lambda: sw.run(1, (0,), 0), lambda: sw.confidence(raw)):
                try:
                    fn()
                    raise AssertionError("world = 2 was accepted")
                except NotImplementedError:
                    pass
    finally:
        e.close()
    return out


def case_ranks_errors(lib, device):
    """The issue's condition on the measure: on the cones crop, one-view wta, bad-1.0 over the valid ground truth, auc <= 0.5 bad -- first for the
    numpy restatement applied to the project's own slabs, then for the device's map (which equals it, bit for bit)."""
    st, e, data = driver(lib, device, confidence=True)
    try:
        lab, raw = st.wta((0,))
        slabs = wv.batch_slabs(e, 0)
        ref = conf_restate(slabs, raw, e.params.min_disparity, 1.0, e.raw_cost_max())[0]
        disp = stereo_disparities(raw)
        rows = {}
        for name, conf in (("restatement", ref), ("device", st.confidences[0])):
            r = lio.sparsification(disp, data["dispGT"], conf, threshold=1.0)
            print(f"cones crop, one-view wta, {name}: auc {r['auc']:.4f}  bad {r['bad']:.4f}  auc_optimal {r['auc_optimal']:.4f}  ratio {r['auc'] / r['bad']:.3f}")
            rows[name] = r
        low = st.confidences[0] < F(TAU)
        valid = (data["dispGT"] > 0) & np.isfinite(data["dispGT"])
        bad = ~(np.abs(disp - data["dispGT"]) <= 1.0)
        print(f"conf < {TAU}: {100 * low[valid].mean():.1f} % of the valid pixels, {100 * bad[valid & low].mean():.1f} % of them bad; the rest {100 * bad[valid & ~low].mean():.1f} % bad")
        for name, r in rows.items():
            assert r["auc_optimal"] <= r["auc"] and 0 < r["bad"] < 1, (name, r)
            assert r["auc"] <= 0.5 * r["bad"], (name, r)
        assert same(ref, st.confidences[0])
        return rows
    finally:
        e.close()


def stereo_disparities(labeling):
    from localexpstereo_amd import stereo
    return stereo.disparities(labeling)


def case_sparsification():
    """io.sparsification on maps whose numbers can be worked out by hand."""
    gt = np.full((2, 5), 4.0, F)
    gt[1, 4] = 0                                                   # invalid: does not count
    disp = gt.copy()
    disp[0, 0], disp[0, 1], disp[1, 4] = 9.0, np.nan, 50.0         # two bad pixels of nine
    conf = np.linspace(1.0, 0.1, 10, dtype=F).reshape(2, 5)        # descending in scan order: the bad pixels come FIRST
    r = lio.sparsification(disp, gt, conf)
    assert abs(r["bad"] - 2 / 9) < 1e-12
    worst = np.mean([min(n, 2) / n for n in range(1, 10)])
    best = np.mean([max(0, n - 7) / n for n in range(1, 10)])
    assert abs(r["auc"] - worst) < 1e-12 and abs(r["auc_optimal"] - best) < 1e-12, r
    r2 = lio.sparsification(disp, gt, 1 - conf)
    assert abs(r2["auc"] - best) < 1e-12 and r2["auc_optimal"] == r["auc_optimal"]
    # a stable sort: equal confidences keep the scan order; a threshold; an explicit mask; no valid pixel
    r3 = lio.sparsification(disp, gt, np.zeros_like(conf))
    assert abs(r3["auc"] - worst) < 1e-12
    assert lio.sparsification(disp, gt, conf, threshold=10.0)["bad"] == 1 / 9
    valid = np.zeros((2, 5), bool); valid[1, :4] = True
    assert lio.sparsification(disp, gt, conf, valid=valid) == dict(bad=0.0, auc=0.0, auc_optimal=0.0)
    assert all(np.isnan(v) for v in lio.sparsification(disp, np.zeros_like(gt), conf).values())
    try:
        lio.sparsification(disp, gt, conf[:1])
        raise AssertionError("maps of different shapes were accepted")
    except ValueError:
        pass
    return r
