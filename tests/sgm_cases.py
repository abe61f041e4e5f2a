"""Cases of tests/test_sgm.py: semi-global matching over a view's cost volume (csrc/les_sgm.h: les_hip_sgm_labels, les_hip_sgm_workspace_bytes;
api.HipCostVolumeEnergy.sgm_labels; stereo.FastGCStereo.sgm, run(labeling="sgm" / "sgm+planes"), MidV3(init="sgm")) on the CPU simulator build and
on the MI355X.

The definition, restated from csrc/les_sgm.h.  The input is a view's volume C [K][H][W], slice k = disparity d0 + k.  Everything in f32, in this
order; min(a, b) is (b < a ? b : a) with the operands in the order written.
    C'(p,k) = C(p,k) if C(p,k) is finite and C(p,k) < th_col, else th_col
    directions r = (dx, dy): (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1); `paths` takes the first 2, 4 or 8
    one direction, q = p - r:   q outside the image: L(p,k) = C'(p,k); otherwise
        m = min_j L(q,j), then m = m + 0 (a zero minimum is +0);  t = L(q,k);  where a neighbour k - 1 / k + 1 exists: n = min(L(q,k-1), L(q,k+1))
        over those that exist, t = min(t, n + P1);  t = min(t, m + P2);  L(p,k) = C'(p,k) + (t - m)
    S = ((L_0 + L_1) + L_2) + ... in direction order
    read-out over S(p, 0..K-1): wtavol_cases.wta_restate (first minimum, parabola offset when subpixel); second output S(p,k*)

References, none of them the code under test: the vectorised numpy restatement below (a row or a column of pixels per step), itself held to a
literal per-pixel, per-disparity loop; its read-out is wtavol_cases.wta_restate.  Tolerances: labels and sums are compared bit for bit everywhere.
Quality: a cap from the issue, not a tuned threshold -- bad-1.0 of the integer-winner SGM map at the default penalties is at most half that of the
arg-min of the same truncated volume (the P1 = P2 = 0 map).

The kernel cases: the full cross product of the axes below, on the simulator and on the device, and one K = 300 case for the V = 8 kernels (CASES:
31 contexts of 6 calls each; the fibre simulator takes a few seconds for all of them).

`python -m tests.sgm_cases` prints the penalty sweep of DESIGN 3.2i (penalty_sweep below) from this restatement."""
import functools

import numpy as np

from localexpstereo_amd import api, synth
from tests import costvol_cases as cc
from tests import crossview_cases as cv
from tests import wtavol_cases as wv

F = np.float32
DIRS = ((+1, 0), (-1, 0), (0, +1), (0, -1), (+1, +1), (-1, -1), (-1, +1), (+1, -1))
SHAPES = ((1, 9), (9, 1), (5, 7), (19, 37), (40, 24))      # a single row, a single column, small, wide, tall: diagonals clip at both kinds of border
KS = (1, 2, 5, 64, 65, 130)                                # no neighbour, both edge lanes, the exact wave width, one past it, V = 4 with padding
PATHS = (2, 4, 8)
TH = F(0.5)                                                # th_col of the kernel cases
D0 = F(3.0)                                                # their min_disparity
CASES = tuple((s, K) for s in SHAPES for K in KS) + (((19, 37), 300),)     # x PATHS x subpixel inside the case; 300: the V = 8 kernels (K 257 .. 512)


def same(x, y):
    return wv.same(x, y)


def kp_of(K):
    return 64 if K <= 64 else 128 if K <= 128 else 256 if K <= 256 else 512


def penalties(th, p1=None, p2=None):
    th = F(th)
    return (F(0.16) * th if p1 is None else F(p1)), (F(1.28) * th if p2 is None else F(p2))


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def truncate(vol, th):
    vol = np.asarray(vol, F)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(vol) & (vol < F(th)), vol, F(th)).astype(F)


def _min(a, b):
    return np.where(b < a, b, a)


def _step(prev, c, p1, p2):
    """prev, c: [K][N] (N pixels whose predecessors hold prev) -> L [K][N]"""
    K = prev.shape[0]
    with np.errstate(all="ignore"):
        m = (prev.min(axis=0) + F(0)).astype(F)
        inf = np.full((1,) + prev.shape[1:], np.inf, F)
        a = np.concatenate([inf, prev[:-1]], 0)
        b = np.concatenate([prev[1:], inf], 0)
        t = prev
        if K > 1:
            t = _min(t, (_min(a, b) + p1).astype(F))
        t = _min(t, (m + p2).astype(F)[None])
        return (c + (t - m[None]).astype(F)).astype(F)


def sgm_direction(ct, dx, dy, p1, p2):
    """ct: the truncated volume [K][H][W] -> L of direction (dx, dy)"""
    K, H, W = ct.shape
    p1, p2 = F(p1), F(p2)
    L = np.empty_like(ct)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, :, x] = ct[:, :, x] if i == 0 else _step(L[:, :, x - dx], ct[:, :, x], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        if i == 0:
            L[:, y] = ct[:, y]
            continue
        if dx == 0:
            L[:, y] = _step(L[:, y - dy], ct[:, y], p1, p2)
            continue
        # a diagonal: pixel x of this row follows pixel x - dx of the row before; the pixel whose predecessor's column lies outside starts a line
        row = ct[:, y].copy()
        if W > 1:
            if dx > 0:
                row[:, 1:] = _step(L[:, y - dy, :-1], ct[:, y, 1:], p1, p2)
            else:
                row[:, :-1] = _step(L[:, y - dy, 1:], ct[:, y, :-1], p1, p2)
        L[:, y] = row
    return L


def sgm_sums(vol, th, p1, p2, paths=8):
    """-> [S after 1 direction, after 2, ... after `paths`], each [K][H][W]"""
    ct = truncate(vol, th)
    out, S = [], None
    for dx, dy in DIRS[:paths]:
        L = sgm_direction(ct, dx, dy, p1, p2)
        S = L if S is None else (S + L).astype(F)
        out.append(S)
    return out


def sgm_restate(vol, th, d0, paths, p1, p2, subpixel=True):
    """-> (labels H x W x 4, sum H x W)"""
    S = sgm_sums(vol, th, p1, p2, paths)[paths - 1]
    lab, cost, _ = wv.wta_restate(S, d0, subpixel)
    return lab, cost


def sgm_direction_loop(ct, dx, dy, p1, p2):
    """The same by a literal per-pixel, per-disparity transcription of the definition (scalar f32 operations)."""
    K, H, W = ct.shape
    p1, p2 = F(p1), F(p2)
    L = np.zeros_like(ct)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    with np.errstate(all="ignore"):
        for y in ys:
            for x in xs:
                qx, qy = x - dx, y - dy
                if not (0 <= qx < W and 0 <= qy < H):
                    L[:, y, x] = ct[:, y, x]
                    continue
                q = L[:, qy, qx]
                m = q[0]
                for j in range(1, K):
                    if q[j] < m:
                        m = q[j]
                m = F(m + F(0))
                for k in range(K):
                    t = q[k]
                    n = None
                    if k - 1 >= 0:
                        n = q[k - 1]
                    if k + 1 <= K - 1:
                        n = q[k + 1] if n is None else (q[k + 1] if q[k + 1] < n else n)
                    if n is not None:
                        u = F(n + p1)
                        t = u if u < t else t
                    u = F(m + p2)
                    t = u if u < t else t
                    L[k, y, x] = F(ct[k, y, x] + F(t - m))
    return L


# ------------------------------------------------------------------------------------------------ volumes
SPECIAL_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "th": TH, "above": 1e6, "negative": -0.75}


def special_positions(H, W, K):
    """(name, y, x, k) of the special entries: image corners, the middle, the borders, at the first, a middle and the last disparity"""
    pix = sorted({(0, 0), (H - 1, W - 1), (H // 2, W // 2), (0, W - 1), (H - 1, 0), (H // 2, 0), (0, W // 2)})
    names = ("nan", "+inf", "-inf", "th", "above", "negative", "tie")
    out = []
    for i, name in enumerate(names):
        y, x = pix[i % len(pix)]
        out.append((name, y, x, (0, K // 2, K - 1)[i % 3]))
    return out


@functools.lru_cache(maxsize=None)
def volume(shape, K, seed=0):
    """The left (seed 0) / right (seed 1) volume of a kernel case: costs on a 1 / 64 grid in [-0.25, 0.875] (values >= th_col, negative ones and ties
    across k happen everywhere by chance as well), the specials at special_positions.  Computed once, shared, left unchanged."""
    H, W = shape
    rng = np.random.default_rng(7000 * seed + 100 * K + 10 * H + W)
    vol = (rng.integers(-16, 57, (K, H, W)) / 64.0).astype(F)
    # a smooth valley so that the recurrence has something to follow
    kk = np.arange(K, dtype=F)[:, None, None]
    centre = (K - 1) * (0.25 + 0.5 * np.arange(W, dtype=F)[None, None, :] / max(W - 1, 1))
    vol = np.where(np.abs(kk - centre) <= 1.5, vol - F(0.5), vol).astype(F)
    for name, y, x, k in special_positions(H, W, K):
        if name == "tie":
            vol[:, y, x] = F(0.25)
            vol[k, y, x] = vol[max(k - 1, 0), y, x] = F(-0.375)
        else:
            vol[k, y, x] = SPECIAL_VALUES[name]
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def restated_sums(shape, K, seed=0, zero=False):
    p1, p2 = (F(0), F(0)) if zero else penalties(TH)
    return sgm_sums(volume(shape, K, seed), TH, p1, p2, 8)


def restated(shape, K, paths, subpixel, seed=0):
    lab, cost, _ = wv.wta_restate(restated_sums(shape, K, seed)[paths - 1], D0, subpixel)
    return lab, cost


# ------------------------------------------------------------------------------------------------ 1. the restatement itself (CPU only)
def case_restatement_matches_loop():
    n = 0
    for shape, K in (((5, 7), 5), ((9, 6), 3)):
        vol = volume(shape, K)
        ct = truncate(vol, TH)
        p1, p2 = penalties(TH)
        for dx, dy in DIRS:
            a, b = sgm_direction(ct, dx, dy, p1, p2), sgm_direction_loop(ct, dx, dy, p1, p2)
            assert same(a, b), (shape, K, dx, dy)
            # P1 = P2 = 0: t = m, so every L is C' + 0
            z = sgm_direction(ct, dx, dy, F(0), F(0))
            assert np.array_equal(z, ct), (shape, K, dx, dy)
            n += 1
        # the read-out is the restatement of les_wtavol.h applied to the summed slabs
        S = sgm_sums(vol, TH, p1, p2, 8)
        assert same(S[7], functools.reduce(lambda s, d: (s + sgm_direction(ct, d[0], d[1], p1, p2)).astype(F), DIRS[1:], sgm_direction(ct, *DIRS[0], p1, p2)))
        for paths in PATHS:
            for subpixel in (False, True):
                lab, cost = sgm_restate(vol, TH, D0, paths, p1, p2, subpixel)
                ll, lc, _ = wv.wta_loop(S[paths - 1], D0, subpixel)
                assert same(lab, ll) and same(cost, lc)
    return n


def case_populations_hold_what_the_cases_need():
    """The stated positions hold the stated specials; the truncation makes every one of them finite and <= th_col; ties across k and a refined
    (non-integer) disparity occur in the outputs the kernels are compared with."""
    n = 0
    for shape in SHAPES:
        for K in KS:
            vol = volume(shape, K)
            ct = truncate(vol, TH)
            assert np.isfinite(ct).all() and (ct <= TH).all()
            for name, y, x, k in special_positions(*shape, K):
                v = vol[k, y, x]
                # (a later special may share a pixel and disparity at the tiny shapes: the last one written holds)
                later = [s for s in special_positions(*shape, K) if s[1:] == (y, x, k)][-1][0]
                if later != name:
                    continue
                ok = dict(nan=np.isnan(v), th=v == TH, above=v == F(1e6), negative=v == F(-0.75), tie=v == F(-0.375)).get(name)
                if name == "+inf":
                    ok = v == np.inf
                if name == "-inf":
                    ok = v == -np.inf
                assert ok, (shape, K, name, v)
                if name in ("nan", "+inf", "-inf", "th", "above"):
                    assert ct[k, y, x] == TH
                if name == "tie" and k > 0:
                    assert vol[k - 1, y, x] == vol[k, y, x] == vol[:, y, x][np.isfinite(vol[:, y, x])].min()
                n += 1
            assert (vol < 0).any() and (vol >= TH).any()
            if K >= 5 and shape[0] * shape[1] > 9:
                lab, _ = restated(shape, K, 8, True)
                assert (lab[..., 2] != np.rint(lab[..., 2])).any(), (shape, K)
    # every kind is really present somewhere at every K
    for K in KS:
        kinds = {s[0] for s in special_positions(19, 37, K)}
        assert kinds == {"nan", "+inf", "-inf", "th", "above", "negative", "tie"}
    return n


# ------------------------------------------------------------------------------------------------ device harness
def guide(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


class Dev:
    """A cost-volume context of the shape (unfiltered aggregation: any image size; min_disparity D0, K disparities, both views) with label and sum
    buffers."""

    def __init__(self, lib, shape, K):
        H, W = shape
        self.e = api.HipCostVolumeEnergy(guide(H, W, 1), guide(H, W, 2), volume(shape, K, 0), volume(shape, K, 1), windR=0, th_col=float(TH),
                                         max_disp=float(D0) + K - 1, min_disp=float(D0), lib=lib, filter="")
        self.H, self.W, P = H, W, H * W
        self.labels, self.sum = api.DeviceBuffer(self.e, P * 16), api.DeviceBuffer(self.e, P * 4)

    def run(self, mode, paths, subpixel, p1=None, p2=None, with_sum=True):
        self.labels.fill(0x5A); self.sum.fill(0x5A)
        assert self.e.sgm_labels(mode, paths, p1, p2, subpixel, self.labels.ptr, self.sum.ptr if with_sum else None) is None
        self.e.synchronize()
        return self.labels.download((self.H, self.W, 4), F), self.sum.download((self.H, self.W), F)

    def close(self):
        self.labels.free(); self.sum.free()
        self.e.close()


def case_kernel_bit_for_bit(lib, shape, K, paths_list=PATHS, subpixels=(False, True)):
    """Labels and sums of the left view against the restatement, as bytes, for every `paths` and subpixel setting of the lists; the workspace size."""
    H, W = shape
    d = Dev(lib, shape, K)
    n = 0
    try:
        assert d.e.sgm_workspace_bytes() == 2 * H * W * kp_of(K) * 4
        for paths in paths_list:
            for subpixel in subpixels:
                want_l, want_c = restated(shape, K, paths, subpixel)
                got_l, got_c = d.run(0, paths, subpixel)
                msg = wv.describe(got_l, want_l, "labels") or wv.describe(got_c, want_c, "sums")
                assert not msg, f"{H}x{W}, K {K}, {paths} paths, subpixel {subpixel}: {msg}"
                z = got_l[..., 2]
                assert (z >= D0).all() and (z <= D0 + F(K - 1)).all()
                n += 1
        # without the second output: the same labels, the sum buffer untouched
        got_l2, guard = d.run(0, paths_list[-1], subpixels[-1], with_sum=False)
        assert same(got_l2, got_l) and (guard.view(np.uint8) == 0x5A).all()
    finally:
        d.close()
    return n


# ------------------------------------------------------------------------------------------------ 3. order and repeat
def case_order_and_repeat(lib, device):
    """Two calls return identical bytes, for the left and the right view, and they are the restatement's; a call after les_hip_wta_labels on the same
    context, and one before it, change nothing in either result; the form that returns tensors; the default penalties."""
    H, W, D = 48, 64, 16
    gl, gr = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    vl, vr = synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43)
    e = api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=20, th_col=0.5, lib=lib)
    P = H * W
    lab, cost = api.DeviceBuffer(e, P * 16), api.DeviceBuffer(e, P * 4)
    try:
        assert e.sgm_workspace_bytes() == 2 * P * 64 * 4
        p1, p2 = e.sgm_penalties()
        assert (p1, p2) == penalties(0.5) == (F(0.16) * F(0.5), F(1.28) * F(0.5))

        def sgm(mode):
            lab.fill(0x5A); cost.fill(0x5A)
            e.sgm_labels(mode, 8, None, None, True, lab.ptr, cost.ptr)
            e.synchronize()
            return lab.download((H, W, 4), F), cost.download((H, W), F)

        def wta(mode):
            lab.fill(0x5A); cost.fill(0x5A)
            e.wta_labels(mode, 0, True, lab.ptr, cost.ptr)
            e.synchronize()
            return lab.download((H, W, 4), F), cost.download((H, W), F)

        first = {m: sgm(m) for m in (0, 1)}
        for m, vol in ((0, vl), (1, vr)):
            want = sgm_restate(vol, 0.5, 0.0, 8, p1, p2, True)
            msg = wv.describe(first[m][0], want[0], "labels") or wv.describe(first[m][1], want[1], "sums")
            assert not msg, f"view {m}: {msg}"
            again = sgm(m)
            assert same(again[0], first[m][0]) and same(again[1], first[m][1]), m
        assert not same(first[0][0], first[1][0])
        w0 = wta(0)                                          # after SGM calls
        s0 = sgm(0)                                          # after a WTA call
        w1 = wta(0)
        assert same(s0[0], first[0][0]) and same(s0[1], first[0][1])
        assert same(w0[0], w1[0]) and same(w0[1], w1[1])
        e2 = api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=20, th_col=0.5, lib=lib)        # a context that has never run SGM
        try:
            l2, c2 = api.DeviceBuffer(e2, P * 16), api.DeviceBuffer(e2, P * 4)
            e2.wta_labels(0, 0, True, l2.ptr, c2.ptr)
            e2.synchronize()
            assert same(l2.download((H, W, 4), F), w0[0]) and same(c2.download((H, W), F), w0[1])
            l2.free(); c2.free()
        finally:
            e2.close()
        t_lab, t_sum = e.sgm_labels(1, device=device)
        e.synchronize()
        assert same(t_lab.cpu().numpy(), first[1][0]) and same(t_sum.cpu().numpy(), first[1][1])
    finally:
        lab.free(); cost.free()
        e.close()


# ------------------------------------------------------------------------------------------------ 4. argument errors
def case_argument_errors(lib):
    """Every refusal: nothing launched, the outputs keep their guard bytes."""
    H, W, D = 48, 64, 16
    gl, vl = synth.make_guide(H, W, 1234), synth.make_volume(D, H, W, 42)
    e = api.HipCostVolumeEnergy(gl, None, vl, None, windR=20, th_col=0.5, lib=lib)           # the left view only
    P = H * W
    lab, cost = api.DeviceBuffer(e, P * 16), api.DeviceBuffer(e, P * 4)
    nan, inf = float("nan"), float("inf")
    try:
        lab.fill(0x5A); cost.fill(0x5A)
        bad = [dict(mode=1), dict(mode=2), dict(mode=-1), dict(labels_ptr=0), dict(paths=0), dict(paths=3), dict(paths=16), dict(paths=-8),
               dict(p1=-0.01), dict(p1=nan), dict(p1=inf, p2=inf), dict(p2=nan), dict(p2=inf), dict(p1=0.2, p2=0.1), dict(p2=-1.0, p1=0.0)]
        for kw in bad:
            a = dict(mode=0, paths=8, p1=0.08, p2=0.64, labels_ptr=lab.ptr)
            a.update(kw)
            rc = e.L.les_hip_sgm_labels(e.h, a["mode"], a["paths"], api.C.c_float(a["p1"]), api.C.c_float(a["p2"]), 1,
                                        api.C.c_void_p(a["labels_ptr"]) if a["labels_ptr"] else None, api.C.c_void_p(cost.ptr))
            assert rc == api.LES_HIP_ERR_ARG, (kw, rc)
        assert e.L.les_hip_sgm_labels(None, 0, 8, api.C.c_float(0.08), api.C.c_float(0.64), 1, api.C.c_void_p(lab.ptr), api.C.c_void_p(cost.ptr)) == api.LES_HIP_ERR_ARG
        try:
            e.sgm_labels(0, 3, None, None, True, lab.ptr, cost.ptr)
            raise AssertionError("paths = 3 was accepted")
        except api.LesHipError as ex:
            assert f"error {api.LES_HIP_ERR_ARG}" in str(ex), str(ex)
        # the image-based energy holds no volume
        im = np.zeros((H, W, 3), np.uint8)
        en = api.HipCostVolumeEnergy.naive(im, im, windR=0, max_disp=15.0, lib=lib, filter="")
        try:
            assert en.sgm_workspace_bytes() == 0
            try:
                en.sgm_labels(0, 8, None, None, True, lab.ptr, cost.ptr)
                raise AssertionError("an image-based context was accepted")
            except api.LesHipError as ex:
                assert f"error {api.LES_HIP_ERR_UNSUPPORTED}" in str(ex), str(ex)
        finally:
            en.close()
        # more disparities than the kernels serve, and more than the volume holds
        eb = api.HipCostVolumeEnergy(gl, None, vl, None, windR=20, th_col=0.5, max_disp=600.0, lib=lib)
        try:
            assert eb.sgm_workspace_bytes() == 0
            assert eb.L.les_hip_sgm_labels(eb.h, 0, 8, api.C.c_float(0.08), api.C.c_float(0.64), 1, api.C.c_void_p(lab.ptr), api.C.c_void_p(cost.ptr)) == api.LES_HIP_ERR_UNSUPPORTED
        finally:
            eb.close()
        eb = api.HipCostVolumeEnergy(gl, None, vl, None, windR=20, th_col=0.5, max_disp=16.0, lib=lib)
        try:
            assert eb.sgm_workspace_bytes() == 0         # (0 wherever les_hip_sgm_labels refuses the context)
            assert eb.L.les_hip_sgm_labels(eb.h, 0, 8, api.C.c_float(0.08), api.C.c_float(0.64), 1, api.C.c_void_p(lab.ptr), api.C.c_void_p(cost.ptr)) == api.LES_HIP_ERR_ARG
        finally:
            eb.close()
        e.synchronize()
        assert (lab.download((P * 16,), np.uint8) == 0x5A).all() and (cost.download((P * 4,), np.uint8) == 0x5A).all()
        assert e.sgm_workspace_bytes() == 2 * P * 64 * 4
    finally:
        lab.free(); cost.free()
        e.close()
    return len(bad) + 5


# ------------------------------------------------------------------------------------------------ 5. quality on the cones crop
def bad_rate(labels, d0, gt, mask, thr=1.0):
    return float((np.abs((labels[..., 2] - F(d0)) - gt)[mask] > thr).mean())


def case_quality(lib, device, D=64):
    """The device AD-Census volume of the cones crop (tests/golden/cones_crop.npz), th_col 0.5, on the pixels costvol_cases.case_quality scores: the
    device maps equal the restatement's bit for bit, and the cap of the module docstring holds for 4 and 8 paths."""
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    vol = cc.dev_volume(lib, imL, imR, D, 0)
    mask = (gt > 0) & np.isfinite(gt) & (np.arange(W)[None, :] - gt >= 0)
    assert mask.sum() >= 8000, int(mask.sum())
    e = api.HipCostVolumeEnergy(imL, None, vol, None, windR=20, th_col=0.5, lib=lib)
    out = dict(pixels=int(mask.sum()))
    try:
        p1, p2 = e.sgm_penalties()

        def device_map(paths, q1, q2, subpixel):
            lab, s = e.sgm_labels(0, paths, q1, q2, subpixel, device=device)
            e.synchronize()
            return lab.cpu().numpy(), s.cpu().numpy()
        base_l, base_s = device_map(8, 0.0, 0.0, False)
        want = sgm_restate(vol, 0.5, 0.0, 8, 0.0, 0.0, False)
        assert same(base_l, want[0]) and same(base_s, want[1])
        assert np.array_equal(base_l[..., 2], truncate(vol, 0.5).argmin(0).astype(F))      # the arg-min of the truncated volume
        out["argmin_bad1.0"] = bad_rate(base_l, 0, gt, mask)
        for paths in (4, 8):
            got = device_map(paths, None, None, False)
            want = sgm_restate(vol, 0.5, 0.0, paths, p1, p2, False)
            msg = wv.describe(got[0], want[0], "labels") or wv.describe(got[1], want[1], "sums")
            assert not msg, f"cones crop, {paths} paths: {msg}"
            out[f"sgm{paths}_bad1.0"], out[f"sgm{paths}_bad2.0"] = bad_rate(got[0], 0, gt, mask), bad_rate(got[0], 0, gt, mask, 2.0)
            out[f"sgm{paths}_subpixel_bad1.0"] = bad_rate(device_map(paths, None, None, True)[0], 0, gt, mask)
        w_lab, _ = e.wta_labels(0, device=device)
        e.synchronize()
        out["wta_guided_filter_bad1.0"] = bad_rate(w_lab.cpu().numpy(), 0, gt, mask)
        print(out)
        for paths in (4, 8):
            assert out[f"sgm{paths}_bad1.0"] <= 0.5 * out["argmin_bad1.0"], out
    finally:
        e.close()
    return out


# ------------------------------------------------------------------------------------------------ 6. drivers
def driver(lib, device, device_cuts, **opts):
    """stereo.FastGCStereo on the cones crop with the cost-volume energy of its AD-Census volumes (both views, 64 disparities, th_col 0.5, guided
    filter of crossview_cases.WINDR), the two layers of crossview_cases.  -> (driver, energy, the volumes' tensors: keep them alive)"""
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    tl, tr = lio.build_volumes(imL, imR, 64, device=device, lib=lib)
    e = api.HipCostVolumeEnergy(imL, imR, tl.data_ptr(), tr.data_ptr(), windR=cv.WINDR, th_col=0.5, max_disp=63.0, volumes_on_device=True, shape=(64, H, W), lib=lib)
    st = stereo.FastGCStereo(e, imL, imR, dict(lambda_=0.5, windR=cv.WINDR, th_col=0.5), device=device, seed=3, device_cuts=device_cuts, **opts)
    st.setEvaluator(lio.Evaluator(np.where(gt > 0, gt, np.inf).astype(F), gt > 0, 1.0), precision=-1.0)
    st.concurrent_views = False
    for u, t in zip(cv.UNITS, cv.TABLE):
        st.addLayer(u, t)
    return st, e, (tl, tr)


def case_driver_sgm(lib, device, device_cuts):
    out = {}
    st, e, keep = driver(lib, device, device_cuts, evaluate_on_device=True)
    try:
        H, W = e.H, e.W
        w_before = st.wta((0,))
        wta_row = st.log[0]
        # two views: valid labels for every pixel, the raw maps are set, one row per view, the post-processing changes the left map
        lab2, raw2 = st.sgm((0, 1))
        assert sorted(st.raw_labelings) == [0, 1] and [r["mode"] for r in st.log] == [0, 1] and same(raw2, st.raw_labelings[0])
        for m in (0, 1):
            r = st.raw_labelings[m]
            assert r.shape == (H, W, 4) and np.isfinite(r).all() and (r[..., [0, 1, 3]] == 0).all() and (r[..., 2] >= 0).all() and (r[..., 2] <= 63).all()
        assert np.isfinite(lab2).all() and not same(lab2, raw2)
        sgm_row = st.log[0]
        print(f"cones crop, left view: WTA all {wta_row['all']:.2f} % energy {wta_row['energy']:.1f}; SGM all {sgm_row['all']:.2f} % nonocc {sgm_row['nonocc']:.2f} % "
              f"energy {sgm_row['energy']:.1f}")
        out.update(wta_all=wta_row["all"], sgm_all=sgm_row["all"], wta_energy=wta_row["energy"], sgm_energy=sgm_row["energy"])
        # the raw map is the kernel's, the costs of the rows are the dense re-scoring's
        k_lab, k_sum = e.sgm_labels(0, device=device)
        e.synchronize()
        assert same(k_lab.cpu().numpy(), raw2)
        lab1, raw1 = st.sgm((0,), paths=4, subpixel=False)
        assert same(lab1, raw1) and (lab1[..., 2] == np.rint(lab1[..., 2])).all() and len(st.log) == 1
        # wta() on the same object returns the same bytes before and after sgm()
        w_after = st.wta((0,))
        assert same(w_before[0], w_after[0]) and same(w_before[1], w_after[1])
        # with 0 iterations run() returns the SGM map; its first row is the SGM map re-scored
        st.log = []
        lab0, raw0 = st.run(0, (0,), 0, labeling="sgm")
        assert same(lab0, raw2) and same(raw0, raw2) and st.log[0]["all"] == sgm_row["all"]
        # one graph-cut iteration from it: bit-identical on repeat, and it does not end above its start
        st.log = []
        a = st.run(1, (0,), 0, labeling="sgm")
        log_a = st.log
        st.log = []
        b = st.run(1, (0,), 0, labeling="sgm")
        assert same(a[0], b[0]) and same(a[1], b[1])
        assert log_a[0]["all"] == sgm_row["all"] and log_a[-1]["energy"] <= log_a[0]["energy"], (log_a[0], log_a[-1])
        print(f"run(1, pmInit=0, labeling='sgm'): energy {log_a[0]['energy']:.1f} -> {log_a[-1]['energy']:.1f}, all {log_a[0]['all']:.2f} -> {log_a[-1]['all']:.2f} %")
        out.update(run_start=log_a[0]["energy"], run_end=log_a[-1]["energy"])
        st.log, st.slant_stats = [], {}
        c = st.run(1, (0,), 0, labeling="sgm+planes")
        assert sorted(st.slant_stats) == [0] and sum(st.slant_stats[0]["kind_pixels"]) == H * W and np.isfinite(c[0]).all()
        out.update(kind_pixels=st.slant_stats[0]["kind_pixels"])
        st.slant_stats = {}
        st.sgm((0,), slanted=True)
        assert sorted(st.slant_stats) == [0]
        try:
            st.run(1, (0,), 0, labeling="sgn")
            raise AssertionError("an unknown start was accepted")
        except ValueError:
            pass
    finally:
        e.close()
        del keep
    # the image-based energy: the start is refused with a ValueError, sgm() with the library's error
    st2, e2 = cv.driver(lib, device, device_cuts)
    try:
        try:
            st2.run(1, (0,), 0, labeling="sgm")
            raise AssertionError("an image-based energy was accepted")
        except ValueError:
            pass
        try:
            st2.sgm((0,))
            raise AssertionError("an image-based energy was accepted")
        except api.LesHipError as ex:
            assert f"error {api.LES_HIP_ERR_UNSUPPORTED}" in str(ex), str(ex)
    finally:
        e2.close()
    return out


def case_driver_midv(lib, device, monkeypatch, layers=None, **opts):
    """MidV3(init="sgm") from the pair alone runs end to end; MidV2(init="sgm") raises a ValueError that names the image-based energy.
    layers, opts: as wtavol_cases.case_driver_midv."""
    from localexpstereo_amd import stereo
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    kw = dict(iterations=1, pmIterations=1, device=device, lib=lib, **opts)
    imL, imR, gt = cc.cones_pair()
    data3 = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
    st, lab, raw = stereo.MidV3(data3, None, None, doDual=True, init="sgm", evaluate_on_device=True, **kw)
    assert lab.shape == gt.shape + (4,) and np.isfinite(lab).all() and len(st.log) == 4
    print(f"MidV3(init='sgm') from the pair: all {[round(r['all'], 2) for r in st.log if 'all' in r]} %, energy {[round(r['energy'], 1) for r in st.log]}")
    try:
        stereo.MidV2(cv.cones_data(), init="sgm", **kw)
        raise AssertionError("MidV2(init='sgm') was accepted")
    except ValueError as ex:
        assert "image-based" in str(ex)
    return dict(midv3_sgm_all=[r["all"] for r in st.log if "all" in r])


# ------------------------------------------------------------------------------------------------ the penalty sweep of DESIGN 3.2i
SWEEP_P1 = (0.04, 0.08, 0.12, 0.16)
SWEEP_P2 = (0.32, 0.64, 0.96, 1.28, 2.0)


def penalty_sweep(lib, D=64):
    """Bad-1.0 in % of the integer-winner map of this restatement on the cones crop (the restated AD-Census volume of costvol_cases, th_col 0.5, the
    pixels case_quality scores) -> {"raw": arg-min of the raw volume, "truncated": of the truncated one, (paths, P1, P2): ...}"""
    imL, imR, gt = cc.cones_pair()
    W = gt.shape[1]
    ta, tc = api.costvol_tables(lib=lib)
    vol = cc.volume(imL, imR, D, 0, 0, ta, tc)
    mask = (gt > 0) & np.isfinite(gt) & (np.arange(W)[None, :] - gt >= 0)
    bad = lambda S: 100.0 * float((np.abs(S.argmin(0).astype(F) - gt)[mask] > 1.0).mean())
    out = dict(raw=bad(vol), truncated=bad(truncate(vol, 0.5)))
    for p1 in SWEEP_P1:
        for p2 in SWEEP_P2:
            S = sgm_sums(vol, 0.5, p1, p2, 8)
            out[(4, p1, p2)], out[(8, p1, p2)] = bad(S[3]), bad(S[7])
    return out


if __name__ == "__main__":
    from localexpstereo_amd import build
    t = penalty_sweep(build.build_sim())            # (the simulator build serves the two cost tables; the package's own library needs a GPU)
    print(f"arg-min of the raw volume {t['raw']:.2f} %, of the truncated one {t['truncated']:.2f} %")
    print("P1 \\ P2 | " + " | ".join(f"{p2}" for p2 in SWEEP_P2) + " || " + " | ".join(f"{p2}" for p2 in SWEEP_P2) + "   (4 paths || 8 paths)")
    for p1 in SWEEP_P1:
        print(f"{p1} | " + " | ".join(f"{t[(4, p1, p2)]:.2f}" for p2 in SWEEP_P2) + " || " + " | ".join(f"{t[(8, p1, p2)]:.2f}" for p2 in SWEEP_P2))
