"""Cases of tests/test_wtavol.py: winner-take-all labels of the aggregated cost volume (csrc/les_wtavol.h: les_hip_slab_argmin,
les_hip_slab_argmin_finish, les_hip_wta_labels; stereo.FastGCStereo.wta and run(labeling="wta")) on the CPU simulator build and on the MI355X.

The definition, restated from csrc/les_wtavol.h.  A pixel has costs c_0 ... c_{K-1}, one per slab; slab k belongs to disparity d0 + k.  k* is the
smallest k whose c_k is the minimum under the comparison c < best from best = +inf, k* = -1: NaN never wins, +inf never wins, of equal costs the
lowest disparity wins, -0 = +0.  c0 = c_{k*}, cm = c_{k*-1}, cp = c_{k*+1}.  In f32, in this order:
    den = (cm - c0) + (cp - c0)        off = 0.5 (cm - cp) / den
when subpixel and 0 < k* < K-1 and cm, cp are finite and den > 0; otherwise off = 0.  Label (0, 0, (float(k*) + off) + d0, 0), cost c0; without a
winner label (0, 0, d0, 0) and cost +inf.

References, none of them the code under test: the vectorised numpy restatement below (np.argmin over the slabs with NaN read as +inf), itself held
to a literal per-pixel loop; for the whole call, the restatement applied to the slabs the project's own batch path writes
(api.Batch(out_slabs=True).run(fronto planes, check=False)) on the same context.  Tolerances: labels and costs are compared bit for bit
everywhere.  Energies: a fusion may raise a view's energy only through the float rounding of the capacities, fusion_cases.RISE |E|.

The simulator legs of the driver cases run with stereo._layers replaced by crossview_cases.sim_layers and a filter radius of 6, as the cross-view
cases do and for their reason; the drivers run on the cones crop of tests/golden (tests/golden/cones cut to 96 x 184, image-based energy, ground
truth present): the full 450 x 375 pair costs the fibre simulator tens of minutes."""
import functools

import numpy as np

from localexpstereo_amd import api, synth
from tests import crossview_cases as cv
from tests import eval_cases as ec
from tests import fusion_cases as fc

F = np.float32
SHAPES = ((5, 7), (33, 130), (48, 64))          # (H, W): one partial workgroup with a 3-pixel tail; H W % 4 == 2 (every other slab unaligned), 5 workgroups; H W % 4 == 0 (the all-vector kernel)
KS = (1, 2, 3, 5, 9)                            # 9: one full block of the 8 slabs in flight plus one
D0 = F(3.0)                                     # min_disparity of the reduction cases' context


def chunkings(K):
    return sorted({1, 2, K, K + 3})


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ restatement, numpy f32
def wta_restate(slabs, d0, subpixel=True):
    """slabs [K][H][W] f32 -> (labels H x W x 4, cost H x W, ks H x W int: k*, -1 without a winner)"""
    slabs = np.asarray(slabs, F)
    K, H, W = slabs.shape
    d0 = F(d0)
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(slabs), F(np.inf), slabs)
        ks = np.argmin(c, axis=0)                                        # the first of the minima; -0 == +0
        none = np.take_along_axis(c, ks[None], 0)[0] == np.inf           # nothing below +inf: no winner
        pick = lambda k: np.take_along_axis(slabs, np.clip(k, 0, K - 1)[None], 0)[0]
        c0, cm, cp = pick(ks), pick(ks - 1), pick(ks + 1)
        ok = (ks > 0) & (ks < K - 1) & np.isfinite(cm) & np.isfinite(cp) & bool(subpixel) & ~none
        den = ((cm - c0) + (cp - c0)).astype(F)
        ok &= den > 0
        off = np.where(ok, (F(0.5) * (cm - cp) / den).astype(F), F(0)).astype(F)
        z = ((ks.astype(F) + off) + d0).astype(F)
    labels = np.zeros((H, W, 4), F)
    labels[..., 2] = np.where(none, d0, z)
    cost = np.where(none, F(np.inf), c0).astype(F)
    return labels, cost, np.where(none, -1, ks)


def wta_loop(slabs, d0, subpixel=True):
    """The same by a literal per-pixel transcription of the definition (scalar f32 operations)."""
    K, H, W = slabs.shape
    labels, cost, kmap = np.zeros((H, W, 4), F), np.zeros((H, W), F), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                best, k_ = F(np.inf), -1
                for k in range(K):
                    if slabs[k, y, x] < best:
                        best, k_ = slabs[k, y, x], k
                if k_ < 0:
                    labels[y, x, 2], cost[y, x], kmap[y, x] = F(d0), F(np.inf), -1
                    continue
                off = F(0)
                if subpixel and 0 < k_ < K - 1:
                    cm, cp = slabs[k_ - 1, y, x], slabs[k_ + 1, y, x]
                    if np.isfinite(cm) and np.isfinite(cp):
                        den = F(F(cm - best) + F(cp - best))
                        if den > 0:
                            off = F(F(F(0.5) * F(cm - cp)) / den)
                labels[y, x, 2], cost[y, x], kmap[y, x] = F(F(F(k_) + off) + F(d0)), best, k_
    return labels, cost, kmap


# ------------------------------------------------------------------------------------------------ slab populations
def positions(K):
    """The slabs a special case is placed at: the first two, the middle, the last two.  With chunks of 2 slab 1 is the last of its chunk and slab 2
    (K = 3, 5) or 4 (K = 9) the first of the next; with chunks of 1 every slab is both."""
    return sorted({0, 1, K // 2, K - 2, K - 1} & set(range(K)))


def specials(K, rng):
    """The special pixels of a K-slab volume -> [(name, costs[K], expected k* or None = whatever the restatement says, off must be 0: bool)]"""
    out = []
    base = lambda: rng.uniform(2.0, 3.0, K).astype(F)
    for j in positions(K):
        c = base(); c[j] = F(1.0)
        out.append((f"minimum on slab {j}", c, j, j in (0, K - 1)))
        if j + 1 < K:
            c = base(); c[j] = c[j + 1] = F(1.25)
            out.append((f"tie of slabs {j} and {j + 1}", c, j, False))
            c = base() + F(1); c[j], c[j + 1] = F(0.0), F(-0.0)
            out.append((f"+0 on slab {j} before -0", c, j, False))
            c = base() + F(1); c[j], c[j + 1] = F(-0.0), F(0.0)
            out.append((f"-0 on slab {j} before +0", c, j, False))
        c = base(); c[j] = F(np.nan)
        out.append((f"NaN candidate on slab {j}", c, None, False))
        for what, val in (("NaN", np.nan), ("+inf", np.inf), ("1e6", 1e6)):
            for side, name in ((-1, "before"), (+1, "after")):
                if 0 <= j + side < K:
                    c = base(); c[j] = F(1.0); c[j + side] = F(val)
                    # a NaN / +inf neighbour switches the refinement off; a 1e6 one is finite and takes part
                    out.append((f"{what} neighbour {name} the minimum on slab {j}", c, j, what != "1e6" or j in (0, K - 1)))
    out.append(("all NaN", np.full(K, np.nan, F), -1, True))
    out.append(("all +inf", np.full(K, np.inf, F), -1, True))
    out.append(("NaN and +inf only", np.where(np.arange(K) % 2 == 0, F(np.nan), F(np.inf)).astype(F), -1, True))
    out.append(("constant", np.full(K, 1.5, F), 0, True))
    return out


@functools.lru_cache(maxsize=None)
def volumes(shape, K):
    """Every (slabs [K][H][W], where) of a shape and K, as many volumes as the shape needs to hold all specials on at most every second pixel;
    where = [(y, x, name, k*, off0)].  Computed once, shared, left unchanged.  The background: random costs on a 1 / 8 grid (ties happen by chance
    as well), so minima fall on every slab."""
    H, W = shape
    rng = np.random.default_rng(1000 * K + W)
    sp = specials(K, rng)
    out, k = [], 0
    while k < len(sp):
        slabs = (rng.integers(8, 64, (K, H, W)) / 8.0).astype(F)
        where = []
        for p in rng.permutation(H * W)[: max(1, (H * W) // 2)]:
            if k == len(sp):
                break
            y, x = divmod(int(p), W)
            name, c, kstar, off0 = sp[k]
            slabs[:, y, x] = c
            where.append((y, x, name, kstar, off0))
            k += 1
        slabs.setflags(write=False)
        out.append((slabs, where))
    return out


@functools.lru_cache(maxsize=None)
def restated(shape, K, subpixel):
    return [wta_restate(slabs, D0, subpixel) for slabs, _ in volumes(shape, K)]


# ------------------------------------------------------------------------------------------------ 1. the restatement itself (CPU only)
def case_restatement_matches_loop():
    n = 0
    for shape in SHAPES[:1] + ((6, 10),):
        for K in KS:
            for subpixel in (False, True):
                for slabs, _ in volumes(shape, K):
                    a, b = wta_restate(slabs, D0, subpixel), wta_loop(slabs, D0, subpixel)
                    assert same(a[0], b[0]) and same(a[1], b[1]) and (a[2] == b[2]).all(), (shape, K, subpixel)
                    n += 1
    return n


def case_populations_hold_what_the_cases_need():
    """Every special case really occurs, at every K that can hold it, and the restatement gives it the stated k* and a zero offset where one is
    stated; the refinement is switched on somewhere (a non-zero offset) and the offsets stay within half a slab."""
    seen = {}
    for shape in SHAPES:
        for K in KS:
            names = set()
            for (slabs, where), (lab, cost, ks) in zip(volumes(shape, K), restated(shape, K, True)):
                off = lab[..., 2] - D0 - np.maximum(ks, 0).astype(F)
                assert (np.abs(off) <= 0.5).all(), (shape, K)
                for y, x, name, kstar, off0 in where:
                    names.add(name)
                    if kstar is not None:
                        assert ks[y, x] == kstar, (shape, K, name, int(ks[y, x]))
                    if off0:
                        assert off[y, x] == 0, (shape, K, name)
                    if name.startswith("NaN candidate"):          # (K = 1: the NaN is the pixel's only cost, nothing wins)
                        assert (ks[y, x] >= 0 and not np.isnan(cost[y, x])) if K > 1 else (ks[y, x] == -1 and cost[y, x] == np.inf)
                    if name.startswith(("+0 on", "-0 on")):
                        assert cost[y, x] == 0 and np.signbit(cost[y, x]) == name.startswith("-0"), (shape, K, name)
                    if kstar == -1:
                        assert cost[y, x] == np.inf and lab[y, x, 2] == D0
                if K >= 3:
                    assert (off != 0).any(), (shape, K)
            want = {n for n, *_ in specials(K, np.random.default_rng(0))}
            assert names == want, (shape, K, want - names)
            seen[K] = names
    # what the issue lists, by K: ties (also across every chunk boundary of chunks of 1 and 2), minima on the first and the last slab, on the last slab
    # of a chunk and the first of the next, NaN as candidate and neighbour, +inf and 1e6 neighbours, an all-NaN pixel, -0 against +0, a constant pixel
    for K in KS:
        assert {"all NaN", "constant", "minimum on slab 0", f"minimum on slab {K - 1}", "NaN candidate on slab 0"} <= seen[K]
    for K in KS[1:]:
        assert {"tie of slabs 0 and 1", "+0 on slab 0 before -0", "-0 on slab 0 before +0", "NaN neighbour after the minimum on slab 0",
                "+inf neighbour before the minimum on slab 1", "1e6 neighbour after the minimum on slab 0"} <= seen[K]
    for K in KS[2:]:
        assert {"tie of slabs 1 and 2", "minimum on slab 1", "minimum on slab 2" if K < 9 else "minimum on slab 4"} <= seen[K]      # chunks of 2: last | first
    return sum(len(v) for v in seen.values())


# ------------------------------------------------------------------------------------------------ device harness
class Dev:
    """An energy context of the shape (image-based cost, no aggregation: any image size; min_disparity D0) and device buffers for the slabs of
    one volume, the state, the labels and the costs."""

    def __init__(self, lib, H, W, kmax):
        im = np.zeros((H, W, 3), np.uint8)
        self.e = api.HipCostVolumeEnergy.naive(im, im, windR=0, max_disp=63.0, min_disp=float(D0), lib=lib, filter="")
        self.H, self.W, P = H, W, H * W
        assert self.e.slab_argmin_state_bytes() >= 20 * P
        self.slabs = api.DeviceBuffer(self.e, kmax * P * 4 + 16)
        self.state = api.DeviceBuffer(self.e, self.e.slab_argmin_state_bytes())
        self.labels, self.cost = api.DeviceBuffer(self.e, P * 16), api.DeviceBuffer(self.e, P * 4)

    def feed(self, slabs, chunk, offset_floats=0):
        """The step calls of one volume in chunks of `chunk` slabs (the state is filled with a guard byte first: k_first = 0 must initialise it)."""
        K, P = slabs.shape[0], self.H * self.W
        base = self.slabs.ptr + 4 * offset_floats
        self.e._chk(self.e.L.les_hip_memcpy_h2d(self.e.h, api.C.c_void_p(base), api._ptr(np.ascontiguousarray(slabs)), slabs.nbytes))
        self.state.fill(0x5A)
        for k0 in range(0, K, chunk):
            self.e.slab_argmin(base + 4 * k0 * P, min(chunk, K - k0), k0, self.state.ptr)

    def finish(self, K, subpixel):
        self.labels.fill(0x5A); self.cost.fill(0x5A)
        self.e.slab_argmin_finish(self.state.ptr, K, self.labels.ptr, self.cost.ptr, subpixel=subpixel)
        self.e.synchronize()
        return self.labels.download((self.H, self.W, 4), F), self.cost.download((self.H, self.W), F)

    def close(self):
        for b in (self.slabs, self.state, self.labels, self.cost):
            b.free()
        self.e.close()


def describe(got, want, what):
    diff = (got.view(np.uint32) != want.view(np.uint32))
    diff = diff.any(-1) if diff.ndim == 3 else diff
    return f"{what}: {int(diff.sum())} pixels differ from the restatement, first at {np.argwhere(diff)[0]}" if diff.any() else ""


# ------------------------------------------------------------------------------------------------ 2. / 3. kernel against the restatement, chunk independence
def case_kernel_bit_for_bit(lib, shape):
    """Every volume of the shape, K, chunking and subpixel setting against the restatement, labels and costs as bits; all chunkings of one input give
    identical bits (also asserted directly); a slab base 4 bytes off the 16-byte grid (the dword path at H W % 4 == 0) gives the same."""
    H, W = shape
    d = Dev(lib, H, W, max(KS))
    n = 0
    try:
        for K in KS:
            for vi, (slabs, _) in enumerate(volumes(shape, K)):
                first = {}
                for chunk in chunkings(K):
                    d.feed(slabs, chunk)
                    for subpixel in (False, True):
                        want_l, want_c, _ = restated(shape, K, subpixel)[vi]
                        got_l, got_c = d.finish(K, subpixel)
                        msg = describe(got_l, want_l, "labels") or describe(got_c, want_c, "costs")
                        assert not msg, f"{H}x{W}, K {K}, volume {vi}, chunks of {chunk}, subpixel {subpixel}: {msg}"
                        if subpixel in first:
                            assert same(got_l, first[subpixel][0]) and same(got_c, first[subpixel][1]), (shape, K, chunk, "chunk independence")
                        first.setdefault(subpixel, (got_l, got_c))
                        n += 1
                d.feed(slabs, 2, offset_floats=1)
                got_l, got_c = d.finish(K, True)
                assert same(got_l, first[True][0]) and same(got_c, first[True][1]), (shape, K, "unaligned slabs")
    finally:
        d.close()
    return n


# ------------------------------------------------------------------------------------------------ 4. the whole call
def contexts(lib):
    """name -> (energy, views): the 64 x 48 x 16 synthetic volumes of the golden fixtures (seeds 42 / 43) under the guided filter with windR 20, both
    views; a cones crop with the image-based energy (16 disparities, radius 6: the simulator serves it too); one bilateral context."""
    H, W, D = 48, 64, 16
    gl, gr = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    vl, vr = synth.make_volume(D, H, W, 42), synth.make_volume(D, H, W, 43)
    imL, imR, _ = ec.cones_images()
    imL, imR = np.ascontiguousarray(imL[20:60, 64:134]), np.ascontiguousarray(imR[20:60, 64:134])
    yield "synthetic volume, guided filter", api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=20, th_col=0.5, lib=lib), (0, 1)
    yield "cones crop, image-based", api.HipCostVolumeEnergy.naive(imL, imR, windR=12, max_disp=15.0, lib=lib), (0, 1)
    yield "synthetic volume, bilateral", api.HipCostVolumeEnergy(gl, gr, vl, vr, windR=4, eps=10.0, th_col=0.5, lib=lib, filter="BF"), (0,)


def batch_slabs(e, mode):
    """The slabs of the K fronto-parallel planes from the project's existing path: one prepared batch of K whole-image calls, out_slabs."""
    K, P = e.num_fronto_planes, e.H * e.W
    rects = [(0, 0, e.W, e.H)] * K
    planes = np.zeros((K, 4), F)
    planes[:, 2] = F(e.params.min_disparity) + np.arange(K, dtype=F)
    b, buf = api.Batch(e, rects, rects, out_slabs=True), api.DeviceBuffer(e, K * P * 4)
    try:
        buf.fill(0x5A)
        b.run(planes, buf.ptr, mode=mode, check=False)
        e.synchronize()
        return buf.download((K, e.H, e.W), F)
    finally:
        buf.free(); b.destroy()


def case_whole_call(lib, device):
    out = {}
    for name, e, views in contexts(lib):
        try:
            K, P = e.num_fronto_planes, e.H * e.W
            assert K == 16
            lab, cost, chk = api.DeviceBuffer(e, P * 16), api.DeviceBuffer(e, P * 4), api.DeviceBuffer(e, P * 4)
            try:
                for m in views:
                    slabs = batch_slabs(e, m)
                    assert np.isfinite(slabs).all()
                    for chunk, subpixel in ((0, True), (5, True), (16, False), (1, True)):
                        want_l, want_c, ks = wta_restate(slabs, e.params.min_disparity, subpixel)
                        lab.fill(0x5A); cost.fill(0x5A)
                        assert e.wta_labels(m, chunk, subpixel, lab.ptr, cost.ptr) is None
                        e.synchronize()
                        got_l, got_c = lab.download((e.H, e.W, 4), F), cost.download((e.H, e.W), F)
                        msg = describe(got_l, want_l, "labels") or describe(got_c, want_c, "costs")
                        assert not msg, f"{name}, view {m}, chunk {chunk}, subpixel {subpixel}: {msg}"
                    # every label is a valid one: the dense re-scoring with the validity check on writes no 1e6
                    chk.fill(0x5A)
                    e.unary_labels(lab.ptr, chk.ptr, mode=m, check=True)
                    e.synchronize()
                    c2 = chk.download((e.H, e.W), F)
                    assert np.isfinite(c2).all() and not (c2 == F(1e6)).any(), (name, m)
                    z = got_l[..., 2]
                    assert (got_l[..., [0, 1, 3]] == 0).all() and (z >= e.params.min_disparity).all() and (z <= e.params.max_disparity).all()
                    out[f"{name}, view {m}"] = dict(distinct_kstar=int(len(np.unique(ks))), refined=int((z != np.rint(z)).sum()))
                    assert len(np.unique(ks)) > 1, (name, m)
                # the form that returns tensors
                t_lab, t_cost = e.wta_labels(views[-1], device=device)
                e.synchronize()
                assert same(t_lab.cpu().numpy(), got_l) and same(t_cost.cpu().numpy(), got_c), name
            finally:
                for b in (lab, cost, chk):
                    b.free()
        finally:
            e.close()
    return out


# ------------------------------------------------------------------------------------------------ 5. stream independence, argument errors
def case_independence_and_errors(lib, device):
    """The same call on a second stream and beside another enqueued kernel (a 64 MB streaming copy on the context's stream) gives the same bits; null
    outputs and a view without data are refused with LES_HIP_ERR_ARG and nothing is written."""
    H, W, D = 48, 64, 16
    gl, vl = synth.make_guide(H, W, 1234), synth.make_volume(D, H, W, 42)
    e = api.HipCostVolumeEnergy(gl, None, vl, None, windR=20, th_col=0.5, lib=lib)           # the left view only
    P = H * W
    lab, cost = api.DeviceBuffer(e, P * 16), api.DeviceBuffer(e, P * 4)
    n = 1 << 24
    big = [api.DeviceBuffer(e, 4 * n) for _ in range(2)]
    try:
        def call(chunk):
            lab.fill(0x5A); cost.fill(0x5A)
            e.wta_labels(0, chunk, True, lab.ptr, cost.ptr)
            e.synchronize()
            return lab.download((H, W, 4), F), cost.download((H, W), F)
        want = call(5)
        big[0].fill(1)
        side = None
        if device == "cuda":
            import torch
            side = torch.cuda.Stream()
            e.set_thread_stream(side.cuda_stream)
        try:
            got = call(5)                                                                      # a second stream
            assert same(got[0], want[0]) and same(got[1], want[1])
            lab.fill(0x5A); cost.fill(0x5A)
            e._chk(e.L.les_hip_calib_copy(api.C.c_void_p(big[0].ptr), api.C.c_void_p(big[1].ptr), n, 0, None))       # default stream: runs beside
            e.wta_labels(0, 5, True, lab.ptr, cost.ptr)
            e.synchronize()
            assert same(lab.download((H, W, 4), F), want[0]) and same(cost.download((H, W), F), want[1])
        finally:
            if side is not None:
                e.set_thread_stream(0, bind=False)
                import torch
                torch.cuda.synchronize()
        # argument errors: nothing launched, the outputs keep their guard bytes
        lab.fill(0x5A); cost.fill(0x5A)
        for args in ((0, 0, True, 0, cost.ptr), (0, 0, True, lab.ptr, 0), (1, 0, True, lab.ptr, cost.ptr), (2, 0, True, lab.ptr, cost.ptr)):
            try:
                e.wta_labels(*args)
                raise AssertionError(f"wta_labels{args} was accepted")
            except api.LesHipError as ex:
                assert f"error {api.LES_HIP_ERR_ARG}" in str(ex), str(ex)
        for fn in (lambda: e.slab_argmin(0, 1, 0, lab.ptr), lambda: e.slab_argmin(lab.ptr, 1, 0, 0), lambda: e.slab_argmin(lab.ptr, -1, 0, cost.ptr),
                   lambda: e.slab_argmin_finish(0, 1, lab.ptr, cost.ptr), lambda: e.slab_argmin_finish(lab.ptr, 1, 0, cost.ptr)):
            try:
                fn()
                raise AssertionError("a bad argument was accepted")
            except api.LesHipError as ex:
                assert f"error {api.LES_HIP_ERR_ARG}" in str(ex), str(ex)
        e.synchronize()
        assert (lab.download((P * 16,), np.uint8) == 0x5A).all() and (cost.download((P * 4,), np.uint8) == 0x5A).all()
    finally:
        for b in big + [lab, cost]:
            b.free()
        e.close()


# ------------------------------------------------------------------------------------------------ 6. drivers
def case_driver_wta(lib, device, device_cuts):
    """FastGCStereo on the cones crop (crossview_cases.driver: image-based energy, ground truth, two layers), device evaluation so that every row has
    its pairwise sum.  -> the rows compared"""
    out = {}
    # the yardstick: the initial row of a default run with the same seed (one random plane per finest-layer cell)
    st, e = cv.driver(lib, device, device_cuts, evaluate_on_device=True)
    try:
        st.run(0, (0,), 0)
        random_row = st.log[0]
    finally:
        e.close()
    st, e = cv.driver(lib, device, device_cuts, evaluate_on_device=True)
    try:
        lab, raw = st.wta((0,))
        assert len(st.log) == 1 and st.log[0]["mode"] == 0 and same(lab, raw) and same(raw, st.raw_labelings[0])
        wta_row = st.log[0]
        print(f"cones crop, left view: random start all {random_row['all']:.2f} % energy {random_row['energy']:.1f}; "
              f"WTA all {wta_row['all']:.2f} % nonocc {wta_row['nonocc']:.2f} % energy {wta_row['energy']:.1f}")
        assert wta_row["all"] < random_row["all"], (wta_row["all"], random_row["all"])
        assert wta_row["energy"] < random_row["energy"], (wta_row["energy"], random_row["energy"])
        out.update(random_all=random_row["all"], wta_all=wta_row["all"], random_energy=random_row["energy"], wta_energy=wta_row["energy"])
        # the host route logs the same rates (its smooth is NaN: no graph-cut context)
        st.evaluate_on_device = False
        st.wta((0,))
        assert st.log[0]["all"] == wta_row["all"] and st.log[0]["nonocc"] == wta_row["nonocc"] and st.log[0]["smooth"] != st.log[0]["smooth"]
        st.evaluate_on_device = True
        # two views: one row per view, the post-processing changes the left map, the raw maps are the single-view ones
        lab2, raw2 = st.wta((0, 1))
        assert [r["mode"] for r in st.log] == [0, 1] and "all" not in st.log[1] and same(raw2, raw) and sorted(st.raw_labelings) == [0, 1]
        assert ec.same_float(st.log[0]["energy"], wta_row["energy"]) and not same(lab2, raw2) and np.isfinite(lab2).all()
        lab3, _ = st.wta((0, 1), post_process=False, subpixel=False)
        assert same(lab3, st.raw_labelings[0]) and (lab3[..., 2] == np.rint(lab3[..., 2])).all()
        # a run that starts from the WTA maps: its first row is the WTA map re-scored, and one graph-cut iteration does not end above it
        st.log = []                                         # (run() appends to the log)
        st.run(1, (0,), 0, labeling="wta")
        assert st.log[0]["all"] == wta_row["all"], (st.log[0]["all"], wta_row["all"])
        print(f"run(1, pmInit=0, labeling='wta'): energy {st.log[0]['energy']:.1f} -> {st.log[-1]['energy']:.1f}, all {st.log[0]['all']:.2f} -> {st.log[-1]['all']:.2f} %")
        assert st.log[-1]["energy"] <= st.log[0]["energy"], (st.log[0]["energy"], st.log[-1]["energy"])
        out.update(run_start=st.log[0]["energy"], run_end=st.log[-1]["energy"])
        try:
            st.run(1, (0,), 0, labeling="wat")
            raise AssertionError("an unknown start was accepted")
        except ValueError:
            pass
        # a WTA map as the second labelling of a fusion move (a device tensor and a host array): the energy does not rise
        start = st.raw_labelings[0]
        t_lab, _ = e.wta_labels(0, device=device)
        for other in (t_lab, raw):
            fused = st.fuse(start, [other])
            E0, E1 = st.log[0]["energy"], st.log[-1]["energy"]
            assert E1 <= E0 + fc.RISE * abs(E0), (E0, E1)
            own = (fused.view(np.uint32) == start.view(np.uint32)).all(-1)
            assert (own | (fused.view(np.uint32) == raw.view(np.uint32)).all(-1)).all()
        out.update(fuse_before=E0, fuse_after=E1)
        st2, e2 = cv.driver(lib, device, device_cuts, world=2)
        try:
            for fn in (lambda: st2.wta((0,)), lambda: st2.run(1, (0,), 0, labeling="wta")):
                try:
                    fn()
                    raise AssertionError("world = 2 was accepted")
                except NotImplementedError:
                    pass
        finally:
            e2.close()
    finally:
        e.close()
    return out


def case_driver_midv(lib, device, monkeypatch, layers=None, **opts):
    """MidV3(init="wta") from the pair alone runs end to end; MidV2() / MidV3() without init return the same bits whether or not init=None is passed.
    layers, opts: as crossview_cases.case_driver_midv2."""
    from localexpstereo_amd import stereo
    from tests import costvol_cases as cc
    if layers is not None:
        monkeypatch.setattr(stereo, "_layers", layers)
    kw = dict(iterations=1, pmIterations=1, device=device, lib=lib, **opts)
    imL, imR, gt = cc.cones_pair()
    data3 = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
    st, lab, raw = stereo.MidV3(data3, None, None, doDual=True, init="wta", evaluate_on_device=True, **kw)
    assert lab.shape == gt.shape + (4,) and np.isfinite(lab).all() and len(st.log) == 4
    st_r, lab_r, raw_r = stereo.MidV3(data3, None, None, doDual=True, evaluate_on_device=True, **kw)
    print(f"MidV3 from the pair: start all {st.log[0]['all']:.2f} % energy {st.log[0]['energy']:.1f} (random start {st_r.log[0]['all']:.2f} %, {st_r.log[0]['energy']:.1f}); "
          f"end {st.log[-1]['all']:.2f} % (random start {st_r.log[-1]['all']:.2f} %)")
    assert st.log[0]["all"] < st_r.log[0]["all"]
    _, lab_a, raw_a = stereo.MidV3(data3, None, None, doDual=True, evaluate_on_device=True, init=None, **kw)
    assert same(lab_a, lab_r) and same(raw_a, raw_r)
    data2 = cv.cones_data()
    _, lab_a, raw_a = stereo.MidV2(data2, **kw)
    _, lab_b, raw_b = stereo.MidV2(data2, init=None, **kw)
    assert same(lab_a, lab_b) and same(raw_a, raw_b)
    st2, lab_c, _ = stereo.MidV2(data2, init="wta", **kw)
    assert np.isfinite(lab_c).all() and not same(lab_c, lab_a)
    return dict(midv3_wta_start_all=st.log[0]["all"], midv3_random_start_all=st_r.log[0]["all"])
