"""Cases of the speckle filter (csrc/les_speckle.h: les_hip_speckle_mask, les_hip_post_process_speckle, FastGCStereo(speckle=)), shared by the
simulator tests (-m "not gpu") and the MI355X tests (-m gpu) of test_speckle.py.  `lib` = the simulator build's path, None = the HIP build.

The definition: d(p) = (a x + b y) + c in float32, un-fused; two 4-neighbours are connected iff both d are finite and |d(p) - d(q)| <= max_diff
(a float32 subtraction and compare); a non-finite pixel is a component of its own; root = the smallest linear index y W + x of the component,
size = its pixel count, speckle iff size <= max_size.  The restatement is a plain union-find over the connected edges; roots, sizes and masks
are exact integers and are compared bit for bit."""
import functools

import numpy as np

from localexpstereo_amd import api
from tests import post_cases as pcs

F32 = np.float32
INF32 = F32(np.inf)


# ------------------------------------------------------------------------------------------------ restatement
def edge_list(d, max_diff):
    """The connected 4-neighbour pairs (p, q), p > q, as two int64 arrays of linear indices."""
    d = np.asarray(d, F32)
    H, W = d.shape
    fin = np.isfinite(d)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    t = F32(max_diff)
    with np.errstate(all="ignore"):
        h = fin[:, 1:] & fin[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= t)
        v = fin[1:] & fin[:-1] & (np.abs(d[1:] - d[:-1]) <= t)
    return np.concatenate([idx[:, 1:][h], idx[1:][v]]), np.concatenate([idx[:, :-1][h], idx[:-1][v]])


def components_ref(d, max_diff):
    """Union-find over the connected edges, the larger root under the smaller: (root, size), H x W int32 each."""
    H, W = np.asarray(d).shape
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p, q in zip(*(a.tolist() for a in edge_list(d, max_diff))):
        a, b = find(p), find(q)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(H * W)], np.int64)
    size = np.bincount(root, minlength=H * W)[root]
    return root.astype(np.int32).reshape(H, W), size.astype(np.int32).reshape(H, W)


def speckle_ref(d, max_size, max_diff):
    """(mask 255 / 0, root, size)."""
    root, size = components_ref(d, max_diff)
    return np.where(size <= max_size, 255, 0).astype(np.uint8), root, size


def components_flood(d, max_diff):
    """The definition read literally, for tiny maps: a flood fill from every pixel not reached yet, in linear order."""
    d = np.asarray(d, F32)
    H, W = d.shape
    root = np.full((H, W), -1, np.int32)
    t = F32(max_diff)

    def connected(a, b):
        with np.errstate(all="ignore"):
            return bool(np.isfinite(a) and np.isfinite(b) and np.abs(F32(a) - F32(b)) <= t)

    for y0 in range(H):
        for x0 in range(W):
            if root[y0, x0] >= 0:
                continue
            root[y0, x0] = y0 * W + x0
            todo = [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and root[yy, xx] < 0 and connected(d[y, x], d[yy, xx]):
                        root[yy, xx] = y0 * W + x0
                        todo.append((yy, xx))
    size = np.bincount(root.ravel(), minlength=H * W)[root]
    return root, size.astype(np.int32)


def case_restatement(with_scipy):
    """components_ref == the flood fill on tiny maps of every input kind; with_scipy: also == scipy's connected components of the same edges."""
    assert {"les_hip_speckle_mask", "les_hip_speckle_tile", "les_hip_post_process_speckle"} <= set(api.SYMBOLS)      # the entries this restates
    n = 0
    for H, W in ((1, 1), (1, 9), (7, 1), (6, 7), (9, 12)):
        for name in INPUTS:
            lab, max_size, max_diff = make_input(name, H, W, th=3, tw=4)
            d = pcs.disparities(lab)
            root, size = components_ref(d, max_diff)
            froot, fsize = components_flood(d, max_diff)
            assert np.array_equal(root, froot) and np.array_equal(size, fsize), (name, H, W)
            if with_scipy:
                from scipy.sparse import coo_matrix
                from scipy.sparse.csgraph import connected_components
                p, q = edge_list(d, max_diff)
                g = coo_matrix((np.ones(p.size, np.int8), (p, q)), shape=(H * W, H * W))
                ncomp, lab_of = connected_components(g, directed=False)
                first = np.full(ncomp, H * W, np.int64)
                np.minimum.at(first, lab_of, np.arange(H * W))
                assert np.array_equal(first[lab_of].reshape(H, W), root), (name, H, W)
                assert ncomp == np.unique(root).size
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ inputs
def _fronto(d):
    lab = np.zeros(d.shape + (4,), F32)
    lab[..., 2] = d
    return lab


def _plant_row_major(d, y0, x0, w, n, value):
    """n pixels in row-major order of the window of width w at (y0, x0): full rows and a partial one, connected."""
    H, W = d.shape
    k = 0
    for y in range(y0, H):
        for x in range(x0, min(x0 + w, W)):
            if k == n:
                return
            d[y, x] = value
            k += 1


def in_constant(H, W, th, tw, rng):
    return _fronto(np.full((H, W), 3.0, F32)), 10, 1.0


def in_checkerboard(H, W, th, tw, rng):
    ys, xs = np.mgrid[0:H, 0:W]
    return _fronto(np.where((ys + xs) % 2 == 0, F32(0.0), np.nextafter(F32(1.0), INF32)).astype(F32)), 1, 1.0


def in_serpentine(H, W, th, tw, rng):
    """A one-pixel-wide path: every even row, joined at alternating ends through the odd rows; it crosses every tile of its rows."""
    d = np.full((H, W), 10.0, F32)
    d[0::2] = 0.0
    for k, y in enumerate(range(1, H, 2)):
        d[y, W - 1 if k % 2 == 0 else 0] = 0.0
    return _fronto(d), 2 * tw, 1.0


def in_comb(H, W, th, tw, rng):
    """The top row and every even column below it: teeth through every tile row."""
    d = np.full((H, W), 10.0, F32)
    d[0] = 0.0
    d[:, 0::2] = 0.0
    return _fronto(d), H - 1, 1.0


def in_blobs(H, W, th, tw, rng):
    """Two constant surfaces and planted blobs (row-major fills of windows of random width) of sizes around max_size."""
    max_size = 12
    d = np.full((H, W), 5.0, F32)
    d[:, W // 2:] = 9.0
    for k in range(max(2, H * W // 150)):
        n = int(rng.integers(max_size - 4, max_size + 6))
        _plant_row_major(d, int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 8)), n, F32(20.0 + 3.0 * (k % 7)))
    return _fronto(d), max_size, 1.0


def in_exact_sizes(H, W, th, tw, rng):
    """Components of exactly max_size and max_size + 1 pixels on a constant map, wherever the shape has room for them."""
    max_size = 9
    d = np.full((H, W), 4.0, F32)
    if H == 1 or W == 1:
        flat = d.reshape(-1)
        flat[1:1 + max_size] = 30.0
        flat[2 + max_size:3 + 2 * max_size] = 40.0
    else:
        _plant_row_major(d, 1, 1, 4, max_size, F32(30.0))               # rows 1 .. 3, columns 1 .. 4
        _plant_row_major(d, 1, 7, 5, max_size + 1, F32(40.0))           # rows 1 .. 2, columns 7 .. 11
        _plant_row_major(d, th - 1, tw - 2, 4, max_size, F32(50.0))     # across a tile corner
        _plant_row_major(d, th + 3, tw - 3, 5, max_size + 1, F32(60.0))
    return _fronto(d), max_size, 1.0


def in_staircase(H, W, th, tw, rng):
    """Steps of exactly max_diff (connected) and nextafter(max_diff, inf) (not), along x in the upper half and along y in the lower one."""
    t = F32(0.75)
    up = np.nextafter(t, INF32)
    saw = np.array([0.0, t, 0.0, up], F32)
    d = np.empty((H, W), F32)
    d[:] = saw[np.arange(W) % 4][None, :]
    d[H // 2:] = saw[np.arange(H - H // 2) % 4][:, None] + F32(8.0)       # 8 + 0.75 (+ 1 ulp of 0.75) is exact in float32
    return _fronto(d), 3, float(t)


def in_slanted(H, W, th, tw, rng):
    """Slanted planes: d comes from a, b and c.  Left part (0.25, -0.125, c): every neighbour within 0.3; right part (0.5, 0.125, c): only the
    vertical ones, so its columns are components; a block of a third plane on top."""
    lab = np.zeros((H, W, 4), F32)
    lab[:, :, :3] = (0.25, -0.125, 2.0)
    lab[:, W // 2:, :3] = (0.5, 0.125, 40.0)
    lab[H // 3:H // 3 + 3, W // 4:W // 4 + 5, :3] = (-0.25, 0.25, 90.0)
    return lab, 14, 0.3


def in_nonfinite(H, W, th, tw, rng):
    """NaN of both signs, +-inf and huge disparities, scattered and in runs, on a constant map."""
    d = np.full((H, W), 3.0, F32)
    m = rng.random((H, W))
    vals = [np.nan, -np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1e12]
    for k, v in enumerate(vals):
        d[(m >= 0.03 * k) & (m < 0.03 * (k + 1))] = v
    if H > 2:
        d[H // 2, : max(1, W // 2)] = np.nan                              # a run of NaN: every pixel alone
        d[H // 2 - 1, W // 3:] = np.inf                                   # a run of +inf: inf - inf is NaN, and they are not finite anyway
    if H > 4:
        d[H // 4, :] = 1e12                                               # a run of one huge value: connected
        d[H // 4 + 1, 0::2] = 3.0e38                                      # |3e38 - (-3e38)| overflows: not connected
        d[H // 4 + 1, 1::2] = -3.0e38
    return _fronto(d), 6, 1.0


INPUTS = dict(constant=in_constant, checkerboard=in_checkerboard, serpentine=in_serpentine, comb=in_comb, blobs=in_blobs, exact_sizes=in_exact_sizes,
              staircase=in_staircase, slanted=in_slanted, nonfinite=in_nonfinite)
BIG_INPUTS = ("constant", "serpentine", "comb", "blobs", "nonfinite")   # at the shape of many workgroups: the chains, the crossings and the races


def make_input(name, H, W, th, tw):
    seed = 1000 + 31 * H + W + sum(map(ord, name))
    lab, max_size, max_diff = INPUTS[name](H, W, th, tw, np.random.default_rng(seed))
    return np.ascontiguousarray(lab, F32), int(max_size), float(max_diff)


@functools.lru_cache(maxsize=None)
def reference(name, H, W, th, tw):
    """(labels, max_size, max_diff, mask, root, size) of an input, computed once and shared by the simulator and the MI355X tests; read-only."""
    lab, max_size, max_diff = make_input(name, H, W, th, tw)
    out = (lab, max_size, max_diff) + speckle_ref(pcs.disparities(lab), max_size, max_diff)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def tile(lib):
    L = api.load(lib)
    th, tw = api.C.c_int(0), api.C.c_int(0)
    assert L.les_hip_speckle_tile(api.C.byref(th), api.C.byref(tw)) == 0
    assert th.value > 0 and tw.value > 0
    return th.value, tw.value


def shapes(lib):
    th, tw = tile(lib)
    return [(1, 1), (1, 2 * tw + 1), (2 * th + 1, 1), (th, tw), (th + 1, tw + 1), (2 * th + 3, 3 * tw + 5)]


def big_shape(lib):
    """16 x 16 tiles and a remainder: many workgroups merge at once (135 000 pixels at the 16 x 32 tile)."""
    th, tw = tile(lib)
    return 16 * th + 5, 16 * tw + 7


# ------------------------------------------------------------------------------------------------ device plumbing
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def context(lib, H, W, windR=2, im=None):
    """A context whose images are `im` (a pair or one image for both; None: constant colour)."""
    if im is None:
        im = np.full((H, W, 3), 90, np.uint8)
    imL, imR = im if isinstance(im, tuple) else (im, im)
    return pcs.context(lib, imL, imR, windR)


def device_components(e, lib, lab, max_size, max_diff):
    """The three forms of the call -- both outputs, each of root / size NULL, both NULL -- and a repeat: (mask, root, size) as arrays."""
    import torch
    dev = _dev(lib)
    t = torch.from_numpy(np.array(lab, F32)).to(dev)
    mask, root, size = (a.cpu().numpy() for a in e.speckle_mask(t, max_size, max_diff, components=True, device=dev))
    again = [a.cpu().numpy() for a in e.speckle_mask(t, max_size, max_diff, components=True, device=dev)]
    assert np.array_equal(mask, again[0]) and np.array_equal(root, again[1]) and np.array_equal(size, again[2]), "a second call differs"
    assert np.array_equal(e.speckle_mask(lab, max_size, max_diff, device=dev).cpu().numpy(), mask), "mask alone differs"
    H, W = mask.shape
    for with_root in (True, False):
        m = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        o = torch.full((H, W), -7, dtype=torch.int32, device=dev)
        e.speckle_mask_ptr(t.data_ptr(), max_size, max_diff, m.data_ptr(), o.data_ptr() if with_root else None, None if with_root else o.data_ptr())
        assert np.array_equal(m.cpu().numpy(), mask) and np.array_equal(o.cpu().numpy(), root if with_root else size), "a NULL output changes the others"
    assert np.array_equal(t.cpu().numpy().view(np.uint32), np.asarray(lab).view(np.uint32)), "the labels were written"
    return mask, root, size


def case_components(lib, name, H, W):
    """root, size and mask == the restatement's, bit for bit."""
    th, tw = tile(lib)
    lab, max_size, max_diff, mask, root, size = reference(name, H, W, th, tw)
    e = context(lib, H, W)
    try:
        got = device_components(e, lib, lab, max_size, max_diff)
        zero = e.speckle_mask(lab, 0, max_diff, device=_dev(lib)).cpu().numpy()
    finally:
        e.close()
    assert np.array_equal(got[1], root), f"{name} {H} x {W}: {int((got[1] != root).sum())} roots differ"
    assert np.array_equal(got[2], size), f"{name} {H} x {W}: {int((got[2] != size).sum())} sizes differ"
    assert np.array_equal(got[0], mask), f"{name} {H} x {W}: {int((got[0] != mask).sum())} mask bytes differ"
    assert not zero.any(), "max_size 0 marks pixels"
    if name == "exact_sizes" and H * W >= 2 * max_size + 4 and (min(H, W) == 1 or (H > th + 6 and W > tw + 3)):
        assert (size == max_size).any() and (size == max_size + 1).any() and mask[size == max_size].all() and not mask[size == max_size + 1].any()
    return dict(components=int(np.unique(root).size), speckle_pixels=int((mask > 0).sum()), largest=int(size.max()))


def _refused(call, code):
    try:
        call()
    except api.LesHipError as ex:
        assert f"error {code}" in str(ex), str(ex)
        return 1
    raise AssertionError("a bad argument was accepted")


def case_refusals(lib):
    """Every refusal of les_hip_speckle_mask and les_hip_post_process_speckle; a refused call writes nothing."""
    import torch
    H, W, dev = 6, 9, _dev(lib)
    lab = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    labR = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    mask = torch.full((H, W), 0x5A, dtype=torch.uint8, device=dev)
    n = 0
    e = context(lib, H, W)
    try:
        A, U = api.LES_HIP_ERR_ARG, api.LES_HIP_ERR_UNSUPPORTED
        for max_size, max_diff in ((-1, 1.0), (3, -0.5), (3, float("nan")), (3, -float("inf"))):
            n += _refused(lambda: e.speckle_mask_ptr(lab.data_ptr(), max_size, max_diff, mask.data_ptr()), A)
            n += _refused(lambda: e.post_process(lab.data_ptr(), labR.data_ptr(), 1.5, 10.0, speckle=(max_size, max_diff)), A)
            n += _refused(lambda: e.post_process(lab.data_ptr(), None, 1.5, 10.0, speckle=(max_size, max_diff)), A)
        n += _refused(lambda: e.speckle_mask_ptr(None, 3, 1.0, mask.data_ptr()), A)
        n += _refused(lambda: e.speckle_mask_ptr(lab.data_ptr(), 3, 1.0, None), A)
        n += _refused(lambda: e.post_process(None, None, 1.5, 10.0, speckle=(3, 1.0)), A)
        assert (mask.cpu().numpy() == 0x5A).all() and not lab.cpu().numpy().any() and not labR.cpu().numpy().any()
        # max_diff = +inf is a valid threshold: every finite pixel joins one component
        assert (e.speckle_mask(lab, H * W, float("inf"), device=dev).cpu().numpy() == 255).all()
    finally:
        e.close()
    e = context(lib, H, W, windR=32)
    try:
        n += _refused(lambda: e.post_process(lab.data_ptr(), labR.data_ptr(), 1.5, 10.0, speckle=(3, 1.0)), U)
        n += _refused(lambda: e.post_process(None, labR.data_ptr(), 1.5, 10.0, speckle=(3, 1.0)), U)
        n += _refused(lambda: e.post_process(lab.data_ptr(), labR.data_ptr(), 1.5, 10.0), U)
    finally:
        e.close()
    return n


# ------------------------------------------------------------------------------------------------ post-processing
POST_SHAPE = (40, 70)           # 3 x 3 tiles of 16 x 32
POST_WINDR = 3
POST_SPECKLE = (12, 1.0)
RANDOM_GUIDE_SEEDS = (41, 42)   # (left, right) guide seeds of the random-guide cases, chosen on the simulator build (see case_post_islands)


def island_scene(H, W, seed):
    """Both views hold the fronto-parallel surface of disparity 2, consistent with each other.  Islands of other disparities are planted so that they
    AGREE across the views (a left island of disparity k at columns x is a right island at columns x - k): the left-right check passes them and
    only the speckle filter finds them.  A few more are planted in one view only (the check finds those too), one of them larger than max_size.
    Tagged (post_cases.tag)."""
    rng = np.random.default_rng(seed)
    LL, LR = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    LL[..., 2] = LR[..., 2] = 2.0
    for k in range(6):
        disp = 5.0 + k
        h, w = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(12, W - w))
        LL[y0:y0 + h, x0:x0 + w, 2] = disp
        LR[y0:y0 + h, x0 - int(disp):x0 - int(disp) + w, 2] = disp
    for lab in (LL, LR):
        for k in range(3):
            y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 4))
            lab[y0:y0 + 2, x0:x0 + 3, 2] = 20.0 + k
    LL[H - 8:H - 3, 20:26, 2] = 30.0                                    # 30 pixels: above max_size, found by the check alone
    return pcs.tag(LL, LR)


def post_speckle_ref(labs, ims, windR, thr, omega, max_size, max_diff):
    """The restatement of post_cases composed with the widened mask.  labs: (LL, LR), either may be None (the one-view form: the speckle mask
    alone).  -> per view present (out, near-ties, stats, speckle mask), None for an absent one."""
    both = labs[0] is not None and labs[1] is not None
    lr = pcs.lr_check_ref(pcs.disparities(labs[0]), pcs.disparities(labs[1]), thr) if both else (None, None)
    res = []
    for lab, f, im in zip(labs, lr, ims):
        if lab is None:
            res.append(None)
            continue
        lab = np.array(lab, F32)
        sp = speckle_ref(pcs.disparities(lab), max_size, max_diff)[0] > 0
        fail = sp | (f > 0) if both else sp
        failb = np.where(fail, 255, 0).astype(np.uint8)
        filled, _ = pcs.fill_ref(lab, failb, pcs.dilate3(failb))
        out, near, stats = pcs.median_ref(filled, failb, im, windR, omega)
        res.append((out, near, stats, sp))
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case_post_zero(lib):
    """Two views, max_size 0: the bytes of les_hip_post_process, on scenes of post_cases."""
    n = 0
    for H, W, scene, windR in ((30, 52, pcs.scene_surfaces(30, 52, 9), 4), (20, 41, pcs.scene_corners(20, 41), 2), (20, 30, pcs.scene_random_nonfinite(20, 30, 5), 2)):
        im = (pcs.image(H, W, 21), pcs.image(H, W, 22))
        e = pcs.context(lib, *im, windR)
        try:
            old = e.post_process_host(*scene)
            new = e.post_process_host(*scene, speckle=(0, 1.0))
            for m in (0, 1):
                one = e.post_process_host(*(scene[v] if v == m else None for v in (0, 1)), speckle=(0, 1.0))
                assert one[1 - m] is None and np.array_equal(_bits(one[m]), _bits(scene[m])), "one view, max_size 0: the labels changed"
        finally:
            e.close()
        for o, g, s in zip(old, new, scene):
            assert np.array_equal(_bits(o), _bits(g))
            n += int((_bits(o) != _bits(s)).any(-1).sum())
    assert n > 0
    return n


def case_post_islands(lib, guide, views):
    """views (0, 1): the widened mask; (0,) / (1,): the one-view form of that view.  guide "const": one colour, every weight is exactly 1 and the
    result equals the restatement bit for bit.  guide "random": post_cases.image of RANDOM_GUIDE_SEEDS; near-ties are accepted as
    post_cases.compare_restatement accepts them, under its condition moves <= 0.001 max(failed, 1).  Seen on the simulator build with seeds
    (41, 42), the first pair tried: two views failed 163 / 203 pixels (50 / 46 of them speckles), one view 50 / 46; the restatement lists 0 near-tie
    candidates in every case, so 0 moves."""
    H, W = POST_SHAPE
    windR, thr, omega = POST_WINDR, 1.5, 10.0
    scene = island_scene(H, W, 17)
    ims = (np.full((H, W, 3), 77, np.uint8),) * 2 if guide == "const" else tuple(pcs.image(H, W, s) for s in RANDOM_GUIDE_SEEDS)
    labs = tuple(scene[m] if m in views else None for m in (0, 1))
    e = pcs.context(lib, *ims, windR)
    try:
        got = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=POST_SPECKLE)
        again = e.post_process_host(*labs, threshold=thr, omega=omega, speckle=POST_SPECKLE)
        plain = e.post_process_host(*scene, threshold=thr, omega=omega) if len(views) == 2 else None
    finally:
        e.close()
    ref = post_speckle_ref(labs, ims, windR, thr, omega, *POST_SPECKLE)
    out = {}
    for m in views:
        want, near, stats, sp = ref[m]
        assert np.array_equal(_bits(got[m]), _bits(again[m])), "a repeated call differs"
        assert sp.any() and stats["failed"] >= int(sp.sum())
        if guide == "const":
            assert np.array_equal(_bits(got[m]), _bits(want)), f"view {m}: {int((_bits(got[m]) != _bits(want)).any(-1).sum())} pixels differ from the restatement"
            moves = 0
        else:
            moves = pcs.compare_restatement(got[m], want, near, "LR"[m])
            print(f"view {m}: failed {stats['failed']}, near-tie candidates {stats['near_ties']}, near-tie moves {moves}")
            assert moves <= 0.001 * max(stats["failed"], 1), stats
        changed = (_bits(got[m]) != _bits(labs[m])).any(-1)
        assert changed.any()
        if len(views) == 1:
            assert not changed[~sp].any(), "a pixel outside the speckle mask changed"
            assert np.isin(got[m][..., 3], labs[m][..., 3]).all(), "a label that is not of the input map was written"
        else:
            assert (_bits(got[m]) != _bits(plain[m])).any(), "the widened mask changed nothing"
        out[m] = dict(failed=stats["failed"], speckle=int(sp.sum()), changed=int(changed.sum()), near_ties=stats["near_ties"], moves=moves)
    return out


# ------------------------------------------------------------------------------------------------ the driver
DRIVER_SPECKLE = (100, 1.0)


def same(a, b):
    return a is b or (a is not None and b is not None and np.array_equal(_bits(a), _bits(b)))


def case_driver_off(lib, device):
    """speckle=None: run, wta and sgm return the bytes they return without the keyword."""
    from tests import sgm_cases as sg
    outs = []
    for kw in ({}, dict(speckle=None)):
        st, e, keep = sg.driver(lib, device, "none", evaluate_on_device=True, **kw)
        try:
            res = [st.wta((0,)), st.wta((0, 1)), st.sgm((0,)), st.sgm((0, 1))]
            st.log = []                                        # (run() appends to the log it finds)
            res.append(st.run(0, (0,), 0, labeling="wta"))
            n_rows, st.log = len(st.log), []
            res.append(st.run(0, (0, 1), 0, labeling="wta"))
            outs.append((res, n_rows, len(st.log)))
        finally:
            e.close()
            del keep
    for a, b in zip(outs[0][0], outs[1][0]):
        assert same(a[0], b[0]) and same(a[1], b[1])
    assert outs[0][1:] == outs[1][1:] == (1, 2), outs[0][1:]       # one view: the start row alone; two views: the final row after it
    assert same(outs[0][0][0][0], outs[0][0][0][1]) and not same(outs[0][0][1][0], outs[0][0][1][1])     # one view raw, two views post-processed


def case_driver_on(lib, device):
    """speckle=(S, t).  One view: the returned map differs from the raw one only inside the raw map's speckle mask, equals
    post_process(raw, None, speckle=), and run()'s log has its final row (recost_after_post honoured).  Two views: the returned map equals
    post_process(rawL, rawR, speckle=)."""
    from tests import sgm_cases as sg
    S, t = DRIVER_SPECKLE
    out = {}
    st, e, keep = sg.driver(lib, device, "none", evaluate_on_device=True, speckle=DRIVER_SPECKLE, recost_after_post=True)
    try:
        H, W = e.H, e.W
        calls = dict(wta=lambda v: st.wta(v), sgm=lambda v: st.sgm(v), run=lambda v: st.run(0, v, 0, labeling="wta"))
        for name, call in calls.items():
            st.log = []                                        # (run() appends to the log it finds)
            lab, raw = call((0,))
            assert same(raw, st.raw_labelings[0]) and sorted(st.raw_labelings) == [0]
            sp = speckle_ref(pcs.disparities(raw), S, t)[0] > 0
            changed = (_bits(lab) != _bits(raw)).any(-1)
            assert sp.any() and changed.any() and not changed[~sp].any(), (name, int(sp.sum()), int(changed.sum()), int(changed[~sp].sum()))
            assert same(lab, e.post_process_host(raw, None, 1.5, st.p["omega"], speckle=DRIVER_SPECKLE)[0]), name
            if name == "run":
                assert [r["index"] for r in st.log] == [0, 1], st.log
                assert st.log[1]["data"] != st.log[0]["data"] and np.isfinite(st.log[1]["energy"])
            out[name] = dict(speckle=int(sp.sum()), changed=int(changed.sum()))
            st.log = []
            lab2, raw2 = call((0, 1))
            want = e.post_process_host(st.raw_labelings[0], st.raw_labelings[1], 1.5, st.p["omega"], speckle=DRIVER_SPECKLE)
            plain = e.post_process_host(st.raw_labelings[0], st.raw_labelings[1], 1.5, st.p["omega"])
            assert same(raw2, st.raw_labelings[0]) and same(lab2, want[0]) and not same(lab2, plain[0]), name
            if name == "run":
                assert [r["index"] for r in st.log] == [0, 1], st.log
        # wta(post_process=False) stays raw
        lab, raw = st.wta((0,), post_process=False)
        assert same(lab, raw)
    finally:
        e.close()
        del keep
    return out
