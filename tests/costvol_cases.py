"""AD-Census matching-cost volumes built on the device (csrc/les_costvol.h): the definition restated in numpy, and the cases tests/test_costvol.py
runs on the CPU simulator build (lib = its path, tensors on "cpu") and on the MI355X (lib = None: the product library, tensors on "cuda").

Everything but the tables is integer arithmetic and one f32 add, so the device results are compared BYTE for byte with the restatement evaluated on
the tables the library returns; the tables themselves are compared with the numpy formula to 1 ulp of f32 (the room two correctly implemented
double exp's can leave after the one rounding to f32)."""
import ctypes as C
import os

import numpy as np

from localexpstereo_amd import api
from tests.util import GOLDEN

F = np.float32
CHUNK = 64                      # kCvDC of csrc/les_costvol.h: the slices one workgroup of les_costvol_kernel walks
SEGMENT = 256                   # kCvTX: the pixels of a row one workgroup owns
GUARD = 64                      # guard floats on either side of a device volume
GUARD_BITS = 0x7FC0BEEF          # (as int32) a quiet NaN with a payload: no cost equals it

OFFSETS = [(dy, dx) for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0)]       # visiting order: bit k = OFFSETS[k]


# ------------------------------------------------------------------------------------------------ the restatement
def grey(im):
    im = np.asarray(im, np.int64)
    return (77 * im[..., 2] + 150 * im[..., 1] + 29 * im[..., 0] + 128) >> 8


def census(im):
    """uint64 [H][W]: bit k is 1 iff the grey value of neighbour OFFSETS[k] (coordinates clamped to the image) is below the centre's."""
    g = grey(im)
    H, W = g.shape
    p = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    sig = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(OFFSETS):
        sig |= (p[3 + dy:3 + dy + H, 4 + dx:4 + dx + W] < g).astype(np.uint64) << np.uint64(k)
    return sig


def census_loop(im):
    """The same, pixel by pixel, straight from the definition."""
    im = np.asarray(im)
    H, W = im.shape[:2]

    def g(y, x):
        b, gr, r = (int(v) for v in im[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])
        return (77 * r + 150 * gr + 29 * b + 128) >> 8

    sig = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            s, k = 0, 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dx == 0 and dy == 0:
                        continue
                    if g(y + dy, x + dx) < g(y, x):
                        s |= 1 << k
                    k += 1
            assert k == 62
            sig[y, x] = s
    return sig


def popcount(a):
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


def tables(lambda_ad=10.0, lambda_census=30.0):
    s, h = np.arange(766, dtype=np.float64), np.arange(63, dtype=np.float64)
    return (0.5 * (1.0 - np.exp(-(s / 3.0) / float(lambda_ad)))).astype(F), (0.5 * (1.0 - np.exp(-h / float(lambda_census)))).astype(F)


def partner_columns(W, d, mode):
    x = np.arange(W)
    return np.clip(x - d if mode == 0 else x + d, 0, W - 1)


def pair_terms(imL, imR, D, mode, d0=0):
    """s, h as int64 [D][H][W]."""
    I, J = (imL, imR) if mode == 0 else (imR, imL)
    sI, sJ = census(I), census(J)
    Ii, Ji = np.asarray(I, np.int64), np.asarray(J, np.int64)
    H, W = sI.shape
    s, h = np.empty((D, H, W), np.int64), np.empty((D, H, W), np.int64)
    for k in range(D):
        xp = partner_columns(W, k + d0, mode)
        s[k] = np.abs(Ii - Ji[:, xp]).sum(-1)
        h[k] = popcount(sI ^ sJ[:, xp])
    return s, h


def volume(imL, imR, D, mode, d0, ta, tc):
    s, h = pair_terms(imL, imR, D, mode, d0)
    return (np.asarray(ta, F)[s] + np.asarray(tc, F)[h]).astype(F)           # one f32 add


def ad_volume(imL, imR, D, mode=0, d0=0):
    """The plain AD volume with the same clamping: mean_c |delta| / 255."""
    s, _ = pair_terms(imL, imR, D, mode, d0)
    return (s / 3.0 / 255.0).astype(F)


# ------------------------------------------------------------------------------------------------ device plumbing
def _dev(lib):
    return "cuda" if lib is None else "cpu"


def _up(a, lib):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(_dev(lib))


def dev_census(lib, im):
    import torch
    H, W = im.shape[:2]
    t = _up(im, lib)
    sig = torch.zeros((H, W), dtype=torch.int64, device=_dev(lib))
    api.census(t.data_ptr(), sig.data_ptr(), H, W, lib=lib)
    return sig.cpu().numpy().view(np.uint64)


def dev_volume(lib, imL, imR, D, mode, d0=0, lambda_ad=10.0, lambda_census=30.0, lead=GUARD):
    """les_hip_build_cost_volume into a buffer with `lead` guard floats before and GUARD after the volume; asserts the guards untouched."""
    import torch
    H, W = imL.shape[:2]
    n = D * H * W
    buf = torch.full((lead + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=_dev(lib))
    tl, tr = _up(imL, lib), _up(imR, lib)
    api.build_cost_volume(tl.data_ptr(), tr.data_ptr(), buf.data_ptr() + 4 * lead, D, H, W, mode, d0=d0, lambda_ad=lambda_ad, lambda_census=lambda_census, lib=lib)
    out = buf.cpu().numpy()
    assert (out[:lead] == GUARD_BITS).all() and (out[lead + n:] == GUARD_BITS).all(), "guard floats overwritten"
    return out[lead:lead + n].view(F).reshape(D, H, W).copy()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def images(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
def case_restatement():
    im = np.random.default_rng(1).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(census(im), census_loop(im))
    two = (np.random.default_rng(2).integers(0, 2, (9, 11, 1)) * 200).astype(np.uint8).repeat(3, axis=2)
    assert np.array_equal(census(two), census_loop(two))
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.integers(0, 1 << 62, 500, dtype=np.uint64), np.array([0, 1, (1 << 62) - 1, (1 << 64) - 1, 1 << 63], np.uint64)])
    assert [int(c) for c in popcount(v)] == [bin(int(x)).count("1") for x in v]
    return len(v)


# ------------------------------------------------------------------------------------------------ 2. tables
def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)          # (non-negative floats: the bit patterns are ordered)
    return int(np.abs(ia - ib).max())


def case_tables(lib):
    worst = 0
    for la, lc in ((10.0, 30.0), (3.5, 7.25), (0.125, 1000.0)):
        ta, tc = api.costvol_tables(la, lc, lib=lib)
        assert ta.shape == (766,) and tc.shape == (63,) and ta.dtype == F and tc.dtype == F
        assert ta[0] == 0.0 and tc[0] == 0.0 and not np.signbit(ta[0]) and not np.signbit(tc[0])
        assert (np.diff(ta) >= 0).all() and (np.diff(tc) >= 0).all()
        assert ta.max() <= 0.5 and tc.max() <= 0.5
        ra, rc = tables(la, lc)
        worst = max(worst, _ulps(ta, ra), _ulps(tc, rc))
        assert _ulps(ta, ra) <= 1 and _ulps(tc, rc) <= 1, (la, lc, _ulps(ta, ra), _ulps(tc, rc))
    return worst


# ------------------------------------------------------------------------------------------------ 3. census
CENSUS_SHAPES = [(1, 1), (7, 9), (5, 300), (33, 257), (3, 1030)]


def case_census(lib, H, W):
    rng = np.random.default_rng(100 + H * 7 + W)
    rand = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    const = np.full((H, W, 3), 93, np.uint8)
    two = np.where(rng.random((H, W, 1)) < 0.5, 40, 41).astype(np.uint8).repeat(3, axis=2)          # two grey levels: many ties
    got = dev_census(lib, rand)
    assert same_bytes(got, census(rand))
    assert not dev_census(lib, const).any()
    assert same_bytes(dev_census(lib, two), census(two))
    return int(popcount(got).sum())


# ------------------------------------------------------------------------------------------------ 4. volume
# (D, H, W, d0): 1 x 1 x 1; small; D > W (deep slices entirely out of view); several workgroups wide with a tail; odd W (unaligned rows, the scalar
# store path) with negative disparities clamping at the other edge; one slice below and one above a multiple of the kernel's chunk of CHUNK slices;
# a segment boundary inside an aligned row
VOLUME_SHAPES = [(1, 1, 1, 0), (9, 7, 40, 0), (70, 3, 50, 0), (5, 2, 600, 0), (37, 5, 263, -3), (2 * CHUNK - 1, 2, 44, 0), (2 * CHUNK + 1, 2, 44, 0),
                 (CHUNK + 1, 2, SEGMENT + 8, -2)]


def case_volume(lib, D, H, W, d0, mode, lead=GUARD):
    imL, imR = images(H, W, 1000 + D + 3 * H + 7 * W + mode)
    ta, tc = api.costvol_tables(lib=lib)
    got = dev_volume(lib, imL, imR, D, mode, d0, lead=lead)
    ref = volume(imL, imR, D, mode, d0, ta, tc)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert (got >= 0).all() and (got < 1).all()
    return float(got.mean())


# ------------------------------------------------------------------------------------------------ 5. against the volume kernels we already have
def case_symmetry(lib, D=24, H=6, W=52):
    """The cost is symmetric in the two pixels, so the right volume the ingest synthesises from the left one (convertVolumeL2R) is the true right
    volume wherever the match lies inside the image, and fillOutOfView erases the rest."""
    import torch
    assert D <= W
    imL, imR = images(H, W, 77)
    dev = _dev(lib)
    left, right = (_up(dev_volume(lib, imL, imR, D, m), lib) for m in (0, 1))
    conv = torch.empty_like(left)
    api.convert_volume_l2r(left.data_ptr(), conv.data_ptr(), D, H, W, lib=lib)
    api.fill_out_of_view(conv.data_ptr(), D, H, W, 1, lib=lib)
    before = right.cpu().numpy().copy()
    api.fill_out_of_view(right.data_ptr(), D, H, W, 1, lib=lib)
    a, b = right.cpu().numpy(), conv.cpu().numpy()
    assert same_bytes(a, b)
    assert str(left.device).startswith(dev)
    return int((a.view(np.uint32) != before.view(np.uint32)).sum())          # entries the fill replaced


# ------------------------------------------------------------------------------------------------ 6. known answers
def case_known_answers(lib, H=9, W=48, k=5, D=8):
    """Identical images: slice 0 is exactly 0.  Both views cut from one wider image, the right one k columns further right: imL(x) = imR(x - k), so
    slice k of the left volume is exactly 0 wherever neither 9-wide census window is clamped differently -- columns k + 4 <= x <= W - 5 (at
    x > W - 5 the left window is clamped at the image border and the right one, k columns inside its image, is not)."""
    wide = np.random.default_rng(5).integers(0, 256, (H, W + k, 3), dtype=np.uint8)
    imL, imR = np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, k:k + W])
    for mode in (0, 1):
        v = dev_volume(lib, imL, imL, D, mode)
        assert not v[0].view(np.uint32).any()
    v0 = dev_volume(lib, imL, imR, D, 0)
    assert not v0[k][:, k + 4:W - 4].view(np.uint32).any()
    assert v0[k][:, :k].any() and all(v0[j][:, k + 4:W - 4].all() for j in range(D) if j != k)        # (random colours: every other entry is positive)
    v1 = dev_volume(lib, imL, imR, D, 1)                     # the right view's volume: imR(x) = imL(x + k), zero for 4 <= x <= W - 5 - k
    assert not v1[k][:, 4:W - 4 - k].view(np.uint32).any()
    return int((v0[k] == 0).sum()), int((v1[k] == 0).sum())


# ------------------------------------------------------------------------------------------------ 7. errors
def case_errors(lib):
    import torch
    L = api.load(lib)
    dev = _dev(lib)
    H, W, D = 4, 12, 3
    imL, imR = images(H, W, 9)
    tl, tr = _up(imL, lib), _up(imR, lib)
    vol = torch.full((D * H * W,), GUARD_BITS, dtype=torch.int32, device=dev)
    sig = torch.full((H * W,), -7, dtype=torch.int64, device=dev)
    nan, inf = float("nan"), float("inf")
    vp, fl = C.c_void_p, C.c_float

    def build(imL_=tl.data_ptr(), imR_=tr.data_ptr(), vol_=vol.data_ptr(), D_=D, H_=H, W_=W, mode=0, d0=0, la=10.0, lc=30.0):
        return L.les_hip_build_cost_volume(vp(imL_), vp(imR_), vp(vol_), D_, H_, W_, mode, d0, fl(la), fl(lc), 0, None)

    refused = [build(imL_=None), build(imR_=None), build(vol_=None), build(D_=0), build(D_=-1), build(H_=0), build(W_=0), build(W_=-5), build(mode=2),
               build(mode=-1)]
    refused += [build(la=v) for v in (0.0, -1.0, inf, -inf, nan)] + [build(lc=v) for v in (0.0, -2.5, inf, nan)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    assert b"" != L.les_hip_last_error()
    assert build(D_=65536, H_=256, W_=256) == api.LES_HIP_ERR_UNSUPPORTED         # 2^32 floats
    assert (vol.cpu().numpy() == GUARD_BITS).all()

    def cen(bgr=tl.data_ptr(), s=sig.data_ptr(), H_=H, W_=W):
        return L.les_hip_census(vp(bgr), vp(s), H_, W_, 0, None)

    refused = [cen(bgr=None), cen(s=None), cen(H_=0), cen(W_=0), cen(H_=-3)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    assert (sig.cpu().numpy() == -7).all()

    ta, tc = np.full(766, 5.0, F), np.full(63, 5.0, F)
    pa, pc = ta.ctypes.data_as(vp), tc.ctypes.data_as(vp)
    refused = [L.les_hip_costvol_tables(fl(10.0), fl(30.0), None, pc), L.les_hip_costvol_tables(fl(10.0), fl(30.0), pa, None)]
    refused += [L.les_hip_costvol_tables(fl(v), fl(30.0), pa, pc) for v in (0.0, -1.0, inf, nan)]
    refused += [L.les_hip_costvol_tables(fl(10.0), fl(v), pa, pc) for v in (0.0, -1.0, inf, nan)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    assert (ta == 5.0).all() and (tc == 5.0).all()
    # the Python layer raises, with the code in the message
    for call in (lambda: api.build_cost_volume(tl.data_ptr(), tr.data_ptr(), vol.data_ptr(), D, H, W, 3, lib=lib), lambda: api.costvol_tables(-1.0, lib=lib),
                 lambda: api.census(0, sig.data_ptr(), H, W, lib=lib)):
        try:
            call()
            raise AssertionError("accepted")
        except api.LesHipError as ex:
            assert "error 1" in str(ex)
    # and a good call still works afterwards
    assert build() == api.LES_HIP_OK and not (vol.cpu().numpy() == GUARD_BITS).any()
    return len(refused)


# ------------------------------------------------------------------------------------------------ 8. quality on the cones crop
def cones_pair():
    z = np.load(os.path.join(GOLDEN, "cones_crop.npz"))
    imL = np.ascontiguousarray(z["imL"])
    W = imL.shape[1]
    return imL, np.ascontiguousarray(z["imR_wide"][:, 64:64 + W]), z["gt"].astype(F)


def wta_bad(vol, gt, mask, thr):
    d = vol.argmin(0).astype(F)
    return float((np.abs(d - gt)[mask] > thr).mean())


def case_quality(lib, D=64):
    imL, imR, gt = cones_pair()
    H, W = gt.shape
    ta, tc = api.costvol_tables(lib=lib)
    got = dev_volume(lib, imL, imR, D, 0)
    assert same_bytes(got, volume(imL, imR, D, 0, 0, ta, tc))
    mask = (gt > 0) & np.isfinite(gt) & (np.arange(W)[None, :] - gt >= 0)            # known ground truth whose match lies inside the right image
    assert mask.sum() >= 8000, int(mask.sum())
    ad = ad_volume(imL, imR, D)
    out = dict(pixels=int(mask.sum()), known=int(((gt > 0) & np.isfinite(gt)).sum()))
    for thr in (1.0, 2.0):
        out[f"adcensus_bad{thr}"] = wta_bad(got, gt, mask, thr)
        out[f"ad_bad{thr}"] = wta_bad(ad, gt, mask, thr)
    print(out)
    assert out["adcensus_bad1.0"] <= 0.5 * out["ad_bad1.0"], out
    return out


# ------------------------------------------------------------------------------------------------ 9. the driver
def case_driver(lib, device, monkeypatch, layer_units=None, **kw):
    """layer_units: None = MidV3's own layers (1 % / 3 % / 9 % of the width: cells of 1, 3 and 10 pixels on the 120-wide crop -- 11 520 cells in the
    finest layer, which the GPU runs in 0.4 s; the fibre simulator did not finish that run in 25 minutes on 8 cores), else the units that replace
    them (the simulator run: everything else of MidV3 is unchanged)."""
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    if layer_units is not None:
        real_layers = stereo._layers
        monkeypatch.setattr(stereo, "_layers", lambda st, sizes: real_layers(st, layer_units))
    imL, imR, gt = cones_pair()
    H, W = gt.shape
    gt_inf = np.where(gt > 0, gt, np.inf).astype(F)
    data = dict(imL=imL, imR=imR, dispGT=gt_inf, nonocc=gt > 0, ndisp=64, gt_prec=-1.0)
    seen = []
    real_build, real_ingest = lio.build_volumes, lio.ingest_volumes

    def spy_build(*a, **k):
        tl, tr = real_build(*a, **k)
        seen.append(("build", tl.cpu().numpy().copy(), tr.cpu().numpy().copy()))
        return tl, tr

    def spy_ingest(*a, **k):
        seen.append(("ingest",))
        return real_ingest(*a, **k)

    monkeypatch.setattr(lio, "build_volumes", spy_build)
    monkeypatch.setattr(lio, "ingest_volumes", spy_ingest)
    st, lab, raw = stereo.MidV3(data, None, None, iterations=1, pmIterations=1, device=device, lib=lib, **kw)
    assert [s[0] for s in seen] == ["build"]
    assert lab.shape == (H, W, 4) and np.isfinite(lab).all()
    tl, tr = real_build(imL, imR, 64, device=device, lib=lib)
    vl, vr = tl.cpu().numpy(), tr.cpu().numpy()
    assert same_bytes(seen[0][1], vl) and same_bytes(seen[0][2], vr)
    # the volumes are the filled builds of the two modes
    for mode, v in ((0, tl), (1, tr)):
        b = _up(dev_volume(lib, imL, imR, 64, mode), lib)
        api.fill_out_of_view(b.data_ptr(), 64, H, W, mode, lib=lib)
        assert same_bytes(b.cpu().numpy(), v.cpu().numpy())
    known = gt > 0
    bad1 = float((np.abs(stereo.disparities(lab) - gt)[known] > 1.0).mean())
    print(f"MidV3 from the stereo pair alone (cones crop, 1 PatchMatch + 1 graph-cut iteration): bad-1.0 {100 * bad1:.1f} % of {int(known.sum())} known pixels; "
          f"log 'all' {[round(r['all'], 2) for r in st.log]}")
    # explicit volumes still go through the ingest: the builder is not called
    seen.clear()
    st2, lab2, _ = stereo.MidV3(data, vl, None, iterations=1, pmIterations=1, device=device, lib=lib, **kw)
    assert [s[0] for s in seen] == ["ingest"]
    assert lab2.shape == (H, W, 4)
    try:
        stereo.MidV3(data, None, vr, iterations=1, pmIterations=1, device=device, lib=lib, **kw)
        raise AssertionError("volR without volL was accepted")
    except ValueError:
        pass
    return bad1
