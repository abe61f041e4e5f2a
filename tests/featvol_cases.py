"""Correlation cost volumes from feature maps and the ZNCC patch descriptor (csrc/les_featvol.h): the definitions restated in numpy, and the cases
tests/test_featvol.py runs on the CPU simulator build (lib = its path, tensors on "cpu") and on the MI355X (lib = None: the product library, tensors
on "cuda").

The descriptor is exact integers, one IEEE double sqrt and division and one rounding: compared BYTE for byte.  The volume is an f32 fma chain:
numpy has no fmaf, so fmaf32 below builds one from float64 (the product of two f32 is exact there; TwoSum gives the residual of the sum; a float64
sum that sits on an f32 midpoint with a non-zero residual is decided by the residual's sign) and case_restatement holds it to fractions.Fraction."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

from localexpstereo_amd import api
from tests import costvol_cases as cc

F = np.float32
SEG, CHUNK, KC = 128, 64, 32        # kFvSeg, kFvChunk, kFvKC of csrc/les_featvol.h: a workgroup's pixels and slices, the channels staged per pass
GUARD, GUARD_BITS = cc.GUARD, cc.GUARD_BITS
U = 2.0 ** -24                      # unit roundoff of f32


# ------------------------------------------------------------------------------------------------ the restatement
def fmaf32(a, b, s):
    """Correctly rounded f32 a * b + s, elementwise (finite operands, no overflow)."""
    a, b, s = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(s, F))
    p, s64 = a.astype(np.float64) * b.astype(np.float64), s.astype(np.float64)          # p exact: 24 + 24 bits
    t = p + s64
    bb = t - p
    e = (p - (t - bb)) + (s64 - bb)                                                      # TwoSum: p + s = t + e exactly
    r = t.astype(F)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(t > r64, np.inf, -np.inf).astype(F))                # the f32 on the other side of t
    o64 = other.astype(np.float64)
    tie = (r64 != t) & (e != 0) & (0.5 * (r64 + o64) == t)                               # t is the midpoint of r and other, the exact sum is not
    return np.where(tie & (np.sign(e) == np.sign(o64 - r64)), other, r).astype(F)


def round_f32(x):
    """A Fraction rounded to the nearest f32, ties to even (|x| below the overflow threshold)."""
    if x == 0:
        return F(0)
    e, ax = 0, abs(x)
    while ax >= 2:
        ax, e = ax / 2, e + 1
    while ax < 1:
        ax, e = ax * 2, e - 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return F(float(n * ulp))                                                             # (n * ulp is an f32: the conversions are exact)


def descriptor(im, ry, rx):
    """float32 [(2 ry + 1)(2 rx + 1)][H][W]: the ZNCC descriptor of the definition."""
    g = cc.grey(im)
    H, W = g.shape
    p = np.pad(g, ((ry, ry), (rx, rx)), mode="edge")
    taps = np.stack([p[ry + dy:ry + dy + H, rx + dx:rx + dx + W] for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)])          # int64 [N][H][W]
    N = taps.shape[0]
    S, Q = taps.sum(0), (taps * taps).sum(0)
    V = N * Q - S * S
    assert (V >= 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        f = ((N * taps - S).astype(np.float64) / np.sqrt((N * V).astype(np.float64))).astype(F)
    return np.ascontiguousarray(np.where(V > 0, f, F(0)).astype(F))


def descriptor_loop(im, ry, rx):
    """The same, pixel by pixel, straight from the definition."""
    import math
    im = np.asarray(im)
    H, W = im.shape[:2]

    def g(y, x):
        b, gr, r = (int(v) for v in im[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])
        return (77 * r + 150 * gr + 29 * b + 128) >> 8

    N = (2 * ry + 1) * (2 * rx + 1)
    out = np.zeros((N, H, W), F)
    for y in range(H):
        for x in range(W):
            taps = [g(y + dy, x + dx) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)]
            S, Q = sum(taps), sum(t * t for t in taps)
            V = N * Q - S * S
            for c, t in enumerate(taps):
                out[c, y, x] = F(float(N * t - S) / math.sqrt(float(N * V))) if V > 0 else F(0)
    return out


def _partners(W, D, mode, d0):
    return np.stack([cc.partner_columns(W, k + d0, mode) for k in range(D)])            # [D][W]


def volume(fL, fR, D, mode, d0=0, alpha=0.5, beta=0.5):
    """The f32 chain of the definition, float32 [D][H][W]."""
    fI, fJ = (fL, fR) if mode == 0 else (fR, fL)
    Cn, H, W = fI.shape
    xp = _partners(W, D, mode, d0)
    s = np.zeros((D, H, W), F)
    for c in range(Cn):
        s = fmaf32(fI[c][None], fJ[c][:, xp].transpose(1, 0, 2), s)
    return fmaf32(F(-F(alpha)), s, F(beta))


def volume64(fL, fR, D, mode, d0=0, alpha=0.5, beta=0.5):
    """beta - alpha s in float64, and sum_c |fI_c fJ_c|."""
    fI, fJ = ((fL, fR) if mode == 0 else (fR, fL))
    fI, fJ = fI.astype(np.float64), fJ.astype(np.float64)
    xp = _partners(fI.shape[2], D, mode, d0)
    prod = fI[:, None] * fJ[:, :, xp].transpose(0, 2, 1, 3)                              # [C][D][H][W]
    return float(F(beta)) - float(F(alpha)) * prod.sum(0), np.abs(prod).sum(0)


def bound(Cn, alpha, ref, sabs):
    """|got - ref| <= alpha gamma_(C+1) sum |a b| + 2^-24 |ref|: the dot-product bound of any summation order plus the final fma's rounding."""
    n = (Cn + 1) * U
    return abs(float(F(alpha))) * (n / (1.0 - n)) * sabs + U * np.abs(ref)


# ------------------------------------------------------------------------------------------------ device plumbing
def dev_features(lib, im, ry, rx):
    """les_hip_patch_features into a guarded buffer; asserts the guards untouched."""
    import torch
    H, W = im.shape[:2]
    n = (2 * ry + 1) * (2 * rx + 1) * H * W
    buf = torch.full((GUARD + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=cc._dev(lib))
    t = cc._up(im, lib)
    api.patch_features(t.data_ptr(), buf.data_ptr() + 4 * GUARD, H, W, ry, rx, lib=lib)
    out = buf.cpu().numpy()
    assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + n:] == GUARD_BITS).all(), "guard floats overwritten"
    return out[GUARD:GUARD + n].view(F).reshape(-1, H, W).copy()


def dev_volume(lib, fL, fR, D, mode, d0=0, alpha=0.5, beta=0.5, lead=GUARD, feat_lead=0):
    """les_hip_build_feature_volume into a buffer with `lead` guard floats before and GUARD after the volume (asserted untouched); the feature maps
    start feat_lead floats into their allocations."""
    import torch
    Cn, H, W = fL.shape
    n = D * H * W
    buf = torch.full((lead + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=cc._dev(lib))
    tl, tr = (cc._up(np.concatenate([np.zeros(feat_lead, F), np.ascontiguousarray(f, F).ravel()]), lib) for f in (fL, fR))
    api.build_feature_volume(tl.data_ptr() + 4 * feat_lead, tr.data_ptr() + 4 * feat_lead, buf.data_ptr() + 4 * lead, Cn, D, H, W, mode, d0=d0, alpha=alpha,
                             beta=beta, lib=lib)
    out = buf.cpu().numpy()
    assert (out[:lead] == GUARD_BITS).all() and (out[lead + n:] == GUARD_BITS).all(), "guard floats overwritten"
    return out[lead:lead + n].view(F).reshape(D, H, W).copy()


def int_features(Cn, H, W, seed):
    """Random integers in -8 .. 8: every partial sum of the chain is exact, so only layout mistakes can change the bytes.  Random, hence asymmetric."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (Cn, H, W)).astype(F), rng.integers(-8, 9, (Cn, H, W)).astype(F)


def unit_features(Cn, H, W, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        f = rng.standard_normal((Cn, H, W))
        out.append(np.ascontiguousarray((f / np.sqrt((f * f).sum(0))).astype(F)))
    return out


def assert_same(got, ref):
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert got.shape == ref.shape and len(bad) == 0, (len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
def case_restatement():
    rng = np.random.default_rng(1)
    im = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    two = (rng.integers(0, 2, (9, 11, 1)) * 200).astype(np.uint8).repeat(3, axis=2)
    for ry, rx in ((2, 2), (1, 3), (0, 0)):
        for a in (im, two):
            assert cc.same_bytes(descriptor(a, ry, rx), descriptor_loop(a, ry, rx))
    # fmaf32 against exact rationals: random triples over a wide range of exponents, sums that cancel, and ties -- a b = +-(1 - i^2 2^-46) next
    # to an s that puts the exact sum just beside an f32 midpoint that the float64 sum lands on
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    s = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F)
    s[:500] = -(a[:500].astype(np.float64) * b[:500].astype(np.float64)).astype(F)          # cancellation: the result is the product's rounding error
    ta, tb, ts = [], [], []
    for i in range(1, 40):
        for sign in (1.0, -1.0):
            M = int(rng.integers(1 << 23, 1 << 24))
            scale = 2.0 ** int(rng.integers(-10, 10))
            ta.append(sign * (1.0 + i * 2.0 ** -23) * scale)
            tb.append(1.0 - i * 2.0 ** -23)
            ts.append((2.0 * M + 1.0 - sign) * scale)
    ta, tb, ts = np.array(ta, F), np.array(tb, F), np.array(ts, F)
    naive = (ta.astype(np.float64) * tb.astype(np.float64) + ts.astype(np.float64)).astype(F)
    a, b, s = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([s, ts])
    got = fmaf32(a, b, s)
    ref = np.array([round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, s)], F)
    assert_same(got, ref)
    double_rounded = int((naive.view(np.uint32) != ref[n:].view(np.uint32)).sum())
    assert double_rounded >= 10, double_rounded          # the ties really are cases that rounding through float64 gets wrong
    return len(a), double_rounded


# ------------------------------------------------------------------------------------------------ 2. descriptors
DESC_SHAPES = [(1, 1), (7, 9), (5, 300), (33, 257)]
DESC_RADII = [(0, 0), (2, 2), (3, 4), (4, 4)]


def desc_images(H, W):
    rng = np.random.default_rng(200 + 7 * H + W)
    rand = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    flat = rand.copy()                                             # flat regions (V = 0) beside texture
    flat[:, : (W + 1) // 2] = 93
    flat[: H // 3] = 17
    two = np.where(rng.random((H, W, 1)) < 0.5, 40, 41).astype(np.uint8).repeat(3, axis=2)          # two grey levels
    return rand, flat, two


def case_descriptor(lib, H, W):
    zeros = 0
    for ry, rx in DESC_RADII:
        for im in desc_images(H, W):
            got, ref = dev_features(lib, im, ry, rx), descriptor(im, ry, rx)
            assert_same(got, ref)
            norm = (got.astype(np.float64) ** 2).sum(0)
            assert (np.abs(norm[norm > 0] - 1.0) < 1e-5).all()
            zeros += int((norm == 0).sum())
    return zeros


# ------------------------------------------------------------------------------------------------ 3. volume on exact data
# (C, D, H, W, d0).  C: 1, 2, 3 (odd: the zero channel that pads K), 25, 64, 65, KC + 1 (a second staging pass of one channel).  W: 1, 31, 33,
# SEG - 1, SEG + 8 (a second segment; W % 4 == 0: the 16-byte store path), 262 (three segments, no multiple of 4).  D: 1, CHUNK - 1, CHUNK + 1,
# 2 CHUNK + 1, D > W.  d0: 0, -3, 5.  H: 1, 3.
VOLUME_CASES = [(1, 1, 1, 1, 0), (2, CHUNK - 1, 3, 31, 0), (3, CHUNK + 1, 1, 33, -3), (25, 2 * CHUNK + 1, 1, SEG - 1, 5), (64, 5, 3, SEG + 8, 0),
                (65, CHUNK + 1, 1, SEG + 8, -3), (KC + 1, 9, 3, 40, 5), (3, 70, 1, 262, 0)]
REAL_CASES = [(25, 2 * CHUNK + 1, 1, SEG - 1, 5), (64, 5, 3, SEG + 8, 0), (64, CHUNK + 1, 1, SEG + 8, -3)]


@functools.lru_cache(maxsize=None)
def _int_case(Cn, D, H, W, d0, mode, alpha, beta):
    fL, fR = int_features(Cn, H, W, 3000 + Cn + 3 * D + 5 * H + 7 * W + mode)
    ref = volume(fL, fR, D, mode, d0, alpha, beta)
    ref.setflags(write=False)
    return fL, fR, ref


def case_volume(lib, Cn, D, H, W, d0, mode, alpha=0.5, beta=0.5, lead=GUARD, feat_lead=0):
    fL, fR, ref = _int_case(Cn, D, H, W, d0, mode, alpha, beta)
    ref64, _ = volume64(fL, fR, D, mode, d0, alpha, beta)
    assert np.array_equal(ref.astype(np.float64), ref64)            # exact data: the chain is the exact value
    got = dev_volume(lib, fL, fR, D, mode, d0, alpha, beta, lead=lead, feat_lead=feat_lead)
    assert_same(got, ref)
    return float(got.mean())


def case_one_hot(lib, mode, Cn=37, D=80, H=2, W=150):
    """Channel x mod C is 1 at column x of both maps; alpha = -1, beta = 0: the entry is 1 iff x = xp mod C, so each names its own pair."""
    f = np.zeros((Cn, H, W), F)
    f[np.arange(W) % Cn, :, np.arange(W)] = 1
    got = dev_volume(lib, f, f, D, mode, alpha=-1.0, beta=0.0)
    x, xp = np.arange(W)[None, :], _partners(W, D, mode, 0)
    ref = np.broadcast_to((((x - xp) % Cn) == 0).astype(F)[:, None, :], (D, H, W))
    assert_same(got, np.ascontiguousarray(ref))
    return int(got.sum())


# ------------------------------------------------------------------------------------------------ 4. volume on real-valued data
@functools.lru_cache(maxsize=None)
def _real_case(Cn, D, H, W, d0, mode):
    fL, fR = unit_features(Cn, H, W, 4000 + Cn + 3 * D + 7 * W + mode)
    chain = volume(fL, fR, D, mode, d0)
    ref, sabs = volume64(fL, fR, D, mode, d0)
    for a in (chain, ref, sabs):
        a.setflags(write=False)
    return fL, fR, chain, ref, sabs


def check_bound(got, Cn, alpha, ref, sabs):
    err, b = np.abs(got.astype(np.float64) - ref), bound(Cn, alpha, ref, sabs)
    worst = float((err / b).max())
    assert (err <= b).all(), worst
    return worst


def case_real(lib, Cn, D, H, W, d0, mode):
    """Returns (worst error / bound, entries that differ from the numpy chain).  The simulator runs the chain itself: the same bytes."""
    fL, fR, chain, ref, sabs = _real_case(Cn, D, H, W, d0, mode)
    got = dev_volume(lib, fL, fR, D, mode, d0)
    worst = check_bound(got, Cn, 0.5, ref, sabs)
    differ = int((got.view(np.uint32) != chain.view(np.uint32)).sum())
    print(f"C {Cn} D {D} H {H} W {W} d0 {d0} mode {mode}: worst error / bound {worst:.3f}; {differ} of {got.size} entries differ from the fmaf chain")
    if lib is not None:
        assert differ == 0
    return worst, differ


# ------------------------------------------------------------------------------------------------ 5. symmetry
def case_symmetry(lib, Cn=25, D=40, H=2, W=90):
    """d0 = 0: the right view's entry (k, y, x) is the left view's (k, y, x + k) wherever x + k < W -- the same products in the same order."""
    fL, fR = unit_features(Cn, H, W, 55)
    v0, v1 = (dev_volume(lib, fL, fR, D, m) for m in (0, 1))
    n = 0
    for k in range(D):
        assert cc.same_bytes(v1[k][:, :W - k], v0[k][:, k:])
        n += H * (W - k)
    return n


# ------------------------------------------------------------------------------------------------ 6. errors
def case_errors(lib):
    import torch
    L = api.load(lib)
    dev = cc._dev(lib)
    Cn, H, W, D = 3, 4, 12, 5
    fL, fR = int_features(Cn, H, W, 9)
    tl, tr = cc._up(fL, lib), cc._up(fR, lib)
    vol = torch.full((D * H * W,), GUARD_BITS, dtype=torch.int32, device=dev)
    nan, inf = float("nan"), float("inf")
    vp, fl = C.c_void_p, C.c_float

    def build(fL_=tl.data_ptr(), fR_=tr.data_ptr(), vol_=vol.data_ptr(), C_=Cn, D_=D, H_=H, W_=W, mode=0, d0=0, alpha=0.5, beta=0.5):
        return L.les_hip_build_feature_volume(vp(fL_), vp(fR_), vp(vol_), C_, D_, H_, W_, mode, d0, fl(alpha), fl(beta), 0, None)

    refused = [build(fL_=None), build(fR_=None), build(vol_=None), build(C_=0), build(C_=-2), build(D_=0), build(D_=-1), build(H_=0), build(W_=0),
               build(W_=-5), build(mode=2), build(mode=-1)]
    refused += [build(alpha=v) for v in (inf, -inf, nan)] + [build(beta=v) for v in (inf, -inf, nan)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    assert b"" != L.les_hip_last_error()
    unsupported = [build(D_=65536, H_=256, W_=256), build(D_=1, H_=65536, W_=4), build(C_=api.FEATVOL_MAX_CHANNELS + 1)]
    assert unsupported == [api.LES_HIP_ERR_UNSUPPORTED] * 3, unsupported
    assert api.FEATVOL_MAX_CHANNELS >= 128
    assert (vol.cpu().numpy() == GUARD_BITS).all()

    im = cc._up(np.random.default_rng(4).integers(0, 256, (H, W, 3), dtype=np.uint8), lib)
    feat = torch.full((81 * H * W,), GUARD_BITS, dtype=torch.int32, device=dev)

    def desc(bgr=im.data_ptr(), f=feat.data_ptr(), H_=H, W_=W, ry=2, rx=2):
        return L.les_hip_patch_features(vp(bgr), vp(f), H_, W_, ry, rx, 0, None)

    refused = [desc(bgr=None), desc(f=None), desc(H_=0), desc(W_=0), desc(H_=-3), desc(ry=-1), desc(rx=-1)]
    assert refused == [api.LES_HIP_ERR_ARG] * len(refused), refused
    unsupported = [desc(ry=api.PATCH_MAX_RADIUS + 1), desc(rx=api.PATCH_MAX_RADIUS + 1), desc(H_=65536, W_=1)]
    assert unsupported == [api.LES_HIP_ERR_UNSUPPORTED] * 3, unsupported
    assert (feat.cpu().numpy() == GUARD_BITS).all()
    a, b = fl(0), fl(0)
    assert L.les_hip_featvol_last_times(None, C.byref(b)) == api.LES_HIP_ERR_ARG and L.les_hip_featvol_last_times(C.byref(a), None) == api.LES_HIP_ERR_ARG
    # the Python layer raises, with the code in the message
    for call, code in ((lambda: api.build_feature_volume(tl.data_ptr(), tr.data_ptr(), vol.data_ptr(), Cn, D, H, W, 3, lib=lib), 1),
                       (lambda: api.patch_features(im.data_ptr(), feat.data_ptr(), H, W, 5, 0, lib=lib), 3)):
        try:
            call()
            raise AssertionError("accepted")
        except api.LesHipError as ex:
            assert f"error {code}" in str(ex)
    # and good calls still work afterwards
    assert build() == api.LES_HIP_OK and desc(ry=4, rx=4) == api.LES_HIP_OK
    if dev == "cuda":
        torch.cuda.synchronize()
    assert not (vol.cpu().numpy() == GUARD_BITS).any() and not (feat.cpu().numpy() == GUARD_BITS).any()
    return len(refused)


def case_python_errors(lib):
    """io.build_volumes and stereo.MidV3 raise ValueError for an unknown cost, a bad patch, and features together with explicit volumes."""
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    imL, imR = cc.images(6, 20, 3)
    dev = cc._dev(lib)
    bad = [dict(cost="ncc"), dict(cost="zncc", patch=(5, 2)), dict(cost="zncc", patch=(2, -1)), dict(cost="zncc", patch=(2,)), dict(cost="zncc", patch=2),
           dict(cost="zncc", patch=(1.5, 2)), dict(features=(1, 2)), dict(features=(np.zeros((3, 6, 20), F),) * 2)]
    for kw in bad:
        try:
            lio.build_volumes(imL, imR, 4, device=dev, lib=lib, **kw)
            raise AssertionError(f"accepted {kw}")
        except ValueError:
            pass
    data = dict(imL=imL, imR=imR, ndisp=4)
    vol = np.zeros((4, 6, 20), F)
    f = cc._up(np.zeros((3, 6, 20), F), lib)
    for kw in (dict(features=(f, f)), dict(cost="zncc"), dict(features=lambda im: f)):
        try:
            stereo.MidV3(data, vol, None, device=dev, lib=lib, **kw)
            raise AssertionError(f"accepted {sorted(kw)} with explicit volumes")
        except ValueError:
            pass
    return len(bad)


# ------------------------------------------------------------------------------------------------ 7. quality on the cones crop
def case_quality(lib, D=64, patch=(2, 2)):
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    fL, fR = (dev_features(lib, im, *patch) for im in (imL, imR))
    assert_same(fL, descriptor(imL, *patch))
    assert_same(fR, descriptor(imR, *patch))
    got = dev_volume(lib, fL, fR, D, 0)
    ref, sabs = volume64(fL, fR, D, 0)
    worst = check_bound(got, fL.shape[0], 0.5, ref, sabs)
    adc = cc.dev_volume(lib, imL, imR, D, 0)
    mask = (gt > 0) & np.isfinite(gt) & (np.arange(W)[None, :] - gt >= 0)            # the mask of costvol_cases.case_quality
    assert mask.sum() >= 8000, int(mask.sum())
    out = dict(pixels=int(mask.sum()), worst_error_over_bound=round(worst, 3))
    for thr in (1.0, 2.0):
        out[f"zncc_bad{thr}"] = cc.wta_bad(got, gt, mask, thr)
        out[f"adcensus_bad{thr}"] = cc.wta_bad(adc, gt, mask, thr)
    print(out)
    assert out["zncc_bad1.0"] <= 0.5 * out["adcensus_bad1.0"], out
    return out


# ------------------------------------------------------------------------------------------------ 8. the driver
class _Stop(Exception):
    pass


def case_driver(lib, device, monkeypatch, layer_units=None, **kw):
    """layer_units: as in costvol_cases.case_driver (None: MidV3's own layers; the simulator run coarsens them)."""
    import torch
    from localexpstereo_amd import io as lio
    from localexpstereo_amd import stereo
    if layer_units is not None:
        real_layers = stereo._layers
        monkeypatch.setattr(stereo, "_layers", lambda st, sizes: real_layers(st, layer_units))
    imL, imR, gt = cc.cones_pair()
    H, W = gt.shape
    D = 64
    data = dict(imL=imL, imR=imR, dispGT=np.where(gt > 0, gt, np.inf).astype(F), nonocc=gt > 0, ndisp=D, gt_prec=-1.0)
    seen, calls = [], dict(adcensus=0, features=0)
    real_build, real_ingest, real_adc, real_fv = lio.build_volumes, lio.ingest_volumes, api.build_cost_volume, api.build_feature_volume

    def spy_build(*a, **k):
        tl, tr = real_build(*a, **k)
        seen.append(("build", tl.cpu().numpy().copy(), tr.cpu().numpy().copy()))
        return tl, tr

    def spy_ingest(*a, **k):
        seen.append(("ingest",))
        return real_ingest(*a, **k)

    def count(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    monkeypatch.setattr(lio, "build_volumes", spy_build)
    monkeypatch.setattr(lio, "ingest_volumes", spy_ingest)
    monkeypatch.setattr(api, "build_cost_volume", count("adcensus", real_adc))
    monkeypatch.setattr(api, "build_feature_volume", count("features", real_fv))
    st, lab, raw = stereo.MidV3(data, None, None, iterations=1, pmIterations=1, device=device, lib=lib, cost="zncc", **kw)
    assert [s[0] for s in seen] == ["build"] and calls == dict(adcensus=0, features=2)
    assert lab.shape == (H, W, 4) and np.isfinite(lab).all()
    # the volumes are the filled builds of the two modes from the two descriptors
    fL, fR = (dev_features(lib, im, 2, 2) for im in (imL, imR))
    for mode in (0, 1):
        b = cc._up(dev_volume(lib, fL, fR, D, mode), lib)
        api.fill_out_of_view(b.data_ptr(), D, H, W, mode, lib=lib)
        assert cc.same_bytes(b.cpu().numpy(), seen[0][1 + mode])
    known = gt > 0
    bad1 = float((np.abs(stereo.disparities(lab) - gt)[known] > 1.0).mean())
    print(f"MidV3 on ZNCC 5 x 5 volumes (cones crop, 1 PatchMatch + 1 graph-cut iteration): bad-1.0 {100 * bad1:.1f} % of {int(known.sum())} known pixels; "
          f"log 'all' {[round(r['all'], 2) for r in st.log]}")

    # from here on MidV3 is stopped once it has its volumes: what it builds is the subject
    def stop(*a, **k):
        raise _Stop()

    monkeypatch.setattr(api, "HipCostVolumeEnergy", stop)

    def volumes_of(**k):
        seen.clear()
        try:
            stereo.MidV3(data, None, None, iterations=1, pmIterations=1, device=device, lib=lib, **k)
            raise AssertionError("the energy was not reached")
        except _Stop:
            pass
        assert [s[0] for s in seen] == ["build"]
        return seen[0][1], seen[0][2]

    zl, zr = volumes_of(cost="zncc")
    tfL, tfR = cc._up(fL, lib), cc._up(fR, lib)
    pl, pr = volumes_of(features=(tfL, tfR))
    assert cc.same_bytes(pl, zl) and cc.same_bytes(pr, zr)
    given = []

    def extractor(im):
        assert im.shape == (H, W, 3) and im.dtype == np.uint8
        given.append(im.copy())
        f = torch.empty((25, H, W), dtype=torch.float32, device=cc._dev(lib))
        t = cc._up(im, lib)
        api.patch_features(t.data_ptr(), f.data_ptr(), H, W, 2, 2, lib=lib)
        if f.is_cuda:
            torch.cuda.synchronize()          # (t lives until the descriptor is there)
        return f

    cl, cr = volumes_of(features=extractor, cost="adcensus")
    assert len(given) == 2 and np.array_equal(given[0], imL) and np.array_equal(given[1], imR)
    assert cc.same_bytes(cl, zl) and cc.same_bytes(cr, zr)
    # the default call still goes through the AD-Census builder and returns its bytes
    calls.update(adcensus=0, features=0)
    al, ar = volumes_of()
    assert calls == dict(adcensus=2, features=0)
    for mode, v in ((0, al), (1, ar)):
        b = cc._up(cc.dev_volume(lib, imL, imR, D, mode), lib)
        api.fill_out_of_view(b.data_ptr(), D, H, W, mode, lib=lib)
        assert cc.same_bytes(b.cpu().numpy(), v)
    assert not cc.same_bytes(al, zl)
    return bad1
