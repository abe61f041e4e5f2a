"""Data formats on either side of the hot path ("next" rows N3/N4 of SURVEY.md section 8(f)).

* matching-cost volumes: headerless little-endian float32 `[ndisp][H][W]` files `im0.acrt` / `im1.acrt`
  (cvutils::io::loadMatBinary(..., readHeader=false), LES/Utilities.hpp:171-201; call sites LES/main.cpp:353-368) and
  their preparation on the device: fillOutOfView (LES/main.cpp:146-176), convertVolumeL2R when im1.acrt is absent
  (LES/main.cpp:178-199, 360-364)
* PFM disparity maps (cvutils::io::read_pfm_file / save_pfm_file, LES/Utilities.hpp:20-137): rows stored bottom-up,
  the writer always emits scale -1/255 (little endian)
* data-set folders (loadData, LES/main.cpp:201-268; Calib, LES/main.cpp:84-144)
* the Evaluator's bad-pixel rates (LES/Evaluator.h:77-81, 133-140)

Host-side file handling is numpy; the volume preparation runs on the GPU through the C ABI.
"""
import os
import re

import numpy as np

from . import api


# ------------------------------------------------------------------------------------------------
# PFM
# ------------------------------------------------------------------------------------------------
def write_pfm(path, image):
    """save_pfm_file (LES/Utilities.hpp:84-137): 'Pf' (1 channel) or 'PF' (3), '%d %d', '%lf' of -1/255, rows bottom-up."""
    a = np.asarray(image, np.float32)
    if a.ndim == 2:
        tag, ch = "Pf", 1
    elif a.ndim == 3 and a.shape[2] == 3:
        tag, ch = "PF", 3
    else:
        raise ValueError("PFM images have 1 or 3 channels")
    h, w = a.shape[:2]
    with open(path, "wb") as f:
        f.write(("%s\n%d %d\n%f\n" % (tag, w, h, -1.0 / 255.0)).encode("ascii"))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def read_pfm(path):
    """read_pfm_file (LES/Utilities.hpp:20-82): negative scale = little endian; the pixel block is the last
    w*h*channels floats of the file (the reference seeks from the end); rows are stored bottom-up."""
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"^(P[fF])\s+(\d+)\s+(\d+)\s+([-+]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][-+]?[0-9]+)?)\s", data)    # %lf of the reference: 1e-05, -3.9e-03, ...
    if not m:
        raise ValueError(f"{path}: not a 1/3 channel PFM file")
    ch = 1 if m.group(1) == b"Pf" else 3
    w, h, scale = int(m.group(2)), int(m.group(3)), float(m.group(4))
    n = w * h * ch
    if len(data) < n * 4:
        raise ValueError(f"{path}: expected {n} floats")
    a = np.frombuffer(data[len(data) - n * 4:], "<f4" if scale < 0 else ">f4").astype(np.float32)
    a = a.reshape(h, w, ch)[::-1]
    return np.ascontiguousarray(a[..., 0] if ch == 1 else a)


# ------------------------------------------------------------------------------------------------
# cost volumes
# ------------------------------------------------------------------------------------------------
def load_cost_volume(path, ndisp, H, W, mmap=True):
    """Raw float32 [ndisp][H][W] (LES/main.cpp:353-357).  Returns None when the file does not exist."""
    if not os.path.exists(path):
        return None
    n = int(ndisp) * int(H) * int(W)
    if os.path.getsize(path) < n * 4:
        raise ValueError(f"{path}: {os.path.getsize(path)} bytes, expected {n * 4} for a {ndisp}x{H}x{W} float32 volume")
    if mmap:
        return np.memmap(path, dtype="<f4", mode="r", shape=(int(ndisp), int(H), int(W)))
    return np.fromfile(path, dtype="<f4", count=n).reshape(int(ndisp), int(H), int(W))


def save_cost_volume(path, vol):
    np.ascontiguousarray(vol, "<f4").tofile(path)


def _valid_masks(valid, H, W, dev):
    """build_volumes' / ingest_volumes' `valid`: a pair (validL, validR) of H x W bool or uint8 host arrays or device tensors, nonzero = valid
    -> the two as contiguous uint8 tensors on dev (None -> None)."""
    import torch
    if valid is None:
        return None
    try:
        pair = tuple(valid)
    except TypeError:
        pair = ()
    if len(pair) != 2:
        raise ValueError("valid: a pair (validL, validR) of H x W masks expected")
    out = []
    for v in pair:
        t = v if torch.is_tensor(v) else torch.from_numpy(np.array(v, order="C"))
        if tuple(t.shape) != (H, W) or t.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid: {H} x {W} bool or uint8 masks expected, got {tuple(t.shape)} {t.dtype}")
        out.append((t.to(dev) != 0).to(torch.uint8).contiguous())
    return out


def _fill(t, mode, masks, d0, mask_fill, **where):
    """The fill that follows a built or loaded volume of view `mode`: fillOutOfView, or with masks (_valid_masks') its widening to the valid image
    (api.fill_invalid with that view's own mask and its partner's; csrc/les_maskvol.h)."""
    D, H, W = t.shape
    if masks is None:
        api.fill_out_of_view(t.data_ptr(), D, H, W, mode, **where)
    else:
        api.fill_invalid(t.data_ptr(), D, H, W, mode, validI=masks[mode].data_ptr(), validJ=masks[1 - mode].data_ptr(), d0=d0, fill=mask_fill, **where)


def ingest_volumes(volL, volR=None, device="cuda", lib=None, valid=None, mask_fill=0.5):
    """The MiddV3 volume preparation of LES/main.cpp:353-368 on the device.  volL / volR: host arrays (or memmaps) of
    shape [D][H][W]; volR None => synthesised from the left volume (convertVolumeL2R) before the fills, exactly in
    the reference's order.  Returns two torch device tensors.
    valid (opt-in, no reference counterpart): a pair (validL, validR) of H x W bool or uint8 masks, host arrays or device tensors -- each
    fillOutOfView becomes its widening to the valid image (api.fill_invalid: an entry matched from or against an invalid pixel takes the
    nearest valid entry of its row and slice; a row of a slice without one is set to mask_fill); the order of the steps is unchanged, and
    convertVolumeL2R reads the filled left volume.  None: today's code path and bytes."""
    import torch
    dev = torch.device(device)
    idx = dev.index or 0 if dev.type == "cuda" else 0
    def upload(v):
        # never alias the caller's (possibly read-only, memory-mapped) array: the fills work in place
        if dev.type == "cuda":
            a = np.ascontiguousarray(v, np.float32)
            if not a.flags.writeable:                     # read-only memmap: stage through a writable (page-cache backed) copy
                a = np.array(a, np.float32, copy=True)
            return torch.from_numpy(a).to(dev)
        return torch.from_numpy(np.array(v, np.float32, copy=True))

    tl = upload(volL)
    D, H, W = tl.shape
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    masks = _valid_masks(valid, H, W, dev)
    _fill(tl, 0, masks, 0, mask_fill, device=idx, stream=stream, lib=lib)                         # LES/main.cpp:358
    if volR is not None:
        tr = upload(volR)
        assert tuple(tr.shape) == (D, H, W)
    else:
        tr = torch.empty_like(tl)
        api.convert_volume_l2r(tl.data_ptr(), tr.data_ptr(), D, H, W, device=idx, stream=stream, lib=lib)   # LES/main.cpp:363
    _fill(tr, 1, masks, 0, mask_fill, device=idx, stream=stream, lib=lib)                         # LES/main.cpp:365
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return tl, tr


COSTS = ("adcensus", "zncc")


def build_volumes(imL, imR, ndisp, device="cuda", lib=None, lambda_ad=10.0, lambda_census=30.0, d0=0, cost="adcensus", patch=(2, 2), features=None,
                  alpha=0.5, beta=0.5, valid=None, mask_fill=0.5):
    """Both views' matching-cost volumes made on the device from the stereo pair alone, in the place of the MC-CNN volumes the reference
    loads (LES/main.cpp:353-357).  imL / imR: H x W x 3 u8 (BGR) host arrays.  Each view is built directly (mode 0 / mode 1; slice k is
    disparity k + d0), then filled like a loaded volume (fillOutOfView, :358 / :365).  Returns two torch device tensors [ndisp][H][W], as
    ingest_volumes does.
    cost "adcensus" (default): the AD-Census cost of csrc/les_costvol.h (lambda_ad, lambda_census).
    cost "zncc": beta - alpha ZNCC of the (2 ry + 1) x (2 rx + 1) grey patches, patch = (ry, rx), radii 0 .. 4: both views' patch
    descriptors (api.patch_features) correlated on the matrix cores (api.build_feature_volume; csrc/les_featvol.h).
    features: a pair (fL, fR) of float32 [C][H][W] tensors on `device`, or a callable that maps an H x W x 3 u8 image to such a tensor
    (called once per view, left first): the volumes are beta - alpha <fI(x), fJ(xp)>, and `cost` is ignored.  The pair or the callable's
    outputs are used AS GIVEN: normalising them is the caller's business (torch.nn.functional.normalize(f, dim=0) makes the costs lie in
    [0, 1] at alpha = beta = 0.5, the range of AD-Census and of mc_threshold = 0.5; alpha = 1, beta = 0 is MC-CNN-fast's raw -dot).
    valid, mask_fill: as for ingest_volumes -- with a pair of masks each view's fill is api.fill_invalid with that view's mask and its
    partner's (csrc/les_maskvol.h); None: today's code path and bytes."""
    import torch
    dev = torch.device(device)
    idx = dev.index or 0 if dev.type == "cuda" else 0
    imL, imR = np.ascontiguousarray(imL, np.uint8), np.ascontiguousarray(imR, np.uint8)
    if imL.ndim != 3 or imL.shape[2] != 3 or imL.shape != imR.shape:
        raise ValueError(f"two H x W x 3 images of one shape expected, got {imL.shape} and {imR.shape}")
    if features is None and cost not in COSTS:
        raise ValueError(f"unknown cost {cost!r}: one of {COSTS}")
    H, W = imL.shape[:2]
    D = int(ndisp)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    masks = _valid_masks(valid, H, W, dev)
    out = []
    if features is not None or cost == "zncc":
        if features is None:
            try:
                ry, rx = (int(r) for r in patch)
                ok = (ry, rx) == tuple(patch) and 0 <= ry <= api.PATCH_MAX_RADIUS and 0 <= rx <= api.PATCH_MAX_RADIUS
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"patch {patch!r}: a pair of integer radii (ry, rx), each 0 .. {api.PATCH_MAX_RADIUS}")
            feats, images = [], []
            for im in (imL, imR):
                ti = torch.from_numpy(im.copy()).to(dev)
                images.append(ti)
                f = torch.empty(((2 * ry + 1) * (2 * rx + 1), H, W), dtype=torch.float32, device=dev)
                api.patch_features(ti.data_ptr(), f.data_ptr(), H, W, ry, rx, device=idx, stream=stream, lib=lib)
                feats.append(f)
        else:
            feats = [features(imL), features(imR)] if callable(features) else list(features)
            if len(feats) != 2 or not all(torch.is_tensor(f) and f.dim() == 3 and f.dtype == torch.float32 and f.device.type == dev.type for f in feats) \
                    or feats[0].shape != feats[1].shape or tuple(feats[0].shape[1:]) != (H, W):
                raise ValueError(f"features: two float32 [C][{H}][{W}] tensors on {dev.type} expected")
            feats = [f.contiguous() for f in feats]
        Cn = int(feats[0].shape[0])
        for mode in (0, 1):
            t = torch.empty((D, H, W), dtype=torch.float32, device=dev)
            api.build_feature_volume(feats[0].data_ptr(), feats[1].data_ptr(), t.data_ptr(), Cn, D, H, W, mode, d0=int(d0), alpha=alpha, beta=beta,
                                     device=idx, stream=stream, lib=lib)
            _fill(t, mode, masks, int(d0), mask_fill, device=idx, stream=stream, lib=lib)
            out.append(t)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)          # (the descriptors and the images live until here)
        return out[0], out[1]
    tiL, tiR = torch.from_numpy(imL.copy()).to(dev), torch.from_numpy(imR.copy()).to(dev)
    for mode in (0, 1):
        t = torch.empty((D, H, W), dtype=torch.float32, device=dev)
        api.build_cost_volume(tiL.data_ptr(), tiR.data_ptr(), t.data_ptr(), D, H, W, mode, d0=int(d0), lambda_ad=lambda_ad, lambda_census=lambda_census,
                              device=idx, stream=stream, lib=lib)
        _fill(t, mode, masks, int(d0), mask_fill, device=idx, stream=stream, lib=lib)
        out.append(t)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------
# data-set folders
# ------------------------------------------------------------------------------------------------
def read_calib(path):
    """Calib (LES/main.cpp:84-144): 'key = value' lines of the Middlebury v3 calib.txt."""
    out = {}
    with open(path) as f:
        for line in f:
            if "=" not in line:
                continue
            k, v = (t.strip() for t in line.split("=", 1))
            if k in ("cam0", "cam1"):
                out[k] = np.array([[float(t) for t in row.split()] for row in v.strip("[]").split(";")], np.float32)
            else:
                try:
                    out[k] = int(v)
                except ValueError:
                    out[k] = float(v)
    return out


def calib3d(calib):
    """api.Calib (les_hip_calib) of a Middlebury v3 calibration -- read_calib's dict, or a plain dict with the keys f, cx, cy, doffs, baseline:
    f = cam0[0][0], cx = cam0[0][2], cy = cam0[1][2] (pixels), doffs (pixels), baseline (the unit the points come out in; Middlebury: mm).
    View m has cx_m = cx + (m ? doffs : 0), and each view's points are in its own camera frame (X right, Y down, Z forward), so
    X_left = X_right + baseline.  An api.Calib passes through."""
    if isinstance(calib, api.Calib):
        return calib
    if "cam0" in calib:
        cam0 = np.asarray(calib["cam0"], np.float32)
        if cam0.shape != (3, 3):
            raise ValueError(f"calib3d: cam0 is a 3 x 3 matrix, not {cam0.shape}")
        f, cx, cy = cam0[0, 0], cam0[0, 2], cam0[1, 2]
    else:
        f, cx, cy = calib["f"], calib["cx"], calib["cy"]
    return api.Calib(float(f), float(cx), float(cy), float(calib.get("doffs", 0.0)), float(calib["baseline"]))


# ------------------------------------------------------------------------------------------------
# rectification of a calibrated raw pair (the transform; the maps and the sampling run on the device: csrc/les_rectify.h)
# ------------------------------------------------------------------------------------------------
def _rotation(w):
    """The rotation matrix of the rotation vector w (Rodrigues), fp64."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.sqrt(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:                                           # (sin th / th and (1 - cos th) / th^2 by their series: exact to fp64 below this angle)
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def _rotation_vector(R):
    """The rotation vector of a rotation matrix by an angle below pi, fp64."""
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.sqrt(a @ a))                               # 2 sin th
    th = float(np.arctan2(0.5 * s, 0.5 * (np.trace(R) - 1.0)))
    return a * 0.5 if s < 1e-8 else a * (th / s)


def fisheye_theta_max(k, fov=None):
    """The largest angle off the axis, radians, at which the fisheye model of csrc/les_fisheye.h with k = (k1, k2, k3, k4) may be used: the
    smallest theta in (0, pi / 2] at which Q(theta) = d theta_d / d theta = 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8 reaches
    0 -- where the polynomial folds back and two rays share a pixel --, shrunk by a relative 1e-6 so that Q > 0 up to it; pi / 2 where there is no
    such root (the roots of the quartic in theta^2: np.roots).  fov: the lens's full field of view in degrees; the result is at most half of it.
    Host numpy."""
    k = np.array(() if k is None else k, np.float64).reshape(-1)
    if k.size > 4:
        raise ValueError(f"fisheye_theta_max: {k.size} coefficients, at most 4 (k1, k2, k3, k4)")
    k = np.concatenate([k, np.zeros(4 - k.size)])
    out = 0.5 * np.pi
    coef = np.array([9.0 * k[3], 7.0 * k[2], 5.0 * k[1], 3.0 * k[0], 1.0])
    if np.any(coef[:4] != 0.0):
        t = np.roots(coef)
        t = t.real[(np.abs(t.imag) <= 1e-9 * np.maximum(1.0, np.abs(t.real))) & (t.real > 0.0)]
        th = np.sqrt(t)
        th = th[th <= 0.5 * np.pi]
        if th.size:
            out = float(th.min()) * (1.0 - 1e-6)
    if fov is not None:
        out = min(out, 0.5 * float(np.radians(float(fov))))
    return float(out)


RECTIFY_MODELS = ("pinhole", "fisheye")


def stereo_rectify(K0, dist0, K1, dist1, R, T, f=None, principal=None, model="pinhole", fov=None):
    """The rectifying transform of a calibrated raw stereo pair (Bouguet's construction), numpy fp64.
    K0, K1: the 3 x 3 pinhole matrices of the raw cameras, zero skew.  dist0, dist1: up to 8 coefficients (k1, k2, p1, p2, k3, k4, k5, k6),
    shorter inputs padded with zeros (the camera model: csrc/les_rectify.h; pixel centres at integer coordinates).  R, T: the rig in the
    stereo-calibration convention X1 = R X0 + T, with X0 and X1 one point in the left and in the right raw camera frame.
    Half of R goes to each camera by the rotation vector +-w/2, which makes the two frames parallel; then both take the smallest rotation that
    brings the baseline onto the x axis with the left camera on the left.  -> dict(R0, R1: the rectifying rotations, raw camera frame ->
    rectified frame, so that R1 X1 = R0 X0 - (baseline, 0, 0); f, cx0, cx1, cy: the new intrinsics, f and cy common to both views -- f defaults
    to (fy0 + fy1) / 2, cy to (cy0 + cy1) / 2, cx0 = K0[0, 2], cx1 = K1[0, 2], principal=(cx0, cx1, cy) overrides the three; baseline = |T|;
    doffs = cx1 - cx0; calib: the api.Calib of the rectified pair (calib3d), with which d + doffs = f baseline / Z as reconstruct assumes;
    K0, K1, dist0, dist1: the inputs as fp64 arrays, dist padded to 8).
    model="fisheye": the raw cameras are equidistant fisheye cameras (the camera model: csrc/les_fisheye.h): dist0, dist1 hold up to 4
    coefficients (k1, k2, k3, k4), padded to 4; the rotations and the new intrinsics are built the same way -- they do not depend on the
    distortion --, and the dict adds model="fisheye" and theta_max0, theta_max1 = fisheye_theta_max(dist, fov) (fov: the lenses' full field of
    view, degrees).  With model="pinhole" the dict is the one above, without these keys.
    ValueError: a skewed K, more than 8 coefficients (4 for "fisheye"), an unknown model, and a rig whose right camera is not to the right of
    the left one: a baseline nearer the y axis than the x axis (a vertical rig), or a right camera on the left."""
    if model not in RECTIFY_MODELS:
        raise ValueError(f"stereo_rectify: unknown model {model!r}: one of {RECTIFY_MODELS}")
    ncoef, names = (8, "k1, k2, p1, p2, k3, k4, k5, k6") if model == "pinhole" else (4, "k1, k2, k3, k4")
    K0, K1, R = (np.array(a, np.float64) for a in (K0, K1, R))
    T = np.array(T, np.float64).reshape(-1)
    if K0.shape != (3, 3) or K1.shape != (3, 3) or R.shape != (3, 3) or T.shape != (3,):
        raise ValueError("stereo_rectify: K0, K1 and R are 3 x 3 matrices, T has 3 entries")
    dist = []
    for K, d in ((K0, dist0), (K1, dist1)):
        if K[0, 1] != 0.0:
            raise ValueError(f"stereo_rectify: a pinhole matrix with skew {K[0, 1]!r}: only zero skew is supported")
        d = np.array(() if d is None else d, np.float64).reshape(-1)
        if d.size > ncoef:
            raise ValueError(f"stereo_rectify: {d.size} distortion coefficients, at most {ncoef} ({names})")
        dist.append(np.concatenate([d, np.zeros(ncoef - d.size)]))
    baseline = float(np.sqrt(T @ T))
    if not baseline > 0.0:
        raise ValueError("stereo_rectify: T is zero: the two cameras share a centre")
    half = _rotation(0.5 * _rotation_vector(R))             # half half = R: X0' = half X0 and X1' = half^T X1 are parallel frames
    t = half.T @ T                                          # X1' = X0' + t
    if abs(t[1]) > abs(t[0]):
        raise ValueError(f"stereo_rectify: the baseline {t.tolist()} is nearer the y axis than the x axis (a vertical rig)")
    if not t[0] < 0.0:
        raise ValueError(f"stereo_rectify: the baseline {t.tolist()} puts camera 1 to the left of camera 0: pass the cameras in the other order")
    e = np.array([-1.0, 0.0, 0.0])                           # where t / |t| goes: the right camera sits at +baseline on the left one's x axis
    w = np.cross(t, e)
    s = float(np.sqrt(w @ w))
    level = _rotation(w * (np.arctan2(s, float(t @ e)) / s)) if s > 0.0 else np.eye(3)
    R0, R1 = level @ half, level @ half.T
    fnew = 0.5 * (K0[1, 1] + K1[1, 1]) if f is None else float(f)
    cx0, cx1, cy = (K0[0, 2], K1[0, 2], 0.5 * (K0[1, 2] + K1[1, 2])) if principal is None else (float(p) for p in principal)
    out = dict(R0=R0, R1=R1, f=float(fnew), cx0=float(cx0), cx1=float(cx1), cy=float(cy), baseline=baseline, doffs=float(cx1 - cx0),
               K0=K0, K1=K1, dist0=dist[0], dist1=dist[1])
    out["calib"] = calib3d(dict(f=out["f"], cx=out["cx0"], cy=out["cy"], doffs=out["doffs"], baseline=baseline))
    if model == "fisheye":
        out.update(model="fisheye", theta_max0=fisheye_theta_max(dist[0], fov), theta_max1=fisheye_theta_max(dist[1], fov))
    return out


# ------------------------------------------------------------------------------------------------
# PLY meshes and point clouds
# ------------------------------------------------------------------------------------------------
_PLY_TYPES = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}


def write_ply(path, vertices, normals=None, colors=None, triangles=None):
    """A binary little-endian PLY: vertices N x 3 float32 (x y z), optional normals N x 3 float32 (nx ny nz), colors N x 3 uint8 RGB
    (red green blue) and triangles M x 3 int32 (vertex_indices: uchar count 3, int indices).  Every value is stored as given, bit for bit."""
    v = np.ascontiguousarray(vertices, "<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    cols = [v]
    if normals is not None:
        n = np.ascontiguousarray(normals, "<f4").reshape(-1, 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(n)
    if colors is not None:
        c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        cols.append(c)
    if any(len(a) != len(v) for a in cols):
        raise ValueError("write_ply: normals and colors need one row per vertex")
    rec = np.empty(len(v), np.dtype(fields))
    names = [f[0] for f in fields]
    for k, a in enumerate(cols):
        for j in range(3):
            rec[names[3 * k + j]] = a[:, j]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'uchar' if t == 'u1' else 'float'} {name}" for name, t in fields]
    tri = None
    if triangles is not None:
        t = np.ascontiguousarray(triangles, "<i4").reshape(-1, 3)
        tri = np.empty(len(t), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        tri["n"] = 3
        tri["v"] = t
        head += [f"element face {len(t)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        if tri is not None:
            f.write(tri.tobytes())


def read_ply(path):
    """What write_ply wrote: dict(vertices, normals, colors, triangles), None for what the file does not hold.  Binary little-endian files whose
    vertex properties are scalars and whose faces are all triangles (list uchar int)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian PLY files are read")
    counts, props, element = {}, {}, None
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"]:
            element = tok[1]
            counts[element], props[element] = int(tok[2]), []
        elif tok[:1] == ["property"]:
            props[element].append(tok[1:])
    if list(counts) not in (["vertex"], ["vertex", "face"]) or any(len(p) != 2 for p in props["vertex"]):
        raise ValueError(f"{path}: a vertex element of scalar properties, then an optional face element, expected")
    dt = np.dtype([(name, _PLY_TYPES[t]) for t, name in props["vertex"]])
    nv = counts["vertex"]
    rec = np.frombuffer(body, dt, nv)
    grab = lambda names, t: np.stack([rec[n] for n in names], 1).astype(t) if all(n in dt.names for n in names) else None
    out = dict(vertices=grab(("x", "y", "z"), np.float32), normals=grab(("nx", "ny", "nz"), np.float32), colors=grab(("red", "green", "blue"), np.uint8),
               triangles=None)
    if "face" in counts:
        if props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
            raise ValueError(f"{path}: faces as 'property list uchar int vertex_indices' expected")
        tri = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), counts["face"], offset=nv * dt.itemsize)
        if not (tri["n"] == 3).all():
            raise ValueError(f"{path}: a face that is not a triangle")
        out["triangles"] = np.ascontiguousarray(tri["v"], np.int32)
    return out


def _imread_bgr(path, gray=False):
    from PIL import Image           # only the data-set loader needs an image decoder
    if not os.path.exists(path):
        return None
    im = Image.open(path)
    if gray:
        return np.asarray(im.convert("L"))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def load_data(input_dir, ndisp=0):
    """loadData (LES/main.cpp:201-268).  Returns dict(imL, imR [BGR uint8], dispGT float32 (inf where unknown for the
    PNG ground truth), nonocc bool, ndisp, gt_prec)."""
    d = input_dir if input_dir.endswith(os.sep) else input_dir + os.sep
    gt_prec = -1.0
    info = d + "info.txt"
    if os.path.exists(info):
        toks = open(info).read().split()
        gt_scale, nd = int(toks[0]), int(toks[1])
        gt_prec = 1.0 / gt_scale
        if ndisp <= 0:
            ndisp = nd
    elif os.path.exists(d + "calib.txt"):
        c = read_calib(d + "calib.txt")
        if ndisp <= 0:
            ndisp = int(c.get("ndisp", 0))
    if ndisp <= 0:
        raise ValueError("ndisp is not specified")
    imL, imR = _imread_bgr(d + "imL.png"), _imread_bgr(d + "imR.png")
    if imL is None or imR is None:
        imL, imR = _imread_bgr(d + "im0.png"), _imread_bgr(d + "im1.png")
    if imL is None or imR is None:
        raise FileNotFoundError(f"image pairs (im0.png, im1.png) or (imL.png, imR.png) not found in {d}")
    gt = _imread_bgr(d + "groundtruth.png", gray=True)
    if gt is not None:
        gtf = gt.astype(np.float32)
        if gt_prec > 0:
            gtf = gtf * np.float32(gt_prec)
        gtf[gt == 0] = np.inf
        gt = gtf
    elif os.path.exists(d + "disp0GT.pfm"):
        gt = read_pfm(d + "disp0GT.pfm")
    else:
        gt = np.zeros(imL.shape[:2], np.float32)
    nonocc = _imread_bgr(d + "nonocc.png", gray=True)
    if nonocc is None:
        nonocc = _imread_bgr(d + "mask0nocc.png", gray=True)
    nonocc = (nonocc == 255) if nonocc is not None else np.ones(imL.shape[:2], bool)
    return dict(imL=imL, imR=imR, dispGT=gt, nonocc=nonocc, ndisp=int(ndisp), gt_prec=gt_prec)


# ------------------------------------------------------------------------------------------------
# Evaluator
# ------------------------------------------------------------------------------------------------
class Evaluator:
    """Bad-pixel rates of LES/Evaluator.h: valid = gt > 0 and finite (:77); a pixel is good when |d - gt| <= threshold
    (:133); all = 100 (1 - good&valid / valid), nonocc = 100 (1 - good&nonocc / |nonocc|) (:137-140)."""

    def __init__(self, dispGT, nonocc_mask, error_threshold=0.5):
        self.gt = np.asarray(dispGT, np.float32)
        self.nonocc = np.asarray(nonocc_mask, bool)
        self.valid = (self.gt > 0) & np.isfinite(self.gt)
        self.threshold = float(error_threshold)

    def evaluate(self, disp):
        with np.errstate(invalid="ignore"):
            good = np.abs(np.asarray(disp, np.float32) - self.gt) <= np.float32(self.threshold)
        nv, nn = int(self.valid.sum()), int(self.nonocc.sum())
        all_ = 100.0 * (1.0 - (good & self.valid).sum() / nv) if nv else float("nan")
        non_ = 100.0 * (1.0 - (good & self.nonocc).sum() / nn) if nn else float("nan")
        return float(all_), float(non_)


def sparsification(disp, gt, conf, valid=None, threshold=1.0):
    """How well a confidence map ranks the errors of a disparity map (the sparsification curve of the confidence literature), in host numpy.
    valid: the pixels that count (None: gt > 0 and finite, as the Evaluator); a valid pixel is bad when not |disp - gt| <= threshold (a
    non-finite disparity is bad).  The valid pixels are ordered by descending confidence with a stable sort (a NaN confidence ranks last);
    -> dict(bad: the bad-pixel rate of all valid pixels, which is what a random order gives in expectation; auc: the mean, over every prefix
    of that order, of the bad-pixel rate of the prefix -- the area under the curve "rate of the n most confident pixels"; auc_optimal: the
    same with the pixels ordered by the error itself, the least any confidence can reach).  Rates are fractions in [0, 1]; NaN without a valid
    pixel."""
    disp, gt, conf = np.asarray(disp, np.float32), np.asarray(gt, np.float32), np.asarray(conf, np.float32)
    if not disp.shape == gt.shape == conf.shape:
        raise ValueError(f"sparsification: maps of one shape, not {disp.shape}, {gt.shape}, {conf.shape}")
    valid = (gt > 0) & np.isfinite(gt) if valid is None else np.asarray(valid, bool)
    n = int(valid.sum())
    if n == 0:
        return dict(bad=float("nan"), auc=float("nan"), auc_optimal=float("nan"))
    with np.errstate(invalid="ignore"):
        err = np.abs(disp[valid].astype(np.float64) - gt[valid])
    err = np.where(np.isnan(err), np.inf, err)
    bad = ~(err <= threshold)
    c = conf[valid].astype(np.float64)
    c = np.where(np.isnan(c), -np.inf, c)
    counts = np.arange(1, n + 1, dtype=np.float64)
    area = lambda order: float((np.cumsum(bad[order], dtype=np.float64) / counts).mean())
    return dict(bad=float(bad.mean()), auc=area(np.argsort(-c, kind="stable")), auc_optimal=area(np.argsort(err, kind="stable")))


def photometric(err, vis, thresh=10.0):
    """A photometric-error map (FastGCStereo.photo_error, api.HipCostVolumeEnergy.photo_error) summed up, in host numpy: -> dict(mean: the mean
    of err over the pixels seen in the other view (vis == 1), accumulated in float64, in grey levels; bad: the fraction of those pixels with
    err > thresh; visible: the fraction of all pixels with vis == 1; occluded: that with vis == 2).  mean and bad are NaN without a visible
    pixel.  No ground truth is involved: a low mean says the labels explain the other image, not that they are right where the image is flat."""
    err, vis = np.asarray(err, np.float32), np.asarray(vis)
    if err.shape != vis.shape:
        raise ValueError(f"photometric: maps of one shape, not {err.shape}, {vis.shape}")
    seen = vis == 1
    n = int(seen.sum())
    e = err[seen].astype(np.float64)
    return dict(mean=float(e.mean()) if n else float("nan"), bad=float((e > thresh).mean()) if n else float("nan"),
                visible=float(n / vis.size) if vis.size else float("nan"), occluded=float((vis == 2).sum() / vis.size) if vis.size else float("nan"))
