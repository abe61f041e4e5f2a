"""ctypes binding of the C ABI in include/localexp_hip.h (liblocalexp_hip.so).

This is plumbing for tests and bench.py: the product is the shared library and the C++ host adapter
(localexpstereo_amd/host/).  The library is loaded from csrc/ in-tree; if it is missing, or no HIP
device is present, everything here raises -- there is no CPU fallback.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "liblocalexp_hip.so")

RECT_DT = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4")])
PLANE_DT = np.dtype([("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("v", "<f4")])

# every symbol include/localexp_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "les_hip_create", "les_hip_create_naive", "les_hip_create_filtered", "les_hip_create_naive_filtered", "les_hip_destroy", "les_hip_last_error", "les_hip_set_stream", "les_hip_set_thread_stream", "les_hip_synchronize",
    "les_hip_unary_one", "les_hip_unary_one_scratch", "les_hip_scratch_create", "les_hip_scratch_destroy", "les_hip_unary_batch", "les_hip_batch_create", "les_hip_batch_destroy",
    "les_hip_batch_num_jobs", "les_hip_batch_kernel_kind", "les_hip_batch_graph_nodes", "les_hip_batch_graph_offsets", "les_hip_batch_expansion_graph", "les_hip_batch_fusion_graph", "les_hip_batch_max_cell_nodes", "les_hip_batch_graph_solver_kind", "les_hip_refresh_volume", "les_hip_set_interpolation", "les_hip_set_max_vdisparity", "les_hip_set_random_vdisparity", "les_hip_batch_solve_graphs", "les_hip_batch_solve_graphs_counted", "les_hip_batch_solve_graphs_tiled", "les_hip_batch_solve_graphs_tiled_stats", "les_hip_batch_tiled_workspace_bytes", "les_hip_batch_apply_masks", "les_hip_batch_apply_masks_labels", "les_hip_batch_run", "les_hip_batch_set_units", "les_hip_batch_propose", "les_hip_batch_wta",
    "les_hip_wta_update", "les_hip_malloc", "les_hip_free",
    "les_hip_memcpy_h2d", "les_hip_memcpy_d2h", "les_hip_memset", "les_hip_get_stats", "les_hip_strip_width", "les_hip_tiled_volume_bytes",
    "les_hip_calib_copy", "les_hip_calib_copy_wide", "les_hip_exchange_create", "les_hip_exchange_destroy", "les_hip_exchange_slot_floats",
    "les_hip_exchange_pack", "les_hip_exchange_unpack", "les_hip_exchange_tiles", "les_hip_fill_out_of_view", "les_hip_convert_volume_l2r", "les_hip_consistency_check", "les_hip_post_process",
    "les_hip_evaluator_create", "les_hip_evaluator_destroy", "les_hip_evaluate", "les_hip_evaluator_rows", "les_hip_batch_region_energy",
    "les_hip_unary_labels", "les_hip_unary_labels_kind",
    "les_hip_costvol_tables", "les_hip_census", "les_hip_build_cost_volume", "les_hip_costvol_last_times",
    "les_hip_patch_features", "les_hip_build_feature_volume", "les_hip_featvol_last_times",
    "les_hip_warp_labels",
    "les_hip_slab_argmin_state_bytes", "les_hip_slab_argmin", "les_hip_slab_argmin_finish", "les_hip_wta_labels",
    "les_hip_sgm_workspace_bytes", "les_hip_sgm_labels", "les_hip_sgm_last_times",
    "les_hip_fit_planes",
    "les_hip_pool_image", "les_hip_pool_volume", "les_hip_create_half", "les_hip_get_image", "les_hip_upsample_labels",
    "les_hip_speckle_mask", "les_hip_speckle_tile", "les_hip_post_process_speckle",
    "les_hip_slab_confidence_state_bytes", "les_hip_slab_confidence", "les_hip_slab_confidence_finish", "les_hip_confidence", "les_hip_post_process_masked",
    "les_hip_reproject", "les_hip_mesh", "les_hip_mesh_tile",
    "les_hip_render_view", "les_hip_blend_views", "les_hip_photo_error",
    "les_hip_rectify_map", "les_hip_remap",
    "les_hip_unrectify_map", "les_hip_unrectify_labels",
    "les_hip_rectify_map_fisheye", "les_hip_unrectify_map_fisheye",
    "les_hip_fill_invalid",
]


PROPOSE_EXPANSION, PROPOSE_RANDOM, PROPOSE_RANSAC, PROPOSE_INIT = 0, 1, 2, 3
LES_HIP_OK, LES_HIP_ERR_ARG, LES_HIP_ERR_DEVICE, LES_HIP_ERR_UNSUPPORTED = 0, 1, 2, 3        # the return codes of include/localexp_hip.h

# Parameters::filterName (LES/StereoEnergy.h:25) -> les_hip_create_filtered's filter.  The reference's CostVolumeEnergy knows the bilateral
# filter as "BL" and NaiveStereoEnergy as "BF" (CostVolumeEnergy given "BF" dereferences a null filter): both names select it for both energies.
FILTER_GF, FILTER_BILATERAL, FILTER_NONE = 0, 1, 2
FILTER_NAMES = {"GF": FILTER_GF, "BF": FILTER_BILATERAL, "BL": FILTER_BILATERAL, "": FILTER_NONE}


def filter_kind(name):
    """les_hip filter enum of a Parameters::filterName ("GFfloat" is not implemented)."""
    if name not in FILTER_NAMES:
        raise ValueError(f"unsupported filter {name!r}: one of {sorted(FILTER_NAMES)}")
    return FILTER_NAMES[name]


class LesHipError(RuntimeError):
    pass


class TiledStats(C.Structure):
    """les_hip_tiled_stats (include/localexp_hip.h)."""
    _fields_ = [("launches", C.c_int), ("unsolved", C.c_int), ("handed_cells", C.c_int), ("handed_nodes", C.c_longlong), ("host_ms", C.c_double)]


class EvalRow(C.Structure):
    """les_hip_eval_row (include/localexp_hip.h)."""
    _fields_ = [("index", C.c_int), ("mode", C.c_int), ("data", C.c_double), ("smooth", C.c_double), ("good_valid", C.c_longlong),
                ("good_nonocc", C.c_longlong), ("n_valid", C.c_longlong), ("n_nonocc", C.c_longlong)]


class Calib(C.Structure):
    """les_hip_calib (include/localexp_hip.h): a rectified pinhole pair; io.calib3d makes one from a Middlebury calib.txt."""
    _fields_ = [("f", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("doffs", C.c_float), ("baseline", C.c_float)]


class Camera(C.Structure):
    """les_hip_camera (include/localexp_hip.h): a raw pinhole camera, dist = (k1, k2, p1, p2, k3, k4, k5, k6)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 8)]


class Fisheye(C.Structure):
    """les_hip_fisheye (include/localexp_hip.h): a raw equidistant fisheye camera, k = (k1, k2, k3, k4), theta_max in (0, pi]."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 4), ("theta_max", C.c_double)]


class Params(C.Structure):
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("D", C.c_int), ("windR", C.c_int), ("eps", C.c_double),
                ("th_col", C.c_float), ("max_disparity", C.c_float), ("min_disparity", C.c_float),
                ("device", C.c_int), ("volumes_on_device", C.c_int)]


_libs = {}


def load(path=None):
    """Load the C-ABI library (default: the in-tree HIP build).  Raises if it does not exist."""
    from_env = path is None and bool(os.environ.get("LES_HIP_LIB"))
    path = os.path.abspath(path or os.environ.get("LES_HIP_LIB") or DEFAULT_LIB)     # LES_HIP_LIB: A/B builds of the same ABI
    if path in _libs:
        return _libs[path]
    # LES_HIP_LIB is a measurement switch between HIP builds.  Anything without a gfx950 code object (the CPU simulator build the
    # tests use, or a stranger's library with the same symbols) is refused, so that an environment variable can never put a
    # CPU path under the package; tests that exercise the simulator pass its path explicitly (or set LES_HIP_ALLOW_SIM=1).
    if from_env and os.path.exists(path) and os.environ.get("LES_HIP_ALLOW_SIM") != "1":
        blob = open(path, "rb").read()
        if b"gfx950" not in blob or b"les_march_kernel" not in blob:
            raise LesHipError(f"LES_HIP_LIB={path} holds no gfx950 code object of this package's kernels; refusing to load it "
                              "(set LES_HIP_ALLOW_SIM=1 only in tests of the simulator build)")
    # PyTorch-ROCm bundles its own HIP runtime.  If this library initialises the system runtime first and torch
    # initialises CUDA/HIP later in the same process, torch reports "No HIP GPUs are available".  Loading torch's
    # runtime first makes both share one copy (bench.py / pm.py use torch tensors for device memory anyway).
    if os.environ.get("LES_HIP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    if not os.path.exists(path):
        raise LesHipError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path)
    vp, ci = C.c_void_p, C.c_int
    sig = {
        "les_hip_create": (ci, [C.POINTER(vp), C.POINTER(Params), vp, vp, vp, vp]),
        "les_hip_batch_graph_nodes": (C.c_longlong, [vp]),
        "les_hip_batch_graph_offsets": (ci, [vp, vp]),
        "les_hip_batch_expansion_graph": (ci, [vp, vp, ci, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp]),
        "les_hip_batch_apply_masks": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "les_hip_batch_fusion_graph": (ci, [vp, vp, ci, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp]),
        "les_hip_batch_apply_masks_labels": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "les_hip_batch_max_cell_nodes": (C.c_longlong, [vp]),
        "les_hip_batch_graph_solver_kind": (ci, [vp]),
        "les_hip_refresh_volume": (ci, [vp, ci]),
        "les_hip_batch_solve_graphs": (ci, [vp, vp, vp, vp, vp, vp]),
        "les_hip_batch_solve_graphs_counted": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "les_hip_batch_solve_graphs_tiled": (ci, [vp, vp, vp, vp, vp, vp, vp, C.c_longlong, C.POINTER(ci), C.POINTER(ci)]),
        "les_hip_batch_solve_graphs_tiled_stats": (ci, [vp, vp, vp, vp, vp, vp, vp, C.c_longlong, C.POINTER(TiledStats)]),
        "les_hip_batch_tiled_workspace_bytes": (C.c_longlong, [vp]),
        "les_hip_calib_copy": (ci, [vp, vp, C.c_size_t, ci, vp]),
        "les_hip_calib_copy_wide": (ci, [vp, vp, C.c_size_t, ci, vp]),
        "les_hip_exchange_create": (ci, [vp, ci, ci, ci, vp, vp, C.POINTER(vp)]),
        "les_hip_exchange_destroy": (None, [vp]),
        "les_hip_exchange_slot_floats": (C.c_longlong, [vp]),
        "les_hip_exchange_pack": (ci, [vp, vp, vp, vp, vp]),
        "les_hip_exchange_unpack": (ci, [vp, vp, vp, vp, vp]),
        "les_hip_exchange_tiles": (ci, [vp, vp, vp, vp, vp]),
        "les_hip_consistency_check": (ci, [vp, vp, vp, C.c_float, vp, vp]),
        "les_hip_post_process": (ci, [vp, vp, vp, C.c_float, C.c_float]),
        "les_hip_create_naive": (ci, [C.POINTER(vp), C.POINTER(Params), vp, vp, C.c_float, C.c_float]),
        "les_hip_create_filtered": (ci, [C.POINTER(vp), C.POINTER(Params), ci, vp, vp, vp, vp]),
        "les_hip_create_naive_filtered": (ci, [C.POINTER(vp), C.POINTER(Params), ci, vp, vp, C.c_float, C.c_float]),
        "les_hip_destroy": (None, [vp]),
        "les_hip_last_error": (C.c_char_p, []),
        "les_hip_set_stream": (ci, [vp, vp]),
        "les_hip_set_thread_stream": (ci, [vp, vp, ci]),
        "les_hip_synchronize": (ci, [vp]),
        "les_hip_unary_one": (ci, [vp, ci, vp, vp, vp, vp, ci, ci]),
        "les_hip_unary_batch": (ci, [vp, ci, ci, vp, vp, vp, vp, ci]),
        "les_hip_unary_one_scratch": (ci, [vp, vp, ci, vp, vp, vp, vp, ci, ci]),
        "les_hip_scratch_create": (ci, [vp, C.POINTER(vp)]),
        "les_hip_scratch_destroy": (None, [vp]),
        "les_hip_batch_create": (ci, [vp, ci, vp, vp, ci, C.POINTER(vp)]),
        "les_hip_batch_destroy": (None, [vp]),
        "les_hip_batch_num_jobs": (ci, [vp]),
        "les_hip_batch_kernel_kind": (ci, [vp, vp, ci]),
        "les_hip_set_interpolation": (ci, [vp, ci]),
        "les_hip_set_max_vdisparity": (ci, [vp, C.c_float]),
        "les_hip_set_random_vdisparity": (ci, [vp, C.c_float]),
        "les_hip_batch_run": (ci, [vp, vp, ci, vp, ci, vp, ci]),
        "les_hip_batch_set_units": (ci, [vp, vp, vp]),
        "les_hip_batch_propose": (ci, [vp, vp, ci, ci, vp, vp, vp]),
        "les_hip_batch_wta": (ci, [vp, vp, vp, vp, vp, vp]),
        "les_hip_wta_update": (ci, [vp, ci, vp, vp, ci, vp, vp, vp]),
        "les_hip_malloc": (ci, [vp, C.POINTER(vp), C.c_size_t]),
        "les_hip_free": (ci, [vp, vp]),
        "les_hip_memcpy_h2d": (ci, [vp, vp, vp, C.c_size_t]),
        "les_hip_memcpy_d2h": (ci, [vp, vp, vp, C.c_size_t]),
        "les_hip_memset": (ci, [vp, vp, ci, C.c_size_t]),
        "les_hip_get_stats": (ci, [vp, ci, vp]),
        "les_hip_strip_width": (ci, [ci]),
        "les_hip_tiled_volume_bytes": (C.c_size_t, [vp, ci]),
        "les_hip_fill_out_of_view": (ci, [vp, ci, ci, ci, ci, ci, vp]),
        "les_hip_convert_volume_l2r": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "les_hip_evaluator_create": (ci, [vp, vp, vp, C.c_float, C.c_float, ci, C.POINTER(vp)]),
        "les_hip_evaluator_destroy": (None, [vp]),
        "les_hip_evaluate": (ci, [vp, vp, ci, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, ci]),
        "les_hip_evaluator_rows": (ci, [vp, vp, vp, ci, C.POINTER(ci)]),
        "les_hip_batch_region_energy": (ci, [vp, vp, ci, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp]),
        "les_hip_unary_labels": (ci, [vp, ci, vp, vp, vp, ci]),
        "les_hip_unary_labels_kind": (ci, [vp, ci]),
        "les_hip_costvol_tables": (ci, [C.c_float, C.c_float, vp, vp]),
        "les_hip_census": (ci, [vp, vp, ci, ci, ci, vp]),
        "les_hip_build_cost_volume": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, C.c_float, C.c_float, ci, vp]),
        "les_hip_costvol_last_times": (ci, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "les_hip_patch_features": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
        "les_hip_build_feature_volume": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, C.c_float, C.c_float, ci, vp]),
        "les_hip_featvol_last_times": (ci, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "les_hip_warp_labels": (ci, [vp, ci, vp, vp, vp, vp]),
        "les_hip_slab_argmin_state_bytes": (C.c_size_t, [ci, ci]),
        "les_hip_slab_argmin": (ci, [vp, vp, ci, ci, vp]),
        "les_hip_slab_argmin_finish": (ci, [vp, vp, ci, ci, vp, vp]),
        "les_hip_wta_labels": (ci, [vp, ci, ci, ci, vp, vp]),
        "les_hip_sgm_workspace_bytes": (C.c_size_t, [vp]),
        "les_hip_sgm_labels": (ci, [vp, ci, ci, C.c_float, C.c_float, ci, vp, vp]),
        "les_hip_sgm_last_times": (ci, [C.POINTER(C.c_float), ci, C.POINTER(ci)]),
        "les_hip_fit_planes": (ci, [vp, ci, vp, vp, vp, vp, vp, ci, C.c_float, C.c_float, C.c_float, C.c_float, ci]),
        "les_hip_pool_image": (ci, [vp, vp, ci, ci, ci, vp]),
        "les_hip_pool_volume": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "les_hip_create_half": (ci, [C.POINTER(vp), vp]),
        "les_hip_get_image": (ci, [vp, ci, vp]),
        "les_hip_upsample_labels": (ci, [vp, vp, ci, vp, vp, vp]),
        "les_hip_speckle_mask": (ci, [vp, vp, ci, C.c_float, vp, vp, vp]),
        "les_hip_speckle_tile": (ci, [C.POINTER(ci), C.POINTER(ci)]),
        "les_hip_post_process_speckle": (ci, [vp, vp, vp, C.c_float, C.c_float, ci, C.c_float]),
        "les_hip_slab_confidence_state_bytes": (C.c_size_t, [ci, ci]),
        "les_hip_slab_confidence": (ci, [vp, vp, vp, ci, ci, C.c_float, vp]),
        "les_hip_slab_confidence_finish": (ci, [vp, vp, C.c_float, vp, vp, vp, vp]),
        "les_hip_confidence": (ci, [vp, ci, vp, ci, C.c_float, C.c_float, vp, vp, vp, vp]),
        "les_hip_post_process_masked": (ci, [vp, vp, vp, C.c_float, C.c_float, ci, C.c_float, vp, vp]),
        "les_hip_reproject": (ci, [vp, ci, vp, vp, C.POINTER(Calib), C.c_float, vp, vp, vp]),
        "les_hip_render_view": (ci, [vp, ci, vp, vp, C.c_float, vp, vp, vp]),
        "les_hip_blend_views": (ci, [vp, C.c_float, C.c_float, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "les_hip_photo_error": (ci, [vp, ci, vp, vp, vp]),
        "les_hip_rectify_map": (ci, [C.POINTER(Camera), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, vp, ci, ci, ci, vp]),
        "les_hip_remap": (ci, [vp, ci, ci, ci, vp, vp, vp, ci, ci, ci, ci, vp]),
        "les_hip_fill_invalid": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, C.c_float, ci, vp]),
        "les_hip_unrectify_map": (ci, [C.POINTER(Camera), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, ci, C.c_double, vp, ci, ci, ci, vp]),
        "les_hip_rectify_map_fisheye": (ci, [C.POINTER(Fisheye), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, vp, ci, ci, ci, vp]),
        "les_hip_unrectify_map_fisheye": (ci, [C.POINTER(Fisheye), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, ci, C.c_double, vp, ci, ci, ci, vp]),
        "les_hip_unrectify_labels": (ci, [vp, ci, ci, vp, vp, ci, ci, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_float, vp, vp, vp, vp, ci, vp]),
        "les_hip_mesh": (ci, [vp, ci, vp, vp, C.c_float, vp, vp, vp, vp]),
        "les_hip_mesh_tile": (ci, [C.POINTER(ci), C.POINTER(ci)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _libs[path] = L
    return L


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _vp(p):
    """A nullable device address (an int, or None / 0 for an optional map that is not there) as the ABI takes it."""
    return C.c_void_p(int(p)) if p else None


def _float_tensor(a, dev):
    """`a` as a contiguous float32 torch tensor on dev: a tensor that is all that already is returned itself, anything else is copied."""
    import torch
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev)          # (a copy: torch wants a writable array)


def _rects(r):
    r = np.asarray(r)
    if r.dtype != RECT_DT:
        r = np.ascontiguousarray(r, np.int32).reshape(-1, 4).view(RECT_DT).reshape(-1)
    return np.ascontiguousarray(r)


def _planes(p):
    p = np.asarray(p)
    if p.dtype != PLANE_DT:
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 4).view(PLANE_DT).reshape(-1)
    return np.ascontiguousarray(p)


def fill_out_of_view(vol_dev_ptr, D, H, W, mode, device=0, stream=0, lib=None):
    """fillOutOfView (LES/main.cpp:146-176) in place on a device volume."""
    L = load(lib)
    rc = L.les_hip_fill_out_of_view(C.c_void_p(int(vol_dev_ptr)), D, H, W, mode, device, C.c_void_p(int(stream)))
    if rc:
        raise LesHipError(L.les_hip_last_error().decode())


def convert_volume_l2r(src_dev_ptr, dst_dev_ptr, D, H, W, device=0, stream=0, lib=None):
    """convertVolumeL2R (LES/main.cpp:178-199): right-view volume synthesised from the left-view one."""
    L = load(lib)
    rc = L.les_hip_convert_volume_l2r(C.c_void_p(int(src_dev_ptr)), C.c_void_p(int(dst_dev_ptr)), D, H, W, device, C.c_void_p(int(stream)))
    if rc:
        raise LesHipError(L.les_hip_last_error().decode())


def _chk_lib(L, rc):
    if rc:
        raise LesHipError(f"liblocalexp_hip error {rc}: {L.les_hip_last_error().decode()}")


FILL_INVALID_CHUNK, FILL_INVALID_MAX_W = 32, 32768     # les_hip_fill_invalid: slices per workgroup, widest row (kMvDC, kMvMaxW of csrc/les_maskvol.h)


def fill_invalid(vol_dev_ptr, D, H, W, mode, validI=None, validJ=None, d0=0, fill=0.5, device=0, stream=0, lib=None):
    """les_hip_fill_invalid: fill_out_of_view with "outside the image" widened to "outside the valid image", in place on a device volume
    [D][H][W] (slice k is disparity k + d0; mode 0: the left view's volume, I = L, J = R; mode 1: the right view's).  validI / validJ: device
    addresses of H x W byte masks of the volume's own view and of its partner view, nonzero = valid, None = all valid.  An entry that the
    reference sees, whose own pixel is valid and whose partner pixel is valid is never written; every other entry takes the bits of the nearest
    such entry of its row and slice (a tie goes right in mode 0, left in mode 1); a row of a slice without one is set to `fill` (finite).  With
    both masks None and d0 = 0: fill_out_of_view's bytes (csrc/les_maskvol.h).  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_fill_invalid(_vp(vol_dev_ptr), D, H, W, mode, int(d0), _vp(validI), _vp(validJ), float(fill), device, C.c_void_p(int(stream))))


def costvol_tables(lambda_ad=10.0, lambda_census=30.0, lib=None):
    """The two tables of the AD-Census cost (csrc/les_costvol.h) as build_cost_volume uses them: ta[0..765] indexed by the summed absolute
    colour difference, tc[0..62] by the Hamming distance of the census signatures."""
    L = load(lib)
    ta, tc = np.empty(766, np.float32), np.empty(63, np.float32)
    _chk_lib(L, L.les_hip_costvol_tables(lambda_ad, lambda_census, _ptr(ta), _ptr(tc)))
    return ta, tc


def census(bgr_dev_ptr, sig_dev_ptr, H, W, device=0, stream=0, lib=None):
    """9 x 7 census signatures (uint64 per pixel) of a device H x W x 3 u8 BGR image.  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_census(C.c_void_p(int(bgr_dev_ptr)), C.c_void_p(int(sig_dev_ptr)), H, W, device, C.c_void_p(int(stream))))


def build_cost_volume(imL_dev_ptr, imR_dev_ptr, vol_dev_ptr, D, H, W, mode, d0=0, lambda_ad=10.0, lambda_census=30.0, device=0, stream=0, lib=None):
    """The AD-Census matching-cost volume of one view (mode 0 left, 1 right) from the two device images into the device float [D][H][W]
    volume; slice k is disparity k + d0.  What the reference reads from an external MC-CNN run (LES/main.cpp:353-357).  Every entry is
    written (out-of-view ones through the clamped column): fill_out_of_view comes after it.  Synchronises the stream."""
    L = load(lib)
    _chk_lib(L, L.les_hip_build_cost_volume(C.c_void_p(int(imL_dev_ptr)), C.c_void_p(int(imR_dev_ptr)), C.c_void_p(int(vol_dev_ptr)), D, H, W, mode, d0,
                                            lambda_ad, lambda_census, device, C.c_void_p(int(stream))))


FEATVOL_MAX_CHANNELS = 512     # kFvMaxC of csrc/les_featvol.h (the one source; tests/featvol_cases.py: case_errors holds this copy to it)
PATCH_MAX_RADIUS = 4           # kFvMaxRadius


def patch_features(bgr_dev_ptr, feat_dev_ptr, H, W, ry=2, rx=2, device=0, stream=0, lib=None):
    """The ZNCC patch descriptor (csrc/les_featvol.h) of a device H x W x 3 u8 BGR image into the device float [(2 ry + 1)(2 rx + 1)][H][W]
    feature map: the zero-mean, unit-norm grey patch around every pixel (zero where the patch is flat), radii 0 .. 4.  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_patch_features(C.c_void_p(int(bgr_dev_ptr)), C.c_void_p(int(feat_dev_ptr)), H, W, ry, rx, device, C.c_void_p(int(stream))))


def build_feature_volume(featL_dev_ptr, featR_dev_ptr, vol_dev_ptr, Cn, D, H, W, mode, d0=0, alpha=0.5, beta=0.5, device=0, stream=0, lib=None):
    """The correlation matching-cost volume of one view (mode 0 left, 1 right) from the two views' device float [Cn][H][W] feature maps into
    the device float [D][H][W] volume: cost = beta - alpha <fI(x), fJ(xp)> as the f32 fma chain of csrc/les_featvol.h, slice k is disparity
    k + d0.  The features are used as given.  Every entry is written (out-of-view ones through the clamped column): fill_out_of_view comes
    after it.  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_build_feature_volume(C.c_void_p(int(featL_dev_ptr)), C.c_void_p(int(featR_dev_ptr)), C.c_void_p(int(vol_dev_ptr)), Cn, D, H, W,
                                               mode, d0, alpha, beta, device, C.c_void_p(int(stream))))


def half_size(n):
    """The pooled size of a dimension of n (csrc/les_pyramid.h): (n + 1) // 2."""
    return (int(n) + 1) // 2


def pool_image(src_dev_ptr, dst_dev_ptr, H, W, device=0, stream=0, lib=None):
    """les_hip_pool_image: a device H x W x 3 u8 image pooled by two into the device half_size(H) x half_size(W) x 3 one, per channel
    (p00 + p01 + p10 + p11 + 2) >> 2 with the source indices clamped (csrc/les_pyramid.h).  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_pool_image(C.c_void_p(int(src_dev_ptr)), C.c_void_p(int(dst_dev_ptr)), H, W, device, C.c_void_p(int(stream))))


def pool_volume(src_dev_ptr, dst_dev_ptr, D, H, W, device=0, stream=0, lib=None):
    """les_hip_pool_volume: a device float [D][H][W] volume pooled by two in every dimension into the device [half_size(D)][half_size(H)]
    [half_size(W)] one: half slice k is full slice 2k, weights (1/4, 1/2, 1/4) over the slices 2k - 1 .. 2k + 1 and the mean of the 2 x 2 pixels,
    source indices clamped, in the fixed f32 order of csrc/les_pyramid.h (exact: the same bytes on every build).  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_pool_volume(C.c_void_p(int(src_dev_ptr)), C.c_void_p(int(dst_dev_ptr)), D, H, W, device, C.c_void_p(int(stream))))


INTERP_NAMES = {"nearest": 0, "linear": 1, "cubic": 2}          # les_hip_remap's interp


def camera(K, dist=()):
    """A Camera (les_hip_camera) of a 3 x 3 pinhole matrix with zero skew and up to 8 distortion coefficients (k1, k2, p1, p2, k3, k4, k5, k6),
    shorter inputs padded with zeros.  A Camera passes through."""
    if isinstance(K, Camera):
        return K
    K = np.asarray(K, np.float64)
    d = np.asarray(dist if dist is not None else (), np.float64).reshape(-1)
    if K.shape != (3, 3) or K[0, 1] != 0.0:
        raise ValueError("camera: K is a 3 x 3 pinhole matrix with zero skew")
    if d.size > 8:
        raise ValueError(f"camera: {d.size} distortion coefficients, at most 8 (k1, k2, p1, p2, k3, k4, k5, k6)")
    return Camera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], (C.c_double * 8)(*np.concatenate([d, np.zeros(8 - d.size)])))


def rectify_map(raw, M, f, cx, cy, map_dev_ptr, H, W, device=0, stream=0, lib=None):
    """les_hip_rectify_map: the device H x W x 2 float map of the raw positions (u, v) of the rectified pixels of one view.  raw: a Camera (or
    what camera() takes as K); M: 3 x 3, a ray of the rectified frame into the raw camera's frame (the transpose of the view's rectifying
    rotation); f, cx, cy: the rectified view's intrinsics.  fp64 in the fixed order of csrc/les_rectify.h, (NaN, NaN) where there is no raw
    position.  Enqueue only."""
    L = load(lib)
    cam = camera(raw)
    m = (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9))
    _chk_lib(L, L.les_hip_rectify_map(C.byref(cam), m, float(f), float(cx), float(cy), _vp(map_dev_ptr), H, W, device, C.c_void_p(int(stream))))


def remap(src_dev_ptr, Hs, Ws, channels, map_dev_ptr, dst_dev_ptr, valid_dev_ptr, H, W, interp=1, device=0, stream=0, lib=None):
    """les_hip_remap: the device Hs x Ws x channels u8 image sampled at the device H x W x 2 float map into the device H x W x channels one;
    interp 0 nearest, 1 linear, 2 cubic (or their INTERP_NAMES); valid_dev_ptr (H x W bytes, 1 / 0) may be None.  A pixel whose map entry is
    not finite or lies outside the source is 0 and invalid (csrc/les_rectify.h).  Enqueue only."""
    L = load(lib)
    _chk_lib(L, L.les_hip_remap(_vp(src_dev_ptr), Hs, Ws, channels, _vp(map_dev_ptr), _vp(dst_dev_ptr), _vp(valid_dev_ptr), H, W,
                                INTERP_NAMES.get(interp, interp), device, C.c_void_p(int(stream))))


UNRECTIFY_STEPS, UNRECTIFY_TOL = 20, 1e-3          # les_hip_unrectify_map's defaults: fixed-point steps, residual bound in raw pixels


def unrectify_map(raw, R, f, cx, cy, map_dev_ptr, Hs, Ws, steps=UNRECTIFY_STEPS, tol=UNRECTIFY_TOL, device=0, stream=0, lib=None):
    """les_hip_unrectify_map: the device Hs x Ws x 2 float map of the rectified positions (xs, ys) of the raw pixels of one view, the inverse of
    rectify_map's map and in its layout (remap takes it).  raw: a Camera (or what camera() takes as K); R: 3 x 3, the view's rectifying
    rotation, raw frame -> rectified frame (the transpose of rectify_map's M); f, cx, cy: the rectified view's intrinsics.  The distortion is
    inverted by `steps` (1 .. 64) additive fixed-point steps and a pixel is kept only where the forward model's residual is at most tol (> 0) raw
    pixels; fp64 in the fixed order of csrc/les_unrectify.h, (NaN, NaN) where a raw pixel has no rectified position.  Enqueue only."""
    L = load(lib)
    cam = camera(raw)
    r = (C.c_double * 9)(*np.asarray(R, np.float64).reshape(9))
    _chk_lib(L, L.les_hip_unrectify_map(C.byref(cam), r, float(f), float(cx), float(cy), int(steps), float(tol), _vp(map_dev_ptr), Hs, Ws, device,
                                        C.c_void_p(int(stream))))


def unrectify_labels(labels_dev_ptr, H, W, drop_dev_ptr, invmap_dev_ptr, Hs, Ws, M, f, cx, cy, doffs, baseline, valid_dev_ptr, points_dev_ptr=None,
                     normals_dev_ptr=None, disparity_dev_ptr=None, z_max=None, device=0, stream=0, lib=None):
    """les_hip_unrectify_labels: the device H x W x 4 label map of one view as geometry on that view's raw grid, through the view's inverse map
    (unrectify_map's, Hs x Ws x 2): per raw pixel the plane of the nearest rectified pixel evaluated at the pixel's own rectified position.
    M: 3 x 3, rectified frame -> raw camera frame (the transpose of the rectifying rotation); f, cx, cy, doffs, baseline: the rectified
    calibration, cx the view's own principal point.  points / normals (Hs x Ws x 3 floats, the raw camera's frame), disparity (Hs x Ws floats)
    may be None; valid: Hs x Ws bytes, 255 / 0; drop (H x W bytes, nonzero = dropped) may be None; z_max None or <= 0: no limit.  NaN where
    invalid (csrc/les_unrectify.h).  Enqueue only."""
    L = load(lib)
    m = (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9))
    _chk_lib(L, L.les_hip_unrectify_labels(_vp(labels_dev_ptr), H, W, _vp(drop_dev_ptr), _vp(invmap_dev_ptr), Hs, Ws, m, float(f), float(cx), float(cy),
                                           float(doffs), float(baseline), float(z_max) if z_max is not None else 0.0, _vp(points_dev_ptr), _vp(normals_dev_ptr),
                                           _vp(disparity_dev_ptr), _vp(valid_dev_ptr), device, C.c_void_p(int(stream))))


FISHEYE_STEPS = 10                                 # les_hip_unrectify_map_fisheye's default: Newton steps (quadratic convergence; five reach 2e-16 rad at 95 degrees)


def fisheye(K, k=(), theta_max=math.pi / 2):
    """A Fisheye (les_hip_fisheye) of a 3 x 3 camera matrix with zero skew, up to 4 coefficients (k1, k2, k3, k4) of the equidistant model of
    csrc/les_fisheye.h, shorter inputs padded with zeros, and the largest calibrated angle theta_max in (0, pi] (io.fisheye_theta_max finds the
    fold of a lens).  A Fisheye passes through."""
    if isinstance(K, Fisheye):
        return K
    K = np.asarray(K, np.float64)
    d = np.asarray(k if k is not None else (), np.float64).reshape(-1)
    if K.shape != (3, 3) or K[0, 1] != 0.0:
        raise ValueError("fisheye: K is a 3 x 3 camera matrix with zero skew")
    if d.size > 4:
        raise ValueError(f"fisheye: {d.size} coefficients, at most 4 (k1, k2, k3, k4)")
    return Fisheye(K[0, 0], K[1, 1], K[0, 2], K[1, 2], (C.c_double * 4)(*np.concatenate([d, np.zeros(4 - d.size)])), float(theta_max))


def rectify_map_fisheye(raw, M, f, cx, cy, map_dev_ptr, H, W, device=0, stream=0, lib=None):
    """les_hip_rectify_map_fisheye: rectify_map for a raw fisheye camera -- raw: a Fisheye (or what fisheye() takes as K); everything else and the
    map's layout as there.  fp64 in the fixed order of csrc/les_fisheye.h, its own atan included; (NaN, NaN) where a rectified pixel's ray lies
    behind the camera or beyond theta_max.  Enqueue only."""
    L = load(lib)
    cam = fisheye(raw)
    m = (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9))
    _chk_lib(L, L.les_hip_rectify_map_fisheye(C.byref(cam), m, float(f), float(cx), float(cy), _vp(map_dev_ptr), H, W, device, C.c_void_p(int(stream))))


def unrectify_map_fisheye(raw, R, f, cx, cy, map_dev_ptr, Hs, Ws, steps=FISHEYE_STEPS, tol=UNRECTIFY_TOL, device=0, stream=0, lib=None):
    """les_hip_unrectify_map_fisheye: unrectify_map for a raw fisheye camera -- raw: a Fisheye (or what fisheye() takes as K); everything else and
    the map's layout as there.  The radial polynomial is inverted by `steps` (1 .. 64) Newton steps and a pixel is kept only where the forward
    model's residual is at most tol (> 0) raw pixels; fp64 in the fixed order of csrc/les_fisheye.h, its own sin and cos included; (NaN, NaN)
    where a raw pixel lies beyond the lens's fold or theta_max, or has no rectified position.  Enqueue only."""
    L = load(lib)
    cam = fisheye(raw)
    r = (C.c_double * 9)(*np.asarray(R, np.float64).reshape(9))
    _chk_lib(L, L.les_hip_unrectify_map_fisheye(C.byref(cam), r, float(f), float(cx), float(cy), int(steps), float(tol), _vp(map_dev_ptr), Hs, Ws, device,
                                                C.c_void_p(int(stream))))


FIT_MAX_RADIUS = 15            # kFitMaxR of csrc/les_planefit.h (the one source; tests/planefit_cases.py: case_independence_and_errors holds this copy to it)
FIT_DEFAULTS = dict(radius=5, sig=10.0, gate0=1.0, gate_slope=0.5, max_slope=2.0, min_support=6)      # of every fit_planes above the C ABI
WARP_MAX_WIDTH = 8192          # kWarpMaxW of csrc/les_crossview.h (the one source; tests/crossview_cases.py: case_width_limit holds this copy to it)


def warp_labels(energy, src_mode, src_ptr, fallback_ptr, out_ptr, hit_ptr=None):
    """les_hip_warp_labels on the context of `energy` (a HipCostVolumeEnergy): see HipCostVolumeEnergy.warp_labels."""
    energy.warp_labels(src_mode, src_ptr, fallback_ptr, out_ptr, hit_ptr)


class DeviceBuffer:
    """A raw device allocation made through the C ABI (used when torch is not wanted)."""

    def __init__(self, energy, nbytes):
        self.e = energy
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        energy._chk(energy.L.les_hip_malloc(energy.h, C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.e._chk(self.e.L.les_hip_memcpy_h2d(self.e.h, C.c_void_p(self.ptr), _ptr(arr), arr.nbytes))

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.e._chk(self.e.L.les_hip_memcpy_d2h(self.e.h, _ptr(out), C.c_void_p(self.ptr), out.nbytes))
        return out

    def fill(self, byte):
        self.e._chk(self.e.L.les_hip_memset(self.e.h, C.c_void_p(self.ptr), byte, self.nbytes))

    def free(self):
        if self.ptr:
            self.e.L.les_hip_free(self.e.h, C.c_void_p(self.ptr))
            self.ptr = None


class Exchange:
    """Plan of the per-set tile exchange between ranks (include/localexp_hip.h: les_hip_exchange_*): `rects_per_rank[r]` = the target
    rects of rank r's cells.  pack / unpack move this rank's tiles into / the other ranks' tiles out of the all-gather buffer; tiles()
    does pack -> ncclAllGather -> unpack inside the library on an ncclComm_t (C++ hosts); the Python driver gathers with torch.distributed."""

    def __init__(self, energy, rank, rects_per_rank):
        self.e, self.rank, self.world = energy, rank, len(rects_per_rank)
        parts = [_rects(r) for r in rects_per_rank]
        first = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
        allr = np.concatenate(parts) if parts else np.zeros(0, RECT_DT)
        h = C.c_void_p()
        energy._chk(energy.L.les_hip_exchange_create(energy.h, rank, self.world, len(allr), _ptr(allr) if len(allr) else None, _ptr(first), C.byref(h)))
        self.h = h
        self.slot_floats = int(energy.L.les_hip_exchange_slot_floats(h))

    def pack(self, labels_ptr, cost_ptr, slot_ptr):
        self.e._chk(self.e.L.les_hip_exchange_pack(self.e.h, self.h, C.c_void_p(int(labels_ptr)), C.c_void_p(int(cost_ptr)), C.c_void_p(int(slot_ptr))))

    def unpack(self, gathered_ptr, labels_ptr, cost_ptr):
        self.e._chk(self.e.L.les_hip_exchange_unpack(self.e.h, self.h, C.c_void_p(int(gathered_ptr)), C.c_void_p(int(labels_ptr)), C.c_void_p(int(cost_ptr))))

    def tiles(self, nccl_comm, labels_ptr, cost_ptr):
        self.e._chk(self.e.L.les_hip_exchange_tiles(self.e.h, self.h, _vp(nccl_comm), C.c_void_p(int(labels_ptr)),
                                                    C.c_void_p(int(cost_ptr))))

    def destroy(self):
        if self.h:
            self.e.L.les_hip_exchange_destroy(self.h)
            self.h = None


class Batch:
    def __init__(self, energy, filter_rects, target_rects, out_slabs=False):
        """out_slabs: False / 0 = every call writes the one H x W map; True / 1 = call i writes slab i of [n][H][W]; k > 1 = call i writes slab
        i // k (k consecutive calls -- the cells of a disjoint set -- share a map: several proposal slots of the set in one launch)."""
        self.e = energy
        self.frs = _rects(filter_rects)
        self.trs = _rects(target_rects)
        self.n = len(self.frs)
        self.out_slabs = int(out_slabs)
        h = C.c_void_p()
        energy._chk(energy.L.les_hip_batch_create(energy.h, self.n, _ptr(self.frs), _ptr(self.trs), int(out_slabs), C.byref(h)))
        self.h = h

    @property
    def num_jobs(self):
        return self.e.L.les_hip_batch_num_jobs(self.h)

    def kernel_kind(self, mode=0):
        """1: the fixed-point march kernel serves this batch, 0: the fp64 strip kernel, 2: the bilateral / unfiltered kernel."""
        return self.e.L.les_hip_batch_kernel_kind(self.e.h, self.h, mode)

    def run(self, planes, out_dev_ptr, mode=0, check=True, planes_on_device=False):
        """planes: host array (n,4) or a device pointer (int) when planes_on_device; out_dev_ptr: int."""
        if planes_on_device:
            pp = C.c_void_p(int(planes))
        else:
            self._planes = _planes(planes)
            assert len(self._planes) == self.n
            pp = _ptr(self._planes)
        self.e._chk(self.e.L.les_hip_batch_run(self.e.h, self.h, mode, pp, int(planes_on_device), C.c_void_p(int(out_dev_ptr)), int(check)))

    def set_units(self, unit_rects):
        self.units = _rects(unit_rects)
        assert len(self.units) == self.n
        self.e._chk(self.e.L.les_hip_batch_set_units(self.e.h, self.h, _ptr(self.units)))

    def propose(self, kind, labels_dev, rng_dev, planes_dev, m=0):
        """kind: PROPOSE_EXPANSION / _RANDOM / _RANSAC / _INIT; all pointers are device addresses (int)."""
        self.e._chk(self.e.L.les_hip_batch_propose(self.e.h, self.h, kind, m, C.c_void_p(int(labels_dev)), C.c_void_p(int(rng_dev)),
                                                   C.c_void_p(int(planes_dev))))

    def wta(self, planes_dev, cur_cost_dev, prop_cost_dev, labels_dev):
        self.e._chk(self.e.L.les_hip_batch_wta(self.e.h, self.h, C.c_void_p(int(planes_dev)), C.c_void_p(int(cur_cost_dev)),
                                               C.c_void_p(int(prop_cost_dev)), C.c_void_p(int(labels_dev))))

    # -- pairwise terms / graph capacities of the expansion moves on the device ("next" row N1)
    def graph_nodes(self):
        return int(self.e.L.les_hip_batch_graph_nodes(self.h))

    def graph_offsets(self):
        off = np.zeros(self.n, np.int64)
        self.e._chk(self.e.L.les_hip_batch_graph_offsets(self.h, _ptr(off)))
        return off

    def expansion_graph(self, planes_dev, labels_dev, cur_dev, prop_dev, payload_dev, mode=0, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01,
                        want_flow0=False):
        """Graph capacities of one lock-step (LES/FastGCStereo.h:425-551 + LES/StereoEnergy.h:398-453) into payload_dev
        (5 floats per node).  Returns the per-cell t-link flow when want_flow0."""
        f0 = np.zeros(self.n, np.float64) if want_flow0 else None
        self.e._chk(self.e.L.les_hip_batch_expansion_graph(self.e.h, self.h, mode, C.c_void_p(int(planes_dev)), C.c_void_p(int(labels_dev)),
                                                           C.c_void_p(int(cur_dev)), C.c_void_p(int(prop_dev)), lambda_, th_smooth, omega, epsilon,
                                                           C.c_void_p(int(payload_dev)), _ptr(f0)))
        return f0

    def fusion_graph(self, labels1_dev, labels_dev, cur_dev, prop_dev, payload_dev, mode=0, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01,
                     want_flow0=False, nonsubmodular_dev=None):
        """Graph capacities of one lock-step of FUSION moves (LES/FastGCStereo.h:241-363; definition: csrc/les_pairwise.h): the current map labels_dev
        against the second map labels1_dev, whose per-pixel unary costs are cur_dev / prop_dev.  Payload as expansion_graph; a mask byte of 255 means
        the pixel takes labels1's label.  nonsubmodular_dev: n int32 on the device that receive every cell's count of truncated (non-submodular)
        pairs, or None.  Returns the per-cell t-link flow when want_flow0."""
        f0 = np.zeros(self.n, np.float64) if want_flow0 else None
        self.e._chk(self.e.L.les_hip_batch_fusion_graph(self.e.h, self.h, mode, C.c_void_p(int(labels1_dev)), C.c_void_p(int(labels_dev)),
                                                        C.c_void_p(int(cur_dev)), C.c_void_p(int(prop_dev)), lambda_, th_smooth, omega, epsilon,
                                                        C.c_void_p(int(payload_dev)), _ptr(f0), _vp(nonsubmodular_dev)))
        return f0

    MAXFLOW_MAX_NODES = 2304          # LES_HIP_MAXFLOW_MAX_NODES

    @property
    def max_cell_nodes(self):
        return int(self.e.L.les_hip_batch_max_cell_nodes(self.h))

    @property
    def graph_solver_kind(self):
        """The most general one-workgroup kernel solve_graphs launches (the kernel is chosen per cell): 0 = only les_maxflow_cell.h, 1 / 2 = les_maxflow.h
        (1024 / 512 threads) for some cell, -1 = a cell above the limit."""
        return int(self.e.L.les_hip_batch_graph_solver_kind(self.h))

    def solve_graphs(self, payload_dev, masks_dev, status_dev, flows_dev=None, unsolved_total_dev=None):
        """Max-flow + segment read-out of every cell's expansion graph on the device (LES/FastGCStereo.h:553-559); cells of at most
        MAXFLOW_MAX_NODES nodes.  masks (uint8 per node), status (int32 per cell: 0 solved, 1 = cut it on the host), flows (float64 per
        cell, optional) are device pointers; unsolved_total (optional): a device int that grows by one per cell that hit the iteration limit."""
        self.e._chk(self.e.L.les_hip_batch_solve_graphs_counted(self.e.h, self.h, C.c_void_p(int(payload_dev)), C.c_void_p(int(masks_dev)), C.c_void_p(int(status_dev)),
                                                                _vp(flows_dev), _vp(unsolved_total_dev)))

    def tiled_workspace_bytes(self):
        """Device scratch les_hip_batch_solve_graphs_tiled needs for this batch (109 bytes per graph node)."""
        return int(self.e.L.les_hip_batch_tiled_workspace_bytes(self.h))

    def solve_graphs_tiled(self, payload_dev, masks_dev, status_dev, workspace_dev, workspace_bytes, flows_dev=None):
        """The same for cells of any size (the coarse layers): region-parallel push-relabel over tiles of the cells, graphs resident in
        device memory (csrc/les_maxflow_tiled.h).  workspace: 256-byte aligned device scratch of tiled_workspace_bytes().  Synchronises
        the calling thread's stream.  -> launches enqueued; self.tiled_unsolved = cells that hit the launch limit (0: every cell was cut);
        self.tiled_stats = the call's les_hip_tiled_stats (cells / nodes the host cores finished from their residual graphs, their milliseconds)."""
        st = TiledStats()
        self.e._chk(self.e.L.les_hip_batch_solve_graphs_tiled_stats(self.e.h, self.h, C.c_void_p(int(payload_dev)), C.c_void_p(int(masks_dev)), C.c_void_p(int(status_dev)),
                                                                    _vp(flows_dev), C.c_void_p(int(workspace_dev)),
                                                                    C.c_longlong(int(workspace_bytes)), C.byref(st)))
        self.tiled_unsolved = st.unsolved
        self.tiled_stats = dict(launches=st.launches, unsolved=st.unsolved, handed_cells=st.handed_cells, handed_nodes=st.handed_nodes, host_ms=st.host_ms)
        return st.launches

    def apply_masks(self, planes_dev, masks_dev, cur_dev, prop_dev, labels_dev):
        """Mask updates of a lock-step on the device (LES/FastGCStereo.h:61-62); masks in graph-node order."""
        self.e._chk(self.e.L.les_hip_batch_apply_masks(self.e.h, self.h, C.c_void_p(int(planes_dev)), C.c_void_p(int(masks_dev)), C.c_void_p(int(cur_dev)),
                                                       C.c_void_p(int(prop_dev)), C.c_void_p(int(labels_dev))))

    def apply_masks_labels(self, labels1_dev, masks_dev, cur_dev, prop_dev, labels_dev):
        """Mask updates of a lock-step of fusion moves: where the mask is non-zero the pixel takes labels1's label and prop's cost."""
        self.e._chk(self.e.L.les_hip_batch_apply_masks_labels(self.e.h, self.h, C.c_void_p(int(labels1_dev)), C.c_void_p(int(masks_dev)), C.c_void_p(int(cur_dev)),
                                                              C.c_void_p(int(prop_dev)), C.c_void_p(int(labels_dev))))

    def region_energy(self, labels_dev, cost_dev, energy_dev, mode=0, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01):
        """Per cell, the energy of the current maps that a move on the cell can change (fusedEnergy of host/ExpansionMove.h, LES/FastGCStereo.h:561-594):
        the costs of its region + the forward pair terms with an endpoint in it.  energy_dev: n float64 on the device.  Enqueue only."""
        self.e._chk(self.e.L.les_hip_batch_region_energy(self.e.h, self.h, mode, C.c_void_p(int(labels_dev)), C.c_void_p(int(cost_dev)), lambda_, th_smooth,
                                                         omega, epsilon, C.c_void_p(int(energy_dev))))

    def destroy(self):
        if self.h:
            self.e.L.les_hip_batch_destroy(self.h)
            self.h = None


class DeviceEvaluator:
    """Evaluator::evaluate's numbers (LES/Evaluator.h:113-187) computed on the device from a view's device maps (include/localexp_hip.h:
    les_hip_evaluator_*).  evaluate() only enqueues; rows() synchronises and reads the log.  One host thread at a time; one object per view."""

    def __init__(self, energy, dispGT=None, nonocc=None, error_threshold=0.5, precision=-1.0, max_rows=4096):
        self.e = energy
        gt = np.ascontiguousarray(dispGT, np.float32) if dispGT is not None else None
        no = np.ascontiguousarray(np.asarray(nonocc, bool), np.uint8) if nonocc is not None else None
        assert gt is None or gt.shape == (energy.H, energy.W)
        assert no is None or no.shape == (energy.H, energy.W)
        self.max_rows = int(max_rows)
        self.has_gt = gt is not None
        h = C.c_void_p()
        self.h = None
        energy._chk(energy.L.les_hip_evaluator_create(energy.h, _ptr(gt), _ptr(no), C.c_float(error_threshold), C.c_float(precision), self.max_rows, C.byref(h)))
        self.h = h

    def evaluate(self, labels_ptr, cost_ptr, mode=0, index=0, lambda_=1.0, th_smooth=1.0, omega=10.0, epsilon=0.01):
        self.e._chk(self.e.L.les_hip_evaluate(self.e.h, self.h, mode, C.c_void_p(int(labels_ptr)), C.c_void_p(int(cost_ptr)), lambda_, th_smooth, omega, epsilon,
                                              int(index)))

    def rows(self):
        """The rows enqueued so far, as dicts: index, mode, data, smooth, energy, the four counts, and all / nonocc computed from the counts as
        io.Evaluator.evaluate does (present whenever the evaluator holds ground truth; NaN when no pixel is valid / non-occluded)."""
        buf = (EvalRow * self.max_rows)()
        n = C.c_int(0)
        self.e._chk(self.e.L.les_hip_evaluator_rows(self.e.h, self.h, buf, self.max_rows, C.byref(n)))
        out = []
        for r in buf[: n.value]:
            row = dict(index=r.index, mode=r.mode, data=r.data, smooth=r.smooth, energy=r.data + r.smooth, good_valid=r.good_valid, good_nonocc=r.good_nonocc,
                       n_valid=r.n_valid, n_nonocc=r.n_nonocc)
            if self.has_gt:          # (NaN where nothing counts, as io.Evaluator)
                row["all"] = float(100.0 * (1.0 - np.int64(r.good_valid) / r.n_valid)) if r.n_valid else float("nan")
                row["nonocc"] = float(100.0 * (1.0 - np.int64(r.good_nonocc) / r.n_nonocc)) if r.n_nonocc else float("nan")
            out.append(row)
        return out

    def close(self):
        if self.h:
            self.e.L.les_hip_evaluator_destroy(self.h)
            self.h = None


class HipCostVolumeEnergy:
    """Python mirror of CostVolumeEnergy (LES/CostVolumeEnergy.h:6-184) over the C ABI.  filter: Parameters::filterName -- "GF" (the guided
    filter, radius windR // 2, eps), "BF" / "BL" (the joint bilateral filter, radius windR, sig2 = eps) or "" (no aggregation).
    interpolate: setInterpolationMethod -- 0 nearest slice, 1 linear (the default), 2 three-point quadratic."""

    def __init__(self, imL, imR, volL, volR, windR=20, eps=1e-4, th_col=0.5, max_disp=None, min_disp=0.0,
                 device=0, volumes_on_device=False, shape=None, lib=None, filter="GF", interpolate=1):
        self.filter = filter_kind(filter)
        self.L = load(lib)
        self.imL = np.ascontiguousarray(imL, np.uint8) if imL is not None else None
        self.imR = np.ascontiguousarray(imR, np.uint8) if imR is not None else None
        im = self.imL if self.imL is not None else self.imR
        self.H, self.W = im.shape[:2]
        if volumes_on_device:
            self.D = int(shape[0])
            vl, vr = _vp(volL), _vp(volR)
            self._keep = None
        else:
            self._keep = [np.ascontiguousarray(v, np.float32) if v is not None else None for v in (volL, volR)]
            v = self._keep[0] if self._keep[0] is not None else self._keep[1]
            self.D = v.shape[0]
            vl, vr = _ptr(self._keep[0]), _ptr(self._keep[1])
        self.max_disp = float(self.D - 1 if max_disp is None else max_disp)
        self.params = Params(self.H, self.W, self.D, windR, eps, th_col, self.max_disp, float(min_disp), device,
                             int(bool(volumes_on_device)))
        h = C.c_void_p()
        self.h = None
        if self.filter == FILTER_GF:
            self._chk(self.L.les_hip_create(C.byref(h), C.byref(self.params), _ptr(self.imL), _ptr(self.imR), vl, vr))
        else:
            self._chk(self.L.les_hip_create_filtered(C.byref(h), C.byref(self.params), self.filter, _ptr(self.imL), _ptr(self.imR), vl, vr))
        self.h = h
        self._keep = None     # host volumes were copied to HBM
        self.interpolate = 1
        if interpolate != 1:
            self.setInterpolationMethod(interpolate)

    @classmethod
    def naive(cls, imL, imR, windR=20, eps=1e-4, alpha=0.9, th_col=10.0, th_grad=2.0, max_disp=63.0, min_disp=0.0, device=0, lib=None,
              filter="GF", max_vdisp=0.0):
        """Python mirror of NaiveStereoEnergy (LES/StereoEnergy.h:629-764; MiddV2 parameters LES/main.cpp:86-121):
        image-based matching cost, no volume.  Every method of the volume-based operator works on it.  filter: as for the constructor.
        max_vdisp: MAX_VDISPARITY (PMStereoBase.h:37): the range [-max_vdisp, max_vdisp] of the vertical disparity Plane::v that
        PROPOSE_INIT draws (createRandomLabel); the cost honours every plane's v whatever this value."""
        self = cls.__new__(cls)
        self.h = None
        self.filter = filter_kind(filter)
        self.L = load(lib)
        self.imL = np.ascontiguousarray(imL, np.uint8)
        self.imR = np.ascontiguousarray(imR, np.uint8)
        self.H, self.W = self.imL.shape[:2]
        self.D = 1
        self.max_disp = float(max_disp)
        self.params = Params(self.H, self.W, 1, windR, eps, th_col, self.max_disp, float(min_disp), device, 0)
        self._keep = None
        h = C.c_void_p()
        self.h = None
        if self.filter == FILTER_GF:
            self._chk(self.L.les_hip_create_naive(C.byref(h), C.byref(self.params), _ptr(self.imL), _ptr(self.imR), C.c_float(alpha), C.c_float(th_grad)))
        else:
            self._chk(self.L.les_hip_create_naive_filtered(C.byref(h), C.byref(self.params), self.filter, _ptr(self.imL), _ptr(self.imR),
                                                           C.c_float(alpha), C.c_float(th_grad)))
        self.h = h
        self.naive_cost = (float(alpha), float(th_grad))       # what raw_cost_max needs of the image-based cost
        self.interpolate = 1      # (no volume: les_hip_set_interpolation refuses this context)
        self.max_vdisp = self.random_vdisp = 0.0
        if max_vdisp:
            self.set_max_vdisparity(max_vdisp)
        return self

    def _chk(self, rc):
        if rc != 0:
            raise LesHipError(f"liblocalexp_hip error {rc}: {self.L.les_hip_last_error().decode()}")

    def close(self):
        if self.h:
            self.L.les_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self._chk(self.L.les_hip_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    def set_thread_stream(self, stream_ptr, bind=True):
        """The calling host thread's launches on this context go to `stream_ptr` (bind=False: back to the context's stream)."""
        self._chk(self.L.les_hip_set_thread_stream(self.h, _vp(stream_ptr), int(bool(bind))))

    def synchronize(self):
        self._chk(self.L.les_hip_synchronize(self.h))

    def strip_width(self):
        return self.L.les_hip_strip_width(self.params.windR // 2)

    def setInterpolationMethod(self, none_lin_quad):
        """CostVolumeEnergy::setInterpolationMethod (LES/CostVolumeEnergy.h:45-48): 0 nearest, 1 linear, 2 quadratic, for every later
        evaluation (prepared batches included).  Not for the image-based energy, and not while another thread evaluates on this context."""
        self._chk(self.L.les_hip_set_interpolation(self.h, int(none_lin_quad)))
        self.interpolate = int(none_lin_quad)

    def set_max_vdisparity(self, max_vdisp):
        """The energy's MAX_VDISPARITY: PROPOSE_INIT draws v in [-max_vdisp, max_vdisp] (0: no draw).  Only the image-based cost reads v."""
        self._chk(self.L.les_hip_set_max_vdisparity(self.h, C.c_float(max_vdisp)))
        self.max_vdisp = float(max_vdisp)

    def set_random_vdisparity(self, max_vdisp):
        """RandomProposer's maxVDisp (LES/Proposer.h:100-148): PROPOSE_RANDOM perturbs v within max_vdisp * 0.5^(m+1), clamped to
        [-max_vdisp, max_vdisp]; 0 (the default) keeps the source label's v."""
        self._chk(self.L.les_hip_set_random_vdisparity(self.h, C.c_float(max_vdisp)))
        self.random_vdisp = float(max_vdisp)

    def refresh_volume(self, mode=0):
        """After the caller refilled the device-resident volume of `mode` in place: cost range / fixed-point scales / tiled copy re-derived."""
        self._chk(self.L.les_hip_refresh_volume(self.h, mode))

    def tiled_volume_bytes(self, mode=0):
        """Bytes of the tiled copy of the view's volume the gather of steep planes reads (0: none, see include/localexp_hip.h)."""
        return int(self.L.les_hip_tiled_volume_bytes(self.h, mode))

    def stats(self, mode=0):
        out = np.empty((self.H, self.W, 3, 4), np.float32)
        self._chk(self.L.les_hip_get_stats(self.h, mode, _ptr(out)))
        return out

    # -- the operator (names follow the reference) ------------------------------------------------
    def ComputeUnaryPotential(self, filterRect, targetRect, costs_map, plane, mode=0, check=True):
        """costs_map is the caller's H x W float32 map; like the reference call site
        (LES/FastGCStereo.h:49) the view costs_map(filterRect) is handed to the operator."""
        assert costs_map.dtype == np.float32 and costs_map.flags.c_contiguous and costs_map.shape == (self.H, self.W)
        fr, tr = _rects([filterRect]), _rects([targetRect])
        pl = _planes([plane])
        origin = costs_map.ctypes.data + 4 * (int(fr["y"][0]) * self.W + int(fr["x"][0]))
        self._chk(self.L.les_hip_unary_one(self.h, mode, _ptr(fr), _ptr(tr), _ptr(pl), C.c_void_p(origin), self.W, int(check)))
        return costs_map

    def scratch(self):
        """A caller-owned scratch handle (struct Reusable of the reference): calls through distinct handles may run concurrently."""
        h = C.c_void_p()
        self._chk(self.L.les_hip_scratch_create(self.h, C.byref(h)))
        return h

    def scratch_free(self, h):
        self.L.les_hip_scratch_destroy(h)

    def ComputeUnaryPotentialScratch(self, scratch, filterRect, targetRect, costs_map, plane, mode=0, check=True):
        """les_hip_unary_one_scratch: the re-entrant operator (ctypes releases the GIL during the call)."""
        fr, tr = _rects([filterRect]), _rects([targetRect])
        pl = _planes([plane])
        origin = costs_map.ctypes.data + 4 * (int(fr["y"][0]) * self.W + int(fr["x"][0]))
        self._chk(self.L.les_hip_unary_one_scratch(self.h, scratch, mode, _ptr(fr), _ptr(tr), _ptr(pl), C.c_void_p(origin), self.W, int(check)))
        return costs_map

    def ComputeUnaryPotentialWithoutCheck(self, filterRect, targetRect, costs_map, plane, mode=0):
        return self.ComputeUnaryPotential(filterRect, targetRect, costs_map, plane, mode, check=False)

    def unary_batch(self, filter_rects, target_rects, planes, costs_map=None, mode=0, check=True):
        if costs_map is None:
            costs_map = np.full((self.H, self.W), np.nan, np.float32)
        frs, trs, pls = _rects(filter_rects), _rects(target_rects), _planes(planes)
        assert len(frs) == len(trs) == len(pls)
        self._chk(self.L.les_hip_unary_batch(self.h, mode, len(frs), _ptr(frs), _ptr(trs), _ptr(pls), _ptr(costs_map), int(check)))
        return costs_map

    def unary_labels(self, labels_ptr, cost_ptr, mode=0, region=None, check=True):
        """les_hip_unary_labels: the unary cost of every pixel's own label (the warm-start branch of initCurrentFast, LES/FastGCStereo.h:116-130)
        in one dense device pass.  labels_ptr / cost_ptr: device addresses of the H x W plane map and the H x W float map; region: (x, y, w, h),
        None = the whole image; pixels outside it are not written.  Enqueue only (the calling thread's stream)."""
        rg = _rects([region]) if region is not None else None
        self._chk(self.L.les_hip_unary_labels(self.h, mode, _ptr(rg), C.c_void_p(int(labels_ptr)), C.c_void_p(int(cost_ptr)), int(check)))

    def unary_labels_kind(self, mode=0):
        """1: the dense kernel (csrc/les_dense.h) serves unary_labels on this context and view, 0: one job per pixel, -1: bad argument."""
        return int(self.L.les_hip_unary_labels_kind(self.h, mode))

    # -- dual-view post-processing (LES/PMStereoBase.h:111-256) on device label maps -----------------
    def consistency_check(self, labelsL_dev, labelsR_dev, failL_dev, failR_dev, threshold=1.5):
        self._chk(self.L.les_hip_consistency_check(self.h, C.c_void_p(int(labelsL_dev)), C.c_void_p(int(labelsR_dev)), C.c_float(threshold),
                                                   C.c_void_p(int(failL_dev)), C.c_void_p(int(failR_dev))))

    def post_process(self, labelsL_dev, labelsR_dev, threshold=1.5, omega=10.0, speckle=None, fail=None):
        """PMStereoBase::postProcess in place on two device label maps (FastGCStereo::run calls it with 1.5).
        speckle=(max_size, max_diff): les_hip_post_process_speckle -- the failure mask of each view widened by the speckle mask of its map
        (speckle_mask); one of the two maps may then be None: the one-view form, whose mask is the speckle mask alone.
        fail=(maskL, maskR): les_hip_post_process_masked -- the caller's own failure masks, device addresses of H x W bytes (nonzero = failed),
        either may be None, OR-ed into each view's mask; the one-view form is allowed as with speckle (without speckle: max_size 0, no speckle mask)."""
        if speckle is None and fail is None:
            self._chk(self.L.les_hip_post_process(self.h, C.c_void_p(int(labelsL_dev)), C.c_void_p(int(labelsR_dev)), C.c_float(threshold), C.c_float(omega)))
            return
        max_size, max_diff = speckle if speckle is not None else (0, 0.0)
        if fail is None:
            self._chk(self.L.les_hip_post_process_speckle(self.h, _vp(labelsL_dev), _vp(labelsR_dev), C.c_float(threshold), C.c_float(omega), int(max_size),
                                                          C.c_float(max_diff)))
            return
        self._chk(self.L.les_hip_post_process_masked(self.h, _vp(labelsL_dev), _vp(labelsR_dev), C.c_float(threshold), C.c_float(omega), int(max_size),
                                                     C.c_float(max_diff), _vp(fail[0]), _vp(fail[1])))

    def post_process_host(self, labelsL, labelsR, threshold=1.5, omega=10.0, speckle=None, fail=None):
        """Convenience form for host label maps (H x W planes): upload, post-process on the device, download.  With speckle=(max_size, max_diff)
        or fail=(maskL, maskR) -- host H x W masks, nonzero / True = failed, either may be None -- either map may be None (post_process); its place
        in the returned pair is None then."""
        maps = (labelsL, labelsR)
        masks = tuple(fail) if fail is not None else (None, None)
        bufs = [DeviceBuffer(self, self.H * self.W * 16) if l is not None else None for l in maps]
        mbufs = [DeviceBuffer(self, self.H * self.W) if m is not None else None for m in masks]
        try:
            for b, l in zip(bufs, maps):
                if b is not None:
                    b.upload(np.ascontiguousarray(l).view(np.float32).reshape(self.H, self.W, 4))
            for b, m in zip(mbufs, masks):
                if b is not None:
                    b.upload((np.asarray(m).reshape(self.H, self.W) != 0).astype(np.uint8))
            self.post_process(*(b.ptr if b is not None else None for b in bufs), threshold, omega, speckle=speckle,
                              fail=None if fail is None else tuple(b.ptr if b is not None else None for b in mbufs))
            out = [b.download((self.H, self.W, 4), np.float32) if b is not None else None for b in bufs]
        finally:
            for b in bufs + mbufs:
                if b is not None:
                    b.free()
        return out

    # -- the tensor wrappers' ingestion of their maps, and their one rule for streams ------------------------------------
    def _device(self, device):
        """The torch device of a wrapper's results: `device`, or this context's GPU (the simulator build takes "cpu")."""
        import torch
        return torch.device(device if device is not None else f"cuda:{self.params.device}")

    def _labels_and_cost(self, device):
        """New (labels, cost) result tensors of wta_labels / sgm_labels: H x W x 4 and H x W float32."""
        import torch
        dev = self._device(device)
        return torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev), torch.empty((self.H, self.W), dtype=torch.float32, device=dev)

    def _label_map(self, labels, dev, who, shape=None, what="label map"):
        """The H x W x 4 float32 label map on dev (shape: another (H, W)): a tensor that is there already is used where it is."""
        h, w = shape or (self.H, self.W)
        s = _float_tensor(labels, dev)
        if tuple(s.shape) != (h, w, 4):
            raise ValueError(f"{who} a {h} x {w} x 4 {what}, not {tuple(s.shape)}")
        return s

    def _label_or_disparity_map(self, src, dev, who, shape=None):
        """fit_planes' source on dev: an H x W x 4 label map or an H x W disparity map, float32."""
        h, w = shape or (self.H, self.W)
        s = _float_tensor(src, dev)
        if tuple(s.shape) not in ((h, w, 4), (h, w)):
            raise ValueError(f"{who} a {h} x {w} x 4 label map or a {h} x {w} disparity map, not {tuple(s.shape)}")
        return s

    def _byte_map(self, mask, dev, who, shape=None):
        """The H x W uint8 mask on dev (nonzero = set): a uint8 tensor that is there already is used where it is."""
        import torch
        h, w = shape or (self.H, self.W)
        if torch.is_tensor(mask):
            m = (mask if mask.dtype == torch.uint8 else mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
        else:
            m = torch.from_numpy((np.asarray(mask) != 0).astype(np.uint8)).to(dev)
        if tuple(m.shape) != (h, w):
            raise ValueError(f"{who} a {h} x {w} mask, not {tuple(m.shape)}")
        return m

    def _staged(self, dev, copied, call, *args, **kwargs):
        """call(*args, **kwargs) on maps a wrapper ingested.  copied: ingestion made a copy (a dtype or device conversion, an upload of an
        array) -- torch made it on ITS current stream and the library reads it on the context's, so torch's stream is waited for before the
        call, and the context after it: the copy goes back to torch's allocator when the wrapper returns and must outlive the launch that
        reads it.  A caller's tensor used where it is (the drivers' case) adds no wait."""
        if copied and dev.type == "cuda":
            import torch
            torch.cuda.current_stream(dev).synchronize()
        call(*args, **kwargs)
        if copied:
            self.synchronize()

    # -- speckle filter (csrc/les_speckle.h; no reference counterpart) ------------------------------------
    def speckle_mask_ptr(self, labels_ptr, max_size, max_diff, mask_ptr, root_ptr=None, size_ptr=None):
        """les_hip_speckle_mask on device addresses (root_ptr and size_ptr may be None).  Synchronises the calling thread's stream."""
        self._chk(self.L.les_hip_speckle_mask(self.h, _vp(labels_ptr), int(max_size), C.c_float(max_diff), _vp(mask_ptr), _vp(root_ptr), _vp(size_ptr)))

    def speckle_mask(self, labels, max_size, max_diff, components=False, device=None):
        """The speckle mask of an H x W x 4 label map (les_hip_speckle_mask): H x W uint8, 255 where the pixel's connected component of the
        disparity map -- 4-neighbours whose finite disparities differ by at most max_diff -- has at most max_size pixels, else 0.  components:
        (mask, root, size), root and size H x W int32 -- per pixel the smallest linear index of its component and the component's pixel
        count.  labels: a float32 torch tensor (on `device`: used where it is) or an array.  All results are new tensors on `device` (None:
        this context's GPU; the simulator build takes "cpu")."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "speckle_mask:")
        mask = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        root = torch.empty((self.H, self.W), dtype=torch.int32, device=dev) if components else None
        size = torch.empty((self.H, self.W), dtype=torch.int32, device=dev) if components else None
        self._staged(dev, s is not labels, self.speckle_mask_ptr, s.data_ptr(), max_size, max_diff, mask.data_ptr(),
                     root.data_ptr() if components else None, size.data_ptr() if components else None)
        return (mask, root, size) if components else mask

    # -- cross-view fusion (csrc/les_crossview.h; no reference counterpart) -----------------------------
    def warp_labels(self, src_mode, src_ptr, fallback_ptr, out_ptr, hit_ptr=None):
        """les_hip_warp_labels: the device label map src_ptr of view src_mode (0 left, 1 right) expressed in the other view's coordinates into
        out_ptr (H x W planes; may be fallback_ptr, not src_ptr): a target pixel some source pixel lands on gets that pixel's plane rewritten for
        the target view (the largest disparity wins), every other one fallback_ptr's plane.  hit_ptr: H x W bytes (1 = warped, 0 = fallback) or
        None.  Enqueue only (the calling thread's stream).  Rows wider than WARP_MAX_WIDTH raise (error 3)."""
        self._chk(self.L.les_hip_warp_labels(self.h, int(src_mode), C.c_void_p(int(src_ptr)), C.c_void_p(int(fallback_ptr)), C.c_void_p(int(out_ptr)),
                                             _vp(hit_ptr)))

    # -- winner-take-all labels of the aggregated cost volume (csrc/les_wtavol.h; no reference counterpart) ---------------
    @property
    def num_fronto_planes(self):
        """K of wta_labels: int(max_disparity - min_disparity) + 1."""
        return int(np.float32(self.params.max_disparity) - np.float32(self.params.min_disparity)) + 1

    def slab_argmin_state_bytes(self):
        """Bytes of the per-pixel state of slab_argmin for this context's image (16-byte aligned device memory, opaque)."""
        return int(self.L.les_hip_slab_argmin_state_bytes(self.H, self.W))

    def slab_argmin(self, slabs_ptr, n, k_first, state_ptr):
        """les_hip_slab_argmin: the running arg-min over one chunk of n slabs ([n][H][W] floats on the device, slab i = slab k_first + i of the
        volume) into the state; k_first == 0 initialises it.  Enqueue only."""
        self._chk(self.L.les_hip_slab_argmin(self.h, _vp(slabs_ptr), int(n), int(k_first), _vp(state_ptr)))

    def slab_argmin_finish(self, state_ptr, K, labels_ptr, cost_ptr, subpixel=True):
        """les_hip_slab_argmin_finish: the state after K slabs -> the H x W plane map (0, 0, k* + off + min_disp, 0) and the H x W cost map."""
        self._chk(self.L.les_hip_slab_argmin_finish(self.h, _vp(state_ptr), int(K), int(bool(subpixel)), _vp(labels_ptr), _vp(cost_ptr)))

    def wta_labels(self, mode=0, chunk=0, subpixel=True, labels_ptr=None, cost_ptr=None, device=None):
        """les_hip_wta_labels: the winner-take-all label map of view `mode` -- per pixel the fronto-parallel plane of least aggregated cost among
        the num_fronto_planes planes at min_disp + k, refined to sub-pixel by the parabola through its neighbours' costs -- and its costs; the
        planes run through the batch path `chunk` at a time (0: the library's default) and each chunk is reduced as it lands.  Asynchronous on
        the calling thread's stream once the context's workspace exists.  With labels_ptr and cost_ptr (device addresses of the H x W x 4 and
        H x W float maps) it writes there and returns None; with neither it returns (labels, cost) as new torch tensors on `device` (None:
        this context's GPU; the simulator build takes "cpu")."""
        if (labels_ptr is None) != (cost_ptr is None):
            raise ValueError("wta_labels: give both labels_ptr and cost_ptr, or neither")
        out = None
        if labels_ptr is None:
            out = self._labels_and_cost(device)
            labels_ptr, cost_ptr = out[0].data_ptr(), out[1].data_ptr()
        self._chk(self.L.les_hip_wta_labels(self.h, int(mode), int(chunk), int(bool(subpixel)), _vp(labels_ptr), _vp(cost_ptr)))
        return out

    # -- the confidence of a label map under the aggregated cost volume (csrc/les_confidence.h; no reference counterpart) ---------------
    def raw_cost_max(self):
        """The largest value a raw matching cost of this context can take (float32): th_col for the volume energy (the costs are truncated
        there), (1 - alpha) th_col + alpha th_grad for the image-based one (its two truncated terms).  The default `scale` of confidence."""
        th = np.float32(self.params.th_col)
        if not hasattr(self, "naive_cost"):
            return th
        alpha, th_grad = (np.float32(v) for v in self.naive_cost)
        return np.float32((np.float32(1) - alpha) * th + alpha * th_grad)

    def slab_confidence_state_bytes(self):
        """Bytes of the per-pixel state of slab_confidence for this context's image (16-byte aligned device memory, opaque)."""
        return int(self.L.les_hip_slab_confidence_state_bytes(self.H, self.W))

    def slab_confidence(self, labels_ptr, slabs_ptr, n, k_first, band, state_ptr):
        """les_hip_slab_confidence: the running own / rival minima over one chunk of n slabs ([n][H][W] floats on the device, slab i = slab
        k_first + i of the volume) into the state; k_first == 0 initialises it from the H x W x 4 label map at labels_ptr (read only then).
        Enqueue only."""
        self._chk(self.L.les_hip_slab_confidence(self.h, _vp(labels_ptr), _vp(slabs_ptr), int(n), int(k_first), C.c_float(band), _vp(state_ptr)))

    def slab_confidence_finish(self, state_ptr, scale, conf_ptr, own_ptr=None, rival_ptr=None, krival_ptr=None):
        """les_hip_slab_confidence_finish: the state -> the H x W confidence map and, where given, the own and rival costs (float) and the
        rival's slab (int32).  Enqueue only."""
        self._chk(self.L.les_hip_slab_confidence_finish(self.h, _vp(state_ptr), C.c_float(scale), _vp(conf_ptr), _vp(own_ptr), _vp(rival_ptr), _vp(krival_ptr)))

    def confidence_ptr(self, mode, labels_ptr, chunk, band, scale, conf_ptr, own_ptr=None, rival_ptr=None, krival_ptr=None):
        """les_hip_confidence on device addresses (own_ptr, rival_ptr and krival_ptr may be None)."""
        self._chk(self.L.les_hip_confidence(self.h, int(mode), _vp(labels_ptr), int(chunk), C.c_float(band), C.c_float(scale), _vp(conf_ptr), _vp(own_ptr),
                                            _vp(rival_ptr), _vp(krival_ptr)))

    def confidence(self, labels, mode=0, band=1.0, scale=None, chunk=0, parts=False, device=None):
        """les_hip_confidence: the confidence in [0, 1] of every pixel of the H x W x 4 label map `labels` under view `mode`'s aggregated cost
        volume -- how much cheaper the aggregated cost is within `band` slabs of the pixel's own disparity than anywhere else on its cost curve,
        (rival - own) / scale clamped (csrc/les_confidence.h); 0 for a label outside the disparity range or not finite, 1 where the band covers
        every finite cost.  scale None: raw_cost_max().  The num_fronto_planes planes run through the batch path `chunk` at a time (0: the
        library's default).  labels: a float32 torch tensor (on `device`: used where it is) or an array.  -> the H x W float32 map as a new
        tensor on `device` (None: this context's GPU; the simulator build takes "cpu"); parts: (conf, own, rival, k_rival), the in-band and
        rival minima (float32, +inf where none) and the rival's slab (int32, -1 where none).  Asynchronous on the calling thread's stream once
        the context's workspace exists where the maps are used where they are; a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "confidence:")
        conf = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        own = torch.empty_like(conf) if parts else None
        rival = torch.empty_like(conf) if parts else None
        kr = torch.empty((self.H, self.W), dtype=torch.int32, device=dev) if parts else None
        self._staged(dev, s is not labels, self.confidence_ptr, mode, s.data_ptr(), chunk, band, self.raw_cost_max() if scale is None else scale,
                     conf.data_ptr(), *(t.data_ptr() if parts else None for t in (own, rival, kr)))
        return (conf, own, rival, kr) if parts else conf

    # -- semi-global matching over the view's own cost volume (csrc/les_sgm.h; no reference counterpart) -------------------
    def sgm_workspace_bytes(self):
        """les_hip_sgm_workspace_bytes: the bytes sgm_labels keeps on the context for the current disparity range (the transposed volume and the
        path sums, 2 H W Kp floats); 0 where sgm_labels would refuse the context."""
        return int(self.L.les_hip_sgm_workspace_bytes(self.h))

    def sgm_penalties(self, p1=None, p2=None):
        """The penalties sgm_labels uses: P1 = 0.16 th_col and P2 = 1.28 th_col where None (as float32)."""
        th = np.float32(self.params.th_col)
        return (np.float32(0.16) * th if p1 is None else np.float32(p1)), (np.float32(1.28) * th if p2 is None else np.float32(p2))

    def sgm_labels(self, mode=0, paths=8, p1=None, p2=None, subpixel=True, labels_ptr=None, cost_ptr=None, device=None):
        """les_hip_sgm_labels: semi-global matching over the raw cost volume of view `mode` -- the costs truncated at th_col, scan-line dynamic
        programming along the first `paths` (2, 4 or 8) directions with penalties p1 <= p2 (None: 0.16 th_col and 1.28 th_col), summed, read out per
        pixel as wta_labels does (first minimum, parabola offset when `subpixel`) -- as the label map (0, 0, k* + off + min_disp, 0) and the summed
        path cost S(p, k*) of the winner (NOT the energy's unary cost).  Not for the image-based energy (error 3).  Asynchronous on the calling
        thread's stream once the context's workspace exists.  With labels_ptr (device address of the H x W x 4 float map; cost_ptr: the H x W float
        map or None) it writes there and returns None; without it returns (labels, cost) as new torch tensors on `device` (None: this context's
        GPU; the simulator build takes "cpu")."""
        if labels_ptr is None and cost_ptr is not None:
            raise ValueError("sgm_labels: cost_ptr without labels_ptr")
        p1, p2 = self.sgm_penalties(p1, p2)
        out = None
        if labels_ptr is None:
            out = self._labels_and_cost(device)
            labels_ptr, cost_ptr = out[0].data_ptr(), out[1].data_ptr()
        self._chk(self.L.les_hip_sgm_labels(self.h, int(mode), int(paths), C.c_float(p1), C.c_float(p2), int(bool(subpixel)), _vp(labels_ptr), _vp(cost_ptr)))
        return out

    def sgm_last_times(self):
        """les_hip_sgm_last_times: the device milliseconds of this thread's last sgm_labels under LES_HIP_SGM_TIMING=1 -- [transpose, one per
        direction ..., read-out]."""
        ms, n = (C.c_float * 10)(), C.c_int(0)
        self._chk(self.L.les_hip_sgm_last_times(ms, 10, C.byref(n)))
        return [float(ms[i]) for i in range(min(n.value, 10))]

    # -- slanted planes fitted to a disparity map (csrc/les_planefit.h; no reference counterpart) --------------------------
    def fit_planes_ptr(self, mode, labels_ptr, disp_ptr, fallback_ptr, out_ptr, kind_ptr=None, **params):
        """les_hip_fit_planes on device addresses (exactly one of labels_ptr / disp_ptr; fallback_ptr and kind_ptr may be None; out_ptr may be
        fallback_ptr).  params: radius, sig, gate0, gate_slope, max_slope, min_support (FIT_DEFAULTS).  Enqueue only once the table of `sig` exists."""
        q = dict(FIT_DEFAULTS, **params)
        if set(q) != set(FIT_DEFAULTS):
            raise TypeError(f"fit_planes: unknown parameters {sorted(set(q) - set(FIT_DEFAULTS))}")
        self._chk(self.L.les_hip_fit_planes(self.h, int(mode), _vp(labels_ptr), _vp(disp_ptr), _vp(fallback_ptr), _vp(out_ptr), _vp(kind_ptr), int(q["radius"]),
                                            C.c_float(q["sig"]), C.c_float(q["gate0"]), C.c_float(q["gate_slope"]), C.c_float(q["max_slope"]), int(q["min_support"])))

    def fit_planes(self, src, mode=0, fallback=None, with_kind=False, device=None, **params):
        """Slanted planes from a disparity map: per pixel of view `mode` an edge-aware weighted least-squares plane through the disparities of its
        window (les_hip_fit_planes).  src: an H x W x 4 label map or an H x W disparity map; fallback: an H x W x 4 label map for the pixels that
        get neither a fit nor their own disparity (None: (0, 0, min_disp, 0)); both float32 torch tensors or arrays (a tensor on `device` is
        used where it is, anything else is copied there).  params: radius=5, sig=10, gate0=1, gate_slope=0.5, max_slope=2, min_support=6.
        -> the H x W x 4 map as a new tensor on `device` (None: this context's GPU; the simulator build takes "cpu"); with_kind: (map, kind), kind
        H x W uint8 -- 2 slanted fit, 1 fronto-parallel at the pixel's own disparity, 0 fallback.  Asynchronous on the calling thread's stream
        where the maps are used where they are; a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_or_disparity_map(src, dev, "fit_planes:")
        fb = self._label_map(fallback, dev, "fit_planes: the fallback is") if fallback is not None else None
        out = torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev)
        kind = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev) if with_kind else None
        labels = s.dim() == 3
        self._staged(dev, s is not src or fb is not fallback, self.fit_planes_ptr, mode, s.data_ptr() if labels else None, None if labels else s.data_ptr(),
                     fb.data_ptr() if fb is not None else None, out.data_ptr(), kind.data_ptr() if with_kind else None, **params)
        return (out, kind) if with_kind else out

    # -- 3D reconstruction: points, normals and a mesh from a label map (csrc/les_reproject.h; no reference counterpart) --------------------
    def reproject_ptr(self, mode, labels_ptr, drop_ptr, calib, z_max, points_ptr, normals_ptr, valid_ptr):
        """les_hip_reproject on device addresses (drop_ptr, points_ptr and normals_ptr may be None; calib: a Calib or None).  Enqueue only."""
        self._chk(self.L.les_hip_reproject(self.h, int(mode), _vp(labels_ptr), _vp(drop_ptr), C.byref(calib) if calib is not None else None,
                                           C.c_float(0.0 if z_max is None else z_max), _vp(points_ptr), _vp(normals_ptr), _vp(valid_ptr)))

    def reproject(self, labels, calib, mode=0, drop=None, z_max=None, device=None):
        """les_hip_reproject: the H x W x 4 label map of view `mode` as 3D geometry -- (points, normals, valid): per pixel the point (X, Y, Z) of
        its disparity d = a x + b y + c and the unit normal of its label's plane, both H x W x 3 float32 in the view's own camera frame (X right,
        Y down, Z forward; the normal faces the camera), and valid, H x W uint8 255 / 0.  calib: a Calib (io.calib3d); Z = f baseline / (d + doffs),
        view 1 has its principal point at cx + doffs, so X_left = X_right + baseline.  A pixel is invalid -- NaN in both maps -- where d is not
        finite, d + doffs <= 0, `drop` (an H x W mask, nonzero = drop) is set, or Z > z_max (z_max None or <= 0: no limit).  The arithmetic is
        fp64 from the float inputs, rounded once (csrc/les_reproject.h).  labels / drop: torch tensors (on `device`: used where they are) or
        arrays.  -> new tensors on `device` (None: this context's GPU; the simulator build takes "cpu").  Asynchronous on the calling thread's
        stream where the maps are used where they are; a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "reproject:")
        m = self._byte_map(drop, dev, "reproject:") if drop is not None else None
        points = torch.empty((self.H, self.W, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((self.H, self.W, 3), dtype=torch.float32, device=dev)
        valid = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        self._staged(dev, s is not labels or m is not drop, self.reproject_ptr, mode, s.data_ptr(), m.data_ptr() if m is not None else None, calib, z_max,
                     points.data_ptr(), normals.data_ptr(), valid.data_ptr())
        return points, normals, valid

    def mesh_tile(self):
        """les_hip_mesh_tile: (pixels a workgroup of the mesh kernels owns, tiles the scan takes per turn)."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.les_hip_mesh_tile(C.byref(a), C.byref(b)))
        return a.value, b.value

    def mesh_ptr(self, mode, labels_ptr, valid_ptr, max_jump, vertex_index_ptr, vertex_pixel_ptr, triangles_ptr, counts_ptr):
        """les_hip_mesh on device addresses (vertex_index H x W int32, vertex_pixel H W int32, triangles 2 (H - 1) (W - 1) x 3 int32, counts two
        int64).  Enqueue only once the context's tile workspace exists."""
        self._chk(self.L.les_hip_mesh(self.h, int(mode), _vp(labels_ptr), _vp(valid_ptr), C.c_float(max_jump), _vp(vertex_index_ptr), _vp(vertex_pixel_ptr),
                                      _vp(triangles_ptr), _vp(counts_ptr)))

    def mesh(self, labels, valid, max_jump, mode=0, device=None):
        """les_hip_mesh: the triangle mesh over the pixel grid of the H x W x 4 label map -- (vertex_index, vertex_pixel, triangles).  Vertex k is
        the k-th pixel of `valid` (H x W, nonzero = valid: reproject's map) in row-major order: vertex_index is H x W int32 (-1 where invalid),
        vertex_pixel[k] the linear pixel index of vertex k.  Two pixels are connected iff both are valid and the un-truncated pairwise term of
        their labels, |l_p(p) - l_q(p)| + |l_p(q) - l_q(q)|, is <= max_jump (inf: every valid neighbour); quad (x, y) yields the triangles
        (p00, p01, p10) and (p10, p01, p11), each iff its three edges are connected, in row-major quad order, as nt x 3 int32 vertex numbers
        whose winding faces the camera.  The order is a function of the inputs alone.  -> new tensors on `device`, cut to the counts (which
        waits for the device)."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "mesh:")
        m = self._byte_map(valid, dev, "mesh:")
        vi = torch.empty((self.H, self.W), dtype=torch.int32, device=dev)
        vpix = torch.empty((self.H * self.W,), dtype=torch.int32, device=dev)
        tri = torch.empty((max(1, 2 * (self.H - 1) * (self.W - 1)), 3), dtype=torch.int32, device=dev)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        # (copied, always: torch wrote the zeros on its stream, and the counts are read next)
        self._staged(dev, True, self.mesh_ptr, mode, s.data_ptr(), m.data_ptr(), max_jump, vi.data_ptr(), vpix.data_ptr(), tri.data_ptr(), counts.data_ptr())
        nv, nt = (int(v) for v in counts.cpu())
        return vi, vpix[:nv], tri[:nt]

    # -- view synthesis and the photometric check (csrc/les_view.h; no reference counterpart) -------------------------------
    def render_view_ptr(self, src_mode, labels_ptr, image_ptr, t, bgr_ptr, disp_ptr, hit_ptr):
        """les_hip_render_view on device addresses (image_ptr None: the context's image of src_mode).  Enqueue only.  Rows wider than
        WARP_MAX_WIDTH raise (error 3)."""
        self._chk(self.L.les_hip_render_view(self.h, int(src_mode), _vp(labels_ptr), _vp(image_ptr), C.c_float(t), _vp(bgr_ptr), _vp(disp_ptr), _vp(hit_ptr)))

    def _image_map(self, image, dev, who):
        """The H x W x 3 uint8 image on dev: a uint8 tensor that is there already is used where it is."""
        import torch
        m = image.to(device=dev, dtype=torch.uint8).contiguous() if torch.is_tensor(image) else torch.from_numpy(np.array(image, dtype=np.uint8, order="C")).to(dev)
        if tuple(m.shape) != (self.H, self.W, 3):
            raise ValueError(f"{who} an {self.H} x {self.W} x 3 uint8 image, not {tuple(m.shape)}")
        return m

    def render_view(self, labels, src_mode=0, t=1.0, image=None, device=None):
        """les_hip_render_view: the view of a camera at fraction t in [0, 1] of the baseline, counted from view src_mode (0 left, 1 right) towards the
        other view, rendered from that view's H x W x 4 label map and its image (image None: the context's; else H x W x 3 uint8 b, g, r) --
        (bgr, disp, hit): H x W x 3 uint8, H x W float32 (the disparity of what is seen, in view src_mode's units; NaN in holes), H x W uint8
        (1 a source pixel landed, 2 a one-column crack between two such pixels closed, 0 a hole, colour 0).  The nearest surface wins a column;
        the colour is the source row sampled linearly (csrc/les_view.h).  t = 0 returns the source image wherever the disparity is finite, t = 1
        is the other view.  labels / image: torch tensors (on `device`: used where they are) or arrays.  -> new tensors on `device` (None: this
        context's GPU; the simulator build takes "cpu").  Asynchronous on the calling thread's stream where the maps are used where they are; a
        map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "render_view:")
        im = self._image_map(image, dev, "render_view:") if image is not None else None
        bgr = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=dev)
        disp = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        hit = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        self._staged(dev, s is not labels or im is not image, self.render_view_ptr, src_mode, s.data_ptr(), im.data_ptr() if im is not None else None, t,
                     bgr.data_ptr(), disp.data_ptr(), hit.data_ptr())
        return bgr, disp, hit

    def blend_views_ptr(self, t, tol, fill, left_ptrs, right_ptrs, bgr_ptr, disp_ptr, src_ptr):
        """les_hip_blend_views on device addresses: left_ptrs / right_ptrs are (bgr, disp, hit) or None.  Enqueue only."""
        l, r = (tuple(q) if q is not None else (None, None, None) for q in (left_ptrs, right_ptrs))
        self._chk(self.L.les_hip_blend_views(self.h, C.c_float(t), C.c_float(tol), int(bool(fill)), *(_vp(q) for q in l + r), _vp(bgr_ptr), _vp(disp_ptr), _vp(src_ptr)))

    def blend_views(self, t, left=None, right=None, tol=1.0, fill=True, device=None):
        """les_hip_blend_views: two renders of the camera at fraction t of the baseline (from the left view) as one image.  left: render_view's
        (bgr, disp, hit) of view 0 at t; right: that of view 1 at 1 - t; either may be None.  Where both see the pixel and their disparities agree
        within tol the colours are mixed (1 - t) : t, where they disagree the nearer one is taken, where one sees it that one; with `fill` a hole
        takes the farther of its nearest neighbours to the left and to the right on the row (csrc/les_view.h).  -> (bgr, disp, src): H x W x 3
        uint8, H x W float32, H x W uint8 (0 hole, 1 left, 2 right, 3 both, 4 filled), new tensors on `device` (None: this context's GPU; the
        simulator build takes "cpu").  Tensors on `device` are used where they are; a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        copied, sides = False, []
        for side in (left, right):
            if side is None:
                sides.append(None)
                continue
            b, d, h = side
            tb, td, th = self._image_map(b, dev, "blend_views:"), _float_tensor(d, dev), self._byte_map_raw(h, dev, "blend_views:")
            if tuple(td.shape) != (self.H, self.W):
                raise ValueError(f"blend_views: an {self.H} x {self.W} disparity map, not {tuple(td.shape)}")
            copied |= tb is not b or td is not d or th is not h
            sides.append((tb, td, th))
        bgr = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=dev)
        disp = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        src = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        self._staged(dev, copied, self.blend_views_ptr, t, tol, fill, *(tuple(q.data_ptr() for q in s) if s is not None else None for s in sides),
                     bgr.data_ptr(), disp.data_ptr(), src.data_ptr())
        return bgr, disp, src

    def _byte_map_raw(self, m, dev, who):
        """The H x W uint8 map on dev with its values kept (a hit map): a uint8 tensor that is there already is used where it is."""
        import torch
        t = m.to(device=dev, dtype=torch.uint8).contiguous() if torch.is_tensor(m) else torch.from_numpy(np.array(m, dtype=np.uint8, order="C")).to(dev)
        if tuple(t.shape) != (self.H, self.W):
            raise ValueError(f"{who} an {self.H} x {self.W} uint8 map, not {tuple(t.shape)}")
        return t

    def photo_error_ptr(self, mode, labels_ptr, err_ptr, vis_ptr):
        """les_hip_photo_error on device addresses.  Enqueue only."""
        self._chk(self.L.les_hip_photo_error(self.h, int(mode), _vp(labels_ptr), _vp(err_ptr), _vp(vis_ptr)))

    def photo_error(self, labels, mode=0, device=None):
        """les_hip_photo_error: the photometric consistency of the H x W x 4 label map of view `mode` with the context's two images, no ground
        truth needed -- (err, vis): vis H x W uint8, 1 where the pixel is seen in the other view (err = the mean absolute difference over b, g, r
        between the other image sampled linearly where the label says the pixel is and the pixel's own colour), 2 where the label map itself says
        it is occluded (a nearer pixel of the row lands on the same column), 0 where it leaves the image or its disparity is not finite; err
        H x W float32, NaN wherever vis != 1 (csrc/les_view.h).  labels: a torch tensor (on `device`: used where it is) or an array.  -> new
        tensors on `device` (None: this context's GPU; the simulator build takes "cpu"); a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_map(labels, dev, "photo_error:")
        err = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        vis = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        self._staged(dev, s is not labels, self.photo_error_ptr, mode, s.data_ptr(), err.data_ptr(), vis.data_ptr())
        return err, vis

    # -- a half-resolution solve as a start (csrc/les_pyramid.h; no reference counterpart) ------------------------------------
    def image(self, mode=0):
        """les_hip_get_image: the H x W x 3 u8 image of view `mode` as the context holds it."""
        out = np.empty((self.H, self.W, 3), np.uint8)
        self._chk(self.L.les_hip_get_image(self.h, int(mode), _ptr(out)))
        return out

    def half(self):
        """les_hip_create_half: a new, independent HipCostVolumeEnergy of the same kind, filter and interpolation at half resolution, built on the
        device from this context's own images and volumes (pooled: csrc/les_pyramid.h).  H, W, D -> half_size of each; max_disp, min_disp and the
        vertical-disparity settings halved; windR -> max(1, (windR + 1) // 2).  It owns its volumes and outlives this context.  A min_disp that
        is not an even integer raises (error 3).  The caller closes it."""
        h = C.c_void_p()
        self._chk(self.L.les_hip_create_half(C.byref(h), self.h))
        o = type(self).__new__(type(self))
        o.L, o.h, o.filter, o._keep = self.L, h, self.filter, None
        p = self.params
        o.H, o.W = half_size(self.H), half_size(self.W)
        o.D = half_size(self.D)
        o.max_disp = float(np.float32(0.5) * np.float32(p.max_disparity))
        o.params = Params(o.H, o.W, o.D, max(1, (p.windR + 1) // 2), p.eps, p.th_col, o.max_disp, float(np.float32(0.5) * np.float32(p.min_disparity)),
                          p.device, p.volumes_on_device)
        o.interpolate = self.interpolate
        if hasattr(self, "naive_cost"):
            o.naive_cost = self.naive_cost
        o.max_vdisp, o.random_vdisp = 0.5 * getattr(self, "max_vdisp", 0.0), 0.5 * getattr(self, "random_vdisp", 0.0)
        o.imL = o.image(0) if self.imL is not None else None
        o.imR = o.image(1) if self.imR is not None else None
        return o

    def upsample_labels_ptr(self, half, mode, src_ptr, out_ptr, kind_ptr=None):
        """les_hip_upsample_labels on device addresses (kind_ptr may be None).  Enqueue only."""
        self._chk(self.L.les_hip_upsample_labels(self.h, half.h, int(mode), _vp(src_ptr), _vp(out_ptr), _vp(kind_ptr)))

    def upsample_labels(self, half, src, mode=0, with_kind=False, device=None):
        """les_hip_upsample_labels: `src`, the half.H x half.W x 4 label map of view `mode` found on `half` (this context's half()), re-expressed
        at this context's resolution, edge-aware: every pixel takes the plane of the nearest-coloured of its four surrounding half pixels,
        rewritten as (a, b, (2c - a / 2) - b / 2, 2v), when that is a valid label here, else the fronto-parallel plane at its clamped disparity
        (csrc/les_pyramid.h).  src: a float32 torch tensor (on `device`: used where it is) or an array.  -> the H x W x 4 map as a new tensor on
        `device` (None: this context's GPU; the simulator build takes "cpu"); with_kind: (map, kind), kind H x W uint8 -- 0 kept, 1 clamped,
        2 non-finite.  Asynchronous on the calling thread's stream
        where the maps are used where they are; a map the wrapper had to copy is waited for (_staged)."""
        import torch
        dev = self._device(device)
        s = self._label_map(src, dev, "upsample_labels:", (half.H, half.W), "label map of the half context")
        out = torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev)
        kind = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev) if with_kind else None
        self._staged(dev, s is not src, self.upsample_labels_ptr, half, mode, s.data_ptr(), out.data_ptr(), kind.data_ptr() if with_kind else None)
        return (out, kind) if with_kind else out

    def wta_update(self, rects, planes, cur_cost_dev, prop_cost_dev, labels_dev, planes_on_device=False):
        rects = _rects(rects)
        if planes_on_device:
            pp = C.c_void_p(int(planes))
        else:
            self._wplanes = _planes(planes)
            pp = _ptr(self._wplanes)
        self._chk(self.L.les_hip_wta_update(self.h, len(rects), _ptr(rects), pp, int(planes_on_device),
                                            C.c_void_p(int(cur_cost_dev)), C.c_void_p(int(prop_cost_dev)), C.c_void_p(int(labels_dev))))
