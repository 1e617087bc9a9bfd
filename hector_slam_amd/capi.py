"""ctypes binding of the C ABI (include/hector_mi355/capi.h) + a thin Python mirror of the
reference's map-representation interface.

``MapRepMultiMap`` keeps the reference's method names and argument meaning
(hector_slam_lib/slam_main/MapRepMultiMap.h, MapRepresentationInterface.h:38-62) so the
parity tests read like calls into the reference.  Everything computes on the GPU through
``libhector_mi355.so``; if the library is missing, or no HIP device is present, construction
raises -- there is no CPU fallback in this package.

torch is imported first on purpose: PyTorch-ROCm bundles its own ``libamdhip64.so`` with the
same SONAME as /opt/rocm's; loading torch first makes the dynamic loader bind this library
to that single HIP runtime, so torch device pointers / streams and ours interoperate.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

try:  # plumbing only (device memory, streams, torch.distributed); see module docstring
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is always present in the target image
    torch = None

from . import build as _build

HSM_OK = 0
LAYOUT_AUTO, LAYOUT_QUAD, LAYOUT_PLANE = 0, 1, 2
PARITY_FAST, PARITY_EXACT, PARITY_RELAXED, PARITY_AUTO = 0, 1, 2, 3
GATHER_AUTO, GATHER_PEER, GATHER_RCCL, GATHER_DIRECT = 0, 1, 2, 3
ORDER_GIVEN, ORDER_MORTON, ORDER_AUTO = 0, 1, 2
EXCHANGE_HANDLE_BYTES = 64
MAX_ALIGN_POINTS = 16384  # HSM_MAX_ALIGN_POINTS
POINTS_TILE = 4096        # kPointsTile of csrc/map_points_kernels.h: cells of a box a workgroup of the extraction takes at a time

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class HsmOpts(C.Structure):
    _fields_ = [("device", C.c_int), ("layout", C.c_int), ("waves_per_scan", C.c_int)]


class HsmError(RuntimeError):
    pass


# every symbol include/hector_mi355/capi.h declares: name -> (restype, argtypes)
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    "hsm_create": (_i, [_f, _i, _i, C.c_uint, _f, _f, C.POINTER(HsmOpts), C.POINTER(_vp)]),
    "hsm_destroy": (None, [_vp]),
    "hsm_reset": (_i, [_vp]),
    "hsm_levels": (_i, [_vp]),
    "hsm_scale_to_map": (_f, [_vp]),
    "hsm_set_update_factor_free": (_i, [_vp, _f]),
    "hsm_set_update_factor_occupied": (_i, [_vp, _f]),
    "hsm_on_map_updated": (_i, [_vp]),
    "hsm_set_parity": (_i, [_vp, _i]),
    "hsm_parity": (_i, [_vp]),
    "hsm_last_launch_parity": (_i, [_vp]),
    "hsm_set_batch_order": (_i, [_vp, _i]),
    "hsm_set_batch_order_refresh": (_i, [_vp, _i]),
    "hsm_batch_order": (_i, [_vp]),
    "hsm_last_launch_sorted": (_i, [_vp]),
    "hsm_match": (_i, [_vp, _f32p, _vp, _i, _f32p, _f32p, _f32p]),
    "hsm_match_trace": (_i, [_vp, _f32p, _vp, _i, _f32p, _f32p, _f32p, _f32p, _i, C.POINTER(_i)]),
    "hsm_match_batch_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "hsm_match_batch": (_i, [_vp, _i, _f32p, _vp, _vp, _i, _f32p, _vp]),
    "hsm_update_by_scan": (_i, [_vp, _f32p, _vp, _i, _f32p]),
    "hsm_update_by_scan_level": (_i, [_vp, _i, _f32p, _vp, _i, _f32p]),
    "hsm_update_by_scans_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "hsm_update_by_scans_device_origos": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "hsm_update_by_scans": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp]),
    "hsm_set_update_gate": (_i, [_vp, _f, _f]),
    "hsm_reset_update_gate": (_i, [_vp]),
    "hsm_update_gate_state": (_i, [_vp, _f32p, C.POINTER(C.c_longlong)]),
    "hsm_update_by_scans_device_gated": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "hsm_update_by_scans_device_gated_origos": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "hsm_slam_scans_device": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_slam_scans_device_origos": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_slam_ranges_tf_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, C.c_double, _vp, _i, _f, _f, _f, _f, _f, _vp,
                                       _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "hsm_slam_ranges_tf_workspace": (C.c_size_t, [_i, _i]),
    "hsm_slam_ranges_tf": (_i, [_vp, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, C.c_double, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp,
                                _vp, _vp, _vp, _vp]),
    "hsm_ingest_laser_scan": (_i, [_vp, _vp, _i, _f, _f, _f, _f, _f, _vp, C.POINTER(_i)]),
    "hsm_ingest_point_cloud": (_i, [_vp, _vp, _i, _vp, _f, _f, _f, _f, _f, _vp, C.POINTER(_i), _vp]),
    "hsm_ingest_laser_scan_tf": (_i, [_vp, _vp, _i, _f, _f, _f, _f, C.c_double, _vp, _f, _f, _f, _f, _f, _vp,
                                      C.POINTER(_i), _vp]),
    "hsm_synchronize": (_i, [_vp]),
    "hsm_match_ingested": (_i, [_vp, _f32p, _f32p, _f32p]),
    "hsm_update_by_ingested": (_i, [_vp, _f32p]),
    "hsm_match_batch_ranges_device": (_i, [_vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "hsm_match_batch_ranges_workspace": (C.c_size_t, [_i, _i]),
    "hsm_match_batch_ranges": (_i, [_vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp]),
    "hsm_ingest_batch_ranges_tf_device": (_i, [_vp, _i, _vp, _i, _f, _f, _f, _f, C.c_double, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp,
                                               _vp, _vp, _vp]),
    "hsm_match_batch_ranges_tf": (_i, [_vp, _i, _vp, _vp, _i, _f, _f, _f, _f, C.c_double, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp,
                                       _vp, _vp]),
    "hsm_occupancy_grid": (_i, [_vp, _i, _vp]),
    "hsm_occupancy_grid_device": (_i, [_vp, _i, _vp, _vp]),
    "hsm_occupancy_changes_device": (_i, [_vp, _i, _vp, _vp, _vp]),
    "hsm_occupancy_changes": (_i, [_vp, _i, _vp, _i32p]),
    "hsm_occupancy_restart": (_i, [_vp, _i]),
    "hsm_map_extents_device": (_i, [_vp, _i, _vp, _vp]),
    "hsm_map_extents": (_i, [_vp, _i, _i32p]),
    "hsm_map_image_device": (_i, [_vp, _i, _vp, _vp, _vp]),
    "hsm_map_image": (_i, [_vp, _i, _vp, _vp]),
    "hsm_map_tiles_device": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "hsm_map_tiles": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "hsm_ray_distances": (_i, [_vp, _i, _f, _f, _f, _i, _f32p, _f32p, _f32p, _f32p]),
    "hsm_ray_distances_device": (_i, [_vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "hsm_cast_scans_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "hsm_cast_scans": (_i, [_vp, _i, _i, _vp, _vp, _i, _f, _vp, _vp]),
    "hsm_score_batch_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "hsm_select_best_device": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_match_score_batch_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "hsm_covariance_batch_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "hsm_match_cov_batch_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp,
                                        _vp]),
    "hsm_covariance_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "hsm_score_window_device": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "hsm_score_window": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "hsm_window_poses_device": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "hsm_select_topk_device": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    "hsm_select_topk_workspace": (C.c_size_t, [_i, _i]),
    "hsm_relocalize_device": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_relocalize_workspace": (C.c_size_t, [_i, _i]),
    "hsm_relocalize": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_score_windows_batch_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "hsm_select_topk_groups_device": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    "hsm_select_topk_groups_workspace": (C.c_size_t, [_i, _i, _i]),
    "hsm_relocalize_batch_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp]),
    "hsm_relocalize_batch_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "hsm_relocalize_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsm_match_score_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "hsm_occupied_points_workspace": (C.c_size_t, [_i]),
    "hsm_occupied_points_device": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    "hsm_occupied_points": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
    "hsm_align_map_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "hsm_align_map": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "hsm_likelihood_states": (_i, [_vp, _i, _i, _f32p, _vp, _i, _f32p]),
    "hsm_residual_states": (_i, [_vp, _i, _i, _f32p, _vp, _i, _f32p]),
    "hsm_covariance_for_poses": (_i, [_vp, _i, _i, _f32p, _vp, _i, _f32p, _f32p, _f32p]),
    "hsm_group_create": (_i, [_f, _i, _i, C.c_uint, _f, _f, _i32p, _i, C.POINTER(_vp)]),
    "hsm_group_destroy": (None, [_vp]),
    "hsm_group_size": (_i, [_vp]),
    "hsm_group_member": (_vp, [_vp, _i]),
    "hsm_group_set_update_factors": (_i, [_vp, _f, _f]),
    "hsm_group_process_scan": (_i, [_vp, _f32p, _vp, _i, _f32p, _i, _f32p, _f32p]),
    "hsm_group_match_batch": (_i, [_vp, _i, _f32p, _vp, _vp, _i, _f32p, _vp]),
    "hsm_group_match_batch_device": (_i, [_vp, _i32p, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "hsm_group_synchronize": (_i, [_vp]),
    "hsm_group_debug_force_p2p": (_i, [_vp, _i]),
    "hsm_shard_bounds": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "hsm_group_set_gather": (_i, [_vp, _i]),
    "hsm_group_gather_mode": (_i, [_vp]),
    "hsm_group_gather_note": (C.c_char_p, [_vp]),
    "hsm_group_gathered": (_vp, [_vp, _i, _i]),
    "hsm_retain_scan": (_i, [_vp, _vp, _i, _f32p]),
    "hsm_exchange_create": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "hsm_exchange_destroy": (None, [_vp]),
    "hsm_exchange_handle": (_i, [_vp, _vp]),
    "hsm_exchange_connect": (_i, [_vp, _vp]),
    "hsm_exchange_connect_local": (_i, [_vp, C.POINTER(_vp)]),
    "hsm_exchange_post": (_i, [_vp, _vp, _i, _i, _vp]),
    "hsm_exchange_wait": (_i, [_vp, _vp, _vp]),
    "hsm_exchange_post_wait": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "hsm_match_batch_device_gather": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "hsm_exchange_epochs": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "hsm_exchange_status": (_i, [_vp]),
    "hsm_exchange_memory_kind": (C.c_char_p, [_vp]),
    "hsm_level_info": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), C.POINTER(_f)]),
    "hsm_map_coords_pose": (_i, [_vp, _i, _f32p, _f32p]),
    "hsm_world_coords_pose": (_i, [_vp, _i, _f32p, _f32p]),
    "hsm_update_index": (_i, [_vp, _i]),
    "hsm_download_level": (_i, [_vp, _i, _vp, _vp]),
    "hsm_upload_level": (_i, [_vp, _i, _vp, _vp]),
    "hsm_download_rows": (_i, [_vp, _i, _i, _i, _f32p]),
    "hsm_download_cells": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i]),
    "hsm_last_update_bbox": (_i, [_vp, _i, _i32p]),
    "hsm_take_dirty_bbox": (_i, [_vp, _i, _i32p]),
    "hsm_copy_map": (_i, [_vp, _vp]),
    "hsm_copy_map_boxes": (_i, [_vp, _vp, _vp]),
    "hsm_merge_map": (_i, [_vp, _vp, _vp]),
    "hsm_merge_map_box": (_i, [_vp, _vp, _vp, _i, _vp]),
    "hsm_group_sync_maps": (_i, [_vp, _i, _vp]),
    "hsm_shift_map": (_i, [_vp, _f, _f, _vp]),
    "hsm_map_start": (_i, [_vp, _f32p]),
    "hsm_download_prob": (_i, [_vp, _i, _f32p]),
    "hsm_hessian_derivs": (_i, [_vp, _i, _f32p, _vp, _i, _f32p, _f32p]),
    "hsm_eval_beams": (_i, [_vp, _i, _f32p, _vp, _i, _vp]),
    "hsm_match_level": (_i, [_vp, _i, _f32p, _vp, _i, _i, _f32p, _f32p]),
    "hsm_debug_set_update_serial": (_i, [_vp, _i, C.c_uint]),
    "hsm_debug_set_coop_barrier": (_i, [_vp, C.c_uint]),
    "hsm_debug_set_coop_mute": (_i, [_vp, _i]),
    "hsm_debug_coop_fallbacks": (_i, [_vp]),
    "hsm_debug_set_schedule": (_i, [_vp, _i, _i]),
    "hsm_debug_batch_order": (_i, [_vp, _i, _vp, _vp, _vp]),
    "hsm_debug_spec_stats": (_i, [_vp, _i, _vp]),
    "hsm_debug_marks_nonzero": (_i, [_vp, _i, _vp]),
    "hsm_debug_sincos": (_i, [_vp, _i, _f32p, _f32p, _f32p]),
    "hsm_debug_expf": (_i, [_vp, _i, _f32p, _f32p, _f32p]),
    "hsm_device_info": (_i, [_vp, _i32p]),
    "hsm_set_clock_probe": (_i, [_vp, _vp]),
    "hsm_gn_iterations_per_match": (_i, [_vp]),
    "hsm_last_launch_kernel": (C.c_char_p, [_vp]),
    "hsm_last_launch_config": (_i, [_vp, _i32p]),
    "hsm_last_error": (C.c_char_p, []),
    "hsm_version": (C.c_char_p, []),
}

_lib = None


def library_path() -> str:
    return _build.LIB


def load_library(build_if_missing: bool = True):
    """dlopen libhector_mi355.so (building it with hipcc when stale) and type every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build_native() if build_if_missing else _build.LIB
    if os.environ.get("HSM_LIB"):  # kernel A/B experiments: an alternative build of the same library
        path = os.environ["HSM_LIB"]
    if not os.path.exists(path):
        raise HsmError(f"{path} not found and could not be built; hector_slam_amd has no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: fail loudly
        fn.restype, fn.argtypes = res, args
    # the node's two per-scan calls a second time with raw-address prototypes: numpy's ndpointer argument check costs
    # ~2 us per array argument, which is a third of a 40 us call (lib["name"] creates a separate function object)
    lib._hsm_match_raw = lib["hsm_match"]
    lib._hsm_match_raw.restype, lib._hsm_match_raw.argtypes = _i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]
    lib._hsm_update_raw = lib["hsm_update_by_scan"]
    lib._hsm_update_raw.restype, lib._hsm_update_raw.argtypes = _i, [_vp, _vp, _vp, _i, _vp]
    _lib = lib
    return lib


def shard_bounds(total: int, rank: int, world: int) -> tuple[int, int]:
    """[begin, end) of shard `rank` of `total` scans over `world` replicas: the library's ONE partitioning rule, asked of the
    library itself (hsm_shard_bounds).  sharding.shard_bounds is the same closed form in Python -- it must not need a HIP
    toolchain or a built library for an index computation; tests/test_sharding_cpu.py holds the two equal."""
    b, e = C.c_int(0), C.c_int(0)
    _check(load_library().hsm_shard_bounds(int(total), int(rank), int(world), C.byref(b), C.byref(e)), "hsm_shard_bounds")
    return b.value, e.value


def match_batch_ranges_workspace(batch: int, n: int) -> int:
    """bytes of the caller-owned workspace hsm_match_batch_ranges_device needs for `batch` scans of n beams (0: sizes it refuses);
    host arithmetic, no device needed"""
    return int(load_library().hsm_match_batch_ranges_workspace(int(batch), int(n)))


def _check(rc: int, what: str):
    if rc != HSM_OK:
        raise HsmError(f"{what} failed ({rc}): {load_library().hsm_last_error().decode()}")


def merge_map(dst, src, src_in_dst):
    """`src`'s pyramid merged into `dst`'s on the device (hsm_merge_map): src_in_dst = (tx, ty, theta), the pose of src's world
    frame in dst's, metres and radians; queued on dst's stream, no host wait"""
    t = np.ascontiguousarray(src_in_dst, np.float32).reshape(-1)
    if t.size != 3:
        raise ValueError("src_in_dst must hold tx, ty, theta")
    _check(dst._lib.hsm_merge_map(dst._h, src._h, t.ctypes.data), "hsm_merge_map")


def merge_map_box(dst, src, src_in_dst, level):
    """the cells of dst's `level` that merge_map(dst, src, src_in_dst) visits (hsm_merge_map_box) -> int32 [x0, y0, x1, y1],
    inclusive, x1 < x0 where src misses the level; host arithmetic only"""
    t = np.ascontiguousarray(src_in_dst, np.float32).reshape(-1)
    if t.size != 3:
        raise ValueError("src_in_dst must hold tx, ty, theta")
    bb = np.empty(4, np.int32)
    _check(dst._lib.hsm_merge_map_box(dst._h, src._h, t.ctypes.data, int(level), bb.ctypes.data), "hsm_merge_map_box")
    return bb


def _addr(a) -> int:
    """address of a numpy array's first element (cheaper than a.ctypes.data)"""
    return a.__array_interface__["data"][0]


def _is_f32c(x) -> bool:
    return type(x) is np.ndarray and x.dtype == np.float32 and x.flags.c_contiguous


def _pts(pts):
    if _is_f32c(pts) and pts.ndim == 2 and pts.shape[1] == 2:
        a = pts
    else:
        a = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
    return a, (_addr(a) if a.size else None), a.shape[0]


def _v(x, n):
    if _is_f32c(x) and x.ndim == 1:
        a = x
    else:
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} floats")
    return a


def _fill(dst, x, n):
    """dst[:] = the n floats of x (ValueError on any other size, as _v)"""
    if type(x) is not np.ndarray:
        x = np.asarray(x, dtype=np.float32)
    if x.size != n:
        raise ValueError(f"expected {n} floats")
    dst[:] = x.reshape(-1)


class _SmallArgs:
    __slots__ = ("buf", "pose", "origo", "out", "cov", "a_pose", "a_origo", "a_out", "a_cov", "lock")

    def __init__(self):
        import threading
        self.buf = np.zeros(3 + 2 + 3 + 9 + 3, np.float32)
        self.pose, self.origo, self.out, self.cov = self.buf[0:3], self.buf[3:5], self.buf[5:8], self.buf[8:17]
        base = _addr(self.buf)
        self.a_pose, self.a_origo, self.a_out, self.a_cov = base, base + 12, base + 20, base + 32
        self.lock = threading.Lock()


_ZERO2 = np.zeros(2, np.float32)


class MapRepMultiMap:
    """GPU-resident multi-resolution map representation (reference: MapRepMultiMap.h:45-173)."""

    def __init__(self, mapResolution: float, mapSizeX: int, mapSizeY: int, numDepth: int,
                 startCoords=(0.5, 0.5), device: int = -1, layout: int = LAYOUT_AUTO,
                 waves_per_scan: int = 0, parity: int | None = None):
        self._lib = load_library()
        self._h = _vp()
        opts = HsmOpts(device, layout, waves_per_scan)
        _check(self._lib.hsm_create(mapResolution, mapSizeX, mapSizeY, numDepth, startCoords[0],
                                    startCoords[1], C.byref(opts), C.byref(self._h)), "hsm_create")
        self._iobuf = _SmallArgs()  # created here, not on first use: two threads' first calls must meet at ONE lock
        if parity is not None:
            self.set_parity(parity)

    def _io(self):
        """small-argument block of the two per-scan calls: one persistent float32 array whose addresses are taken ONCE
        (extracting an array's address costs ~1 us, a 3-float copy 0.3 us); the lock keeps concurrent Python callers
        of one map apart (ctypes releases the GIL during the call)"""
        io = getattr(self, "_iobuf", None)
        if io is None:
            io = self._iobuf = _SmallArgs()
        return io

    def set_parity(self, mode: int):
        """PARITY_FAST (tree summation) / PARITY_EXACT (the reference's beam-order fp32 chains: bit-identical poses)"""
        _check(self._lib.hsm_set_parity(self._h, mode), "hsm_set_parity")

    def parity(self) -> int:
        return self._lib.hsm_parity(self._h)

    def set_batch_order(self, order: int):
        """ORDER_AUTO (default) / ORDER_GIVEN / ORDER_MORTON: how a batch is laid out on the device (hsm_set_batch_order)"""
        _check(self._lib.hsm_set_batch_order(self._h, order), "hsm_set_batch_order")

    def set_batch_order_refresh(self, launches: int):
        """a stream's permutation serves that many launches of the same batch size before it is computed again (default 16)"""
        _check(self._lib.hsm_set_batch_order_refresh(self._h, launches), "hsm_set_batch_order_refresh")

    def batch_order(self) -> int:
        return self._lib.hsm_batch_order(self._h)

    def last_launch_sorted(self) -> bool:
        return bool(self._lib.hsm_last_launch_sorted(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hsm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- MapRepresentationInterface -------------------------------------------------
    def reset(self): _check(self._lib.hsm_reset(self._h), "hsm_reset")
    def getScaleToMap(self) -> float: return self._lib.hsm_scale_to_map(self._h)
    def getMapLevels(self) -> int: return self._lib.hsm_levels(self._h)
    def onMapUpdated(self): _check(self._lib.hsm_on_map_updated(self._h), "hsm_on_map_updated")

    def setUpdateFactorFree(self, v: float):
        _check(self._lib.hsm_set_update_factor_free(self._h, v), "hsm_set_update_factor_free")

    def setUpdateFactorOccupied(self, v: float):
        _check(self._lib.hsm_set_update_factor_occupied(self._h, v), "hsm_set_update_factor_occupied")

    def matchData(self, beginEstimateWorld, dataContainer, covMatrix=None, origo=_ZERO2):
        """-> (newEstimateWorld[3], covMatrix[9] column-major); cov is in/out like the reference."""
        a, p, n = _pts(dataContainer)
        io = self._io()
        with io.lock:
            _fill(io.pose, beginEstimateWorld, 3)
            _fill(io.origo, origo, 2)
            if covMatrix is None:
                io.cov[:] = 0.0
            else:
                _fill(io.cov, covMatrix, 9)
            rc = self._lib._hsm_match_raw(self._h, io.a_pose, p, n, io.a_origo, io.a_out, io.a_cov)
            out, cov = io.out.copy(), io.cov.copy()
        if rc != HSM_OK:
            _check(rc, "hsm_match")
        return out, cov

    def updateByScan(self, dataContainer, robotPoseWorld, origo=_ZERO2):
        a, p, n = _pts(dataContainer)
        io = self._io()
        with io.lock:
            _fill(io.pose, robotPoseWorld, 3)
            _fill(io.origo, origo, 2)
            rc = self._lib._hsm_update_raw(self._h, io.a_pose, p, n, io.a_origo)
        if rc != HSM_OK:
            _check(rc, "hsm_update_by_scan")

    def synchronize(self):
        """wait for queued device work (updateByScan returns once its kernels are queued)"""
        _check(self._lib.hsm_synchronize(self._h), "hsm_synchronize")

    # ---- GridMap accessors (host mirror support) ---------------------------------------
    def level_info(self, level: int):
        sx, sy, cell, scale = _i(), _i(), _f(), _f()
        _check(self._lib.hsm_level_info(self._h, level, C.byref(sx), C.byref(sy), C.byref(cell),
                                        C.byref(scale)), "hsm_level_info")
        return sx.value, sy.value, cell.value, scale.value

    def getMapCoordsPose(self, level, world):
        out = np.empty(3, np.float32)
        _check(self._lib.hsm_map_coords_pose(self._h, level, _v(world, 3), out), "hsm_map_coords_pose")
        return out

    def getWorldCoordsPose(self, level, mp):
        out = np.empty(3, np.float32)
        _check(self._lib.hsm_world_coords_pose(self._h, level, _v(mp, 3), out), "hsm_world_coords_pose")
        return out

    def getUpdateIndex(self, level=0) -> int:
        return self._lib.hsm_update_index(self._h, level)

    def download_level(self, level):
        sx, sy, _, _ = self.level_info(level)
        lo = np.empty((sy, sx), np.float32)
        ui = np.empty((sy, sx), np.int32)
        _check(self._lib.hsm_download_level(self._h, level, lo.ctypes.data, ui.ctypes.data), "hsm_download_level")
        return lo, ui

    def upload_level(self, level, logodds, update_index=None):
        lo = np.ascontiguousarray(logodds, np.float32)
        ui = None if update_index is None else np.ascontiguousarray(update_index, np.int32)
        _check(self._lib.hsm_upload_level(self._h, level, lo.ctypes.data, None if ui is None else ui.ctypes.data),
               "hsm_upload_level")

    def download_rows(self, level, y0, y1):
        sx, _, _, _ = self.level_info(level)
        out = np.empty((max(y1 - y0, 0), sx), np.float32)
        _check(self._lib.hsm_download_rows(self._h, level, y0, y1, out.reshape(-1) if out.size else
                                           np.zeros(1, np.float32)), "hsm_download_rows")
        return out

    def last_update_bbox(self, level):
        bb = np.empty(4, np.int32)
        _check(self._lib.hsm_last_update_bbox(self._h, level, bb), "hsm_last_update_bbox")
        return bb

    def take_dirty_bbox(self, level):
        bb = np.empty(4, np.int32)
        _check(self._lib.hsm_take_dirty_bbox(self._h, level, bb), "hsm_take_dirty_bbox")
        return bb

    def copy_map_from(self, src, boxes=None):
        """this context's pyramid becomes `src`'s, on the device (hsm_copy_map), or with boxes [levels, 4] = x0, y0, x1, y1
        inclusive its cells inside one box per level (hsm_copy_map_boxes); queued, no host wait"""
        if boxes is None:
            _check(self._lib.hsm_copy_map(self._h, src._h), "hsm_copy_map")
            return
        bx = np.ascontiguousarray(boxes, np.int32).reshape(-1)
        if bx.size != 4 * self.getMapLevels():
            raise ValueError("boxes must hold x0, y0, x1, y1 for every level")
        _check(self._lib.hsm_copy_map_boxes(self._h, src._h, bx.ctypes.data), "hsm_copy_map_boxes")

    def align_map_from(self, src, src_level, src_bbox, every, max_points, search_level, guess, step, half, k):
        """`src`'s map aligned to this one on the device (hsm_align_map): the occupied cells of src_bbox (None: the whole level) of
        `src_level`, every `every`-th of them and max_points at most, relocalised on this context in the window (step, half) around
        `guess`.  Synchronous -> (src_in_dst float32 [3], cov float32 [9], likelihood, counts int32 [2], window_index); without a
        winner src_in_dst is the guess, the likelihood NaN, the index -1 and cov zeros."""
        g = np.ascontiguousarray(guess, np.float32).reshape(3)
        st, hf = self._window(step, half)
        bb = None if src_bbox is None else (C.c_int * 4)(*[int(v) for v in src_bbox])
        out, cov = np.empty(3, np.float32), np.zeros(9, np.float32)
        lh, cnt, idx = np.empty(1, np.float32), np.empty(2, np.int32), np.empty(1, np.int32)
        _check(self._lib.hsm_align_map(self._h, src._h, int(src_level), bb, int(every), int(max_points), int(search_level),
                                       g.ctypes.data, st, hf, int(k), out.ctypes.data, cov.ctypes.data, lh.ctypes.data,
                                       cnt.ctypes.data, idx.ctypes.data), "hsm_align_map")
        return out, cov, lh[0], cnt, int(idx[0])

    def map_start(self):
        """the start coordinates the geometry currently derives from (hsm_map_start) -> float32 [2]"""
        out = np.empty(2, np.float32)
        _check(self._lib.hsm_map_start(self._h, out), "hsm_map_start")
        return out

    def start_for_shift(self, kx, ky):
        """the start coordinates that move the window by (kx, ky) cells of the COARSEST level: float32(start + k * 2^(levels-1) / size)"""
        sx, sy, _, _ = self.level_info(0)
        m = 1 << (self.getMapLevels() - 1)
        s = self.map_start().astype(np.float64)
        return np.array([s[0] + kx * m / sx, s[1] + ky * m / sy]).astype(np.float32)

    def shift_map(self, start):
        """the window moves so that the geometry is hsm_create's for `start`; cell contents keep their world position
        (hsm_shift_map); queued, no host wait -> level 0's displacement (dx, dy) in cells"""
        d = np.zeros(2, np.int32)
        _check(self._lib.hsm_shift_map(self._h, float(np.float32(start[0])), float(np.float32(start[1])), d.ctypes.data), "hsm_shift_map")
        return int(d[0]), int(d[1])

    def download_prob(self, level):
        sx, sy, _, _ = self.level_info(level)
        out = np.empty((sy, sx), np.float32)
        _check(self._lib.hsm_download_prob(self._h, level, out.reshape(-1)), "hsm_download_prob")
        return out

    # ---- rows next to the path (ROS-node side) -------------------------------------
    def ingest_laser_scan(self, ranges, angle_min, angle_increment, range_min, range_max, scale_to_map=None):
        """rosLaserScanToDataContainer on the device; returns the (n_valid, 2) endpoints (host copy)."""
        r = np.ascontiguousarray(ranges, np.float32).reshape(-1)
        out = np.empty((r.size, 2), np.float32)
        m = _i()
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_ingest_laser_scan(self._h, r.ctypes.data if r.size else None, r.size, angle_min,
                                               angle_increment, range_min, range_max, s, out.ctypes.data,
                                               C.byref(m)), "hsm_ingest_laser_scan")
        return out[:m.value].copy()

    def ingest_point_cloud(self, pts_xyz, tf_rows, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min,
                           laser_z_max, scale_to_map=None):
        """rosPointCloudToDataContainer on the device; tf_rows = laser->base transform, 12 doubles [R | t]
        row major.  Returns (endpoints (m, 2), origo (2,))."""
        p = np.ascontiguousarray(pts_xyz, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(tf_rows, np.float64).reshape(12)
        out = np.empty((max(p.shape[0], 1), 2), np.float32)
        origo = np.empty(2, np.float32)
        m = _i()
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_ingest_point_cloud(self._h, p.ctypes.data if p.size else None, p.shape[0],
                                                T.ctypes.data, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min,
                                                laser_z_max, s, out.ctypes.data, C.byref(m), origo.ctypes.data),
               "hsm_ingest_point_cloud")
        return out[:m.value].copy(), origo

    def ingest_laser_scan_tf(self, ranges, angle_min, angle_increment, range_min, range_max, range_cutoff, tf_rows,
                             sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map=None):
        """projectLaser + rosPointCloudToDataContainer fused on the device (the node's default path)"""
        r = np.ascontiguousarray(ranges, np.float32).reshape(-1)
        T = np.ascontiguousarray(tf_rows, np.float64).reshape(12)
        out = np.empty((max(r.size, 1), 2), np.float32)
        origo = np.empty(2, np.float32)
        m = _i()
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_ingest_laser_scan_tf(self._h, r.ctypes.data if r.size else None, r.size, angle_min,
                                                  angle_increment, range_min, range_max, range_cutoff, T.ctypes.data,
                                                  sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max,
                                                  s, out.ctypes.data, C.byref(m), origo.ctypes.data),
               "hsm_ingest_laser_scan_tf")
        return out[:m.value].copy(), origo

    def match_ingested(self, beginEstimateWorld, covMatrix=None):
        out = np.empty(3, np.float32)
        cov = np.zeros(9, np.float32) if covMatrix is None else _v(covMatrix, 9).copy()
        _check(self._lib.hsm_match_ingested(self._h, _v(beginEstimateWorld, 3), out, cov), "hsm_match_ingested")
        return out, cov

    def update_by_ingested(self, robotPoseWorld):
        _check(self._lib.hsm_update_by_ingested(self._h, _v(robotPoseWorld, 3)), "hsm_update_by_ingested")

    def likelihood_states(self, level, states_map, pts):
        """OccGridMapUtil::getLikelihoodForState for a batch of map-frame states; pts in level-0 units"""
        st = np.ascontiguousarray(states_map, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        out = np.empty(st.shape[0], np.float32)
        _check(self._lib.hsm_likelihood_states(self._h, level, st.shape[0], st.reshape(-1), p, n, out),
               "hsm_likelihood_states")
        return out

    def residual_states(self, level, states_map, pts):
        """OccGridMapUtil::getResidualForState for a batch of map-frame states"""
        st = np.ascontiguousarray(states_map, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        out = np.empty(st.shape[0], np.float32)
        _check(self._lib.hsm_residual_states(self._h, level, st.shape[0], st.reshape(-1), p, n, out),
               "hsm_residual_states")
        return out

    def covariance_for_poses(self, level, poses_map, pts):
        """OccGridMapUtil::getCovarianceForPose + getCovMatrixWorldCoords for a batch of map-frame poses
        -> (cov_map [B,9], cov_world [B,9], likelihoods [B,7]); matrices column major"""
        st = np.ascontiguousarray(poses_map, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        B = st.shape[0]
        cm, cw, lh = (np.zeros((B, 9), np.float32), np.zeros((B, 9), np.float32), np.zeros((B, 7), np.float32))
        _check(self._lib.hsm_covariance_for_poses(self._h, level, B, st.reshape(-1), p, n, cm.reshape(-1),
                                                  cw.reshape(-1), lh.reshape(-1)), "hsm_covariance_for_poses")
        return cm, cw, lh

    def map_metadata(self, level=0):
        """(origin_x, origin_y, resolution) as HectorMappingRos::setServiceGetMapData publishes them (:546-553)"""
        sx, sy, cell, _ = self.level_info(level)
        w = self.getWorldCoordsPose(level, np.zeros(3, np.float32))  # getWorldCoords(Vector2f::Zero())
        half = np.float32(cell) * np.float32(0.5)
        return float(np.float32(w[0]) - half), float(np.float32(w[1]) - half), float(cell)

    def ray_distances(self, level, begin_world, end_world, origin_xy=None, resolution=None):
        """DistanceMeasurementProvider::getDist for a batch of rays -> (dist[n], hit[n,2]; NaN where no hit)"""
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 2)
        e = np.ascontiguousarray(end_world, np.float32).reshape(-1, 2)
        ox, oy, res = self.map_metadata(level)
        if origin_xy is not None:
            ox, oy = origin_xy
        if resolution is not None:
            res = resolution
        dist = np.empty(b.shape[0], np.float32)
        hit = np.full((b.shape[0], 2), np.nan, np.float32)
        if b.shape[0]:
            _check(self._lib.hsm_ray_distances(self._h, level, ox, oy, res, b.shape[0], b.reshape(-1), e.reshape(-1),
                                               dist, hit.reshape(-1)), "hsm_ray_distances")
        return dist, hit

    def ray_distances_device(self, level, n, d_begin_world, d_end_world, d_out_dist, d_out_hit=0, origin_xy=None, resolution=None,
                             stream=0):
        """Raw device pointers (ints), asynchronous on ``stream``: ``ray_distances`` for ``n`` rays, on the level's own
        metadata unless ``origin_xy`` / ``resolution`` say otherwise."""
        ox, oy, res = self.map_metadata(level)
        if origin_xy is not None:
            ox, oy = origin_xy
        if resolution is not None:
            res = resolution
        _check(self._lib.hsm_ray_distances_device(self._h, level, ox, oy, res, n, d_begin_world or None, d_end_world or None,
                                                  d_out_dist or None, d_out_hit or None, stream or None),
               "hsm_ray_distances_device")

    def cast_scans_device(self, level, batch, d_poses_world, d_beam_angles, n, range_max, d_out_ranges, d_out_hit=0, stream=0):
        """Raw device pointers (ints), asynchronous on ``stream``: the expected range of each of ``n`` beams (angles in the sensor
        frame) from each of ``batch`` sensor poses on ``level``; -resolution where a beam hits nothing."""
        _check(self._lib.hsm_cast_scans_device(self._h, level, batch, d_poses_world or None, d_beam_angles or None, n, range_max,
                                               d_out_ranges or None, d_out_hit or None, stream or None), "hsm_cast_scans_device")

    def cast_scans(self, level, poses_world, beam_angles, range_max):
        """Host arrays: -> (ranges[B, n], hit[B, n, 2]; NaN where no hit)"""
        p = np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(beam_angles, np.float32).reshape(-1)
        B, n = p.shape[0], a.shape[0]
        ranges = np.empty((B, n), np.float32)
        hit = np.full((B, n, 2), np.nan, np.float32)
        if B and n:
            _check(self._lib.hsm_cast_scans(self._h, level, B, _addr(p), _addr(a), n, range_max, _addr(ranges), _addr(hit)),
                   "hsm_cast_scans")
        return ranges, hit

    def occupancy_grid(self, level=0):
        """publishMap's int8 grid: -1 unknown, 0 free, 100 occupied"""
        sx, sy, _, _ = self.level_info(level)
        out = np.empty((sy, sx), np.int8)
        _check(self._lib.hsm_occupancy_grid(self._h, level, out.ctypes.data), "hsm_occupancy_grid")
        return out

    def occupancy_grid_device(self, level, d_out, stream=0):
        """Raw device pointer (int): the whole int8 grid of ``level`` into device memory, queued on the context's stream."""
        _check(self._lib.hsm_occupancy_grid_device(self._h, level, d_out or None, stream or None), "hsm_occupancy_grid_device")

    def occupancy_changes_device(self, level, d_grid, d_out_bbox=0, stream=0):
        """Raw device pointers (ints): the cells of ``level`` that may have changed since its last export, into the caller's
        persistent device grid; ``d_out_bbox`` (int32 [4]) receives the box, 0,0,-1,-1 when nothing changed.  No host wait."""
        _check(self._lib.hsm_occupancy_changes_device(self._h, level, d_grid or None, d_out_bbox or None, stream or None),
               "hsm_occupancy_changes_device")

    def occupancy_changes(self, level, grid):
        """The same into the caller's host grid (int8 [sy, sx], C-contiguous, updated in place) -> the box x0,y0,x1,y1."""
        sx, sy, _, _ = self.level_info(level)
        if not (isinstance(grid, np.ndarray) and grid.dtype == np.int8 and grid.shape == (sy, sx) and grid.flags.c_contiguous
                and grid.flags.writeable):
            raise ValueError("occupancy_changes: grid must be a writeable C-contiguous int8 array of shape (sy, sx)")
        bb = np.empty(4, np.int32)
        _check(self._lib.hsm_occupancy_changes(self._h, level, grid.ctypes.data, bb), "hsm_occupancy_changes")
        return bb

    def occupancy_restart(self, level=-1):
        """the next occupancy_changes* of ``level`` (-1: every level) exports the whole level"""
        _check(self._lib.hsm_occupancy_restart(self._h, level), "hsm_occupancy_restart")

    # ---- known extents, the map image, pose tiles -------------------------------------------
    def map_extents_device(self, level, d_out_box, stream=0):
        """Raw device pointer (int): the inclusive hull x0,y0,x1,y1 of ``level``'s known cells into int32 [4] on the device,
        0,0,-1,-1 without one.  No host wait."""
        _check(self._lib.hsm_map_extents_device(self._h, level, d_out_box or None, stream or None), "hsm_map_extents_device")

    def map_extents(self, level=0, half_open=False):
        """GridMapBase::getMapExtends: int32 [4] x0,y0,x1,y1 inclusive, 0,0,-1,-1 without a known cell.  ``half_open``:
        HectorMapTools::getMapExtends's topLeft / bottomRight, x0,y0,x1+1,y1+1, or None where it returns false."""
        bb = np.empty(4, np.int32)
        _check(self._lib.hsm_map_extents(self._h, level, bb), "hsm_map_extents")
        if not half_open:
            return bb
        return None if bb[2] < bb[0] else bb + np.int32([0, 0, 1, 1])

    def crop_box(self, level, crop=None):
        """``crop`` (x0,y0,x1,y1 inclusive; None: the whole level) clamped to ``level`` as map_image* clamps it, or None where
        it misses the level"""
        sx, sy, _, _ = self.level_info(level)
        if crop is None:
            return 0, 0, sx - 1, sy - 1
        x0, y0, x1, y1 = max(int(crop[0]), 0), max(int(crop[1]), 0), min(int(crop[2]), sx - 1), min(int(crop[3]), sy - 1)
        return None if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)

    def map_image_device(self, level, crop, d_out, stream=0):
        """Raw device pointer (int): the y-flipped byte image (free 255, occupied 0, unknown 127) of ``crop`` clamped to
        ``level`` (``crop_box`` says how large it is) into device memory, queued on the context's stream."""
        c = None if crop is None else np.ascontiguousarray(crop, np.int32).reshape(4)
        _check(self._lib.hsm_map_image_device(self._h, level, None if c is None else c.ctypes.data, d_out or None, stream or None),
               "hsm_map_image_device")

    def map_image(self, level=0, crop=None):
        """map_to_image_node's full image, or that of a cell box: uint8 [hgt, w], row 0 the box's top map row; (0, 0) where the
        crop misses the level"""
        box = self.crop_box(level, crop)
        if box is None:
            return np.zeros((0, 0), np.uint8)
        out = np.empty((box[3] - box[1] + 1, box[2] - box[0] + 1), np.uint8)
        c = np.asarray(box, np.int32)
        _check(self._lib.hsm_map_image(self._h, level, c.ctypes.data, out.ctypes.data), "hsm_map_image")
        return out

    def map_tiles_device(self, level, batch, d_poses_world, tile_w, tile_h, d_out_tiles, d_out_boxes=0, stream=0):
        """Raw device pointers (ints): one ``tile_w`` x ``tile_h`` window of the map image clamped around each of ``batch``
        world poses [batch, 3]; ``d_out_boxes`` (int32 [batch, 4]) receives the windows' inclusive cell boxes.  No host wait."""
        _check(self._lib.hsm_map_tiles_device(self._h, level, batch, d_poses_world or None, tile_w, tile_h, d_out_tiles or None,
                                              d_out_boxes or None, stream or None), "hsm_map_tiles_device")

    def map_tiles(self, level, poses_world, tile_w=64, tile_h=64):
        """Host arrays: -> (tiles uint8 [B, tile_h, tile_w], boxes int32 [B, 4])"""
        p = np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)
        tiles = np.empty((p.shape[0], tile_h, tile_w), np.uint8)
        boxes = np.empty((p.shape[0], 4), np.int32)
        _check(self._lib.hsm_map_tiles(self._h, level, p.shape[0], _addr(p), tile_w, tile_h, _addr(tiles), _addr(boxes)),
               "hsm_map_tiles")
        return tiles, boxes

    # ---- batched extension ---------------------------------------------------------------
    def match_batch(self, begin_world, pts, offsets=None, want_cov=True):
        """Host arrays in/out.  ``offsets`` None = every hypothesis uses the same scan ``pts``."""
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        out = np.empty_like(b)
        cov = np.zeros((b.shape[0], 9), np.float32) if want_cov else None
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        _check(self._lib.hsm_match_batch(self._h, b.shape[0], b.reshape(-1), p,
                                         None if offs is None else offs.ctypes.data,
                                         n if offs is None else 0, out.reshape(-1),
                                         None if cov is None else cov.ctypes.data), "hsm_match_batch")
        return out, cov

    def match_batch_device(self, batch, d_begin, d_pts, d_offsets, shared_n, d_out_pose, d_out_cov, stream=0):
        """Raw device pointers (ints), asynchronous on ``stream`` (a hipStream_t value)."""
        _check(self._lib.hsm_match_batch_device(self._h, batch, d_begin, d_pts, d_offsets or None, shared_n,
                                                d_out_pose, d_out_cov or None, stream or None),
               "hsm_match_batch_device")

    def score_batch_device(self, level, batch, d_poses_world, d_pts, d_offsets, shared_n, d_out_likelihood, d_out_residual=0,
                           stream=0):
        """Raw device pointers (ints), asynchronous on ``stream``: likelihood / residual of ``batch`` WORLD poses on ``level``."""
        _check(self._lib.hsm_score_batch_device(self._h, level, batch, d_poses_world or None, d_pts or None, d_offsets or None,
                                                shared_n, d_out_likelihood or None, d_out_residual or None, stream or None),
               "hsm_score_batch_device")

    def select_best_device(self, groups, d_group_offsets, group_size, d_scores, d_poses_world, d_out_index, d_out_score=0,
                           d_out_pose_world=0, stream=0):
        """Raw device pointers: per group the index of the highest score (NaN never wins, ties -> lowest index, none -> -1)."""
        _check(self._lib.hsm_select_best_device(self._h, groups, d_group_offsets or None, group_size, d_scores or None,
                                                d_poses_world or None, d_out_index or None, d_out_score or None,
                                                d_out_pose_world or None, stream or None), "hsm_select_best_device")

    def match_score_batch_device(self, batch, d_begin, d_pts, d_offsets, shared_n, d_out_pose, d_out_cov, score_level,
                                 d_out_likelihood, d_out_residual=0, groups=0, d_group_offsets=0, group_size=0, d_out_index=0,
                                 d_out_score=0, d_out_best_pose=0, stream=0):
        """match_batch_device -> score_batch_device -> (groups > 0) select_best_device as one call on ``stream``."""
        _check(self._lib.hsm_match_score_batch_device(
            self._h, batch, d_begin or None, d_pts or None, d_offsets or None, shared_n, d_out_pose or None, d_out_cov or None,
            score_level, d_out_likelihood or None, d_out_residual or None, groups, d_group_offsets or None, group_size,
            d_out_index or None, d_out_score or None, d_out_best_pose or None, stream or None), "hsm_match_score_batch_device")

    def covariance_batch_device(self, level, batch, d_poses_world, d_pts, d_offsets, shared_n, d_out_cov_world=0, d_out_cov_map=0,
                                d_out_lh7=0, d_out_likelihood=0, stream=0):
        """Raw device pointers (ints), asynchronous on ``stream``: the sigma-point covariance (world [B,9] / map [B,9], column major),
        the seven sigma-point likelihoods [B,7] and the pose's own likelihood [B] of ``batch`` WORLD poses on ``level``."""
        _check(self._lib.hsm_covariance_batch_device(self._h, level, batch, d_poses_world or None, d_pts or None, d_offsets or None,
                                                     shared_n, d_out_cov_world or None, d_out_cov_map or None, d_out_lh7 or None,
                                                     d_out_likelihood or None, stream or None), "hsm_covariance_batch_device")

    def match_cov_batch_device(self, batch, d_begin, d_pts, d_offsets, shared_n, d_out_pose, d_out_cov, cov_level, d_out_cov_world=0,
                               d_out_cov_map=0, d_out_lh7=0, d_out_likelihood=0, groups=0, d_group_offsets=0, group_size=0,
                               d_out_index=0, d_out_score=0, d_out_best_pose=0, stream=0):
        """match_batch_device -> covariance_batch_device -> (groups > 0) select_best_device as one call on ``stream``."""
        _check(self._lib.hsm_match_cov_batch_device(
            self._h, batch, d_begin or None, d_pts or None, d_offsets or None, shared_n, d_out_pose or None, d_out_cov or None,
            cov_level, d_out_cov_world or None, d_out_cov_map or None, d_out_lh7 or None, d_out_likelihood or None, groups,
            d_group_offsets or None, group_size, d_out_index or None, d_out_score or None, d_out_best_pose or None, stream or None),
            "hsm_match_cov_batch_device")

    def covariance_batch(self, level, poses_world, pts, offsets=None):
        """hsm_covariance_batch: host arrays in and out; ``offsets`` None = every pose against the one scan ``pts``.
        -> (cov_world [B,9], cov_map [B,9], likelihoods [B,7], likelihood [B]); matrices column major"""
        w = np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        B = w.shape[0]
        cw, cm, l7, lh = (np.zeros((B, 9), np.float32), np.zeros((B, 9), np.float32), np.zeros((B, 7), np.float32),
                          np.zeros(B, np.float32))
        _check(self._lib.hsm_covariance_batch(self._h, level, B, w.ctypes.data, p, None if offs is None else offs.ctypes.data,
                                              n if offs is None else 0, cw.ctypes.data, cm.ctypes.data, l7.ctypes.data,
                                              lh.ctypes.data), "hsm_covariance_batch")
        return cw, cm, l7, lh

    def update_by_scans_device(self, count, d_poses_world, d_pts, d_offsets, shared_n, max_beams=0, origo=None, stream=0):
        """Raw device pointers (ints): integrate ``count`` posed scans in order, queued on the context's stream behind what
        ``stream`` holds now.  No host wait, no download: the poses may be a batched matcher's output."""
        o = None if origo is None else _v(origo, 2)
        _check(self._lib.hsm_update_by_scans_device(self._h, count, d_poses_world or None, d_pts or None, d_offsets or None,
                                                    shared_n, max_beams, None if o is None else o.ctypes.data, stream or None),
               "hsm_update_by_scans_device")

    def set_update_gate(self, min_dist, min_angle):
        """thresholds of the device-side movement gate (HectorSlamProcessor.h:62-63: 0.4 / 0.13)"""
        _check(self._lib.hsm_set_update_gate(self._h, float(min_dist), float(min_angle)), "hsm_set_update_gate")

    def reset_update_gate(self):
        _check(self._lib.hsm_reset_update_gate(self._h), "hsm_reset_update_gate")

    def update_gate_state(self):
        """(lastMapUpdatePose [3], updates applied by gated calls since creation); waits for the queued work"""
        pose, total = np.empty(3, np.float32), C.c_longlong(0)
        _check(self._lib.hsm_update_gate_state(self._h, pose, C.byref(total)), "hsm_update_gate_state")
        return pose, int(total.value)

    def update_by_scans_device_gated(self, count, d_poses_world, d_pts, d_offsets, shared_n, max_beams=0, origo=None, d_force=0,
                                     d_out_applied=0, stream=0):
        """``update_by_scans_device`` behind the movement gate of HectorSlamProcessor::update: scan k is integrated where pose k
        differs enough from the last integrated pose, or ``d_force[k]`` (device bytes) is set; ``d_out_applied`` (device int32
        [count]) receives the decisions.  The host waits for nothing."""
        o = None if origo is None else _v(origo, 2)
        _check(self._lib.hsm_update_by_scans_device_gated(self._h, count, d_poses_world or None, d_pts or None, d_offsets or None,
                                                          shared_n, max_beams, None if o is None else o.ctypes.data,
                                                          d_force or None, d_out_applied or None, stream or None),
               "hsm_update_by_scans_device_gated")

    def slam_scans_device(self, count, d_start_pose, d_hint_deltas, d_pts, d_offsets, max_beams, origo, d_force, d_out_pose,
                          d_out_cov=0, d_out_applied=0, stream=0):
        """Raw device pointers (ints): HectorSlamProcessor::update for ``count`` scans in order -- match, gate, update -- queued
        in one call; scan k's hint is scan k-1's pose (+ ``d_hint_deltas[k]``)."""
        o = None if origo is None else _v(origo, 2)
        _check(self._lib.hsm_slam_scans_device(self._h, count, d_start_pose or None, d_hint_deltas or None, d_pts or None,
                                               d_offsets or None, max_beams, None if o is None else o.ctypes.data, d_force or None,
                                               d_out_pose or None, d_out_cov or None, d_out_applied or None, stream or None),
               "hsm_slam_scans_device")

    def update_by_scans_device_origos(self, count, d_poses_world, d_pts, d_offsets, shared_n, max_beams=0, d_origos=0, stream=0):
        """``update_by_scans_device`` with one origo per scan on the device (``d_origos`` float32 [count, 2], 0 = 0,0)."""
        _check(self._lib.hsm_update_by_scans_device_origos(self._h, count, d_poses_world or None, d_pts or None, d_offsets or None,
                                                           shared_n, max_beams, d_origos or None, stream or None),
               "hsm_update_by_scans_device_origos")

    def update_by_scans_device_gated_origos(self, count, d_poses_world, d_pts, d_offsets, shared_n, max_beams=0, d_origos=0,
                                            d_force=0, d_out_applied=0, stream=0):
        """``update_by_scans_device_gated`` with one origo per scan on the device."""
        _check(self._lib.hsm_update_by_scans_device_gated_origos(self._h, count, d_poses_world or None, d_pts or None,
                                                                 d_offsets or None, shared_n, max_beams, d_origos or None,
                                                                 d_force or None, d_out_applied or None, stream or None),
               "hsm_update_by_scans_device_gated_origos")

    def slam_scans_device_origos(self, count, d_start_pose, d_hint_deltas, d_pts, d_offsets, max_beams, d_origos, d_force,
                                 d_out_pose, d_out_cov=0, d_out_applied=0, stream=0):
        """``slam_scans_device`` with one origo per scan on the device: a forced scan's coarse levels integrate the points
        and the origo of the last matched scan, as the reference does."""
        _check(self._lib.hsm_slam_scans_device_origos(self._h, count, d_start_pose or None, d_hint_deltas or None, d_pts or None,
                                                      d_offsets or None, max_beams, d_origos or None, d_force or None,
                                                      d_out_pose or None, d_out_cov or None, d_out_applied or None,
                                                      stream or None), "hsm_slam_scans_device_origos")

    @staticmethod
    def slam_ranges_tf_workspace(count, n):
        """bytes of the workspace of ``slam_ranges_tf_device`` (0 for sizes it refuses); host arithmetic only"""
        return int(load_library().hsm_slam_ranges_tf_workspace(int(count), int(n)))

    def slam_ranges_tf_device(self, count, d_start_pose, d_hint_deltas, d_ranges, n, angle_min, angle_increment, range_min,
                              range_max, range_cutoff, d_tf_rows, shared_tf, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min,
                              laser_z_max, scale_to_map, d_force, d_out_pose, d_out_cov, d_out_applied, d_out_counts, d_workspace,
                              workspace_bytes, stream=0):
        """Raw device pointers (ints): a log of raw scans and a transform per scan through the node's tf conversion and the
        whole HectorSlamProcessor::update loop, queued in one call; the host waits for nothing."""
        _check(self._lib.hsm_slam_ranges_tf_device(
            self._h, count, d_start_pose or None, d_hint_deltas or None, d_ranges or None, n, angle_min, angle_increment, range_min,
            range_max, range_cutoff, d_tf_rows or None, int(bool(shared_tf)), sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min,
            laser_z_max, scale_to_map, d_force or None, d_out_pose or None, d_out_cov or None, d_out_applied or None,
            d_out_counts or None, d_workspace or None, workspace_bytes, stream or None), "hsm_slam_ranges_tf_device")

    def slam_ranges_tf(self, start_pose, hint_deltas, ranges, angle_min, angle_increment, range_min, range_max, range_cutoff,
                       tf_rows, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map=None, force=None,
                       cov=None):
        """Host arrays: ``ranges`` [count, n] and ``tf_rows`` [count, 12] (or [12]: one transform for every scan) through the
        one-call entry -> dict(pose [count, 3], cov [count, 9], applied, counts [count], origo [count, 2]); synchronous.
        ``cov`` presets the covariances (a scan that keeps no beam leaves its row untouched)."""
        r = np.ascontiguousarray(ranges, np.float32)
        if r.ndim != 2:
            raise ValueError("ranges must be [count, n]")
        count, n = r.shape
        T = np.ascontiguousarray(tf_rows, np.float64)
        shared = T.size == 12 and T.ndim == 1
        if not shared and T.shape != (count, 12):
            raise ValueError("tf_rows must be [12] or [count, 12]")
        sp = None if start_pose is None else _v(start_pose, 3)
        dl = None if hint_deltas is None else np.ascontiguousarray(hint_deltas, np.float32).reshape(count, 3)
        fo = None if force is None else np.ascontiguousarray(force, np.uint8).reshape(count)
        out = {"pose": np.empty((count, 3), np.float32),
               "cov": np.zeros((count, 9), np.float32) if cov is None else np.array(cov, np.float32).reshape(count, 9),
               "applied": np.empty(count, np.int32), "counts": np.empty(count, np.int32), "origo": np.empty((count, 2), np.float32)}
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_slam_ranges_tf(
            self._h, count, None if sp is None else sp.ctypes.data, None if dl is None else dl.ctypes.data,
            r.ctypes.data if r.size else None, n, angle_min, angle_increment, range_min, range_max, range_cutoff, T.ctypes.data,
            int(shared), sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, s, None if fo is None else fo.ctypes.data,
            out["pose"].ctypes.data, out["cov"].ctypes.data, out["applied"].ctypes.data, out["counts"].ctypes.data,
            out["origo"].ctypes.data), "hsm_slam_ranges_tf")
        return out

    def update_by_scans(self, poses_world, pts, offsets=None, origo=None):
        """Host arrays: a map from a log of posed scans in one call.  ``offsets`` None = every pose integrates the one scan ``pts``."""
        w = np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        o = None if origo is None else _v(origo, 2)
        _check(self._lib.hsm_update_by_scans(self._h, w.shape[0], w.ctypes.data, p, None if offs is None else offs.ctypes.data,
                                             n if offs is None else 0, None if o is None else o.ctypes.data), "hsm_update_by_scans")

    def score_batch(self, level, poses_world, pts, offsets=None):
        """(likelihood, residual) of WORLD poses on ``level``; ``offsets`` None = every pose against the one scan ``pts``.
        Host arrays in and out, through torch device buffers on the current stream."""
        w = torch.as_tensor(np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)).cuda()
        a, _, n = _pts(pts)
        d_pts = torch.as_tensor(a).cuda()
        d_offs = None if offsets is None else torch.as_tensor(np.ascontiguousarray(offsets, np.int32)).cuda()
        out = torch.empty((2, w.shape[0]), dtype=torch.float32, device="cuda")
        self.score_batch_device(level, w.shape[0], w.data_ptr(), d_pts.data_ptr() if n else 0,
                                0 if d_offs is None else d_offs.data_ptr(), n if d_offs is None else 0, out[0].data_ptr(),
                                out[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
        lh, res = out.cpu().numpy()
        return lh.copy(), res.copy()

    # ---- a window of poses around a DEVICE centre (capi.h "relocalisation"): step = (m, m, rad), half = three half-extents ----
    @staticmethod
    def window_count(half) -> int:
        hx, hy, ht = (int(v) for v in half)
        return 0 if min(hx, hy, ht) < 0 else (2 * hx + 1) * (2 * hy + 1) * (2 * ht + 1)

    @staticmethod
    def _window(step, half):
        return (C.c_float * 3)(*[float(v) for v in step]), (C.c_int * 3)(*[int(v) for v in half])

    @staticmethod
    def select_topk_workspace(count, k) -> int:
        return int(load_library().hsm_select_topk_workspace(int(count), int(k)))

    @staticmethod
    def relocalize_workspace(window_count, k) -> int:
        return int(load_library().hsm_relocalize_workspace(int(window_count), int(k)))

    @staticmethod
    def align_map_workspace(cells, window_count, k, max_points) -> int:
        return int(load_library().hsm_align_map_workspace(int(cells), int(window_count), int(k), int(max_points)))

    # ---- a level's occupied cells as a point set in level-0 units (capi.h "another context's map aligned to this one") ----
    @staticmethod
    def occupied_points_workspace(cells) -> int:
        return int(load_library().hsm_occupied_points_workspace(int(cells)))

    def occupied_points_device(self, level, bbox, every, max_points, d_out_pts, d_out_count, d_workspace, workspace_bytes, stream=0):
        """device pointers as ints; bbox = (x0, y0, x1, y1) inclusive or None for the whole level; asynchronous on ``stream``"""
        bb = None if bbox is None else (C.c_int * 4)(*[int(v) for v in bbox])
        _check(self._lib.hsm_occupied_points_device(self._h, int(level), bb, int(every), int(max_points), d_out_pts or None,
                                                    d_out_count or None, d_workspace or None, workspace_bytes, stream or None),
               "hsm_occupied_points_device")

    def occupied_points(self, level, bbox=None, every=1, max_points=None):
        """host arrays -> (points float32 [count[0], 2], counts int32 [2] = written, kept before the cap); max_points None: the
        level's cell count, which never truncates"""
        if max_points is None:
            sx, sy, _, _ = self.level_info(level)
            max_points = sx * sy
        bb = None if bbox is None else (C.c_int * 4)(*[int(v) for v in bbox])
        pts, cnt = np.empty((max(int(max_points), 0), 2), np.float32), np.zeros(2, np.int32)
        _check(self._lib.hsm_occupied_points(self._h, int(level), bb, int(every), int(max_points),
                                             pts.ctypes.data if pts.size else None, cnt.ctypes.data), "hsm_occupied_points")
        return pts[:cnt[0]], cnt

    def score_window_device(self, level, d_center, step, half, d_pts, n, d_out_likelihood, d_out_residual=0, stream=0):
        """likelihood / residual of the scan at every pose of the window (device pointers as ints; asynchronous on ``stream``)."""
        st, hf = self._window(step, half)
        _check(self._lib.hsm_score_window_device(self._h, level, d_center or None, st, hf, d_pts or None, n,
                                                 d_out_likelihood or None, d_out_residual or None, stream or None),
               "hsm_score_window_device")

    def score_window(self, level, center_world, step, half, pts):
        """host arrays: (likelihood [W], residual [W])"""
        c = np.ascontiguousarray(center_world, np.float32).reshape(3)
        a, p, n = _pts(pts)
        W = self.window_count(half)
        st, hf = self._window(step, half)
        lh, res = np.empty(max(W, 0), np.float32), np.empty(max(W, 0), np.float32)
        _check(self._lib.hsm_score_window(self._h, level, c.ctypes.data, st, hf, p, n, lh.ctypes.data, res.ctypes.data),
               "hsm_score_window")
        return lh, res

    def window_poses_device(self, d_center, step, half, d_index, count, d_out_pose, stream=0):
        st, hf = self._window(step, half)
        _check(self._lib.hsm_window_poses_device(self._h, d_center or None, st, hf, d_index or None, count, d_out_pose or None,
                                                 stream or None), "hsm_window_poses_device")

    def select_topk_device(self, count, d_scores, k, d_out_index, d_out_score, d_workspace, workspace_bytes, stream=0):
        _check(self._lib.hsm_select_topk_device(self._h, count, d_scores or None, k, d_out_index or None, d_out_score or None,
                                                d_workspace or None, workspace_bytes, stream or None), "hsm_select_topk_device")

    def relocalize_device(self, search_level, d_center, step, half, k, d_pts, n, d_workspace, workspace_bytes, d_out_cand_pose,
                          d_out_cand_cov, d_out_cand_likelihood, d_out_best_pose, d_out_best_score, d_out_best_index, stream=0):
        """window score -> top k -> poses -> match -> score on level 0 -> winner, one call on ``stream`` (capi.h)."""
        st, hf = self._window(step, half)
        _check(self._lib.hsm_relocalize_device(
            self._h, search_level, d_center or None, st, hf, k, d_pts or None, n, d_workspace or None, workspace_bytes,
            d_out_cand_pose or None, d_out_cand_cov or None, d_out_cand_likelihood or None, d_out_best_pose or None,
            d_out_best_score or None, d_out_best_index or None, stream or None), "hsm_relocalize_device")

    def relocalize(self, search_level, center_world, step, half, k, pts, want_cov=True):
        """hsm_relocalize: host arrays.  Returns a dict: cand_pose [k,3], cand_cov [k,9] or None, cand_likelihood [k], best_pose [3]
        (NaN without a winner), best_score, best_index (the window index of the winner's start, -1 if none)."""
        c = np.ascontiguousarray(center_world, np.float32).reshape(3)
        a, p, n = _pts(pts)
        st, hf = self._window(step, half)
        r = {"cand_pose": np.empty((k, 3), np.float32), "cand_cov": np.zeros((k, 9), np.float32) if want_cov else None,
             "cand_likelihood": np.empty(k, np.float32), "best_pose": np.full(3, np.nan, np.float32)}
        bs, bi = np.empty(1, np.float32), np.empty(1, np.int32)
        _check(self._lib.hsm_relocalize(self._h, search_level, c.ctypes.data, st, hf, k, p, n, r["cand_pose"].ctypes.data,
                                        r["cand_cov"].ctypes.data if want_cov else None, r["cand_likelihood"].ctypes.data,
                                        r["best_pose"].ctypes.data, bs.ctypes.data, bi.ctypes.data), "hsm_relocalize")
        r.update(best_score=bs[0], best_index=int(bi[0]))
        return r

    # ---- a batch of scans, each in its own window of one shared shape (capi.h "relocalisation of a BATCH of scans") ----
    @staticmethod
    def select_topk_groups_workspace(groups, group_size, k) -> int:
        return int(load_library().hsm_select_topk_groups_workspace(int(groups), int(group_size), int(k)))

    @staticmethod
    def relocalize_batch_workspace(batch, window_count, k, total_points) -> int:
        return int(load_library().hsm_relocalize_batch_workspace(int(batch), int(window_count), int(k), int(total_points)))

    def score_windows_batch_device(self, level, batch, d_centers, step, half, d_pts, d_offsets, shared_n, d_out_likelihood,
                                   d_out_residual=0, stream=0):
        """window b around centre b against scan b (CSR ``d_offsets``, or 0 and one scan of ``shared_n`` beams), one launch (device
        pointers as ints; asynchronous on ``stream``)."""
        st, hf = self._window(step, half)
        _check(self._lib.hsm_score_windows_batch_device(self._h, level, batch, d_centers or None, st, hf, d_pts or None,
                                                        d_offsets or None, shared_n, d_out_likelihood or None,
                                                        d_out_residual or None, stream or None), "hsm_score_windows_batch_device")

    def score_windows_batch(self, level, centers_world, step, half, pts, offsets=None):
        """(likelihood [B, W], residual [B, W]); ``offsets`` None: one scan for every window.  Host arrays in and out, through
        torch device buffers on the current stream, like score_batch."""
        c = torch.as_tensor(np.ascontiguousarray(centers_world, np.float32).reshape(-1, 3)).cuda()
        a, _, n = _pts(pts)
        B, W = c.shape[0], self.window_count(half)
        d_pts = torch.as_tensor(a).cuda()
        d_offs = None if offsets is None else torch.as_tensor(np.ascontiguousarray(offsets, np.int32)).cuda()
        out = torch.empty((2, B, max(W, 0)), dtype=torch.float32, device="cuda")
        self.score_windows_batch_device(level, B, c.data_ptr() if B else 0, step, half, d_pts.data_ptr() if n else 0,
                                        0 if d_offs is None else d_offs.data_ptr(), n if d_offs is None else 0, out[0].data_ptr(),
                                        out[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
        lh, res = out.cpu().numpy()
        return lh.copy(), res.copy()

    def select_topk_groups_device(self, groups, group_size, d_scores, k, d_out_index, d_out_score, d_workspace, workspace_bytes,
                                  stream=0):
        _check(self._lib.hsm_select_topk_groups_device(self._h, groups, group_size, d_scores or None, k, d_out_index or None,
                                                       d_out_score or None, d_workspace or None, workspace_bytes, stream or None),
               "hsm_select_topk_groups_device")

    def relocalize_batch_device(self, search_level, batch, d_centers, step, half, k, d_pts, d_offsets, shared_n, total_points,
                                d_workspace, workspace_bytes, d_out_cand_pose, d_out_cand_cov, d_out_cand_likelihood,
                                d_out_cand_index, d_out_best_pose, d_out_best_score, d_out_best_index, stream=0):
        """hsm_relocalize_device for ``batch`` scans, scan b in the window around centre b, one call on ``stream`` (capi.h)."""
        st, hf = self._window(step, half)
        _check(self._lib.hsm_relocalize_batch_device(
            self._h, search_level, batch, d_centers or None, st, hf, k, d_pts or None, d_offsets or None, shared_n, total_points,
            d_workspace or None, workspace_bytes, d_out_cand_pose or None, d_out_cand_cov or None, d_out_cand_likelihood or None,
            d_out_cand_index or None, d_out_best_pose or None, d_out_best_score or None, d_out_best_index or None,
            stream or None), "hsm_relocalize_batch_device")

    def relocalize_batch(self, search_level, centers_world, step, half, k, pts, offsets=None, want_cov=True):
        """hsm_relocalize_batch: host arrays.  Returns a dict: cand_pose [B,k,3], cand_cov [B,k,9] or None, cand_likelihood [B,k],
        cand_index [B,k], best_pose [B,3] (NaN without a winner), best_score [B], best_index [B] (window indices, -1 if none)."""
        c = np.ascontiguousarray(centers_world, np.float32).reshape(-1, 3)
        B = c.shape[0]
        a, p, n = _pts(pts)
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        st, hf = self._window(step, half)
        r = {"cand_pose": np.empty((B, k, 3), np.float32), "cand_cov": np.zeros((B, k, 9), np.float32) if want_cov else None,
             "cand_likelihood": np.empty((B, k), np.float32), "cand_index": np.empty((B, k), np.int32),
             "best_pose": np.full((B, 3), np.nan, np.float32), "best_score": np.empty(B, np.float32),
             "best_index": np.empty(B, np.int32)}
        _check(self._lib.hsm_relocalize_batch(
            self._h, search_level, B, c.ctypes.data if B else None, st, hf, k, p, None if offs is None else offs.ctypes.data,
            n if offs is None else 0, r["cand_pose"].ctypes.data, r["cand_cov"].ctypes.data if want_cov else None,
            r["cand_likelihood"].ctypes.data, r["cand_index"].ctypes.data, r["best_pose"].ctypes.data,
            r["best_score"].ctypes.data, r["best_index"].ctypes.data), "hsm_relocalize_batch")
        return r

    def match_score_batch(self, begin_world, pts, offsets=None, score_level=0, group_size=None, group_offsets=None, want_cov=True):
        """hsm_match_score_batch: host arrays in/out.  Returns a dict: pose [B,3], cov [B,9] or None, likelihood [B], residual [B],
        and -- with ``group_size`` or ``group_offsets`` -- best_index [G], best_score [G], best_pose [G,3] (NaN where a group
        has no winner)."""
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 3)
        B = b.shape[0]
        a, p, n = _pts(pts)
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        goffs = None if group_offsets is None else np.ascontiguousarray(group_offsets, np.int32)
        G = 0 if group_size is None and goffs is None else (goffs.size - 1 if goffs is not None else (B // group_size if group_size else 0))
        r = {"pose": np.empty_like(b), "cov": np.zeros((B, 9), np.float32) if want_cov else None,
             "likelihood": np.empty(B, np.float32), "residual": np.empty(B, np.float32)}
        if G:
            r.update(best_index=np.empty(G, np.int32), best_score=np.empty(G, np.float32),
                     best_pose=np.full((G, 3), np.nan, np.float32))
        _check(self._lib.hsm_match_score_batch(
            self._h, B, b.ctypes.data, p, None if offs is None else offs.ctypes.data, n if offs is None else 0,
            r["pose"].ctypes.data, r["cov"].ctypes.data if want_cov else None, score_level, r["likelihood"].ctypes.data,
            r["residual"].ctypes.data, G, None if goffs is None else goffs.ctypes.data, group_size or 0,
            r["best_index"].ctypes.data if G else None, r["best_score"].ctypes.data if G else None,
            r["best_pose"].ctypes.data if G else None), "hsm_match_score_batch")
        return r

    def match_batch_ranges(self, begin_world, ranges, angle_min, angle_increment, range_min, range_max, scale_to_map=None,
                           want_cov=True):
        """B raw LaserScans of one geometry (``ranges`` [B, n]) -> (pose [B, 3], cov [B, 9] or None, counts [B]): the node's
        rosLaserScanToDataContainer and matchData per scan, converted and matched on the device.  Host arrays in/out."""
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(ranges, np.float32)
        B = b.shape[0]
        if r.ndim != 2 or r.shape[0] != B:
            raise ValueError("ranges must be [B, n] with B = len(begin_world)")
        n = r.shape[1]
        out = np.empty_like(b)
        cov = np.zeros((B, 9), np.float32) if want_cov else None
        counts = np.empty(B, np.int32)
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_match_batch_ranges(self._h, B, b.ctypes.data, r.ctypes.data if r.size else None, n, angle_min,
                                                angle_increment, range_min, range_max, s, out.ctypes.data,
                                                None if cov is None else cov.ctypes.data, counts.ctypes.data),
               "hsm_match_batch_ranges")
        return out, cov, counts

    def match_batch_ranges_device(self, batch, d_begin, d_ranges, n, angle_min, angle_increment, range_min, range_max,
                                  scale_to_map, d_out_pose, d_out_cov, d_out_counts, d_workspace, workspace_bytes, stream=0):
        """Raw device pointers (ints), asynchronous on ``stream`` (a hipStream_t value); the workspace is the caller's
        (match_batch_ranges_workspace(batch, n) bytes)."""
        _check(self._lib.hsm_match_batch_ranges_device(self._h, batch, d_begin, d_ranges or None, n, angle_min, angle_increment,
                                                       range_min, range_max, scale_to_map, d_out_pose, d_out_cov or None,
                                                       d_out_counts or None, d_workspace, workspace_bytes, stream or None),
               "hsm_match_batch_ranges_device")

    match_batch_ranges_workspace = staticmethod(match_batch_ranges_workspace)

    def ingest_batch_ranges_tf_device(self, batch, d_ranges, n, angle_min, angle_increment, range_min, range_max, range_cutoff,
                                      d_tf_rows, shared_tf, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max,
                                      scale_to_map, d_out_pts, d_out_offsets, d_out_counts, d_out_origo=0, stream=0):
        """Raw device pointers (ints), asynchronous on ``stream``: B raw scans + a laser->base transform per scan (``d_tf_rows``
        [B, 12] doubles, or [12] with ``shared_tf``) through the node's default tf path -> the CSR container of the batched
        entries (``d_out_pts`` [max(B*n, 1), 2], ``d_out_offsets`` [B+1], ``d_out_counts`` [B]) and the origos [B, 2]."""
        _check(self._lib.hsm_ingest_batch_ranges_tf_device(
            self._h, batch, d_ranges or None, n, angle_min, angle_increment, range_min, range_max, range_cutoff, d_tf_rows or None,
            int(bool(shared_tf)), sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map, d_out_pts or None,
            d_out_offsets or None, d_out_counts or None, d_out_origo or None, stream or None), "hsm_ingest_batch_ranges_tf_device")

    def match_batch_ranges_tf(self, begin_world, ranges, angle_min, angle_increment, range_min, range_max, range_cutoff, tf_rows,
                              sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map=None, want_cov=True,
                              cov=None):
        """B raw LaserScans of one geometry (``ranges`` [B, n]) through the node's default tf path (``tf_rows`` [B, 12], or [12]:
        one transform for every scan), then matchData per scan -> (pose [B, 3], cov [B, 9] or None, counts [B], origo [B, 2]).
        Host arrays in/out; ``cov`` presets the covariances (a scan that keeps no beam leaves its row untouched)."""
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(ranges, np.float32)
        B = b.shape[0]
        if r.ndim != 2 or r.shape[0] != B:
            raise ValueError("ranges must be [B, n] with B = len(begin_world)")
        T = np.ascontiguousarray(tf_rows, np.float64)
        shared = T.size == 12 and T.ndim == 1
        if not shared and T.shape != (B, 12):
            raise ValueError("tf_rows must be [12] or [B, 12]")
        n = r.shape[1]
        out = np.empty_like(b)
        if want_cov:
            cov = np.zeros((B, 9), np.float32) if cov is None else np.array(cov, np.float32).reshape(B, 9)
        else:
            cov = None
        counts, origo = np.empty(B, np.int32), np.empty((B, 2), np.float32)
        s = self.getScaleToMap() if scale_to_map is None else scale_to_map
        _check(self._lib.hsm_match_batch_ranges_tf(self._h, B, b.ctypes.data, r.ctypes.data if r.size else None, n, angle_min,
                                                   angle_increment, range_min, range_max, range_cutoff, T.ctypes.data,
                                                   int(shared), sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max,
                                                   s, out.ctypes.data, None if cov is None else cov.ctypes.data,
                                                   counts.ctypes.data, origo.ctypes.data), "hsm_match_batch_ranges_tf")
        return out, cov, counts, origo

    def match_batch_device_gather(self, batch, d_begin, d_pts, d_offsets, shared_n, d_out_pose, d_out_cov, exchange, first_row, lag,
                                  d_out_all, stream=0):
        """match_batch_device + one step of `exchange` (a PoseExchange) in one call; the launch carries the exchange where it can"""
        _check(self._lib.hsm_match_batch_device_gather(self._h, batch, d_begin, d_pts, d_offsets, shared_n, d_out_pose, d_out_cov or None,
                                                       exchange._h, int(first_row), int(lag), d_out_all or None, stream),
               "hsm_match_batch_device_gather")

    def device_info(self):
        a = np.empty(4, np.int32)
        _check(self._lib.hsm_device_info(self._h, a), "hsm_device_info")
        return {"device": int(a[0]), "compute_units": int(a[1]), "clock_khz": int(a[2]), "memory_clock_khz": int(a[3])}

    def set_clock_probe(self, d_stamps4: int):
        """device pointer (int) to four uint64 words, or 0: see hsm_set_clock_probe"""
        _check(self._lib.hsm_set_clock_probe(self._h, d_stamps4 or None), "hsm_set_clock_probe")

    def gn_iterations_per_match(self) -> int:
        return self._lib.hsm_gn_iterations_per_match(self._h)

    def last_launch_config(self):
        cfg = np.empty(5, np.int32)
        _check(self._lib.hsm_last_launch_config(self._h, cfg), "hsm_last_launch_config")
        return {"layout": {1: "quad", 2: "plane"}.get(int(cfg[0]), "?"), "waves_per_scan": int(cfg[1]),
                "block": int(cfg[2]), "grid": int(cfg[3]), "beams_per_lane_in_vgprs": max(int(cfg[4]), 0),
                "texel_cache": bool(cfg[4] < 0), "beams_per_lane": abs(int(cfg[4])),
                "kernel": (self._lib.hsm_last_launch_kernel(self._h) or b"").decode(),
                "parity": {PARITY_EXACT: "exact", PARITY_RELAXED: "relaxed", PARITY_AUTO: "auto"}.get(self.parity(), "fast"),
                "parity_effective": {PARITY_EXACT: "exact", PARITY_RELAXED: "relaxed"}.get(
                    self._lib.hsm_last_launch_parity(self._h), "fast")}

    # ---- parity / debug ---------------------------------------------------------------------
    def hessian_derivs(self, level, pose_map, pts_level):
        a, p, n = _pts(pts_level)
        H = np.empty(9, np.float32)
        d = np.empty(3, np.float32)
        _check(self._lib.hsm_hessian_derivs(self._h, level, _v(pose_map, 3), p, n, H, d), "hsm_hessian_derivs")
        return H.reshape(3, 3).T.copy(), d

    def eval_beams(self, level, pose_map, pts_level):
        a, p, n = _pts(pts_level)
        out = np.empty((n, 4), np.float32)
        _check(self._lib.hsm_eval_beams(self._h, level, _v(pose_map, 3), p, n, out.ctypes.data if n else None),
               "hsm_eval_beams")
        return out

    def debug_sincos(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        s, c = np.empty_like(x), np.empty_like(x)
        _check(self._lib.hsm_debug_sincos(self._h, x.size, x, s, c), "hsm_debug_sincos")
        return s, c

    def debug_expf(self, x):
        """device expf(x) and getGridProbability(x)"""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        e, p = np.empty_like(x), np.empty_like(x)
        _check(self._lib.hsm_debug_expf(self._h, x.size, x, e, p), "hsm_debug_expf")
        return e, p

    def debug_marks_nonzero(self, level):
        """(non-zero words of the dense update's byte map, non-zero words of the end-cell bitmap): both 0 between updates"""
        out = np.zeros(2, np.uint64)
        _check(self._lib.hsm_debug_marks_nonzero(self._h, level, out.ctypes.data), "hsm_debug_marks_nonzero")
        return int(out[0]), int(out[1])

    def debug_set_coop_barrier(self, value):
        _check(self._lib.hsm_debug_set_coop_barrier(self._h, int(value) & 0xffffffff), "hsm_debug_set_coop_barrier")

    def debug_set_coop_mute(self, block_plus_one):
        _check(self._lib.hsm_debug_set_coop_mute(self._h, int(block_plus_one)), "hsm_debug_set_coop_mute")

    def debug_spec_stats(self, enable=True):
        """(boundaries, candidate == carry, shifted, re-run) of the speculative-carry matcher's stitching passes since the last call"""
        out = (C.c_ulonglong * 4)()
        _check(self._lib.hsm_debug_spec_stats(self._h, 1 if enable else 0, C.cast(out, _vp)), "hsm_debug_spec_stats")
        return tuple(int(x) for x in out)

    def debug_coop_fallbacks(self):
        return int(self._lib.hsm_debug_coop_fallbacks(self._h))

    def debug_set_schedule(self, level, gn_steps=1):
        """batched entries run `level` only, with `gn_steps` GN steps (1 + maxIterations); level < 0 restores the schedule"""
        _check(self._lib.hsm_debug_set_schedule(self._h, int(level), int(gn_steps)), "hsm_debug_set_schedule")

    def debug_batch_order(self, batch, d_begin, d_perm_out, stream=0):
        """the batch-order sort alone, raw device pointers (ints), asynchronous on ``stream``: d_perm_out[slot] = scan"""
        _check(self._lib.hsm_debug_batch_order(self._h, int(batch), d_begin, d_perm_out, stream or None), "hsm_debug_batch_order")

    def match_trace(self, begin_world, pts, origo=_ZERO2):
        """matchData with the hook trace: (pose, cov, trace [steps, 12]) -- per GN step the map-frame estimate after the
        step [3] and the H of that step [9], column major (hsm_match_trace)"""
        a, p, n = _pts(pts)
        steps_cap = self.gn_iterations_per_match()
        trace = np.zeros((steps_cap, 12), np.float32)
        out, cov, steps = np.empty(3, np.float32), np.zeros(9, np.float32), C.c_int()
        _check(self._lib.hsm_match_trace(self._h, _v(begin_world, 3), p, n, _v(origo, 2), out, cov, trace.reshape(-1),
                                         steps_cap, C.byref(steps)), "hsm_match_trace")
        return out, cov, trace[:steps.value]

    def match_level(self, level, begin_world, pts_level, max_iter, cov=None):
        a, p, n = _pts(pts_level)
        out = np.empty(3, np.float32)
        c = np.zeros(9, np.float32) if cov is None else _v(cov, 9).copy()
        _check(self._lib.hsm_match_level(self._h, level, _v(begin_world, 3), p, n, max_iter, out, c),
               "hsm_match_level")
        return out, c

    def update_by_scan_level(self, level, pose_world, pts_level, origo_level=_ZERO2):
        a, p, n = _pts(pts_level)
        _check(self._lib.hsm_update_by_scan_level(self._h, level, _v(pose_world, 3), p, n, _v(origo_level, 2)),
               "hsm_update_by_scan_level")

    def build_map(self, poses, scans, origo=_ZERO2):
        """Ground-truth-posed map building on every level (same recipe as the oracle's build_map)."""
        for pose, pts in zip(poses, scans):
            for lvl in range(self.getMapLevels()):
                f = np.float32(1.0 / 2.0 ** lvl)
                self.update_by_scan_level(lvl, pose, np.asarray(pts, np.float32) * f,
                                          np.asarray(origo, np.float32) * f)
            self.onMapUpdated()


class MapRepGroup:
    """single-process multi-GPU group (hsm_group_*): one pyramid replica per listed device"""

    def __init__(self, mapResolution, mapSizeX, mapSizeY, numDepth, devices, startCoords=(0.5, 0.5)):
        self._lib = load_library()
        self._g = _vp()
        dev = np.ascontiguousarray(devices, np.int32)
        _check(self._lib.hsm_group_create(mapResolution, mapSizeX, mapSizeY, numDepth, startCoords[0], startCoords[1],
                                          dev, dev.size, C.byref(self._g)), "hsm_group_create")

    def close(self):
        if getattr(self, "_g", None):
            self._lib.hsm_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return self._lib.hsm_group_size(self._g)

    def member(self, i):
        """borrowed view of replica i (do not close it)"""
        m = MapRepMultiMap.__new__(MapRepMultiMap)
        m._lib = self._lib
        m._h = _vp(self._lib.hsm_group_member(self._g, i))
        m.close = lambda: None
        return m

    def set_update_factors(self, free, occ):
        _check(self._lib.hsm_group_set_update_factors(self._g, free, occ), "hsm_group_set_update_factors")

    def process_scan(self, hint_world, pts, origo=_ZERO2, do_update=True, cov=None):
        a, p, n = _pts(pts)
        out = np.empty(3, np.float32)
        c = np.zeros(9, np.float32) if cov is None else _v(cov, 9).copy()
        _check(self._lib.hsm_group_process_scan(self._g, _v(hint_world, 3), p, n, _v(origo, 2), 1 if do_update else 0,
                                                out, c), "hsm_group_process_scan")
        return out, c

    def match_batch_device(self, counts, d_begin, d_pts, d_offsets, shared_n, root, d_out_pose_all, d_out_cov_all=0):
        """device-resident shards: per-replica lists of raw device pointers (ints); asynchronous (synchronize() waits)"""
        R = self.size()
        cnt = np.ascontiguousarray(counts, np.int32)
        arr = lambda v: (C.c_void_p * R)(*[C.c_void_p(int(x) if x else None) for x in v])
        b, p = arr(d_begin), arr(d_pts)
        o = arr(d_offsets) if d_offsets is not None else None
        _check(self._lib.hsm_group_match_batch_device(self._g, cnt, b, p, o, shared_n, root, d_out_pose_all,
                                                      d_out_cov_all or None), "hsm_group_match_batch_device")

    def synchronize(self):
        _check(self._lib.hsm_group_synchronize(self._g), "hsm_group_synchronize")

    def sync_maps(self, from_, boxes=None):
        """replica `from_`'s pyramid (boxes [levels, 4]: its cells inside one box per level) into every other replica, on the
        device; asynchronous (synchronize() waits)"""
        bx = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1)
        if bx is not None and bx.size != 4 * self.member(0).getMapLevels():
            raise ValueError("boxes must hold x0, y0, x1, y1 for every level")
        _check(self._lib.hsm_group_sync_maps(self._g, from_, None if bx is None else bx.ctypes.data), "hsm_group_sync_maps")

    def set_gather(self, mode: int):
        """GATHER_AUTO / GATHER_DIRECT / GATHER_RCCL / GATHER_PEER for match_batch_device (DIRECT or RCCL asked for explicitly raise
        if unavailable)"""
        _check(self._lib.hsm_group_set_gather(self._g, mode), "hsm_group_set_gather")

    def debug_force_p2p(self, on: bool):
        """test hook: the RCCL gather sends every shard, the root's too, through grouped ncclSend / ncclRecv"""
        _check(self._lib.hsm_group_debug_force_p2p(self._g, 1 if on else 0), "hsm_group_debug_force_p2p")

    def gather_mode(self):
        """("direct" | "rccl" | "peer", note): what match_batch_device gathers with (takes the decision if it is still open)"""
        m = self._lib.hsm_group_gather_mode(self._g)
        return {GATHER_PEER: "peer", GATHER_RCCL: "rccl", GATHER_DIRECT: "direct"}.get(m, "undecided"), self._lib.hsm_group_gather_note(self._g).decode()

    def gathered(self, replica, want_cov=False):
        """device pointer (int, 0 = none) of the all-gathered poses / Hessians replica `replica` holds after a direct / RCCL gather"""
        return int(self._lib.hsm_group_gathered(self._g, replica, 1 if want_cov else 0) or 0)

    def match_batch(self, begin_world, pts, offsets=None, want_cov=True):
        b = np.ascontiguousarray(begin_world, np.float32).reshape(-1, 3)
        a, p, n = _pts(pts)
        out = np.empty_like(b)
        cov = np.zeros((b.shape[0], 9), np.float32) if want_cov else None
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        _check(self._lib.hsm_group_match_batch(self._g, b.shape[0], b.reshape(-1), p,
                                               None if offs is None else offs.ctypes.data, n if offs is None else 0,
                                               out.reshape(-1), None if cov is None else cov.ctypes.data),
               "hsm_group_match_batch")
        return out, cov


class PoseExchange:
    """hsm_exchange_*: this rank's end of the device-side gather of sharded result rows (capi.h; protocol in
    csrc/pose_exchange.h).  `handle()` is what the other processes need (64 bytes, any channel); `connect(handles)` maps their
    mailboxes; inside ONE process `connect_local(list of PoseExchange in rank order)` uses peer access instead."""

    def __init__(self, rank: int, world: int, total_rows: int, cols: int = 3, depth: int = 4, device: int = -1):
        self._lib = load_library()
        h = _vp()
        _check(self._lib.hsm_exchange_create(int(device), int(rank), int(world), int(total_rows), int(cols), int(depth), C.byref(h)),
               "hsm_exchange_create")
        self._h = h
        self.rank, self.world, self.total_rows, self.cols, self.depth = rank, world, total_rows, cols, depth

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hsm_exchange_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def handle(self) -> bytes:
        buf = C.create_string_buffer(EXCHANGE_HANDLE_BYTES)
        _check(self._lib.hsm_exchange_handle(self._h, C.cast(buf, _vp)), "hsm_exchange_handle")
        return buf.raw

    def connect(self, handles):
        """handles: the world x 64-byte IPC handles in rank order (bytes, or a list of bytes)"""
        blob = b"".join(handles) if not isinstance(handles, (bytes, bytearray)) else bytes(handles)
        if len(blob) != self.world * EXCHANGE_HANDLE_BYTES:
            raise ValueError(f"expected {self.world} handles of {EXCHANGE_HANDLE_BYTES} bytes")
        buf = C.create_string_buffer(blob, len(blob))
        _check(self._lib.hsm_exchange_connect(self._h, C.cast(buf, _vp)), "hsm_exchange_connect")

    def connect_local(self, ranks):
        arr = (_vp * self.world)(*[r._h for r in ranks])
        _check(self._lib.hsm_exchange_connect_local(self._h, arr), "hsm_exchange_connect_local")

    def post(self, d_rows: int, first_row: int, n_rows: int, stream: int = 0):
        _check(self._lib.hsm_exchange_post(self._h, d_rows, int(first_row), int(n_rows), stream), "hsm_exchange_post")

    def wait(self, d_out_all: int, stream: int = 0):
        _check(self._lib.hsm_exchange_wait(self._h, d_out_all, stream), "hsm_exchange_wait")

    def post_wait(self, d_rows: int, first_row: int, n_rows: int, lag: int, d_out_all: int, stream: int = 0):
        _check(self._lib.hsm_exchange_post_wait(self._h, d_rows, int(first_row), int(n_rows), int(lag), d_out_all, stream),
               "hsm_exchange_post_wait")

    def epochs(self):
        p, w = C.c_ulonglong(0), C.c_ulonglong(0)
        _check(self._lib.hsm_exchange_epochs(self._h, C.byref(p), C.byref(w)), "hsm_exchange_epochs")
        return p.value, w.value

    def check(self):
        """raises HsmError if a wait timed out (call after synchronising the stream)"""
        _check(self._lib.hsm_exchange_status(self._h), "hsm_exchange_status")

    def memory_kind(self) -> str:
        return self._lib.hsm_exchange_memory_kind(self._h).decode()


def pose_difference_larger_than(p1, p2, dist_thresh, ang_thresh) -> bool:
    """util::poseDifferenceLargerThan (hector_slam_lib/util/UtilFunctions.h:73-92), fp32."""
    p1 = np.asarray(p1, np.float32)
    p2 = np.asarray(p2, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = p1[:2] - p2[:2]
        if np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1])) > np.float32(dist_thresh):
            return True
        ang = np.float32(p1[2] - p2[2])
        if ang > np.pi:
            ang = np.float32(np.float64(ang) - np.pi * 2.0)
        elif ang < -np.pi:
            ang = np.float32(np.float64(ang) + np.pi * 2.0)
        return bool(abs(ang) > np.float32(ang_thresh))


class HectorSlamProcessor:
    """Glue of HectorSlamProcessor::update (slam_main/HectorSlamProcessor.h:71-124) over the
    GPU map representation: match -> threshold test -> updateByScan -> onMapUpdated."""

    def __init__(self, mapResolution, mapSizeX, mapSizeY, startCoords, multi_res_size, **kw):
        self.mapRep = MapRepMultiMap(mapResolution, mapSizeX, mapSizeY, multi_res_size, startCoords, **kw)
        self.lastScanMatchCov = np.zeros(9, np.float32)
        self.reset()
        self.paramMinDistanceDiffForMapUpdate = np.float32(0.4)
        self.paramMinAngleDiffForMapUpdate = np.float32(0.13)

    def reset(self):
        fmax = np.finfo(np.float32).max
        self.lastMapUpdatePose = np.array([fmax, fmax, fmax], np.float32)
        self.lastScanMatchPose = np.zeros(3, np.float32)
        self.mapRep.reset()  # (hsm_reset: the device-side gate goes back to FLT_MAX with it)
        self.mapRep.reset_update_gate()

    def setMapUpdateMinDistDiff(self, v): self.paramMinDistanceDiffForMapUpdate = np.float32(v)
    def setMapUpdateMinAngleDiff(self, v): self.paramMinAngleDiffForMapUpdate = np.float32(v)

    def update_scans_device(self, count, d_start_pose, d_hint_deltas, d_pts, d_offsets, d_out_pose, d_out_cov=0,
                            d_out_applied=0, d_force=0, max_beams=0, origo=None, stream=0):
        """``update()`` for a log of ``count`` scans that are on the device (raw pointers as ints), queued in one call with
        this processor's thresholds: nothing is waited for and nothing comes back to the host -- lastScanMatchPose /
        lastMapUpdatePose of the device-side loop are read with ``device_state()``.  The host-side ``update()`` keeps its own
        lastMapUpdatePose: drive one processor through one of the two."""
        self.mapRep.set_update_gate(self.paramMinDistanceDiffForMapUpdate, self.paramMinAngleDiffForMapUpdate)
        self.mapRep.slam_scans_device(count, d_start_pose, d_hint_deltas, d_pts, d_offsets, max_beams, origo, d_force,
                                      d_out_pose, d_out_cov, d_out_applied, stream)

    def device_state(self):
        """(lastMapUpdatePose, updates applied) of the device-side loop; waits for it"""
        return self.mapRep.update_gate_state()
    def setUpdateFactorFree(self, v): self.mapRep.setUpdateFactorFree(v)
    def setUpdateFactorOccupied(self, v): self.mapRep.setUpdateFactorOccupied(v)
    def getLastScanMatchPose(self): return self.lastScanMatchPose
    def getLastScanMatchCovariance(self): return self.lastScanMatchCov

    def update(self, dataContainer, poseHintWorld, map_without_matching=False, origo=_ZERO2):
        if not map_without_matching:
            new_pose, self.lastScanMatchCov = self.mapRep.matchData(poseHintWorld, dataContainer,
                                                                    self.lastScanMatchCov, origo)
        else:
            new_pose = np.asarray(poseHintWorld, np.float32).copy()
        self.lastScanMatchPose = new_pose
        if pose_difference_larger_than(new_pose, self.lastMapUpdatePose, self.paramMinDistanceDiffForMapUpdate,
                                       self.paramMinAngleDiffForMapUpdate) or map_without_matching:
            self.mapRep.updateByScan(dataContainer, new_pose, origo)
            self.mapRep.onMapUpdated()
            self.lastMapUpdatePose = new_pose.copy()
