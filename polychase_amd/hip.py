"""ctypes binding of the C ABI in include/polychase_hip.h (polychase_amd/lib/libpolychase_hip.so).

Thin and literal: one Python method per C entry point.  There is NO fallback: importing works
without a GPU (so symbol checks can run on CPU), but `Context()` raises when no gfx950 device is
usable, and `load()` raises when the library has not been built.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

PC_MAX_TARGETS = 8
KERNEL_CLASSES = ["gray", "pyramid", "min_eig", "nms", "sort", "suppress", "lk", "compact", "lk_fb", "lk_corr"]
# Classes that Context.timing() lists only once they have launched: with the minimum-correlation check off nothing of it is
# enqueued, and the dictionary of such a context stays the one its readers (bench.py's breakdown, launch-count tests) know.
TIMING_CLASSES_LISTED_ON_USE = ("lk_corr",)

# every symbol include/polychase_hip.h declares (tests check they are all exported)
SYMBOLS = [
    "pc_gftt_default_options", "pc_flow_default_options", "pc_last_error", "pc_version",
    "pc_context_create", "pc_context_destroy", "pc_context_synchronize", "pc_context_stream",
    "pc_runtime_init", "pc_context_set_arithmetic", "pc_context_get_arithmetic", "pc_context_download",
    "pc_gray_default_conversion", "pc_context_set_gray_conversion", "pc_context_get_gray_conversion", "pc_float_transfer_table",
    "pc_gray_quantize_weights", "pc_float_transfer_index",
    "pc_lens_default_model", "pc_lens_build_map", "pc_lens_map_from_stmap", "pc_lens_map_valid", "pc_context_set_lens_map",
    "pc_context_get_lens_map_size",
    "pc_context_enable_timing", "pc_context_get_timing", "pc_context_get_busy_time", "pc_context_reset_timing",
    "pc_debug_lk_profile", "pc_debug_lk_x86_stats", "pc_debug_detection_paths", "pc_debug_llt9", "pc_debug_lm_decide",
    "pc_debug_live_resources",
    "pc_frame_create", "pc_frame_destroy", "pc_frame_set_rgb", "pc_frame_set_rgb_f32", "pc_frame_set_gray", "pc_frame_set_pixels",
    "pc_host_buffer_alloc", "pc_host_buffer_free",
    "pc_frame_num_levels", "pc_frame_level_size", "pc_frame_download_gray", "pc_frame_download_level",
    "pc_frame_download_deriv", "pc_frame_download_level16", "pc_frame_detect", "pc_frame_download_min_eig", "pc_frame_num_candidates",
    "pc_frame_num_keypoints", "pc_frame_download_keypoints", "pc_frame_set_keypoints", "pc_frame_set_mask",
    "pc_frame_set_mask_polygons", "pc_frame_download_mask", "pc_analyzer_set_mask_polygons",
    "pc_frame_download_choked_mask", "pc_lk_track_masked", "pc_analyzer_set_target_mask_margin",
    "pc_lk_track_correlated", "pc_analyzer_set_min_correlation",
    "pc_lk_track_normalized", "pc_analyzer_set_normalize",
    "pc_lk_track_affine", "pc_analyzer_set_affine_refinement",
    "pc_lk_track_search", "pc_analyzer_set_search_radius",
    "pc_lk_track_window_masked", "pc_frame_download_window_weights", "pc_analyzer_set_mask_windows",
    "pc_lk_track", "pc_lk_track_filtered", "pc_lk_track_fb", "pc_lk_track_filtered_fb",
    "pc_analyzer_create", "pc_analyzer_destroy", "pc_analyzer_reset", "pc_analyzer_put_frame", "pc_analyzer_put_frame_f32", "pc_analyzer_put_frame_pixels",
    "pc_analyzer_has_frame", "pc_analyzer_frame_ingested",
    "pc_analyzer_set_keypoints", "pc_analyzer_submit", "pc_analyzer_pending", "pc_analyzer_collect",
    "pc_analyzer_set_device_log", "pc_analyzer_device_log_used", "pc_analyzer_redirect_device_log",
    "pc_analyzer_set_host_records", "pc_analyzer_set_fb_threshold", "pc_analyzer_set_mask",
    "pc_peer_buffer_alloc", "pc_peer_buffer_free", "pc_peer_buffer_export", "pc_peer_buffer_open", "pc_peer_buffer_close",
    "pc_peer_copy_async", "pc_peer_buffer_download",
    "pc_comm_unique_id", "pc_comm_create", "pc_comm_destroy", "pc_comm_world_size", "pc_comm_rank", "pc_comm_all_gather_log",
    "pc_comm_send", "pc_comm_recv",
    "pc_mesh_create", "pc_mesh_set_mask", "pc_mesh_destroy", "pc_raycast_pixels", "pc_raycast_pixels_sweep",
    "pc_mesh_render",
    "pc_corr_set_create", "pc_corr_set_destroy", "pc_corr_set_clear", "pc_corr_set_recycle", "pc_corr_set_append", "pc_corr_set_size",
    "pc_corr_set_download", "pc_pnp_problem_from_set",
    "pc_pnp_problem_create", "pc_pnp_problem_destroy", "pc_pnp_normal_equations", "pc_pnp_normal_equations_cost",
    "pc_pnp_solve", "pc_pnp_total_cost", "pc_track_solve_frame", "pc_track_frame_upload", "pc_track_frame_launch", "pc_track_frame_launch_chained", "pc_corr_set_reserve", "pc_context_pci_bus_id", "pc_track_frame_finish",
    "pc_track_download_points",
    "pc_refine_problem_create", "pc_refine_problem_create_parts", "pc_refine_problem_destroy", "pc_refine_total_cost", "pc_refine_normal_equations", "pc_refine_problem_timing",
]


ARITH_CANONICAL, ARITH_LK_X86_ORDER, ARITH_SOBEL_FMA, ARITH_OPENCV_X86 = 0, 1, 2, 3
ARITH_SOBEL_ROW_FMA = 4   # on top of the others (include/polychase_hip.h: PC_ARITH_SOBEL_ROW_FMA)
# pc_debug_detection_paths (PC_DETECT_PATH_SLOTS counters, in this order)
DETECT_PATH_NAMES = ("finished", "fast_path", "redo_candidates", "redo_keypoints", "redo_overflow_1", "redo_overflow_2",
                     "redo_overflow_4", "redo_forced")
DETECT_PATH_SLOTS = len(DETECT_PATH_NAMES)


class GfttOptions(C.Structure):
    """GFTTOptions (reference cpp/feature_detection/gftt.h:5-21)."""
    _fields_ = [("quality_level", C.c_double), ("min_distance", C.c_double), ("block_size", C.c_int),
                ("gradient_size", C.c_int), ("max_corners", C.c_int), ("use_harris", C.c_int),
                ("harris_k", C.c_double), ("grid_rows", C.c_int), ("grid_cols", C.c_int)]


class FlowOptions(C.Structure):
    """OpticalFlowOptions (reference cpp/opticalflow.h:27-33)."""
    _fields_ = [("window_size", C.c_int), ("max_level", C.c_int), ("term_max_iters", C.c_int),
                ("term_epsilon", C.c_double), ("min_eigen_threshold", C.c_double)]


class GrayConversion(C.Structure):
    """pc_gray_conversion (include/polychase_hip.h)."""
    _fields_ = [("weight_r", C.c_int32), ("weight_g", C.c_int32), ("weight_b", C.c_int32), ("float_table", C.c_void_p)]


class LensModel(C.Structure):
    """pc_lens_model (include/polychase_hip.h)."""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "zoom")]


LENS_FRAC_BITS = 8                            # PC_LENS_FRAC_BITS
LENS_INVALID = -2 ** 31                       # PC_LENS_INVALID
TRANSFER_ENTRIES = 20481                      # PC_TRANSFER_ENTRIES
TRANSFER_KINDS = {"srgb": 1, "gamma": 2}      # PC_TRANSFER_SRGB, PC_TRANSFER_GAMMA
DEFAULT_GRAY_WEIGHTS = (9798, 19235, 3735)


class FrameResult(C.Structure):
    """pc_frame_result (include/polychase_hip.h)."""
    _fields_ = [("frame1", C.c_int32), ("n_keypoints", C.c_int32), ("keypoints_detected", C.c_int32),
                ("keypoints_xy", C.POINTER(C.c_float)), ("n_targets", C.c_int32),
                ("targets", C.c_int32 * 8), ("row_offset", C.c_int64 * 9),
                ("src_indices", C.POINTER(C.c_uint32)), ("tgt_xy", C.POINTER(C.c_float)),
                ("flow_err", C.POINTER(C.c_float))]


_PNP_CAMERA_FIELDS = [("q_xyzw", np.float32, (4,)), ("t", np.float32, (3,)), ("fx", np.float32), ("fy", np.float32), ("cx", np.float32),
                      ("cy", np.float32), ("aspect_ratio", np.float32), ("convention_opencv", np.int32)]
# pc_pnp_camera, pc_pnp_solve_options and pc_lm_debug_state (include/polychase_hip.h) as numpy record types: 4-byte words only
PNP_CAMERA_DTYPE = np.dtype(_PNP_CAMERA_FIELDS)
PNP_SOLVE_OPTIONS_DTYPE = np.dtype(
    [("max_iterations", np.int32), ("initial_lambda", np.float32), ("min_lambda", np.float32), ("max_lambda", np.float32),
     ("gradient_tol", np.float32), ("step_tol", np.float32), ("loss_type", np.int32), ("loss_scale", np.float32),
     ("optimize_focal_length", np.int32), ("optimize_principal_point", np.int32), ("f_low", np.float32), ("f_high", np.float32),
     ("cx_low", np.float32), ("cx_high", np.float32), ("cy_low", np.float32), ("cy_high", np.float32),
     ("max_inlier_error", np.float32), ("rounds_hint", np.int32)])
LM_DEBUG_STATE_DTYPE = np.dtype(
    [("cam", PNP_CAMERA_DTYPE), ("cam_new", PNP_CAMERA_DTYPE), ("R", np.float32, (9,)), ("t", np.float32, (3,)), ("fx", np.float32),
     ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("aspect_ratio", np.float32), ("convention_opencv", np.int32),
     ("sweep_optimize_focal", np.int32), ("sweep_optimize_pp", np.int32), ("JtJ", np.float32, (81,)), ("diag", np.float32, (9,)),
     ("Jtr", np.float32, (9,)), ("step", np.float32, (9,)), ("cost", np.float32), ("initial_cost", np.float32),
     ("lambda", np.float32), ("v", np.float32), ("grad_norm", np.float32), ("step_norm", np.float32), ("iterations", np.int32),
     ("invalid_steps", np.int32), ("rebuild", np.int32), ("phase", np.int32), ("done", np.int32), ("n_valid", np.int32),
     ("status", np.int32), ("optimize_focal", np.int32), ("optimize_pp", np.int32)])
LM_DEBUG_STATE_WORDS = 169                    # PC_LM_DEBUG_STATE_WORDS
assert LM_DEBUG_STATE_DTYPE.itemsize == 4 * LM_DEBUG_STATE_WORDS and PNP_CAMERA_DTYPE.itemsize == 52
LM_DECIDE_WAVE, LM_DECIDE_SERIAL, LM_DECIDE_BARE = 0, 1, 2


class PolychaseHipError(RuntimeError):
    pass


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    path = _build.hip_library_path()
    if not os.path.exists(path):
        raise PolychaseHipError(
            f"{path} is missing: run `python -m polychase_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the hot path.")
    # One HIP runtime per process: torch wheels bundle their own libamdhip64.so (SONAME
    # libamdhip64.so.7, same as /opt/rocm's).  Loading torch FIRST makes our DT_NEEDED entry resolve
    # to the copy torch already mapped; the other order maps two runtimes and the second one finds
    # "no HIP GPUs".  Without torch the library uses /opt/rocm/lib via its RUNPATH.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI
        pass
    L = C.CDLL(path)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.pc_runtime_init.argtypes = [ip, ip]
    L.pc_runtime_init(None, None)   # GPU_MAX_HW_QUEUES before this library's first HIP call (include/polychase_hip.h)
    L.pc_last_error.restype = C.c_char_p
    L.pc_version.restype = C.c_char_p
    L.pc_gftt_default_options.argtypes = [C.POINTER(GfttOptions)]
    L.pc_flow_default_options.argtypes = [C.POINTER(FlowOptions)]
    L.pc_context_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.pc_context_destroy.argtypes = [vp]
    L.pc_context_destroy.restype = None
    L.pc_context_synchronize.argtypes = [vp]
    L.pc_context_stream.argtypes = [vp]
    L.pc_context_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.pc_context_set_arithmetic.argtypes = [vp, C.c_int]
    L.pc_context_get_arithmetic.argtypes = [vp]
    L.pc_gray_default_conversion.argtypes = [C.POINTER(GrayConversion)]
    L.pc_gray_default_conversion.restype = None
    L.pc_context_set_gray_conversion.argtypes = [vp, C.POINTER(GrayConversion)]
    L.pc_context_get_gray_conversion.argtypes = [vp, C.POINTER(GrayConversion), vp]
    L.pc_float_transfer_table.argtypes = [C.c_int, C.c_double, C.c_double, vp]
    L.pc_gray_quantize_weights.argtypes = [C.POINTER(C.c_double), C.POINTER(GrayConversion)]
    L.pc_float_transfer_index.argtypes = [vp, C.c_int, vp]
    L.pc_lens_default_model.argtypes = [C.POINTER(LensModel)]
    L.pc_lens_default_model.restype = None
    L.pc_lens_build_map.argtypes = [C.POINTER(LensModel), C.c_int, C.c_int, vp]
    L.pc_lens_map_from_stmap.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.pc_lens_map_valid.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip]
    L.pc_context_set_lens_map.argtypes = [vp, vp, C.c_int, C.c_int]
    L.pc_context_get_lens_map_size.argtypes = [vp, ip, ip]
    L.pc_context_stream.restype = vp
    L.pc_context_enable_timing.argtypes = [vp, C.c_int]
    L.pc_context_get_timing.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_double)]
    L.pc_context_get_busy_time.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.pc_context_reset_timing.argtypes = [vp]
    L.pc_debug_lk_profile.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.pc_debug_lk_x86_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_ulonglong)]
    L.pc_debug_detection_paths.argtypes = [vp, C.c_int, C.POINTER(C.c_ulonglong)]
    L.pc_debug_llt9.argtypes = [vp, vp, vp, vp, vp, ip]
    L.pc_debug_lm_decide.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.pc_debug_live_resources.argtypes = [C.POINTER(C.c_int * 4)]
    L.pc_frame_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.pc_frame_destroy.argtypes = [vp]
    L.pc_frame_destroy.restype = None
    L.pc_frame_set_rgb.argtypes = [vp, vp, vp, C.c_size_t, C.c_int]
    L.pc_frame_set_gray.argtypes = [vp, vp, vp, C.c_size_t, C.c_int]
    L.pc_frame_set_rgb_f32.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, C.c_int]
    L.pc_frame_set_pixels.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int]
    L.pc_frame_num_levels.argtypes = [vp]
    L.pc_frame_level_size.argtypes = [vp, C.c_int, ip, ip]
    L.pc_frame_download_gray.argtypes = [vp, vp, vp]
    L.pc_frame_download_level.argtypes = [vp, vp, C.c_int, vp]
    L.pc_frame_download_deriv.argtypes = [vp, vp, C.c_int, vp]
    L.pc_frame_download_level16.argtypes = [vp, vp, C.c_int, vp]
    L.pc_host_buffer_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.pc_host_buffer_free.argtypes = [vp]
    L.pc_host_buffer_free.restype = None
    L.pc_frame_detect.argtypes = [vp, vp, C.POINTER(GfttOptions)]
    L.pc_frame_set_mask.argtypes = [vp, vp, vp, C.c_size_t, C.c_int]
    L.pc_frame_set_mask_polygons.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    L.pc_frame_download_mask.argtypes = [vp, vp, vp]
    L.pc_frame_download_choked_mask.argtypes = [vp, vp, C.c_int, vp]
    L.pc_frame_download_min_eig.argtypes = [vp, vp, vp]
    L.pc_frame_num_candidates.argtypes = [vp, vp, ip]
    L.pc_frame_num_keypoints.argtypes = [vp, vp, ip]
    L.pc_frame_download_keypoints.argtypes = [vp, vp, vp, C.c_int]
    L.pc_frame_set_keypoints.argtypes = [vp, vp, vp, C.c_int]
    L.pc_lk_track.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), vp, vp, vp]
    L.pc_lk_track_filtered.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), vp, vp, vp, vp]
    L.pc_lk_track_fb.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_double, vp, vp, vp, vp, vp]
    L.pc_lk_track_filtered_fb.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_double, vp, vp, vp, vp]
    L.pc_lk_track_masked.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_double, C.c_int, vp, vp, vp]
    L.pc_lk_track_correlated.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_double, C.c_double, C.c_int, vp, vp,
                                         vp, vp]
    L.pc_lk_track_normalized.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_int, C.c_double, C.c_double, C.c_int,
                                         vp, vp, vp, vp, vp]
    L.pc_lk_track_affine.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                     vp, vp, vp, vp, vp, vp, vp]
    L.pc_lk_track_search.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                     C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pc_analyzer_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(GfttOptions), C.POINTER(FlowOptions), C.c_int,
                                     C.c_int, C.POINTER(vp)]
    L.pc_analyzer_destroy.argtypes = [vp]
    L.pc_analyzer_destroy.restype = None
    L.pc_analyzer_put_frame.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.c_int, C.c_int]
    L.pc_analyzer_put_frame_f32.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.c_int, C.c_int, C.c_int]
    L.pc_analyzer_put_frame_pixels.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]
    L.pc_analyzer_has_frame.argtypes = [vp, C.c_int32]
    L.pc_analyzer_frame_ingested.argtypes = [vp, C.c_int32]
    L.pc_analyzer_set_keypoints.argtypes = [vp, C.c_int32, vp, C.c_int]
    L.pc_analyzer_submit.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.c_int]
    L.pc_analyzer_pending.argtypes = [vp]
    L.pc_analyzer_collect.argtypes = [vp, C.POINTER(FrameResult)]
    L.pc_analyzer_set_device_log.argtypes = [vp, vp, C.c_size_t]
    L.pc_analyzer_device_log_used.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pc_analyzer_reset.argtypes = [vp]
    L.pc_analyzer_redirect_device_log.argtypes = [vp, vp, C.c_size_t]
    L.pc_analyzer_set_host_records.argtypes = [vp, C.c_int]
    L.pc_analyzer_set_fb_threshold.argtypes = [vp, C.c_double]
    L.pc_analyzer_set_mask.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.pc_analyzer_set_mask_polygons.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    L.pc_analyzer_set_target_mask_margin.argtypes = [vp, C.c_int]
    L.pc_analyzer_set_min_correlation.argtypes = [vp, C.c_double]
    L.pc_analyzer_set_normalize.argtypes = [vp, C.c_int]
    L.pc_analyzer_set_affine_refinement.argtypes = [vp, C.c_int]
    L.pc_analyzer_set_search_radius.argtypes = [vp, C.c_int]
    L.pc_lk_track_window_masked.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.POINTER(FlowOptions), C.c_int, C.c_double, C.c_int,
                                            vp, vp, vp, vp, vp, vp]
    L.pc_frame_download_window_weights.argtypes = [vp, vp, C.c_int, vp]
    L.pc_analyzer_set_mask_windows.argtypes = [vp, C.c_int]
    L.pc_peer_buffer_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(vp)]
    L.pc_peer_buffer_free.argtypes = [C.c_int, vp]
    L.pc_peer_buffer_export.argtypes = [C.c_int, vp, C.c_char_p]
    L.pc_peer_buffer_open.argtypes = [C.c_int, C.c_char_p, C.POINTER(vp)]
    L.pc_peer_buffer_close.argtypes = [C.c_int, vp]
    L.pc_peer_copy_async.argtypes = [C.c_int, vp, vp, C.c_size_t, vp]
    L.pc_peer_buffer_download.argtypes = [C.c_int, vp, vp, C.c_size_t]
    L.pc_comm_unique_id.argtypes = [vp]
    L.pc_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.pc_comm_destroy.argtypes = [vp]
    L.pc_comm_destroy.restype = None
    L.pc_comm_world_size.argtypes = [vp]
    L.pc_comm_rank.argtypes = [vp]
    L.pc_comm_all_gather_log.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pc_comm_send.argtypes = [vp, vp, C.c_uint64, C.c_int]
    L.pc_comm_recv.argtypes = [vp, vp, C.c_uint64, C.c_int]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise PolychaseHipError(f"polychase_hip error {rc}: {load().pc_last_error().decode()}")


def gftt_options(**kw) -> GfttOptions:
    o = GfttOptions()
    load().pc_gftt_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def quantize_channel_weights(weights) -> tuple:
    """user weights (r, g, b) -> the three 15-bit integers of pc_gray_conversion (pc_gray_quantize_weights: the library's own
    quantiser, the one the analysis driver calls); ValueError for what it refuses"""
    w = [float(c) for c in weights]
    if len(w) != 3:
        raise ValueError(f"channel weights must be three values, got {tuple(weights)}")
    c = GrayConversion()
    if load().pc_gray_quantize_weights((C.c_double * 3)(*w), C.byref(c)) != 0:
        raise ValueError(load().pc_last_error().decode())
    return (c.weight_r, c.weight_g, c.weight_b)


def transfer_index(values) -> np.ndarray:
    """table entries of float32 values, by the function the kernels compile, on the host (pc_float_transfer_index)"""
    v = np.ascontiguousarray(values, dtype=np.float32).ravel()
    out = np.empty(len(v), np.uint32)
    _check(load().pc_float_transfer_index(v.ctypes.data, len(v), out.ctypes.data))
    return out.reshape(np.shape(values))


def float_transfer_table(kind: str, gamma: float = 2.2, exposure: float = 0.0) -> np.ndarray:
    """the built-in float transfer table (pc_float_transfer_table): kind "srgb" or "gamma" -> uint8 [TRANSFER_ENTRIES]"""
    if kind not in TRANSFER_KINDS:
        raise ValueError(f"float transfer kind must be one of {sorted(TRANSFER_KINDS)}, got {kind!r}")
    out = np.empty(TRANSFER_ENTRIES, np.uint8)
    _check(load().pc_float_transfer_table(TRANSFER_KINDS[kind], float(gamma), float(exposure), out.ctypes.data))
    return out


def lens_model(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, zoom=1.0) -> LensModel:
    """pc_lens_model of the ORIGINAL frames' camera (include/polychase_hip.h has the polynomial)"""
    return LensModel(*(float(v) for v in (fx, fy, cx, cy, k1, k2, k3, p1, p2, zoom)))


def _lens_map_array(q) -> np.ndarray:
    q = np.asarray(q)
    if q.dtype != np.int32 or q.ndim != 3 or q.shape[2] != 2:
        raise ValueError(f"a lens map is int32 (H, W, 2), got {q.dtype} {q.shape}")
    return np.ascontiguousarray(q)


def lens_build_map(model: LensModel, width: int, height: int) -> np.ndarray:
    """the lens map int32 (H, W, 2) of a polynomial model, on the host (pc_lens_build_map); ValueError for what it refuses"""
    q = np.empty((max(int(height), 0), max(int(width), 0), 2), np.int32)
    if load().pc_lens_build_map(C.byref(model), int(width), int(height), q.ctypes.data) != 0:
        raise ValueError(load().pc_last_error().decode())
    return q


def lens_map_from_stmap(st, flip_v: bool = True) -> np.ndarray:
    """float32 STmap (H, W, 2) in [0, 1] -> lens map int32 (H, W, 2), on the host (pc_lens_map_from_stmap)"""
    st = np.asarray(st)
    if st.dtype != np.float32 or st.ndim != 3 or st.shape[2] != 2:
        raise ValueError(f"an STmap is float32 (H, W, 2), got {st.dtype} {st.shape}")
    st = np.ascontiguousarray(st)
    q = np.empty(st.shape, np.int32)
    if load().pc_lens_map_from_stmap(st.ctypes.data, st.shape[1], st.shape[0], 1 if flip_v else 0, q.ctypes.data) != 0:
        raise ValueError(load().pc_last_error().decode())
    return q


def lens_map_valid(q, erode: int = 0) -> np.ndarray:
    """the validity plane uint8 (H, W), 255 / 0, of a lens map, eroded by `erode` pixels, on the host (pc_lens_map_valid)"""
    q = _lens_map_array(q)
    out = np.empty(q.shape[:2], np.uint8)
    if load().pc_lens_map_valid(q.ctypes.data, q.shape[1], q.shape[0], int(erode), out.ctypes.data, None) != 0:
        raise ValueError(load().pc_last_error().decode())
    return out


def live_resources() -> tuple[int, int, int, int]:
    """(device allocations, pinned allocations, streams, events) the library's objects own in this process right now
    (pc_debug_live_resources)"""
    out = (C.c_int * 4)()
    _check(load().pc_debug_live_resources(C.byref(out)))
    return tuple(out)


def flow_options(**kw) -> FlowOptions:
    o = FlowOptions()
    load().pc_flow_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Context:
    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(load().pc_context_create(device, C.byref(self._h)))

    def close(self):
        if self._h:
            load().pc_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_arithmetic(self, flags: int):
        """ARITH_CANONICAL | ARITH_LK_X86_ORDER | ARITH_SOBEL_FMA | ARITH_SOBEL_ROW_FMA (include/polychase_hip.h: pc_context_set_arithmetic)."""
        _check(load().pc_context_set_arithmetic(self._h, int(flags)))

    @property
    def arithmetic(self) -> int:
        return load().pc_context_get_arithmetic(self._h)

    def set_gray_conversion(self, weights=None, float_table=None):
        """Gray conversion of the RGB frames put from now on (pc_context_set_gray_conversion).  weights: None = the default's
        (9798, 19235, 3735), else three integers 0..32768 with sum 32768 (quantize_channel_weights makes them from user weights);
        float_table: None = the `(x * 255).astype(uint8)` rule, else uint8 [TRANSFER_ENTRIES].  Both None: the default."""
        c = GrayConversion()
        load().pc_gray_default_conversion(C.byref(c))
        if weights is not None:
            c.weight_r, c.weight_g, c.weight_b = (int(v) for v in weights)
        if float_table is not None:
            float_table = np.ascontiguousarray(float_table)
            if float_table.dtype != np.uint8 or float_table.shape != (TRANSFER_ENTRIES,):
                raise ValueError(f"float_table must be uint8 [{TRANSFER_ENTRIES}], got {float_table.dtype} {float_table.shape}")
            c.float_table = float_table.ctypes.data
        _check(load().pc_context_set_gray_conversion(self._h, C.byref(c)))

    def gray_conversion(self):
        """-> ((weight_r, weight_g, weight_b), float table uint8 [TRANSFER_ENTRIES] or None) in force (pc_context_get_gray_conversion)"""
        c = GrayConversion()
        table = np.empty(TRANSFER_ENTRIES, np.uint8)
        _check(load().pc_context_get_gray_conversion(self._h, C.byref(c), table.ctypes.data))
        return (c.weight_r, c.weight_g, c.weight_b), (table if c.float_table else None)

    def set_lens_map(self, q=None):
        """Lens map of the frames put from now on (pc_context_set_lens_map): int32 (H, W, 2), the source position of every
        undistorted pixel in 1 / 256 px (lens_build_map, lens_map_from_stmap); None clears it."""
        if q is None:
            _check(load().pc_context_set_lens_map(self._h, None, 0, 0))
            return
        q = _lens_map_array(q)
        _check(load().pc_context_set_lens_map(self._h, q.ctypes.data, q.shape[1], q.shape[0]))

    def lens_map_size(self) -> tuple:
        """-> (width, height) of the lens map in force, (0, 0) without one (pc_context_get_lens_map_size)"""
        w, h = C.c_int(), C.c_int()
        _check(load().pc_context_get_lens_map_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def synchronize(self):
        _check(load().pc_context_synchronize(self._h))

    @property
    def stream(self) -> int:
        return load().pc_context_stream(self._h)

    def enable_timing(self, classes=True):
        """classes: True = all, False = none, or an iterable of KERNEL_CLASSES names."""
        if classes is True:
            mask = (1 << len(KERNEL_CLASSES)) - 1
        elif not classes:
            mask = 0
        else:
            mask = sum(1 << KERNEL_CLASSES.index(c) for c in classes)
        _check(load().pc_context_enable_timing(self._h, mask))

    def reset_timing(self):
        _check(load().pc_context_reset_timing(self._h))

    def timing(self) -> dict:
        """{class: (launches, total ms)} since reset_timing(); the classes of TIMING_CLASSES_LISTED_ON_USE only with launches"""
        out = {}
        for k, name in enumerate(KERNEL_CLASSES):
            n, ms = C.c_int(), C.c_double()
            _check(load().pc_context_get_timing(self._h, k, C.byref(n), C.byref(ms)))
            if n.value or name not in TIMING_CLASSES_LISTED_ON_USE:
                out[name] = (n.value, ms.value)
        return out

    def lk_profile(self) -> list:
        """per-phase cycle sums of the LK kernel since the last call (zeros unless the library was built with -DPC_LK_PROFILE)"""
        out = (C.c_ulonglong * 16)()
        _check(load().pc_debug_lk_profile(self._h, out))
        return list(out)

    def lk_x86_stats(self, enable: bool = True) -> dict:
        """counters of the x86 summation order on the two-keypoint LK kernel since counting was enabled
        (include/polychase_hip.h: pc_debug_lk_x86_stats); enable=True restarts counting, False stops it"""
        out = (C.c_ulonglong * 4)()
        _check(load().pc_debug_lk_x86_stats(self._h, 1 if enable else 0, out))
        return {"iterations_proven_exact": out[0], "iterations_x86_order": out[1], "keypoint_levels": out[2],
                "keypoint_levels_x86_order": out[3]}

    def detection_paths(self, reset: bool = False) -> dict:
        """how the detections of this context ended since the last reset (include/polychase_hip.h:
        pc_debug_detection_paths): finished, on the fast path, and redone on the slow path per reason"""
        out = (C.c_ulonglong * DETECT_PATH_SLOTS)()
        _check(load().pc_debug_detection_paths(self._h, 1 if reset else 0, out))
        return dict(zip(DETECT_PATH_NAMES, (int(v) for v in out)))

    def llt9(self, a: np.ndarray, b: np.ndarray):
        """the device solver's 9x9 float32 Cholesky + solve -> (L, x, positive_definite)"""
        a = np.ascontiguousarray(a, np.float32).reshape(9, 9)
        b = np.ascontiguousarray(b, np.float32).reshape(9)
        l, x, ok = np.zeros((9, 9), np.float32), np.zeros(9, np.float32), C.c_int()
        _check(load().pc_debug_llt9(self._h, a.ctypes.data, b.ctypes.data, l.ctypes.data, x.ctypes.data, C.byref(ok)))
        return l, x, bool(ok.value)

    def lm_decide(self, mode: int, options: np.ndarray, initial: np.ndarray, sums: np.ndarray, max_rounds: int = 1 << 30):
        """the device solver's decision step on scripted sums (pc_debug_lm_decide): options PNP_SOLVE_OPTIONS_DTYPE [n],
        initial PNP_CAMERA_DTYPE [n], sums float32 [n][rounds][56] -> LM_DEBUG_STATE_DTYPE [n][rounds], the state after each round"""
        options = np.ascontiguousarray(options, PNP_SOLVE_OPTIONS_DTYPE)
        initial = np.ascontiguousarray(initial, PNP_CAMERA_DTYPE)
        sums = np.ascontiguousarray(sums, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 56 or options.shape != (sums.shape[0],) or initial.shape != (sums.shape[0],):
            raise ValueError(f"sums must be [n][rounds][56] with n options and cameras, got {sums.shape}, {options.shape}, {initial.shape}")
        states = np.zeros(sums.shape[:2], LM_DEBUG_STATE_DTYPE)
        _check(load().pc_debug_lm_decide(self._h, int(mode), sums.shape[0], sums.shape[1], int(max_rounds), options.ctypes.data,
                                         initial.ctypes.data, sums.ctypes.data, states.ctypes.data))
        return states

    def busy_ms(self, kernel_class: str) -> float:
        """wall time during which at least one launch of the class was executing (launches may overlap)"""
        ms = C.c_double()
        _check(load().pc_context_get_busy_time(self._h, KERNEL_CLASSES.index(kernel_class), C.byref(ms)))
        return ms.value


def _ptr(a):
    """numpy array (host) or torch tensor (host or device) -> (address, is_device, row_pitch_bytes)."""
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data, 0, a.strides[0]
    # torch tensor
    assert a.is_contiguous()
    if a.is_cuda:
        # the library enqueues on its own HIP stream: the tensor must be complete before it is read
        import torch
        torch.cuda.current_stream(a.device).synchronize()
    return a.data_ptr(), 1 if a.is_cuda else 0, a.stride(0) * a.element_size()


def _mask_ptr(mask, w: int, h: int):
    """detection mask -> (address, is_device, row_pitch_bytes): uint8 (H, W), numpy (rows may be strided: a view of a wider
    array) or a torch tensor, host or device, whose rows are contiguous (they too may lie a pitch >= W apart).  ValueError for
    anything else (the reference CHECKs CV_8UC1 and the image's size)."""
    if str(mask.dtype) not in ("uint8", "torch.uint8"):
        raise ValueError(f"detection mask must be uint8, got {mask.dtype}")
    if tuple(mask.shape) != (h, w):
        raise ValueError(f"detection mask must have shape {(h, w)}, got {tuple(mask.shape)}")
    if isinstance(mask, np.ndarray):
        if w > 1 and mask.strides[1] != 1 or (h > 1 and mask.strides[0] < w):
            mask = np.ascontiguousarray(mask)
        return mask, mask.ctypes.data, 0, (mask.strides[0] if h > 1 else w)
    if (w > 1 and mask.stride(1) != 1) or (h > 1 and mask.stride(0) < w):
        raise ValueError(f"detection mask tensor must have contiguous rows at least {w} bytes apart, got strides {tuple(mask.stride())}")
    if mask.is_cuda:
        # the library enqueues on its own HIP stream: the tensor must be complete before it is read
        import torch
        torch.cuda.current_stream(mask.device).synchronize()
    return mask, mask.data_ptr(), 1 if mask.is_cuda else 0, (mask.stride(0) if h > 1 else w)


MASK_MAX_POLYGONS, MASK_MAX_VERTICES, MASK_SUBPIXEL = 32, 4096, 16   # PC_MASK_* of include/polychase_hip.h
TARGET_MASK_MAX_MARGIN = 31   # PC_TARGET_MASK_MAX_MARGIN


def _polygon_arrays(polys):
    """polygons (a sequence of (K, 2) array-likes) -> (xy float32 (sum K, 2), counts int32): the arguments of
    pc_frame_set_mask_polygons.  ValueError for a wrong shape; everything else is the library's to refuse."""
    polys = [np.asarray(p, dtype=np.float32) for p in polys]
    for p in polys:
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"a polygon must have shape (K, 2), got {p.shape}")
    xy = np.ascontiguousarray(np.concatenate(polys, axis=0) if polys else np.zeros((0, 2), np.float32))
    return xy, np.array([len(p) for p in polys], np.int32)


def _is_float32(a) -> bool:
    return str(a.dtype) in ("float32", "torch.float32")


PIXEL_U8, PIXEL_U16, PIXEL_F16, PIXEL_F32 = 0, 1, 2, 3   # pc_pixel_type of include/polychase_hip.h
_PIXEL_TYPES = {"uint8": PIXEL_U8, "uint16": PIXEL_U16, "float16": PIXEL_F16, "float32": PIXEL_F32}
_PIXEL_CHANNELS = {PIXEL_U8: (1, 3, 4), PIXEL_U16: (3, 4), PIXEL_F16: (3, 4), PIXEL_F32: (3, 4)}
ACCEPTED_FRAMES = "uint8 (H, W, 3|4), uint16 (H, W, 3|4), float16 (H, W, 3|4) or float32 (H, W, 3|4)"


def pixel_type_of(a) -> int:
    """the pc_pixel_type of a numpy array's or a torch tensor's dtype; ValueError for a dtype the library does not take"""
    name = str(a.dtype).replace("torch.", "")
    if name not in _PIXEL_TYPES:
        raise ValueError(f"a frame must be {ACCEPTED_FRAMES}, got dtype {a.dtype}")
    return _PIXEL_TYPES[name]


def _pixels_args(img, w: int, h: int):
    """frame of any accepted type -> (address, row_pitch_bytes, pixel_type, channels, on_device); uint8 (H, W) is a gray frame.
    ValueError for any other dtype or shape."""
    ptype = pixel_type_of(img)
    shape = tuple(img.shape)
    channels = 1 if len(shape) == 2 else (shape[2] if len(shape) == 3 else 0)
    if shape[:2] != (h, w) or channels not in _PIXEL_CHANNELS[ptype]:
        raise ValueError(f"a {w} x {h} frame must be {ACCEPTED_FRAMES}, got {img.dtype} {shape}")
    p, dev, pitch = _ptr(img)
    return p, pitch, ptype, int(channels), dev


class Frame:
    """Gray image + LK pyramid + keypoints of one video frame, resident in HBM."""

    def __init__(self, ctx: Context, width: int, height: int, window_size: int = 10, max_level: int = 3):
        self.ctx, self.w, self.h, self.win = ctx, width, height, window_size
        self._h = C.c_void_p()
        _check(load().pc_frame_create(ctx._h, width, height, window_size, max_level, C.byref(self._h)))

    def close(self):
        if self._h and self.ctx._h:
            load().pc_frame_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rgb(self, rgb):
        """uint8 (H, W, 3), or float32 (H, W, 3|4) as Blender hands frames out (converted on the GPU)."""
        p, dev, pitch = _ptr(rgb)
        if _is_float32(rgb):
            assert tuple(rgb.shape[:2]) == (self.h, self.w) and len(rgb.shape) == 3, rgb.shape
            _check(load().pc_frame_set_rgb_f32(self.ctx._h, self._h, p, pitch, int(rgb.shape[2]), dev))
        else:
            assert tuple(rgb.shape) == (self.h, self.w, 3), rgb.shape
            _check(load().pc_frame_set_rgb(self.ctx._h, self._h, p, pitch, dev))
        self._keep = rgb  # device sources must outlive the async kernels

    def set_pixels(self, img):
        """A frame of any type the library takes (pc_frame_set_pixels): uint8 (H, W, 3|4) or (H, W), uint16, float16 or float32
        (H, W, 3|4); numpy, or a torch tensor on the host or the device.  Every channel becomes a byte on the GPU by the rule of
        its type; the planes stay 8-bit."""
        p, pitch, ptype, channels, dev = _pixels_args(img, self.w, self.h)
        _check(load().pc_frame_set_pixels(self.ctx._h, self._h, p, pitch, ptype, channels, dev))
        self._keep = img  # device sources must outlive the async kernels

    def set_gray(self, gray):
        assert tuple(gray.shape) == (self.h, self.w), gray.shape
        p, dev, pitch = _ptr(gray)
        _check(load().pc_frame_set_gray(self.ctx._h, self._h, p, pitch, dev))
        self._keep = gray

    @property
    def num_levels(self) -> int:
        return load().pc_frame_num_levels(self._h)

    def level_size(self, level: int):
        w, h = C.c_int(), C.c_int()
        _check(load().pc_frame_level_size(self._h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def gray(self) -> np.ndarray:
        out = np.empty((self.h, self.w), np.uint8)
        _check(load().pc_frame_download_gray(self.ctx._h, self._h, out.ctypes.data))
        return out

    def level(self, l: int) -> np.ndarray:
        w, h = self.level_size(l)
        out = np.empty((h + 2 * self.win, w + 2 * self.win), np.uint8)
        _check(load().pc_frame_download_level(self.ctx._h, self._h, l, out.ctypes.data))
        return out

    def deriv(self, l: int) -> np.ndarray:
        w, h = self.level_size(l)
        out = np.empty((h + 2 * self.win, w + 2 * self.win, 2), np.int16)
        _check(load().pc_frame_download_deriv(self.ctx._h, self._h, l, out.ctypes.data))
        return out

    def level16(self, l: int) -> np.ndarray:
        """the uint16 plane the LK kernels read (pixel << 7), padded like level()"""
        w, h = self.level_size(l)
        out = np.empty((h + 2 * self.win, w + 2 * self.win), np.uint16)
        _check(load().pc_frame_download_level16(self.ctx._h, self._h, l, out.ctypes.data))
        return out

    def set_mask(self, mask):
        """Detection mask of the next detect() (pc_frame_set_mask): uint8 (H, W), non-zero = detect here; None clears it."""
        if mask is None:
            _check(load().pc_frame_set_mask(self.ctx._h, self._h, None, 0, 0))
            self._keep_mask = None
            return
        keep, p, dev, pitch = _mask_ptr(mask, self.w, self.h)
        _check(load().pc_frame_set_mask(self.ctx._h, self._h, p, pitch, dev))
        self._keep_mask = keep if dev else None   # a device mask is read stream-ordered

    def set_mask_polygons(self, polys, invert: bool = False):
        """Detection mask of the next detect() as closed polygons, rasterised on the GPU (pc_frame_set_mask_polygons has the
        fill rule): a sequence of (K, 2) float32 array-likes in pixel coordinates; [] = everything off (on with invert)."""
        xy, counts = _polygon_arrays(polys)
        _check(load().pc_frame_set_mask_polygons(self.ctx._h, self._h, xy.ctypes.data, counts.ctypes.data, len(counts), int(bool(invert))))
        self._keep_mask = None

    def mask(self) -> np.ndarray:
        """The mask plane in force, uint8 (H, W) (pc_frame_download_mask); an error when the frame has no mask on."""
        out = np.empty((self.h, self.w), np.uint8)
        _check(load().pc_frame_download_mask(self.ctx._h, self._h, out.ctypes.data))
        return out

    def choked_mask(self, margin: int) -> np.ndarray:
        """The choked plane of the mask in force, uint8 (H, W), 255 / 0: on where every pixel of the frame within `margin` in
        both axes is on (pc_frame_download_choked_mask); margin 0..31."""
        out = np.empty((self.h, self.w), np.uint8)
        _check(load().pc_frame_download_choked_mask(self.ctx._h, self._h, int(margin), out.ctypes.data))
        return out

    def window_weights(self, level: int) -> np.ndarray:
        """The weight plane of pyramid level `level` under the mask in force, with its padding: uint8 (h_l + 2 win, w_l + 2 win),
        255 / 0 (pc_frame_download_window_weights; include/polychase_hip.h: pc_lk_track_window_masked has the rule)."""
        w, h = self.level_size(level)
        out = np.empty((h + 2 * self.win, w + 2 * self.win), np.uint8)
        _check(load().pc_frame_download_window_weights(self.ctx._h, self._h, int(level), out.ctypes.data))
        return out

    def detect(self, opt: GfttOptions | None = None):
        opt = opt or gftt_options()
        _check(load().pc_frame_detect(self.ctx._h, self._h, C.byref(opt)))

    def min_eig(self) -> np.ndarray:
        out = np.empty((self.h, self.w), np.float32)
        _check(load().pc_frame_download_min_eig(self.ctx._h, self._h, out.ctypes.data))
        return out

    @property
    def num_candidates(self) -> int:
        n = C.c_int()
        _check(load().pc_frame_num_candidates(self.ctx._h, self._h, C.byref(n)))
        return n.value

    @property
    def num_keypoints(self) -> int:
        n = C.c_int()
        _check(load().pc_frame_num_keypoints(self.ctx._h, self._h, C.byref(n)))
        return n.value

    def keypoints(self) -> np.ndarray:
        n = self.num_keypoints
        out = np.empty((n, 2), np.float32)
        _check(load().pc_frame_download_keypoints(self.ctx._h, self._h, out.ctypes.data, n))
        return out

    def set_keypoints(self, xy: np.ndarray):
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        _check(load().pc_frame_set_keypoints(self.ctx._h, self._h, xy.ctypes.data, len(xy)))


# the [T,N,...] output arrays of the pc_lk_track* calls: trailing shape and type by name
_LK_OUT = {"xy": ((2,), np.float32), "st": ((), np.uint8), "err": ((), np.float32), "bxy": ((2,), np.float32), "bst": ((), np.uint8),
           "corr": ((), np.float32), "am": ((4,), np.float32), "ast": ((), np.uint8), "sd": ((2,), np.int16), "sst": ((), np.uint8)}


def _target_handles(targets):
    return (C.c_void_p * len(targets))(*[f._h for f in targets])


def _lk_call(symbol: str, ctx: Context, frame1: Frame, targets: list[Frame], opt, options: tuple, names: tuple):
    """One pc_lk_track* call: `options` follow the flow options, then the zeroed output arrays `names` (None: a null pointer).
    -> the arrays as a tuple, None where the name is."""
    opt = opt or flow_options()
    n, t = frame1.num_keypoints, len(targets)
    out = tuple(None if k is None else np.zeros((t, n) + _LK_OUT[k][0], _LK_OUT[k][1]) for k in names)
    _check(getattr(load(), symbol)(ctx._h, frame1._h, _target_handles(targets), t, C.byref(opt), *options,
                                   *[None if a is None else a.ctypes.data for a in out]))
    return out


def _lk_call_filtered(symbol: str, ctx: Context, frame1: Frame, targets: list[Frame], opt, options: tuple):
    """One pc_lk_track_filtered* call -> per target (src_indices u32 [M], tgt_xy f32 [M,2], err f32 [M])."""
    opt = opt or flow_options()
    n, t = frame1.num_keypoints, len(targets)
    rows = max(1, n * t)
    idx = np.zeros(rows, np.uint32)
    xy = np.zeros((rows, 2), np.float32)
    err = np.zeros(rows, np.float32)
    off = np.zeros(t + 1, np.int64)
    _check(getattr(load(), symbol)(ctx._h, frame1._h, _target_handles(targets), t, C.byref(opt), *options, idx.ctypes.data, xy.ctypes.data,
                                   err.ctypes.data, off.ctypes.data))
    return [(idx[a:b].copy(), xy[a:b].copy(), err[a:b].copy()) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def lk_track(ctx: Context, frame1: Frame, targets: list[Frame], opt: FlowOptions | None = None):
    """Raw LK outputs: next_xy [T,N,2], status [T,N], err [T,N]."""
    return _lk_call("pc_lk_track", ctx, frame1, targets, opt, (), ("xy", "st", "err"))


def lk_track_filtered(ctx: Context, frame1: Frame, targets: list[Frame], opt: FlowOptions | None = None):
    """status==1 rows per target: list of (src_indices u32 [M], tgt_xy f32 [M,2], err f32 [M])."""
    return _lk_call_filtered("pc_lk_track_filtered", ctx, frame1, targets, opt, ())


def lk_track_fb(ctx: Context, frame1: Frame, targets: list[Frame], fb_threshold: float, opt: FlowOptions | None = None):
    """lk_track with the forward-backward check (include/polychase_hip.h: pc_lk_track_fb): next_xy [T,N,2], final status
    [T,N], err [T,N], back_xy [T,N,2], back_status [T,N].  fb_threshold == 0: lk_track and zeros."""
    return _lk_call("pc_lk_track_fb", ctx, frame1, targets, opt, (float(fb_threshold),), ("xy", "st", "err", "bxy", "bst"))


def lk_track_masked(ctx: Context, frame1: Frame, targets: list[Frame], fb_threshold: float, margin: int, opt: FlowOptions | None = None):
    """lk_track_fb without the back outputs, plus the target-side mask test (include/polychase_hip.h: pc_lk_track_masked): a row
    whose end point lies where the choked mask of its target is off gets status 0; a target without a mask keeps its rows.
    margin -1: lk_track_fb.  -> next_xy [T,N,2], final status [T,N], err [T,N]."""
    return _lk_call("pc_lk_track_masked", ctx, frame1, targets, opt, (float(fb_threshold), int(margin)), ("xy", "st", "err"))


def lk_track_correlated(ctx: Context, frame1: Frame, targets: list[Frame], min_correlation: float, fb_threshold: float = 0.0,
                        margin: int = -1, opt: FlowOptions | None = None, corr: bool = True):
    """lk_track_masked plus the minimum-correlation check (include/polychase_hip.h: pc_lk_track_correlated): a row whose reference
    and matched windows correlate below min_correlation gets status 0; 0 = no filter.  corr=True also returns the scores (0 where
    the record reached the pass with status 0); corr=False with min_correlation 0 is lk_track_masked.
    -> next_xy [T,N,2], final status [T,N], err [T,N], corr [T,N] or None."""
    return _lk_call("pc_lk_track_correlated", ctx, frame1, targets, opt, (float(min_correlation), float(fb_threshold), int(margin)),
                    ("xy", "st", "err", "corr" if corr else None))


def lk_track_normalized(ctx: Context, frame1: Frame, targets: list[Frame], normalize: int = 1, min_correlation: float = 0.0,
                        fb_threshold: float = 0.0, margin: int = -1, opt: FlowOptions | None = None):
    """brightness-normalised LK (include/polychase_hip.h: pc_lk_track_normalized): with normalize 1 the forward launch, and the
    backward launch where fb_threshold > 0, track g (J - mean J) against (I - mean I); with 0 it is lk_track_correlated without
    scores plus the back outputs of lk_track_fb.
    -> next_xy [T,N,2], final status [T,N], err [T,N], back_xy [T,N,2], back_status [T,N]."""
    return _lk_call("pc_lk_track_normalized", ctx, frame1, targets, opt,
                    (int(normalize), float(min_correlation), float(fb_threshold), int(margin)), ("xy", "st", "err", "bxy", "bst"))


def lk_track_affine(ctx: Context, frame1: Frame, targets: list[Frame], affine: int = 1, normalize: int = 0, min_correlation: float = 0.0,
                    fb_threshold: float = 0.0, margin: int = -1, opt: FlowOptions | None = None):
    """affine refinement of the forward rows (include/polychase_hip.h: pc_lk_track_affine): with affine 1 one more launch directly
    after the forward one refines every end point at level 0 under a 6-parameter warp of the window, and the checks judge the
    refined rows; with 0 it is lk_track_normalized.  affine 1 with normalize 1 is refused.
    -> next_xy [T,N,2], final status [T,N], err [T,N], back_xy [T,N,2], back_status [T,N], affine_m [T,N,4] (m11, m12, m21, m22),
    affine_state [T,N] (0 not run, 1 accepted, 2 left unchanged)."""
    return _lk_call("pc_lk_track_affine", ctx, frame1, targets, opt,
                    (int(affine), int(normalize), float(min_correlation), float(fb_threshold), int(margin)),
                    ("xy", "st", "err", "bxy", "bst", "am", "ast"))


def lk_track_search(ctx: Context, frame1: Frame, targets: list[Frame], search_radius: int, affine: int = 0, normalize: int = 0,
                    min_correlation: float = 0.0, fb_threshold: float = 0.0, margin: int = -1, opt: FlowOptions | None = None):
    """search prepass of the forward rows (include/polychase_hip.h: pc_lk_track_search): with search_radius 1..256 one more launch
    directly after the forward one finds an integer displacement per (keypoint, target) pair by block matching, runs LK once more
    from it and keeps the record with the smaller patch error; with 0 it is lk_track_affine.  A radius with normalize 1 is refused.
    -> next_xy [T,N,2], final status [T,N], err [T,N], back_xy [T,N,2], back_status [T,N], affine_m [T,N,4], affine_state [T,N],
    search_d [T,N,2] int16 (level-0 pixels), search_state [T,N] (0 no displacement, 1 record replaced, 2 record kept)."""
    return _lk_call("pc_lk_track_search", ctx, frame1, targets, opt,
                    (int(search_radius), int(affine), int(normalize), float(min_correlation), float(fb_threshold), int(margin)),
                    ("xy", "st", "err", "bxy", "bst", "am", "ast", "sd", "sst"))


def lk_track_window_masked(ctx: Context, frame1: Frame, targets: list[Frame], mask_windows: int = 1, fb_threshold: float = 0.0,
                           margin: int = -1, opt: FlowOptions | None = None):
    """masked windows (include/polychase_hip.h: pc_lk_track_window_masked): with mask_windows 1 the template pixels outside the
    mask of frame1 -- and, in the backward pass, of a masked target -- carry no weight; with 0 it is lk_track_masked plus the back
    outputs of lk_track_fb.
    -> next_xy [T,N,2], final status [T,N], err [T,N], back_xy [T,N,2], back_status [T,N], touched [N] (1: the keypoint's window
    has an off sample at some level, and its rows were tracked under the rule)."""
    opt = opt or flow_options()
    n, t = frame1.num_keypoints, len(targets)
    out = tuple(np.zeros((t, n) + _LK_OUT[k][0], _LK_OUT[k][1]) for k in ("xy", "st", "err", "bxy", "bst")) + (np.zeros(n, np.uint8),)
    _check(load().pc_lk_track_window_masked(ctx._h, frame1._h, _target_handles(targets), t, C.byref(opt), int(mask_windows),
                                            float(fb_threshold), int(margin), *[a.ctypes.data for a in out]))
    return out


def lk_track_filtered_fb(ctx: Context, frame1: Frame, targets: list[Frame], fb_threshold: float, opt: FlowOptions | None = None):
    """lk_track_filtered on the final status of the forward-backward check (pc_lk_track_filtered_fb)."""
    return _lk_call_filtered("pc_lk_track_filtered_fb", ctx, frame1, targets, opt, (float(fb_threshold),))


class Analyzer:
    """pc_analyzer: pipelined per-clip engine (ring of resident frames + asynchronous frame1 jobs)."""

    def __init__(self, ctx: Context, width: int, height: int, gftt: GfttOptions | None = None,
                 flow: FlowOptions | None = None, ring_frames: int = 17, max_jobs: int = 3):
        self.ctx, self.w, self.h = ctx, width, height
        self.gftt = gftt or gftt_options()
        self.flow = flow or flow_options()
        self._h = C.c_void_p()
        self._keep = {}
        self._keep_mask, self._keep_masks = None, {}   # the device mask in force / per ring slot, of the frame put under it
        self._target_margin = -1
        _check(load().pc_analyzer_create(ctx._h, width, height, C.byref(self.gftt), C.byref(self.flow), ring_frames,
                                         max_jobs, C.byref(self._h)))
        self.ring = ring_frames

    def close(self):
        if self._h and self.ctx._h:
            load().pc_analyzer_destroy(self._h)
        self._h = C.c_void_p()
        self._keep = {}
        self._keep_mask, self._keep_masks = None, {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """No resident frame, no job, no log, no mask; allocations kept (pc_analyzer_reset)."""
        _check(load().pc_analyzer_reset(self._h))
        self._keep = {}
        self._keep_mask, self._keep_masks = None, {}

    def put_frame(self, frame_id: int, rgb, will_detect: bool = True):
        p, dev, pitch = _ptr(rgb)
        if _is_float32(rgb):
            assert tuple(rgb.shape[:2]) == (self.h, self.w) and len(rgb.shape) == 3, rgb.shape
            _check(load().pc_analyzer_put_frame_f32(self._h, frame_id, p, pitch, int(rgb.shape[2]), dev,
                                                    1 if will_detect else 0))
        else:
            assert tuple(rgb.shape) == (self.h, self.w, 3), rgb.shape
            _check(load().pc_analyzer_put_frame(self._h, frame_id, p, pitch, dev, 1 if will_detect else 0))
        if dev:
            self._keep[frame_id % self.ring] = rgb  # device sources must outlive the async kernels
        # ... and so must the device mask this frame's detection copies: until the slot takes its next frame, whatever
        # set_mask is given in between
        self._keep_masks[frame_id % self.ring] = self._keep_mask if will_detect or self._target_margin >= 0 else None

    def put_frame_pixels(self, frame_id: int, img, will_detect: bool = True):
        """put_frame for a frame of any type the library takes (pc_analyzer_put_frame_pixels; Frame.set_pixels has the list)"""
        p, pitch, ptype, channels, dev = _pixels_args(img, self.w, self.h)
        _check(load().pc_analyzer_put_frame_pixels(self._h, frame_id, p, pitch, ptype, channels, dev, 1 if will_detect else 0))
        if dev:
            self._keep[frame_id % self.ring] = img
        self._keep_masks[frame_id % self.ring] = self._keep_mask if will_detect or self._target_margin >= 0 else None

    def has_frame(self, frame_id: int) -> bool:
        return bool(load().pc_analyzer_has_frame(self._h, frame_id))

    def set_keypoints(self, frame_id: int, xy: np.ndarray):
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        _check(load().pc_analyzer_set_keypoints(self._h, frame_id, xy.ctypes.data, len(xy)))

    def submit(self, frame1: int, targets):
        t = list(targets)
        arr = (C.c_int32 * max(1, len(t)))(*t)
        _check(load().pc_analyzer_submit(self._h, frame1, arr, len(t)))

    @property
    def pending(self) -> int:
        return load().pc_analyzer_pending(self._h)

    def set_device_log(self, tensor):
        """tensor: torch uint8 CUDA tensor (or None) that receives the device-resident record log."""
        if tensor is None:
            _check(load().pc_analyzer_set_device_log(self._h, None, 0))
            self._log = None
            return
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.element_size() == 1
        _check(load().pc_analyzer_set_device_log(self._h, tensor.data_ptr(), tensor.numel()))
        self._log = tensor

    def redirect_device_log(self, tensor):
        """The following jobs append to `tensor` from offset 0; nothing is waited for (pc_analyzer_redirect_device_log)."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.element_size() == 1
        _check(load().pc_analyzer_redirect_device_log(self._h, tensor.data_ptr(), tensor.numel()))
        self._log = tensor

    def set_host_records(self, enabled: bool):
        _check(load().pc_analyzer_set_host_records(self._h, 1 if enabled else 0))

    def set_fb_threshold(self, fb_threshold: float):
        """forward-backward check for the jobs submitted from now on; 0 = off (pc_analyzer_set_fb_threshold)"""
        _check(load().pc_analyzer_set_fb_threshold(self._h, float(fb_threshold)))

    def set_min_correlation(self, min_correlation: float):
        """minimum correlation for the jobs submitted from now on; 0 = off, 0 < v <= 1 (pc_analyzer_set_min_correlation)"""
        _check(load().pc_analyzer_set_min_correlation(self._h, float(min_correlation)))

    def set_normalize(self, normalize):
        """brightness-normalised LK for the jobs submitted from now on; 0 / False = off, 1 / True = on (pc_analyzer_set_normalize)"""
        _check(load().pc_analyzer_set_normalize(self._h, int(normalize)))

    def set_affine_refinement(self, affine):
        """affine refinement for the jobs submitted from now on; 0 / False = off, 1 / True = on, refused while normalize is on
        (pc_analyzer_set_affine_refinement)"""
        _check(load().pc_analyzer_set_affine_refinement(self._h, int(affine)))

    def set_mask_windows(self, on: bool):
        """masked windows for the frames put and the jobs submitted from now on (pc_analyzer_set_mask_windows): every frame put
        while a mask is in force gets its weight planes, and template pixels outside the mask carry no weight; refused beside
        normalize, the affine refinement, a search radius or a minimum correlation"""
        _check(load().pc_analyzer_set_mask_windows(self._h, int(on)))

    def set_search_radius(self, search_radius: int):
        """search prepass for the jobs submitted from now on; 0 = off, 1..256 = the radius in pixels, refused while normalize is on
        (pc_analyzer_set_search_radius)"""
        _check(load().pc_analyzer_set_search_radius(self._h, int(search_radius)))

    def set_target_mask_margin(self, margin: int):
        """target-side masks for the frames put from now on: -1 = off, 0..31 = the margin (pc_analyzer_set_target_mask_margin);
        every frame put then takes the mask in force, and rows that end where its choked plane is off are dropped"""
        _check(load().pc_analyzer_set_target_mask_margin(self._h, int(margin)))
        self._target_margin = int(margin)

    def set_mask(self, mask):
        """Detection mask of the frames put from now on with will_detect (pc_analyzer_set_mask): uint8 (H, W), non-zero =
        detect here; None = no mask.  A device tensor is held here until the ring slots of the frames put under it are reused;
        the caller must leave its contents unmodified until frame_ingested() for those frames."""
        if mask is None:
            _check(load().pc_analyzer_set_mask(self._h, None, 0, 0))
            self._keep_mask = None
            return
        keep, p, dev, pitch = _mask_ptr(mask, self.w, self.h)
        _check(load().pc_analyzer_set_mask(self._h, p, pitch, dev))
        self._keep_mask = keep if dev else None

    def set_mask_polygons(self, polys, invert: bool = False):
        """The same as closed polygons, rasterised on the GPU when a frame is put (pc_analyzer_set_mask_polygons; arguments
        as Frame.set_mask_polygons).  The vertices are consumed before the call returns."""
        xy, counts = _polygon_arrays(polys)
        _check(load().pc_analyzer_set_mask_polygons(self._h, xy.ctypes.data, counts.ctypes.data, len(counts), int(bool(invert))))
        self._keep_mask = None

    @property
    def device_log_used(self) -> int:
        n = C.c_size_t()
        _check(load().pc_analyzer_device_log_used(self._h, C.byref(n)))
        return n.value

    def collect_raw(self) -> FrameResult:
        r = FrameResult()
        _check(load().pc_analyzer_collect(self._h, C.byref(r)))
        return r

    def collect(self, copy: bool = True):
        """-> (frame1, keypoints [N,2], detected, {frame2: (src_idx, tgt_xy, err)})"""
        r = self.collect_raw()
        n = r.n_keypoints
        if n and not r.keypoints_xy:     # set_host_records(False): the records left through the device log only
            return r.frame1, None, bool(r.keypoints_detected), {int(r.targets[t]): None for t in range(r.n_targets)}
        kps = np.ctypeslib.as_array(r.keypoints_xy, shape=(n, 2)) if n else np.zeros((0, 2), np.float32)
        flows = {}
        for t in range(r.n_targets):
            a, b = int(r.row_offset[t]), int(r.row_offset[t + 1])
            if b > a:
                idx = np.ctypeslib.as_array(r.src_indices, shape=(b,))[a:b]
                xy = np.ctypeslib.as_array(r.tgt_xy, shape=(b, 2))[a:b]
                err = np.ctypeslib.as_array(r.flow_err, shape=(b,))[a:b]
            else:
                idx, xy, err = np.zeros(0, np.uint32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
            flows[int(r.targets[t])] = (idx.copy(), xy.copy(), err.copy()) if copy else (idx, xy, err)
        return r.frame1, (kps.copy() if copy else kps), bool(r.keypoints_detected), flows
