"""akaze_hip -- Python host mirror of the CUDA-AKAZE interface over libhipakaze's C ABI.

This is harness code (tests, bench): the product is the C-ABI shared library
``cuda-akaze_amd/libhipakaze.so`` and the C++ header ``include/akaze.h``.  The
names below follow the reference's API (akaze.h:10-30, akaze_structures.h:19-59)
so the parity tests read like the reference's demo (main.cpp:128-233):

    initAkazeData / freeAkazeData / cuMatch / Akazer.init / Akazer.detectAndCompute

There is NO CPU fallback: importing works anywhere (the library loads without a
GPU so symbol tests can run), but every compute call raises ``HakError`` when no
HIP device is usable, and a missing ``libhipakaze.so`` raises at import.
"""
import ctypes as C
import os

import numpy as np

# One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7, and a process that
# loads /opt/rocm's copy first makes torch see "No HIP GPUs" (and vice versa: measured on the GPU
# box, tools/probe_runtime.py).  Importing torch first lets libhipakaze.so bind to the runtime
# torch already loaded (same soname); without torch the library uses /opt/rocm's.
try:
    import torch as _torch  # noqa: F401
except ImportError:          # pure C-ABI use without PyTorch
    _torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# HAK_LIB selects another build of the same library (A/B measurements of compiler flags / kernel variants); never a fallback
LIB_PATH = os.environ.get("HAK_LIB") or os.path.join(os.path.dirname(_HERE), "libhipakaze.so")

FLEN = 61            # akaze_structures.h:29
MAX_DIST = 96        # akazed.cu:11
PM_G1, PM_G2, WEICKERT, CHARBONNIER = 0, 1, 2, 3   # akaze_structures.h:53-59

# akaze_structures.h:19-40 (104 bytes; numpy adds the 3 padding bytes explicitly)
POINT_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("response", "<f4"), ("size", "<f4"), ("angle", "<f4"),
    ("features", "u1", (FLEN,)), ("_pad", "u1", (3,)),
    ("match", "<i4"), ("distance", "<i4"), ("match_x", "<f4"), ("match_y", "<f4"),
])
assert POINT_DTYPE.itemsize == 104
MATCH_PAIR_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                             ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])      # hak_match_pair
assert MATCH_PAIR_DTYPE.itemsize == 32
HOMOGRAPHY_DTYPE = np.dtype([("H", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4"),
                             ("n", "<i4")])                                                   # hak_homography
assert HOMOGRAPHY_DTYPE.itemsize == 52
FUNDAMENTAL_DTYPE = np.dtype([("F", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("root", "<i4"),
                              ("n", "<i4")])                                                  # hak_fundamental
assert FUNDAMENTAL_DTYPE.itemsize == 52
INTRINSICS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])     # hak_intrinsics
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("in_front", "<i4"), ("candidate", "<i4"),
                       ("n", "<i4")])                                                         # hak_pose
assert INTRINSICS_DTYPE.itemsize == 16 and POSE_DTYPE.itemsize == 64
CORR3D_DTYPE = np.dtype([("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("u", "<f4"), ("v", "<f4"), ("src3d", "<i4"), ("src2d", "<i4"),
                         ("pad", "<i4")])                                                     # hak_corr3d
ABS_POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("solution", "<i4"),
                           ("n", "<i4")])                                                     # hak_abs_pose
assert CORR3D_DTYPE.itemsize == 32 and ABS_POSE_DTYPE.itemsize == 64
TRIANGULATION_DTYPE = np.dtype([("n", "<i4"), ("kept", "<i4"), ("rejected", "<i4", (3,)), ("model", "<i4"),
                                ("pad", "<i4", (2,))])                                        # hak_triangulation
assert TRIANGULATION_DTYPE.itemsize == 32
VIEW_IDENTITY, VIEW_RELATIVE, VIEW_ABSOLUTE = 0, 1, 2                                         # HAK_VIEW_*


class HakError(RuntimeError):
    pass


class hak_config(C.Structure):
    _fields_ = [
        ("noctaves", C.c_int), ("max_scale", C.c_int), ("per", C.c_float), ("kcontrast", C.c_float),
        ("soffset", C.c_float), ("reordering", C.c_int), ("derivative_factor", C.c_float),
        ("dthreshold", C.c_float), ("diffusivity", C.c_int), ("descriptor_pattern_size", C.c_int),
        ("max_pts", C.c_int), ("upright", C.c_int), ("batch", C.c_int),
    ]


class hak_traffic(C.Structure):
    _fields_ = [("fed_px_steps", C.c_double), ("fed_bytes", C.c_double), ("all_stage_bytes", C.c_double),
                ("fed_launches", C.c_int), ("fed_fused_bytes", C.c_double), ("hessian_bytes", C.c_double),
                ("prologue_bytes", C.c_double), ("describe_bytes", C.c_double), ("nms_bytes", C.c_double)]


PROF = dict(fed=0, lowpass=1, flow=2, hessian=3, contrast=4, down=5, extrema=6, nms=7, describe=8, match=9)

# every symbol include/hipakaze.h declares: name -> (restype, argtypes)
_vp, _fp, _ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
SYMBOLS = {
    "hak_device_count": (C.c_int, []),
    "hak_set_device": (C.c_int, [C.c_int]),
    "hak_last_error": (C.c_char_p, []),
    "hak_default_config": (None, [C.POINTER(hak_config)]),
    "hak_create": (C.c_int, [C.POINTER(hak_config), C.c_int, C.c_int, C.POINTER(_vp)]),
    "hak_destroy": (None, [_vp]),
    "hak_set_stream": (C.c_int, [_vp, _vp]),
    "hak_sync": (C.c_int, [_vp]),
    "hak_wait_event": (C.c_int, [_vp, _vp]),
    "hak_phase_event": (C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    "hak_set_concurrency": (C.c_int, [_vp, C.c_int]),
    "hak_set_null_order": (C.c_int, [_vp, C.c_int]),
    "hak_set_retain_best": (C.c_int, [_vp, C.c_int]),
    "hak_set_retain_grid": (C.c_int, [_vp, C.c_int]),
    "hak_detect_and_compute": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _ip, _vp, C.c_int]),
    "hak_detect_and_compute_pair": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _ip, _ip, _vp, _vp, C.c_int, C.c_int]),
    "hak_detect_and_compute_batch": (C.c_int, [_vp, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, C.c_int]),
    "hak_fast_detect_and_compute": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _ip, _vp, C.c_int]),
    "hak_fast_detect_and_compute_batch": (C.c_int, [_vp, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, C.c_int]),
    "hak_match": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp]),
    "hak_match_batch": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "hak_match_knn2": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip, _vp]),
    "hak_match_knn2_batch": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "hak_find_homography": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_uint, C.c_int, _vp, _vp]),
    "hak_find_homography_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_float, C.c_uint, C.c_int, _vp, _vp]),
    "hak_find_fundamental": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_find_fundamental_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_refine_fundamental": (C.c_int, [_vp, _vp, C.c_int, C.c_float, C.c_int, _vp, _vp]),
    "hak_refine_fundamental_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_float, C.c_int, _vp, _vp]),
    "hak_find_essential": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_find_essential_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, _vp, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_recover_pose": (C.c_int, [_vp, _vp, C.c_int, _fp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp]),
    "hak_recover_pose_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp]),
    "hak_refine_pose": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_float, C.c_float, C.c_int, _vp, _vp, _vp]),
    "hak_refine_pose_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, _vp, C.c_float, C.c_float, C.c_int, _vp, _vp, _vp]),
    "hak_link_tracks": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _ip, _vp]),
    "hak_link_tracks_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, _vp, _vp, C.c_long, _vp, C.c_int, C.c_int, _vp, C.c_long, _vp]),
    "hak_solve_pnp": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_solve_pnp_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, C.c_int, C.c_float, C.c_uint, _vp, _vp]),
    "hak_refine_pnp": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_float, C.c_int, _vp, _vp]),
    "hak_refine_pnp_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, C.c_float, C.c_int, _vp, _vp]),
    "hak_triangulate": (C.c_int, [_vp, _vp, C.c_int, _fp, _fp, _vp, _vp, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "hak_triangulate_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp,
                                        C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "hak_match_guided": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _fp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip, _vp]),
    "hak_match_guided_batch": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "hak_match_epipolar": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _fp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip, _vp]),
    "hak_match_epipolar_batch": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "hak_match_projected": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _fp, _vp, C.c_float, C.c_int, C.c_int, C.c_int,
                                      C.c_int, _vp, _ip, _vp]),
    "hak_match_projected_batch": (C.c_int, [_vp, _vp, C.c_long, _vp, C.c_int, _vp, _vp, _vp, C.c_long, _vp, C.c_int, _vp, C.c_long, _vp, C.c_int,
                                            C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_long,
                                            _vp]),
    "hak_points_alloc": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "hak_points_free": (C.c_int, [_vp]),
    "hak_image_alloc": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, _ip]),
    "hak_image_upload": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    "hak_image_free": (C.c_int, [_vp]),
    "hak_ingest_u8": (C.c_int, [_vp, _vp, C.c_long, C.c_int, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hak_host_alloc": (C.c_int, [C.POINTER(_vp), C.c_long]),
    "hak_host_free": (C.c_int, [_vp]),
    "hak_download_batch": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp]),
    "hak_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_long]),
    "hak_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_long]),
    "hak_fed_tau": (C.c_int, [C.c_float, C.c_int, C.c_float, C.c_int, _fp, C.c_int]),
    "hak_gauss_taps": (None, [C.c_float, C.c_int, _fp]),
    "hak_compare_indices": (None, [_ip, _ip]),
    "hak_describe_plan_query": (C.c_int, [C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "hak_describe_order_query": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint)]),
    "hak_describe_order_bin": (C.c_int, [C.c_float]),
    "hak_query_schedule": (C.c_int, [_vp, _ip, _ip, _fp, _fp]),
    "hak_query_geometry": (C.c_int, [_vp, _ip]),
    "hak_query_traffic": (C.c_int, [_vp, C.c_int, C.POINTER(hak_traffic)]),
    "hak_prof_enable": (C.c_int, [_vp, C.c_int]),
    "hak_prof_read": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), _ip]),
    "hak_prof_reset": (C.c_int, [_vp]),
}
# the TEST ABI (include/hipakaze_test.h -> libhipakaze_test.so): stage operators, plane introspection, probes
TEST_SYMBOLS = {
    "hak_debug_plane": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "hak_debug_kcontrast": (C.c_int, [_vp, C.c_int, _fp]),
    "hak_debug_arena_layout": (C.c_int, [_vp, C.POINTER(C.c_long), C.c_int]),
    "hak_debug_arena_read": (C.c_int, [_vp, C.c_int, _vp]),
    "hak_debug_arena_write": (C.c_int, [_vp, C.c_int, _vp]),
    "hak_op_lowpass": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]),
    "hak_op_down_smooth": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hak_op_kcontrast": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_float, _fp, _fp, _ip]),
    "hak_op_flow": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "hak_op_nld_steps": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _fp, C.c_int]),
    "hak_op_nld_steps_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int]),
    "hak_op_fed_cycle": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int,
                                   _fp, _fp, C.c_int]),
    "hak_op_rcp_check": (C.c_int, [C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong)]),
    "hak_op_smooth_flow": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "hak_op_hessian": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    # ... and their twins on the integer FAST path (int32 planes, uint8 images, integer contrast factors)
    "hak_op_fast_conv_u8": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]),
    "hak_op_fast_lowpass": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]),
    "hak_op_fast_base": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, _ip, _ip, _ip, _ip]),
    "hak_op_fast_down_smooth": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hak_op_fast_kcontrast": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_float, _ip, _ip, _ip]),
    "hak_op_fast_flow": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hak_op_fast_smooth_flow": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hak_op_fast_nld_steps": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _fp, C.c_int]),
    "hak_op_fast_nld_steps_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int]),
    "hak_op_fast_fed_cycle": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int,
                                        C.c_int, _ip, _fp, C.c_int]),
    "hak_op_fast_level_tile": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, _ip, _fp, C.c_int, _ip]),
    "hak_op_fast_hessian": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_op_hessian_planes": (C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_op_fast_hessian_planes": (C.c_int, [_vp, _vp, _vp, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_op_fast_base_planes": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, _ip, _ip, _ip,
                                          _ip]),
    "hak_op_hessian_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_op_fast_hessian_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_debug_set_plane": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "hak_op_tail_begin": (C.c_int, [_vp]),
    "hak_op_tail_level": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "hak_op_tail_det_level": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "hak_op_tail_seed": (C.c_int, [_vp, _vp, _vp]),
    "hak_debug_tail_total": (C.c_int, [_vp, _ip]),
    "hak_op_fast_tail_level": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int]),
    "hak_op_fast_tail_det_level": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int]),
    "hak_debug_tail_maps": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_long), _ip]),
    "hak_op_tail_finish": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_op_orient_describe": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "hak_op_fast_orient_describe": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "hak_op_copy_probe": (C.c_int, [C.c_long, C.c_int, C.POINTER(C.c_double)]),
    "hak_op_copy_probe_shapes": (C.c_int, [C.c_long, C.c_int, C.POINTER(C.c_double), C.c_int]),
    "hak_op_stream_probe": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hak_op_hess_probe": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hak_debug_fill_match_scratch": (C.c_int, [_vp, C.c_int]),
    "hak_op_ransac_shape": (C.c_int, [C.c_int, C.c_int, _ip, _ip]),
    "hak_op_match_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "hak_debug_ransac_scratch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "hak_op_gather_probe": (C.c_int, [C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback for the HIP path)")
TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libhipakaze_test.so")


class _Libs:
    """`lib.<symbol>`: the product ABI from libhipakaze.so; hak_op_* / hak_debug_* from libhipakaze_test.so, which is loaded on
    first use (tests and bench only) and links against the product library next to it"""

    def __init__(self):
        self.product = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        self.test = None
        for name, (res, args) in SYMBOLS.items():
            try:
                f = getattr(self.product, name)      # AttributeError here = ABI drift between header and library
            except AttributeError:
                if os.environ.get("HAK_LIB"):        # an older build loaded for an A/B run may lack the newest entry points
                    continue
                raise
            f.restype, f.argtypes = res, args
            setattr(self, name, f)

    def load_test(self):
        if self.test is None:
            if not os.path.exists(TEST_LIB_PATH):
                raise ImportError(f"{TEST_LIB_PATH} is missing: build it with `make -C cuda-akaze_amd/csrc`")
            self.test = C.CDLL(TEST_LIB_PATH)
            for name, (res, args) in TEST_SYMBOLS.items():
                f = getattr(self.test, name)
                f.restype, f.argtypes = res, args
                setattr(self, name, f)
        return self.test

    def __getattr__(self, name):                     # only reached for names not bound yet
        if name in TEST_SYMBOLS:
            self.load_test()
            return self.__dict__[name]
        raise AttributeError(name)


lib = _Libs()


def check(status):
    if status != 0:
        raise HakError(lib.hak_last_error().decode() or f"libhipakaze status {status}")


def iAlignUp(a, b):
    """cuda_utils.h:160"""
    return a - a % b + b if a % b else a


def device_count():
    return lib.hak_device_count()


def default_config(**kw):
    cfg = hak_config()
    lib.hak_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


# ----------------------------------------------------------------- host helpers
def fed_tau(T, M=1, tau_max=0.25, reordering=True):
    buf = np.zeros(4096, np.float32)
    n = lib.hak_fed_tau(T, M, tau_max, int(reordering), buf.ctypes.data_as(_fp), 4096)
    if n < 0:
        raise HakError("FED cycle too long")
    return buf[:n].copy()


def gauss_taps(var, radius):
    buf = np.zeros(8, np.float32)
    lib.hak_gauss_taps(var, radius, buf.ctypes.data_as(_fp))
    return buf[:radius + 1].copy()


def compare_indices():
    a = np.zeros(488, np.int32)
    b = np.zeros(488, np.int32)
    lib.hak_compare_indices(a.ctypes.data_as(_ip), b.ctypes.data_as(_ip))
    return a, b


def describe_plan(pattern_size):
    """(planned, pos[7][64], cell[7][64]) of hak_describe_plan_query"""
    pos = np.zeros((7, 64), np.uint32)
    cell = np.zeros((7, 64), np.uint32)
    ok = lib.hak_describe_plan_query(pattern_size, pos.ctypes.data_as(C.POINTER(C.c_uint)), cell.ctypes.data_as(C.POINTER(C.c_uint)))
    return bool(ok), pos, cell


def describe_order(pattern_size, row):
    """(NB, slots[7][64]) of hak_describe_order_query: row < NB the gather order of angle bin `row`, row NB the window order"""
    slots = np.zeros((7, 64), np.uint32)
    nb = lib.hak_describe_order_query(pattern_size, row, slots.ctypes.data_as(C.POINTER(C.c_uint)))
    return nb, slots


def describe_order_bin(angle):
    """the order-table row k_describe_runs takes for a keypoint angle (hak_describe_order_bin)"""
    return lib.hak_describe_order_bin(C.c_float(angle))


# ------------------------------------------------------ reference-shaped API
class AkazeData:
    """akaze_structures.h:44-50 {num_pts, max_pts, h_data, d_data}"""

    def __init__(self):
        self.num_pts = 0
        self.max_pts = 0
        self.h_data = None      # numpy structured array (POINT_DTYPE) or None
        self.d_data = None      # device pointer (int) or None
        self.h_pinned = None    # address of h_data when it lives in pinned host memory


def initAkazeData(data, max_pts, host, dev, pinned=False):
    """akaze.cpp:26-40.  pinned=True gives h_data in device-visible host memory, as the C++ layer's initAkazeData does
    (host/akaze.cpp): detectAndCompute then delivers records and count inside its launch sequence."""
    data.num_pts = 0
    data.max_pts = max_pts
    data.h_pinned = None
    if host and pinned:
        hp = _vp()
        check(lib.hak_host_alloc(C.byref(hp), max_pts * POINT_DTYPE.itemsize))
        data.h_pinned = hp.value
        buf = (C.c_uint8 * (max_pts * POINT_DTYPE.itemsize)).from_address(hp.value)
        data.h_data = np.frombuffer(buf, dtype=POINT_DTYPE)
        data.h_data[:] = np.zeros(1, POINT_DTYPE)[0]
    else:
        data.h_data = np.zeros(max_pts, POINT_DTYPE) if host else None
    data.d_data = None
    if dev:
        p = _vp()
        check(lib.hak_points_alloc(C.byref(p), max_pts))
        data.d_data = p.value


def freeAkazeData(data):
    """akaze.cpp:43-52"""
    if data.d_data is not None:
        check(lib.hak_points_free(data.d_data))
    data.d_data = None
    data.h_data = None
    if getattr(data, "h_pinned", None):
        check(lib.hak_host_free(data.h_pinned))
        data.h_pinned = None
    data.num_pts = 0
    data.max_pts = 0


class Akazer:
    """akaze.h:18-67.  ``whp0`` is (width, height, pitch) like the reference's int3."""

    def __init__(self):
        self._ctx = None
        self._cfg = default_config()
        self._retain_best = False
        self._retain_grid = 0
        self.whp = (0, 0, 0)

    def init(self, whp0, noctaves=4, max_scale=4, per=0.7, kcontrast=0.03, soffset=1.6, reordering=True,
             derivative_factor=1.5, dthreshold=0.001, diffusivity=PM_G2, descriptor_pattern_size=10,
             max_pts=10000, upright=False, batch=1, retain_best=False, retain_grid=0):
        self.whp = tuple(whp0)
        self._retain_best = bool(retain_best)
        self._retain_grid = self._checked_grid(retain_grid)
        self._cfg = default_config(
            noctaves=noctaves, max_scale=max_scale, per=per, kcontrast=kcontrast, soffset=soffset,
            reordering=int(reordering), derivative_factor=derivative_factor, dthreshold=dthreshold,
            diffusivity=int(diffusivity), descriptor_pattern_size=descriptor_pattern_size,
            max_pts=max_pts, upright=int(upright), batch=batch)
        self._make_ctx(self.whp[0], self.whp[1])

    def _make_ctx(self, w, h):
        self.close()
        ctx = _vp()
        check(lib.hak_create(C.byref(self._cfg), w, h, C.byref(ctx)))
        self._ctx = ctx
        self._ctx_wh = (w, h)
        if self._retain_best:
            check(lib.hak_set_retain_best(ctx, 1))
        if self._retain_grid:
            check(lib.hak_set_retain_grid(ctx, self._retain_grid))

    def set_retain_best(self, on=True):
        """hak_set_retain_best: an image with more survivors than its clamp keeps its strongest ones instead of the raster-order
        prefix (hipakaze.h states the rule).  Remembered: a context re-created for another image size keeps the mode."""
        self._retain_best = bool(on)
        if self._ctx is not None:
            check(lib.hak_set_retain_best(self._ctx, int(self._retain_best)))

    @staticmethod
    def _checked_grid(G):
        G = int(G)
        if G != 0 and not 8 <= G <= 128:
            raise ValueError("retain_grid: the cell size must be 0 (off) or between 8 and 128")
        return G

    def set_retain_grid(self, G):
        """hak_set_retain_grid: an image with more survivors than its clamp keeps the best of every G x G pixel cell (8 <= G <= 128;
        0: off; hipakaze.h states the rule).  While on it decides the policy whatever set_retain_best says.  Remembered: a context
        re-created for another image size keeps the mode."""
        self._retain_grid = self._checked_grid(G)
        if self._ctx is not None:
            check(lib.hak_set_retain_grid(self._ctx, self._retain_grid))

    @property
    def ctx(self):
        if self._ctx is None:
            raise HakError("Akazer.init() has not been called")
        return self._ctx

    def detectAndCompute(self, image, result, whp0, desc=True):
        """akaze.cpp:101-150.  ``image`` = device pointer (int) to float32 [0,1], pitch whp0[2]."""
        w, h, p = whp0
        if self._ctx is None or self._ctx_wh != (w, h):       # akaze.cpp:109: size differs from init -> new arena
            self._make_ctx(w, h)
        n = C.c_int(0)
        hptr = result.h_data.ctypes.data if result.h_data is not None else None
        check(lib.hak_detect_and_compute(self.ctx, image, p, result.d_data, result.max_pts, C.byref(n), hptr, int(desc)))
        result.num_pts = n.value

    def detectAndComputePair(self, image1, image2, result1, result2, whp0, desc=True, match=True):
        """build-side addition (akaze.h): both images + cuMatch(result1, result2) as one launch sequence and one synchronisation.
        The context must have been init()-ed with batch >= 2."""
        w, h, p = whp0
        if self._ctx is None or self._ctx_wh != (w, h):
            self._make_ctx(w, h)
        n1, n2 = C.c_int(0), C.c_int(0)
        h1 = result1.h_data.ctypes.data if result1.h_data is not None else None
        h2 = result2.h_data.ctypes.data if result2.h_data is not None else None
        check(lib.hak_detect_and_compute_pair(self.ctx, image1, image2, p, result1.d_data, result2.d_data, result1.max_pts, result2.max_pts,
                                              C.byref(n1), C.byref(n2), h1, h2, int(desc), int(match)))
        result1.num_pts, result2.num_pts = n1.value, n2.value

    def fastDetectAndCompute(self, image, result, whp0, desc=True):
        """akaze.h:30, akaze.cpp:153-201 -- integer FAST path.  ``image`` = device pointer to uint8, pitch whp0[2] bytes."""
        w, h, p = whp0
        if self._ctx is None or self._ctx_wh != (w, h):
            self._make_ctx(w, h)
        n = C.c_int(0)
        hptr = result.h_data.ctypes.data if result.h_data is not None else None
        check(lib.hak_fast_detect_and_compute(self.ctx, image, p, result.d_data, result.max_pts, C.byref(n), hptr, int(desc)))
        result.num_pts = n.value

    # -- introspection used by tests
    def plane(self, kind, octave, sublevel, img=0):
        whp = self.geometry()[octave]
        out = np.zeros((whp[1], whp[0]), np.float32)
        check(lib.hak_debug_plane(self.ctx, img, kind, octave, sublevel, out.ctypes.data))
        return out

    def arena_layout(self):
        """hak_debug_arena_layout: {"ms", "elements" (32-bit words per image), "batch", "octaves": [{"w", "h", "p", "smooth", "flow", "tmp",
        "lt": [ms offsets], "dxy": [ms offsets]}]} -- the layout as the library holds it, offsets in elements from the image's first"""
        n = lib.hak_debug_arena_layout(self.ctx, None, 0)
        if n < 0:
            check(1)
        buf = (C.c_long * n)()
        assert lib.hak_debug_arena_layout(self.ctx, buf, n) == n
        noct, ms = int(buf[0]), int(buf[1])
        per = 6 + 2 * ms
        octs = []
        for o in range(noct):
            q = [int(v) for v in buf[4 + o * per:4 + (o + 1) * per]]
            octs.append(dict(w=q[0], h=q[1], p=q[2], smooth=q[3], flow=q[4], tmp=q[5], lt=q[6:6 + ms], dxy=q[6 + ms:6 + 2 * ms]))
        return dict(ms=ms, elements=int(buf[2]), batch=int(buf[3]), octaves=octs)

    def arena_read(self, img=0):
        """hak_debug_arena_read: the whole arena of batch image `img` as uint32 words"""
        out = np.zeros(self.arena_layout()["elements"], np.uint32)
        check(lib.hak_debug_arena_read(self.ctx, img, out.ctypes.data))
        return out

    def arena_write(self, words, img=0):
        words = np.ascontiguousarray(words, np.uint32)
        assert words.shape == (self.arena_layout()["elements"],), words.shape
        check(lib.hak_debug_arena_write(self.ctx, img, words.ctypes.data))

    def set_plane(self, kind, octave, sublevel, plane, img=0):
        """hak_debug_set_plane: dense (h, w) float32 -> plane (0 Lt, 2 Lx, 3 Ly) of the level.  An int32 array (a plane of the FAST
        path) goes in bit for bit: the entry point copies words"""
        plane = np.asarray(plane)
        plane = np.ascontiguousarray(plane).view(np.float32) if plane.dtype == np.int32 else np.ascontiguousarray(plane, np.float32)
        w, h, _ = self.geometry()[octave]
        assert plane.shape == (h, w), (plane.shape, (h, w))
        check(lib.hak_debug_set_plane(self.ctx, img, kind, octave, sublevel, plane.ctypes.data))

    # -- detector tail / descriptors on hand-made inputs (hipakaze.h hak_op_tail_*; tests/test_gpu_literal.py)
    def tail_begin(self):
        check(lib.hak_op_tail_begin(self.ctx))

    def tail_level(self, octave, sublevel, lplane):
        lplane = np.ascontiguousarray(lplane, np.float32)
        check(lib.hak_op_tail_level(self.ctx, octave, sublevel, lplane.ctypes.data))

    def tail_det_level(self, octave, sublevel, det):
        det = np.ascontiguousarray(det, np.float32)
        check(lib.hak_op_tail_det_level(self.ctx, octave, sublevel, det.ctypes.data))

    def fast_tail_level(self, octave, sublevel, lplane, threshold=65):
        lplane = np.ascontiguousarray(lplane, np.int32)
        check(lib.hak_op_fast_tail_level(self.ctx, octave, sublevel, lplane.ctypes.data, int(threshold)))

    def fast_tail_det_level(self, octave, sublevel, det, threshold=65):
        det = np.ascontiguousarray(det, np.int32)
        check(lib.hak_op_fast_tail_det_level(self.ctx, octave, sublevel, det.ctypes.data, int(threshold)))

    def tail_maps(self):
        """hak_debug_tail_maps, between tail_begin and tail_finish: (response words (h, w) uint32, layers (h, w) int32 with -1 for an
        empty pixel, candidate words in arrival order, the list's capacity, the candidate count)"""
        w, h, _ = self.geometry()[0]
        resp, layer = np.zeros((h, w), np.uint32), np.zeros((h, w), np.int32)
        cap, n = C.c_long(0), C.c_int(0)
        check(lib.hak_debug_tail_maps(self.ctx, resp.ctypes.data, layer.ctypes.data, None, C.byref(cap), C.byref(n)))
        cand = np.zeros(cap.value, np.uint64)
        check(lib.hak_debug_tail_maps(self.ctx, None, None, cand.ctypes.data, None, None))
        return resp, layer, cand[:max(min(n.value, cap.value), 0)], cap.value, n.value

    def tail_seed(self, response, layer):
        """response: (h, w) float32 (or int32 for the FAST path's map), layer: (h, w) int32, < 0 = no candidate"""
        response = np.ascontiguousarray(response)
        assert response.dtype.itemsize == 4
        layer = np.ascontiguousarray(layer, np.int32)
        check(lib.hak_op_tail_seed(self.ctx, response.ctypes.data, layer.ctypes.data))

    def tail_finish(self, max_pts=1000, refine=False, fast=False):
        """NMS + emit (+ refine) -> host records in raster order"""
        data = AkazeData()
        initAkazeData(data, max_pts, True, True)
        try:
            n = C.c_int(0)
            check(lib.hak_op_tail_finish(self.ctx, data.d_data, max_pts, int(refine), int(fast), C.byref(n)))
            k = min(n.value, max_pts)
            if k:
                check(lib.hak_memcpy_d2h(data.h_data.ctypes.data, data.d_data, k * POINT_DTYPE.itemsize))
            return data.h_data[:k].copy(), n.value
        finally:
            freeAkazeData(data)

    def tail_total(self):
        """hak_debug_tail_total: the survivors of the last tail_finish before the clamp to max_pts"""
        n = C.c_int(0)
        check(lib.hak_debug_tail_total(self.ctx, C.byref(n)))
        return n.value

    def orient_describe(self, points, desc=1, fast=False):
        """orientation + MLDB (desc=1) or MLDB with the records' own angles (desc=2) on host records; returns them updated.
        fast=True: hak_op_fast_orient_describe -- refinement + orientation + MLDB of the integer FAST path on int32 planes"""
        points = np.ascontiguousarray(points)
        assert points.dtype == POINT_DTYPE and len(points) >= 1
        data = AkazeData()
        initAkazeData(data, len(points), False, True)
        try:
            check(lib.hak_memcpy_h2d(data.d_data, points.ctypes.data, points.nbytes))
            op = lib.hak_op_fast_orient_describe if fast else lib.hak_op_orient_describe
            check(op(self.ctx, data.d_data, len(points), int(desc)))
            out = np.zeros(len(points), POINT_DTYPE)
            check(lib.hak_memcpy_d2h(out.ctypes.data, data.d_data, out.nbytes))
            return out
        finally:
            freeAkazeData(data)

    def fast_orient_describe(self, points, desc=1):
        return self.orient_describe(points, desc, fast=True)

    def kcontrast(self, img=0):
        v = C.c_float()
        check(lib.hak_debug_kcontrast(self.ctx, img, C.byref(v)))
        return v.value

    def geometry(self):
        buf = np.zeros(3 * 8, np.int32)
        n = lib.hak_query_geometry(self.ctx, buf.ctypes.data_as(_ip))
        return [tuple(int(v) for v in buf[3 * o:3 * o + 3]) for o in range(n)]

    def schedule(self):
        ns = np.zeros(40, np.int32); ss = np.zeros(40, np.int32)
        sz = np.zeros(40, np.float32); bd = np.zeros(40, np.float32)
        n = lib.hak_query_schedule(self.ctx, ns.ctypes.data_as(_ip), ss.ctypes.data_as(_ip),
                                   sz.ctypes.data_as(_fp), bd.ctypes.data_as(_fp))
        m = n * self._cfg.max_scale
        return dict(noct=n, nsteps=ns[:m].copy(), sigma_size=ss[:m].copy(), sizes=sz[:m].copy(), borders=bd[:m].copy())

    def traffic(self, npts_hint=0):
        t = hak_traffic()
        check(lib.hak_query_traffic(self.ctx, npts_hint, C.byref(t)))
        return t

    def close(self):
        if self._ctx is not None:
            lib.hak_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ctx_of(akazer):
    """the context of an optional Akazer; None: the call runs without one"""
    return akazer.ctx if akazer is not None else None


def cuMatch(result1, result2, akazer=None):
    """akaze.h:14, akaze.cpp:55-64: fills match/distance/match_x/match_y of result1."""
    ctx = _ctx_of(akazer)
    hptr = result1.h_data.ctypes.data if result1.h_data is not None else None
    check(lib.hak_match(ctx, result1.d_data, result1.num_pts, result2.d_data, result2.num_pts, hptr))


def cuMatchKnn(result1, result2, ratio=(1, 1), cross_check=True, max_dist=0, akazer=None):
    """Match post-processing (hipakaze.h hak_match_knn2): 2-NN ratio test of the reference's unused
    gMatch (akazed.cu:2028-2122) + symmetric cross-check + device-side compaction.  Updates result1 like
    cuMatch and returns the accepted matches (MATCH_PAIR_DTYPE, ascending query index)."""
    import torch
    ctx = _ctx_of(akazer)
    n1 = result1.num_pts
    d_out = torch.zeros(max(n1, 1) * MATCH_PAIR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(n1, 1), MATCH_PAIR_DTYPE)
    cnt = C.c_int(0)
    hptr = result1.h_data.ctypes.data if result1.h_data is not None else None
    check(lib.hak_match_knn2(ctx, result1.d_data, n1, result2.d_data, result2.num_pts, int(ratio[0]), int(ratio[1]),
                             int(cross_check), int(max_dist), hptr, d_out.data_ptr(), C.byref(cnt), h_out.ctypes.data))
    return h_out[:cnt.value].copy()


def _match_gated(entry, result1, result2, model, radius, ratio, cross_check, max_dist, akazer):
    """the call behind cuMatchGuided and cuMatchEpipolar: `entry` re-matches result1 against result2 under the nine floats of `model`"""
    import torch
    ctx = _ctx_of(akazer)
    n1 = result1.num_pts
    m = np.ascontiguousarray(np.asarray(model, np.float32).reshape(9))
    d_out = torch.zeros(max(n1, 1) * MATCH_PAIR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(n1, 1), MATCH_PAIR_DTYPE)
    cnt = C.c_int(0)
    hptr = result1.h_data.ctypes.data if result1.h_data is not None else None
    check(entry(ctx, result1.d_data, n1, result2.d_data, result2.num_pts, m.ctypes.data_as(_fp), float(radius), int(ratio[0]),
                int(ratio[1]), int(cross_check), int(max_dist), hptr, d_out.data_ptr(), C.byref(cnt), h_out.ctypes.data))
    return h_out[:cnt.value].copy()


def cuMatchGuided(result1, result2, H, radius=8.0, ratio=(4, 5), cross_check=True, max_dist=0, akazer=None):
    """Guided matching (hipakaze.h hak_match_guided): re-matches result1 against result2 under the homography H (9 values, row-major,
    e.g. findHomography's record["H"]): every query is searched only among the train points within `radius` pixels of where H sends
    it; ratio test and cross-check inside that neighbourhood.  Updates result1 like cuMatch and returns the accepted matches
    (MATCH_PAIR_DTYPE, ascending query index)."""
    return _match_gated(lib.hak_match_guided, result1, result2, H, radius, ratio, cross_check, max_dist, akazer)


def cuMatchEpipolar(result1, result2, F, radius=2.0, ratio=(4, 5), cross_check=True, max_dist=0, akazer=None):
    """Epipolar guided matching (hipakaze.h hak_match_epipolar): re-matches result1 against result2 under the fundamental matrix F
    (9 values, row-major, (x2 y2 1) F (x1 y1 1)^T = 0, e.g. findFundamental's record["F"]): every query is searched only among the
    train points closer than `radius` pixels to its epipolar line; ratio test and cross-check inside that band.  Updates result1
    like cuMatch and returns the accepted matches (MATCH_PAIR_DTYPE, ascending query index)."""
    return _match_gated(lib.hak_match_epipolar, result1, result2, F, radius, ratio, cross_check, max_dist, akazer)


def _device_records(a, dtype):
    """(device uint8 tensor, record count) of a host structured array or of a device tensor of such records (used in place)"""
    import torch
    if isinstance(a, torch.Tensor):
        d = a.contiguous()
        return d, d.numel() * d.element_size() // dtype.itemsize
    host = np.ascontiguousarray(a, dtype)
    n = len(host)
    return (torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda() if n else torch.zeros(32, dtype=torch.uint8, device="cuda")), n


def _out_buffers(n, xyz=False):
    """the device outputs of a call over n records, never empty: (mask of max(n, 1) bytes, with `xyz` the points of 3 * max(n, 1)
    floats, else None)"""
    import torch
    return (torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda"),
            torch.zeros(3 * max(n, 1), dtype=torch.float32, device="cuda") if xyz else None)


def _out_host(n, d_mask, d_xyz=None):
    """what a call over n records returns of _out_buffers: (mask uint8 (n,),) and, with d_xyz, xyz float32 (n, 3)"""
    mask = (d_mask[:n].cpu().numpy(),)
    return mask if d_xyz is None else mask + (d_xyz[:3 * n].cpu().numpy().reshape(n, 3),)


def findHomography(matches, iterations=1024, threshold=3.0, seed=0, refine=True, akazer=None):
    """RANSAC homography over a match list (hipakaze.h hak_find_homography), on the device.  `matches`: the MATCH_PAIR_DTYPE
    array cuMatchKnn returns (host), or a device tensor of such records (then it is used in place).  Returns (record of
    HOMOGRAPHY_DTYPE, inlier mask as a uint8 numpy array); record["H"].reshape(3, 3) maps (x1, y1, 1) to image 2."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    d_mask, _ = _out_buffers(n)
    out = np.zeros((), HOMOGRAPHY_DTYPE)
    check(lib.hak_find_homography(ctx, d_m.data_ptr(), n, int(iterations), float(threshold), int(seed) & 0xFFFFFFFF, int(bool(refine)),
                                  d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)


def findFundamental(matches, iterations=1024, threshold=1.0, seed=0, akazer=None):
    """RANSAC fundamental matrix over a match list (hipakaze.h hak_find_fundamental), on the device.  `matches` as findHomography's.
    Returns (record of FUNDAMENTAL_DTYPE, inlier mask as a uint8 numpy array); F = record["F"].reshape(3, 3) satisfies
    (x2, y2, 1) F (x1, y1, 1)^T = 0 for the inliers.  The seven-point model of the winning sample; refineFundamental refits it over its
    inliers."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    d_mask, _ = _out_buffers(n)
    out = np.zeros((), FUNDAMENTAL_DTYPE)
    check(lib.hak_find_fundamental(ctx, d_m.data_ptr(), n, int(iterations), float(threshold), int(seed) & 0xFFFFFFFF,
                                   d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)


def refineFundamental(matches, record, threshold=1.0, rounds=3, akazer=None):
    """Rank-2 least-squares refit of a fundamental matrix over its inliers, iterated up to `rounds` (1..8) times (hipakaze.h
    hak_refine_fundamental), on the device.  `matches` as findHomography's; `record`: a FUNDAMENTAL_DTYPE record, findFundamental's
    or an earlier refit's (it is not modified).  Returns (record, inlier mask as a uint8 numpy array): record["root"] == 3 when a
    refit was accepted, and record["inliers"] is never below the input F's count at `threshold`."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    d_mask, _ = _out_buffers(n)
    out = np.array(record, FUNDAMENTAL_DTYPE).reshape(())
    check(lib.hak_refine_fundamental(ctx, d_m.data_ptr(), n, float(threshold), int(rounds), d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)


def intrinsics(K):
    """an INTRINSICS_DTYPE record from (fx, fy, cx, cy), a 3 x 3 pinhole matrix (zero skew) or such a record"""
    if isinstance(K, np.ndarray) and K.dtype == INTRINSICS_DTYPE:
        return K.reshape(()).copy()
    K = np.asarray(K, np.float64)
    return np.array((K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(4)), INTRINSICS_DTYPE)


def findEssential(matches, K1, K2=None, iterations=1024, threshold=1.0, seed=0, akazer=None):
    """Five-point RANSAC essential matrix over a match list under known intrinsics (hipakaze.h hak_find_essential), on the device.
    `matches` as findHomography's; K1, K2 as recoverPose's.  Returns (record of FUNDAMENTAL_DTYPE, inlier mask as a uint8 numpy
    array): record["F"] is K2^-T E K1^-1 scaled to largest |entry| 1, scored in pixels as findFundamental's, record["root"] is
    16 + the root of the winner's degree-10 polynomial; recoverPose, refinePose and matchEpipolar take the record as it is."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    k1 = intrinsics(K1)
    k2 = k1 if K2 is None else intrinsics(K2)
    d_mask, _ = _out_buffers(n)
    out = np.zeros((), FUNDAMENTAL_DTYPE)
    check(lib.hak_find_essential(ctx, d_m.data_ptr(), n, k1.ctypes.data, k2.ctypes.data, int(iterations), float(threshold),
                                 int(seed) & 0xFFFFFFFF, d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)


def recoverPose(matches, F_or_record, K1, K2=None, threshold=1.0, max_depth=float("inf"), akazer=None):
    """Relative pose from a fundamental matrix and the cameras' intrinsics (hipakaze.h hak_recover_pose), on the device.
    `matches` as findHomography's; `F_or_record`: 9 values, row-major, or a FUNDAMENTAL_DTYPE record (one with hypothesis < 0 has
    no model and gives the no-pose record); K1, K2: (fx, fy, cx, cy), a 3 x 3 matrix or an INTRINSICS_DTYPE record, K2 = K1 when
    omitted.  Returns (record of POSE_DTYPE, mask uint8 (n,), xyz float32 (n, 3)): X2 = R X1 + t with |t| = 1, the mask marks the
    inliers of F in front of both cameras, xyz their points in the first camera's frame in units of the baseline; candidate = -1
    means no pose."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    if getattr(F_or_record, "dtype", None) is not None and F_or_record.dtype.names:
        f = np.array(F_or_record["F"], np.float32).reshape(9)
        if int(F_or_record["hypothesis"]) < 0:
            f = np.full(9, np.nan, np.float32)                          # no model: the rule's step 1
    else:
        f = np.ascontiguousarray(np.asarray(F_or_record, np.float32).reshape(9))
    k1 = intrinsics(K1)
    k2 = k1 if K2 is None else intrinsics(K2)
    d_mask, d_xyz = _out_buffers(n, xyz=True)
    out = np.zeros((), POSE_DTYPE)
    check(lib.hak_recover_pose(ctx, d_m.data_ptr(), n, f.ctypes.data_as(_fp), k1.ctypes.data, k2.ctypes.data, float(threshold),
                               float(max_depth), d_mask.data_ptr(), d_xyz.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask, d_xyz)


def refinePose(matches, K1, record, K2=None, threshold=1.0, max_depth=float("inf"), rounds=3, akazer=None):
    """Calibrated Gauss-Newton refit of a relative pose over the matches that count under it, iterated up to `rounds` (1..8) times
    (hipakaze.h hak_refine_pose), on the device.  `matches` as findHomography's; K1, K2, max_depth as recoverPose's; `record`: a
    POSE_DTYPE record, recoverPose's or an earlier refit's (it is not modified).  Returns (record, mask uint8 (n,), xyz float32
    (n, 3)) as recoverPose does, under the refitted pose: record["candidate"] == 4 when a refit was accepted, and
    record["in_front"] is never below the input pose's count under its own F at `threshold`."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    k1 = intrinsics(K1)
    k2 = k1 if K2 is None else intrinsics(K2)
    d_mask, d_xyz = _out_buffers(n, xyz=True)
    out = np.array(record, POSE_DTYPE).reshape(())
    check(lib.hak_refine_pose(ctx, d_m.data_ptr(), n, k1.ctypes.data, k2.ctypes.data, float(threshold), float(max_depth), int(rounds),
                              d_mask.data_ptr(), d_xyz.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask, d_xyz)


def _host_view(v):
    """(twelve float32 {R row-major, t} or None for the identity, has a model) of a view given as None, twelve numbers, or a
    POSE_DTYPE / ABS_POSE_DTYPE record"""
    if v is None:
        return None, True
    model = True
    if getattr(v, "dtype", None) is not None and v.dtype.names:
        model = int(v["candidate"] if "candidate" in v.dtype.names else v["hypothesis"]) >= 0
        v = np.concatenate([np.asarray(v["R"], np.float32).reshape(9), np.asarray(v["t"], np.float32).reshape(3)])
    m = np.ascontiguousarray(np.asarray(v, np.float32).reshape(12))
    return m, bool(model and np.isfinite(m).all())


def triangulate(matches, viewA, viewB, KA, KB=None, threshold=2.0, max_depth=float("inf"), min_sin=0.0, akazer=None):
    """3-D points of a match list under two known views (hipakaze.h hak_triangulate), on the device.  `matches` as
    findHomography's, (x1, y1) seen by view A and (x2, y2) by view B; a view is None (the identity), twelve floats {R row-major, t}
    with Xc = R X + t, a POSE_DTYPE record (recoverPose's) or an ABS_POSE_DTYPE record (solvePnP's, refinePnP's); KA, KB as
    recoverPose's K1, K2.  Returns (record of TRIANGULATION_DTYPE, mask uint8 (n,), xyz float32 (n, 3)): the mask marks the
    matches that pass the parallax gate (the sine of the rays' angle >= min_sin), the depth gate (0 < depth < max_depth in both
    cameras) and the reprojection gate (below `threshold` px in both images); xyz holds their points in the frame the views map
    from, zeros elsewhere.  A record view without a model, or with a non-finite entry, is step 1 of the rule, which needs no
    device: the no-model record (model = 0), an all-zero mask and all-zero points."""
    ctx = _ctx_of(akazer)
    d_m, n = _device_records(matches, MATCH_PAIR_DTYPE)
    (a, model_a), (b, model_b) = _host_view(viewA), _host_view(viewB)
    ka = intrinsics(KA)
    kb = ka if KB is None else intrinsics(KB)
    out = np.zeros((), TRIANGULATION_DTYPE)
    if not (model_a and model_b):
        out["n"] = n
        return out, np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    d_mask, d_xyz = _out_buffers(n, xyz=True)
    check(lib.hak_triangulate(ctx, d_m.data_ptr(), n, a.ctypes.data_as(_fp) if a is not None else None,
                              b.ctypes.data_as(_fp) if b is not None else None, ka.ctypes.data, kb.ctypes.data, float(threshold),
                              float(max_depth), float(min_sin), d_mask.data_ptr(), d_xyz.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask, d_xyz)


def linkTracks(matchesA, xyzA, matchesB, maskA=None, max_index=None, akazer=None):
    """Joins the match list of images (I0, I1) with its points (recoverPose's xyz, (nA, 3) float32) and the match list of images
    (I1, I2) on the shared image into 3-D to 2-D correspondences (hipakaze.h hak_link_tracks), on the device.  The lists as
    findHomography's; maskA: nA bytes (recoverPose's front mask) or None; max_index: a bound above every keypoint index of I1
    (default: one above the largest train index of a host list A).  Returns a CORR3D_DTYPE array in ascending order of B."""
    import torch
    ctx = _ctx_of(akazer)
    d_a, na = _device_records(matchesA, MATCH_PAIR_DTYPE)
    d_b, nb = _device_records(matchesB, MATCH_PAIR_DTYPE)
    if max_index is None:
        if isinstance(matchesA, torch.Tensor):
            raise HakError("linkTracks: max_index is needed with a device list")
        max_index = int(np.asarray(matchesA["train"]).max()) + 1 if na else 1
    d_xyz = xyzA.contiguous() if isinstance(xyzA, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(xyzA, np.float32).reshape(-1)).cuda() if na else torch.zeros(4, dtype=torch.float32, device="cuda")
    d_mask = None
    if maskA is not None:
        d_mask = maskA.contiguous() if isinstance(maskA, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(maskA, np.uint8).reshape(-1)).cuda() if na else torch.zeros(4, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(max(nb, 1) * CORR3D_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    out = np.zeros(max(nb, 1), CORR3D_DTYPE)
    count = C.c_int(0)
    check(lib.hak_link_tracks(ctx, d_a.data_ptr(), na, d_mask.data_ptr() if d_mask is not None else None, d_xyz.data_ptr(),
                              d_b.data_ptr(), nb, int(max_index), d_out.data_ptr(), C.byref(count), out.ctypes.data))
    return out[:count.value].copy()


def matchProjected(matchesA, xyzA, result_desc, result2, view, K, radius=8.0, ratio=(4, 5), cross_check=True, max_dist=0, maskA=None,
                   akazer=None):
    """Projection-guided matching (hipakaze.h hak_match_projected): re-matches 3-D points against the keypoints of a new image under
    its known pose, on the device.  `matchesA`: the match list the points came from, as findHomography's (only `train` is read: the
    keypoint of result_desc whose descriptor stands for the landmark); xyzA: its points, (nA, 3) float32 (recoverPose's or
    triangulate's); maskA: nA bytes or None; result_desc, result2: AkazeData of the image `train` indexes and of the new image;
    `view`: the new image's pose in the forms triangulate accepts (None, twelve floats {R row-major, t}, a POSE_DTYPE or an
    ABS_POSE_DTYPE record); K as recoverPose's.  Every landmark is searched only among the keypoints of result2 within `radius`
    pixels of its projection; ratio test and cross-check inside that neighbourhood.  Returns a CORR3D_DTYPE array in ascending
    landmark order: src3d = the landmark's index in matchesA, src2d = the KEYPOINT index in result2.  A record view without a model
    gives the empty list (step 7 of the rule, which needs no device)."""
    import torch
    ctx = _ctx_of(akazer)
    d_a, na = _device_records(matchesA, MATCH_PAIR_DTYPE)
    m, model = _host_view(view)
    if not model:
        return np.zeros(0, CORR3D_DTYPE)
    d_xyz = xyzA.contiguous() if isinstance(xyzA, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(xyzA, np.float32).reshape(-1)).cuda() if na else torch.zeros(4, dtype=torch.float32, device="cuda")
    d_mask = None
    if maskA is not None:
        d_mask = maskA.contiguous() if isinstance(maskA, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(maskA, np.uint8).reshape(-1)).cuda() if na else torch.zeros(4, dtype=torch.uint8, device="cuda")
    k = intrinsics(K)
    d_out = torch.zeros(max(na, 1) * CORR3D_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    out = np.zeros(max(na, 1), CORR3D_DTYPE)
    count = C.c_int(0)
    check(lib.hak_match_projected(ctx, d_a.data_ptr(), na, d_mask.data_ptr() if d_mask is not None else None, d_xyz.data_ptr(),
                                  result_desc.d_data, result_desc.num_pts, result2.d_data, result2.num_pts,
                                  m.ctypes.data_as(_fp) if m is not None else None, k.ctypes.data, float(radius), int(ratio[0]),
                                  int(ratio[1]), int(cross_check), int(max_dist), d_out.data_ptr(), C.byref(count), out.ctypes.data))
    return out[:count.value].copy()


def solvePnP(corr, K, iterations=1024, threshold=2.0, seed=0, akazer=None):
    """RANSAC absolute pose from 3-D to 2-D correspondences by the three-point solve (hipakaze.h hak_solve_pnp), on the device.
    `corr`: the CORR3D_DTYPE array linkTracks returns (host), or a device tensor of such records (used in place); K: (fx, fy, cx, cy),
    a 3 x 3 matrix or an INTRINSICS_DTYPE record.  Returns (record of ABS_POSE_DTYPE, inlier mask as a uint8 numpy array):
    Xc = R X + t in the units of the points; hypothesis = -1 means no model."""
    ctx = _ctx_of(akazer)
    d_c, n = _device_records(corr, CORR3D_DTYPE)
    k = intrinsics(K)
    d_mask, _ = _out_buffers(n)
    out = np.zeros((), ABS_POSE_DTYPE)
    check(lib.hak_solve_pnp(ctx, d_c.data_ptr(), n, k.ctypes.data, int(iterations), float(threshold), int(seed) & 0xFFFFFFFF,
                            d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)


def refinePnP(corr, K, record, threshold=2.0, rounds=3, akazer=None):
    """Gauss-Newton refit of an absolute pose over its inliers, iterated up to `rounds` (1..8) times (hipakaze.h hak_refine_pnp), on
    the device.  `corr` and K as solvePnP's; `record`: an ABS_POSE_DTYPE record, solvePnP's or an earlier refit's (it is not
    modified).  Returns (record, inlier mask as a uint8 numpy array): record["solution"] == 4 when a refit was accepted, and
    record["inliers"] is never below the input pose's count at `threshold`."""
    ctx = _ctx_of(akazer)
    d_c, n = _device_records(corr, CORR3D_DTYPE)
    k = intrinsics(K)
    d_mask, _ = _out_buffers(n)
    out = np.array(record, ABS_POSE_DTYPE).reshape(())
    check(lib.hak_refine_pnp(ctx, d_c.data_ptr(), n, k.ctypes.data, float(threshold), int(rounds), d_mask.data_ptr(), out.ctypes.data))
    return (out,) + _out_host(n, d_mask)
