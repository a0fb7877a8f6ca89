"""ctypes binding of libslamgpu.so (include/slamgpu.h) and the reference-shaped Python surface.

Classes mirror the reference's C++ classes for this path:
  ORBextractor   src/orb_features/orb_extractor.h:25-93  (Compute, Get* tables, GetImagePyramid)
  OrbMatcher     src/orb_features/orb_matcher.h:14-119   (DescriptorDistance, SearchByProjection)
  Optimizer      src/optimizer/optimizer.h:13-50         (PoseOptimization; include/slamgpu_optimizer.h)
  StereoFrontend the stereo Frame ctor's hot part (frame.cpp:61-111) batched over frames.
The library is the only compute path: there is no CPU fallback, and every entry point raises if
libslamgpu.so is missing or a HIP call fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# SLAMGPU_LIB: load another build of the same library (A/B kernel experiments under tools/).
LIB_PATH = os.environ.get("SLAMGPU_LIB") or os.path.join(_PKG, "libslamgpu.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

F2F_QUERY_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("last_angle", "<f4"), ("last_octave", "<i4"),
                            ("mp_id", "<i4"), ("blocks", "<i4"), ("pad", "<i4"),
                            ("desc", "u1", (32,))])
F2F_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("tlc_z", "<f4"),
                           ("baseline", "<f4"), ("th", "<f4"), ("mono", "<i4"),
                           ("check_ori", "<i4"), ("pad", "<i4")])
MPS_QUERY_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"),
                            ("view_cos", "<f4"), ("level", "<i4"), ("in_view", "<i4"),
                            ("is_bad", "<i4"), ("mp_id", "<i4"), ("blocks", "<i4"),
                            ("pad", "<i4", (3,)), ("desc", "u1", (32,))])
# slamgpu_reloc_query / slamgpu_reloc_pose (include/slamgpu.h): a map point of the relocalisation
# candidate keyframe, the current frame's pose with the window factor and ORBdist.
RELOC_QUERY_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("max_dist", "<f4"), ("min_dist", "<f4"),
                              ("kf_angle", "<f4"), ("mp_id", "<i4"), ("skip", "<i4"),
                              ("desc", "u1", (32,))])
RELOC_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)),
                             ("th", "<f4"), ("orb_dist", "<i4"), ("check_ori", "<i4")])
assert RELOC_QUERY_DTYPE.itemsize == 64 and RELOC_POSE_DTYPE.itemsize == 72
# slamgpu_init_query / slamgpu_init_search (include/slamgpu.h): keypoint i1 of the initial frame
# for SearchForInitialization, and the call's parameters.
INIT_QUERY_DTYPE = np.dtype([("angle", "<f4"), ("octave", "<i4"), ("pad", "<i4", (6,)),
                             ("desc", "u1", (32,))])
INIT_SEARCH_DTYPE = np.dtype([("nnratio", "<f4"), ("window_size", "<i4"), ("check_ori", "<i4"),
                              ("pad", "<i4")])
assert INIT_QUERY_DTYPE.itemsize == 64 and INIT_SEARCH_DTYPE.itemsize == 16
# slamgpu_sim3_match (include/slamgpu_optimizer.h): one OptimizeSim3 correspondence.
SIM3_MATCH_DTYPE = np.dtype([("x1c", "<f4", (3,)), ("x2c", "<f4", (3,)), ("u1", "<f4"),
                             ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("octave1", "<i4"),
                             ("octave2", "<i4")])
# slamgpu_sim3_ransac_job / slamgpu_sim3_hyp (include/slamgpu_sim3solver.h): one candidate of the
# RANSAC Sim3 solver, one hypothesis (mR12i, mt12i, ms12i, mnInliersi) of its schedule.
SIM3_RANSAC_JOB_DTYPE = np.dtype([("match_begin", "<i4"), ("n", "<i4"), ("draw_begin", "<i4"),
                                  ("n_its", "<i4"), ("min_inliers", "<i4"), ("fix_scale", "<i4")])
SIM3_HYP_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"),
                           ("n_inliers", "<i4"), ("pad", "<i4", (2,))])
SIM3_MAX_MATCHES = 4096
SIM3_RANSAC_MAX_ITS = 300
# slamgpu_pnp_match / slamgpu_pnp_ransac_job / slamgpu_pnp_hyp (include/slamgpu_pnpsolver.h): one
# correspondence of the RANSAC EPnP solver (mvP3Dw, mvP2D, the keypoint's octave), one candidate,
# one hypothesis or refined pose (mRi, mti as float, the inlier count, the running best).
PNP_MATCH_DTYPE = np.dtype([("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("octave", "<i4")])
PNP_JOB_DTYPE = np.dtype([("match_begin", "<i4"), ("n", "<i4"), ("draw_begin", "<i4"),
                          ("n_its", "<i4"), ("min_inliers", "<i4"), ("pad", "<i4")])
PNP_HYP_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("n_inliers", "<i4"),
                          ("best", "<i4"), ("pad", "<i4", (2,))])
PNP_MAX_MATCHES = 4096
PNP_RANSAC_MAX_ITS = 512
assert PNP_MATCH_DTYPE.itemsize == 24 and PNP_JOB_DTYPE.itemsize == 24
assert PNP_HYP_DTYPE.itemsize == 64
# slamgpu_init_job / _hyp / _result / _motion (include/slamgpu_initializer.h): one pair of frames
# of the monocular Initializer, one H or F hypothesis, the per-job selection, one motion hypothesis.
INIT_JOB_DTYPE = np.dtype([("key1_begin", "<i4"), ("n1", "<i4"), ("key2_begin", "<i4"),
                           ("n2", "<i4"), ("draw_begin", "<i4"), ("n_its", "<i4"),
                           ("K", "<f4", (4,)), ("sigma", "<f4"), ("pad", "<i4")])
INIT_HYP_DTYPE = np.dtype([("M", "<f4", (9,)), ("score", "<f4"), ("pad", "<i4", (2,))])
INIT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("best", "<i4", (2,)),
                              ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("model", "<i4"),
                              ("n_motions", "<i4"), ("norm", "<f4", (8,)), ("pad", "<i4", (3,))])
INIT_MOTION_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("n_good", "<i4"),
                              ("cos_parallax", "<f4"), ("pad", "<i4", (2,))])
INIT_MAX_KEYS = 8192
INIT_MAX_ITS = 512
INIT_MAX_MOTIONS = 8
assert INIT_JOB_DTYPE.itemsize == 48 and INIT_HYP_DTYPE.itemsize == 48
assert INIT_RESULT_DTYPE.itemsize == 80 and INIT_MOTION_DTYPE.itemsize == 64
# slamgpu_sim3_edge (include/slamgpu_optimizer.h): one EdgeSim3 of the essential graph.
SIM3_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("pad", "<i4", (2,)), ("Sji", "<f8", (8,))])
# slamgpu_pose_edge (include/slamgpu_optimizer.h): one PoseOptimization correspondence.
POSE_EDGE_DTYPE = np.dtype([("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"),
                            ("octave", "<i4")])
POSE_MAX_EDGES = 16384  # == SLAMGPU_POSE_MAX_EDGES
# slamgpu_ba_obs (include/slamgpu_optimizer.h): one LocalBundleAdjustment observation.
BA_OBS_DTYPE = np.dtype([("keyframe", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"),
                         ("octave", "<i4")])
assert KP_DTYPE.itemsize == 28 and F2F_QUERY_DTYPE.itemsize == 64 and POSE_EDGE_DTYPE.itemsize == 28
assert F2F_POSE_DTYPE.itemsize == 72 and MPS_QUERY_DTYPE.itemsize == 80
assert SIM3_RANSAC_JOB_DTYPE.itemsize == 24 and SIM3_HYP_DTYPE.itemsize == 64

EXPORTS = [
    "slamgpu_create", "slamgpu_destroy", "slamgpu_last_error", "slamgpu_kp_capacity",
    "slamgpu_scale_tables", "slamgpu_orb_scale_tables", "slamgpu_extract", "slamgpu_get_pyramid_level",
    "slamgpu_frame_stereo", "slamgpu_frontend_device", "slamgpu_sync",
    "slamgpu_download_keypoints", "slamgpu_download_stereo", "slamgpu_device_results",
    "slamgpu_frame_record_bytes", "slamgpu_pack_frame_records_device",
    "slamgpu_descriptor_distance", "slamgpu_search_by_projection_frame",
    "slamgpu_search_by_projection_mps", "slamgpu_search_by_projection_frame_device",
    "slamgpu_search_by_projection_mps_device", "slamgpu_search_by_projection_reloc",
    "slamgpu_search_by_projection_reloc_device", "slamgpu_debug_level_keys",
    "slamgpu_frame_mono", "slamgpu_search_for_initialization",
    "slamgpu_search_for_initialization_device",
    "slamgpu_make_vo_queries_device", "slamgpu_timing_start", "slamgpu_timing_stop",
    "slamgpu_set_extract_fork",
    "slamgpu_trace_marker",
    "slamgpu_timing_read", "slamgpu_pose_optimization", "slamgpu_pose_optimization_device",
    "slamgpu_optimizer_last_error", "slamgpu_coop_slots_in_use", "slamgpu_local_bundle_adjustment",
    "slamgpu_local_bundle_adjustment_device", "slamgpu_local_ba_workspace_bytes",
    "slamgpu_global_bundle_adjustment", "slamgpu_optimize_sim3", "slamgpu_optimize_sim3_device",
    "slamgpu_optimize_essential_graph",
    "slamgpu_local_ba_linearize_device", "slamgpu_set_distortion", "slamgpu_undistort_points",
    "slamgpu_undistort_keypoints_device", "slamgpu_download_undistorted_keypoints",
    # include/slamgpu_bow.h
    "slamgpu_bow_last_error", "slamgpu_vocab_load_text", "slamgpu_vocab_create",
    "slamgpu_vocab_destroy", "slamgpu_vocab_info", "slamgpu_vocab_nodes", "slamgpu_bow_transform",
    "slamgpu_bow_transform_device", "slamgpu_search_by_bow", "slamgpu_search_by_bow_device",
    "slamgpu_distinctive_descriptors", "slamgpu_distinctive_descriptors_device", "slamgpu_gray",
    "slamgpu_gray_device", "slamgpu_bow_score", "slamgpu_bow_score_device",
    # include/slamgpu_kfdb.h
    "slamgpu_kfdb_last_error", "slamgpu_kfdb_create", "slamgpu_kfdb_destroy",
    "slamgpu_kfdb_set_bow", "slamgpu_kfdb_set_bow_device", "slamgpu_kfdb_set_covisible",
    "slamgpu_kfdb_set_covisible_device", "slamgpu_kfdb_add", "slamgpu_kfdb_erase",
    "slamgpu_kfdb_clear", "slamgpu_kfdb_add_device", "slamgpu_kfdb_erase_device",
    "slamgpu_kfdb_clear_device", "slamgpu_kfdb_detect_scratch_bytes",
    "slamgpu_kfdb_detect_loop_candidates", "slamgpu_kfdb_detect_loop_candidates_device",
    "slamgpu_kfdb_detect_relocalization_candidates",
    "slamgpu_kfdb_detect_relocalization_candidates_device",
    # include/slamgpu_kfmatch.h
    "slamgpu_kfmatch_last_error", "slamgpu_search_for_triangulation",
    "slamgpu_search_for_triangulation_device", "slamgpu_fuse", "slamgpu_fuse_device",
    "slamgpu_create_new_map_points", "slamgpu_create_new_map_points_device",
    "slamgpu_create_new_map_points_scratch_bytes",
    # include/slamgpu_loopmatch.h
    "slamgpu_loopmatch_last_error", "slamgpu_fuse_sim3", "slamgpu_fuse_sim3_device",
    "slamgpu_search_by_projection_sim3", "slamgpu_search_by_projection_sim3_scratch_bytes",
    "slamgpu_search_by_projection_sim3_device", "slamgpu_search_by_sim3",
    "slamgpu_search_by_sim3_device",
    # include/slamgpu_sim3solver.h
    "slamgpu_sim3solver_last_error", "slamgpu_sim3_ransac", "slamgpu_sim3_ransac_device",
    # include/slamgpu_pnpsolver.h
    "slamgpu_pnpsolver_last_error", "slamgpu_pnp_ransac", "slamgpu_pnp_ransac_device",
    # include/slamgpu_initializer.h
    "slamgpu_initializer_last_error", "slamgpu_init_ransac", "slamgpu_init_ransac_device",
    # include/slamgpu_io.h
    "slamgpu_io_last_error", "slamgpu_kitti_load_images", "slamgpu_kitti_image_path",
    "slamgpu_png_info", "slamgpu_png_decode", "slamgpu_imread_png",
]


def unpack_frame_record(rec, kp_cap):
    """Host view of one slamgpu_pack_frame_records_device record (uint8 array) -> dict of the
    left/right keypoints and descriptors, u_right and depth, trimmed to the keypoint counts."""
    rec = np.asarray(rec, np.uint8).reshape(-1)
    kc = kp_cap
    nl, nr = rec[128 * kc:128 * kc + 8].view(np.int32)
    kps = rec[:56 * kc].view(KP_DTYPE).reshape(2, kc)
    desc = rec[56 * kc:120 * kc].reshape(2, kc, 32)
    return {"kps_left": kps[0, :nl], "kps_right": kps[1, :nr], "desc_left": desc[0, :nl],
            "desc_right": desc[1, :nr], "u_right": rec[120 * kc:124 * kc].view(np.float32)[:nl],
            "depth": rec[124 * kc:128 * kc].view(np.float32)[:nl]}


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float)]


class DeviceView(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("nkps", C.c_void_p),
                ("u_right", C.c_void_p), ("depth", C.c_void_p), ("kp_cap", C.c_int),
                ("kps_un", C.c_void_p)]


class BaLinear(C.Structure):
    """slamgpu_ba_linear: device pointers of the linearisation outputs."""
    _fields_ = [(n, C.c_void_p) for n in ("chi2", "hpl", "hll", "bl", "hpp", "bp", "chi")]


class SlamGpuError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libslamgpu.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run `python -m slam_framework_amd.build`")
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7. Loaded first, it
        # also satisfies our library's libamdhip64.so.7 dependency; loaded after us, it would
        # map a second runtime next to /opt/rocm's and fail to initialise the device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, ip, fp, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
        L.slamgpu_create.argtypes = [ip, C.POINTER(OrbParams), ip, ip, ip, C.POINTER(vp)]
        L.slamgpu_destroy.argtypes = [vp]
        L.slamgpu_destroy.restype = None
        L.slamgpu_last_error.argtypes = [vp]
        L.slamgpu_last_error.restype = C.c_char_p
        L.slamgpu_kp_capacity.argtypes = [vp]
        L.slamgpu_scale_tables.argtypes = [vp, vp, vp, vp, vp, vp]
        if hasattr(L, "slamgpu_orb_scale_tables"):  # absent from older A/B builds (tools/abl)
            L.slamgpu_orb_scale_tables.argtypes = [C.POINTER(OrbParams), vp, vp, vp, vp, vp]
        L.slamgpu_extract.argtypes = [vp, vp, sz, vp, vp, ip, C.POINTER(ip)]
        L.slamgpu_get_pyramid_level.argtypes = [vp, ip, ip, vp, sz, C.POINTER(ip), C.POINTER(ip)]
        L.slamgpu_frame_stereo.argtypes = [vp, vp, vp, sz, C.POINTER(Camera)]
        L.slamgpu_frontend_device.argtypes = [vp, vp, vp, sz, sz, ip, C.POINTER(Camera), vp]
        L.slamgpu_sync.argtypes = [vp, vp]
        L.slamgpu_download_keypoints.argtypes = [vp, ip, vp, vp, ip, C.POINTER(ip)]
        L.slamgpu_download_stereo.argtypes = [vp, ip, vp, vp, ip, C.POINTER(ip)]
        L.slamgpu_device_results.argtypes = [vp, C.POINTER(DeviceView)]
        L.slamgpu_frame_record_bytes.argtypes = [vp]
        L.slamgpu_frame_record_bytes.restype = sz
        L.slamgpu_pack_frame_records_device.argtypes = [vp, ip, ip, vp, vp]
        L.slamgpu_descriptor_distance.argtypes = [vp, vp]
        L.slamgpu_search_by_projection_frame.argtypes = [vp, ip, vp, ip, vp, vp, vp, ip,
                                                         C.POINTER(ip)]
        L.slamgpu_search_by_projection_mps.argtypes = [vp, ip, vp, ip, fp, ip, vp, vp, ip,
                                                       C.POINTER(ip)]
        L.slamgpu_search_by_projection_frame_device.argtypes = [
            vp, vp, ip, vp, vp, ip, vp, vp, vp, C.c_int64, vp, ip, vp]
        L.slamgpu_search_by_projection_mps_device.argtypes = [
            vp, vp, ip, vp, vp, ip, fp, ip, vp, vp, C.c_int64, vp, ip, vp]
        L.slamgpu_search_by_projection_reloc.argtypes = [vp, ip, vp, ip, vp, vp, vp, ip,
                                                         C.POINTER(ip)]
        L.slamgpu_search_by_projection_reloc_device.argtypes = [
            vp, vp, ip, vp, vp, ip, vp, vp, vp, C.c_int64, vp, ip, vp]
        if hasattr(L, "slamgpu_frame_mono"):  # absent from older A/B builds (SLAMGPU_LIB)
            L.slamgpu_frame_mono.argtypes = [vp, vp, sz, C.POINTER(Camera)]
            L.slamgpu_search_for_initialization.argtypes = [vp, ip, vp, ip, vp, vp, vp,
                                                            C.POINTER(ip)]
            L.slamgpu_search_for_initialization_device.argtypes = [
                vp, vp, ip, vp, vp, ip, vp, vp, vp, vp, ip, vp]
        L.slamgpu_debug_level_keys.argtypes = [vp, ip, ip, ip, vp, ip, C.POINTER(ip)]
        L.slamgpu_make_vo_queries_device.argtypes = [vp, vp, ip, vp, vp, vp, ip, vp]
        L.slamgpu_timing_start.argtypes = [vp, C.c_char_p, ip]
        L.slamgpu_set_extract_fork.argtypes = [vp, ip]
        L.slamgpu_timing_stop.argtypes = [vp, vp]
        if hasattr(L, "slamgpu_trace_marker"):  # absent from older A/B builds (tools/abl)
            L.slamgpu_trace_marker.argtypes = [ip, vp]
        L.slamgpu_timing_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(ip)]
        L.slamgpu_pose_optimization.argtypes = [C.POINTER(Camera), vp, ip, vp, ip, vp, vp,
                                                C.POINTER(ip)]
        L.slamgpu_pose_optimization_device.argtypes = [C.POINTER(Camera), vp, ip, vp, vp, ip, vp,
                                                       vp, vp, vp, vp]
        L.slamgpu_local_bundle_adjustment.argtypes = [C.POINTER(Camera), vp, ip, vp, vp, ip, vp,
                                                      ip, vp, vp, vp, vp, C.POINTER(ip)]
        L.slamgpu_global_bundle_adjustment.argtypes = [C.POINTER(Camera), vp, ip, vp, vp, ip, vp,
                                                       ip, vp, vp, ip, ip, vp, C.POINTER(ip)]
        L.slamgpu_optimize_sim3.argtypes = [vp, vp, vp, vp, ip, vp, ip, fp, ip, vp, vp,
                                            C.POINTER(ip)]
        L.slamgpu_optimize_sim3_device.argtypes = [vp, vp, vp, vp, ip, vp, vp, ip, fp, ip, vp, vp,
                                                   vp, vp, vp]
        L.slamgpu_optimize_essential_graph.argtypes = [ip, vp, vp, vp, ip, ip, ip, vp, vp, vp, ip,
                                                       C.POINTER(ip)]
        L.slamgpu_local_ba_workspace_bytes.argtypes = [ip, ip, ip]
        L.slamgpu_local_ba_workspace_bytes.restype = sz
        L.slamgpu_local_bundle_adjustment_device.argtypes = [
            C.POINTER(Camera), vp, ip, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, sz, ip, ip, ip, vp,
            vp]
        L.slamgpu_local_ba_linearize_device.argtypes = [
            C.POINTER(Camera), vp, ip, vp, ip, vp, vp, vp, vp, vp, C.POINTER(BaLinear), vp, vp, sz,
            ip, ip, ip, vp]
        L.slamgpu_set_distortion.argtypes = [vp, vp, ip]
        L.slamgpu_undistort_points.argtypes = [C.POINTER(Camera), vp, ip, vp, vp, ip]
        L.slamgpu_undistort_keypoints_device.argtypes = [
            C.POINTER(Camera), vp, ip, vp, C.c_int64, vp, ip, vp, C.c_int64, ip, ip, vp]
        L.slamgpu_download_undistorted_keypoints.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
        if hasattr(L, "slamgpu_png_decode"):  # include/slamgpu_io.h (absent from older A/B builds)
            L.slamgpu_io_last_error.argtypes = []
            L.slamgpu_io_last_error.restype = C.c_char_p
            L.slamgpu_kitti_load_images.argtypes = [C.c_char_p, vp, ip, C.POINTER(ip)]
            L.slamgpu_kitti_image_path.argtypes = [C.c_char_p, ip, ip, C.c_char_p, sz]
            L.slamgpu_png_info.argtypes = [vp, sz, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
            L.slamgpu_png_decode.argtypes = [vp, sz, vp, sz, sz, C.POINTER(ip), C.POINTER(ip),
                                             C.POINTER(ip)]
            L.slamgpu_imread_png.argtypes = [C.c_char_p, vp, sz, sz, C.POINTER(ip), C.POINTER(ip),
                                             C.POINTER(ip)]
        if hasattr(L, "slamgpu_sim3_ransac"):  # include/slamgpu_sim3solver.h (absent from older A/B builds)
            L.slamgpu_sim3solver_last_error.argtypes = []
            L.slamgpu_sim3solver_last_error.restype = C.c_char_p
            L.slamgpu_sim3_ransac.argtypes = [vp, vp, vp, vp, ip, vp, ip, vp, ip, ip, ip, vp, vp,
                                              vp, C.POINTER(ip)]
            L.slamgpu_sim3_ransac_device.argtypes = [vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, ip,
                                                     ip, ip, vp, vp, vp, vp, vp]
        if hasattr(L, "slamgpu_pnp_ransac"):  # include/slamgpu_pnpsolver.h (absent from older A/B builds)
            L.slamgpu_pnpsolver_last_error.argtypes = []
            L.slamgpu_pnpsolver_last_error.restype = C.c_char_p
            L.slamgpu_pnp_ransac.argtypes = [vp, vp, ip, fp, vp, ip, vp, ip, ip, vp, vp, vp, vp,
                                             vp, C.POINTER(ip)]
            L.slamgpu_pnp_ransac_device.argtypes = [vp, vp, ip, fp, vp, ip, vp, ip, vp, ip, ip,
                                                    ip, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "slamgpu_init_ransac"):  # include/slamgpu_initializer.h (absent from older A/B builds)
            L.slamgpu_initializer_last_error.argtypes = []
            L.slamgpu_initializer_last_error.restype = C.c_char_p
            L.slamgpu_init_ransac.argtypes = [vp, vp, ip, vp, ip, vp, fp, vp, ip, vp, vp, vp, vp,
                                              vp, vp, vp]
            L.slamgpu_init_ransac_device.argtypes = [vp, vp, ip, vp, ip, vp, ip, vp, ip, ip, ip,
                                                     vp, vp, vp, vp, vp, vp, vp, vp]
        L.slamgpu_optimizer_last_error.argtypes = []
        L.slamgpu_optimizer_last_error.restype = C.c_char_p
        if hasattr(L, "slamgpu_coop_slots_in_use"):  # diagnostic (absent from older A/B builds)
            L.slamgpu_coop_slots_in_use.argtypes = [C.c_int]
            L.slamgpu_coop_slots_in_use.restype = C.c_int
        _lib = L
    return _lib


def trace_marker(mark_id, stream=None):
    """slamgpu_trace_marker: an empty kernel with a 1 x mark_id grid on `stream` (a mark in a
    profiler's kernel trace; bench.py brackets its timed region with ids 1 and 2)."""
    rc = lib().slamgpu_trace_marker(int(mark_id), C.c_void_p(stream or 0))
    if rc != 0:
        raise SlamGpuError(f"slamgpu_trace_marker: error {rc}")


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a.data_ptr()))  # torch tensor


class Context:
    """Owns one slamgpu_ctx (one device, one stream, workspaces for max_frames stereo pairs)."""

    def __init__(self, cols, rows, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th_fast=20,
                 min_th_fast=7, max_frames=1, device=0):
        self.params = OrbParams(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast)
        self.cols, self.rows, self.nlevels = cols, rows, nlevels
        self.max_frames = max_frames
        h = C.c_void_p()
        rc = lib().slamgpu_create(device, C.byref(self.params), cols, rows, max_frames,
                                  C.byref(h))
        self.h = h
        if rc != 0:
            assert not h, "slamgpu_create returns no context on failure"
            self.h = None
            msg = lib().slamgpu_last_error(None).decode()
            raise SlamGpuError(f"slamgpu_create failed ({rc}): {msg}")
        self.kp_cap = lib().slamgpu_kp_capacity(self.h)

    def check(self, rc):
        if rc != 0:
            raise SlamGpuError(f"slamgpu error {rc}: {lib().slamgpu_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            lib().slamgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scale_tables(self):
        n = self.nlevels
        arrs = [np.zeros(n, np.float32) for _ in range(4)] + [np.zeros(n, np.int32)]
        self.check(lib().slamgpu_scale_tables(self.h, *[_ptr(a) for a in arrs]))
        return arrs

    def extract(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.rows, self.cols)
        kps = np.zeros(self.kp_cap, KP_DTYPE)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n = C.c_int()
        self.check(lib().slamgpu_extract(self.h, _ptr(img), img.strides[0], _ptr(kps), _ptr(desc),
                                         self.kp_cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def pyramid_level(self, img, level):
        w, h = C.c_int(), C.c_int()
        self.check(lib().slamgpu_get_pyramid_level(self.h, img, level, None, 0, C.byref(w),
                                                   C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self.check(lib().slamgpu_get_pyramid_level(self.h, img, level, _ptr(out), w.value,
                                                   C.byref(w), C.byref(h)))
        return out

    def debug_level_keys(self, img, level, stage):
        """Packed (x_rel, y_rel, score) keys of one level: stage 0 FAST, 1 octree output."""
        n = C.c_int()
        cap = 1 << 17
        out = np.zeros(cap, np.uint32)
        self.check(lib().slamgpu_debug_level_keys(self.h, img, level, stage, _ptr(out), cap,
                                                  C.byref(n)))
        return out[:n.value].copy()

    def frame_stereo(self, left, right, cam):
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        self.cam = Camera(*cam)
        self.check(lib().slamgpu_frame_stereo(self.h, _ptr(left), _ptr(right), left.strides[0],
                                              C.byref(self.cam)))

    def frame_mono(self, img, cam):
        """slamgpu_frame_mono: the monocular Frame ctor's hot part; the image's results become the
        context's frame 0 (keypoints(0), stereo(0) = all -1, undistorted_keypoints(0), searches)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.rows, self.cols)
        self.cam = Camera(*cam)
        self.check(lib().slamgpu_frame_mono(self.h, _ptr(img), img.strides[0], C.byref(self.cam)))

    def frontend_device(self, d_left, d_right, frame_stride, pitch, n_frames, cam, stream=None):
        """d_left/d_right: device pointers (int) or torch uint8 CUDA tensors."""
        self.cam = Camera(*cam)
        pl = d_left if isinstance(d_left, int) else int(d_left.data_ptr())
        pr = d_right if isinstance(d_right, int) else int(d_right.data_ptr())
        self.check(lib().slamgpu_frontend_device(self.h, C.c_void_p(pl), C.c_void_p(pr),
                                                 frame_stride, pitch, n_frames,
                                                 C.byref(self.cam), C.c_void_p(stream or 0)))

    def set_distortion(self, dist_coef):
        """Frame DistCoef k1 k2 p1 p2 [k3] (None or [] clears)."""
        d = np.ascontiguousarray(dist_coef if dist_coef is not None else [], np.float32)
        self.check(lib().slamgpu_set_distortion(self.h, _ptr(d) if d.size else None, d.size))

    def undistorted_keypoints(self, frame):
        kps = np.zeros(self.kp_cap, KP_DTYPE)
        n = C.c_int()
        self.check(lib().slamgpu_download_undistorted_keypoints(self.h, frame, _ptr(kps),
                                                                self.kp_cap, C.byref(n)))
        return kps[:n.value].copy()

    def sync(self, stream=None):
        self.check(lib().slamgpu_sync(self.h, C.c_void_p(stream or 0)))

    # downloads fill capacity-sized buffers and return views of their first n entries (no
    # zero-fill, no second copy: the single-frame call pattern times these)
    def keypoints(self, img):
        kps = np.empty(self.kp_cap, KP_DTYPE)
        desc = np.empty((self.kp_cap, 32), np.uint8)
        n = C.c_int()
        self.check(lib().slamgpu_download_keypoints(self.h, img, _ptr(kps), _ptr(desc),
                                                    self.kp_cap, C.byref(n)))
        return kps[:n.value], desc[:n.value]

    def stereo(self, frame):
        ur = np.empty(self.kp_cap, np.float32)
        depth = np.empty(self.kp_cap, np.float32)
        n = C.c_int()
        self.check(lib().slamgpu_download_stereo(self.h, frame, _ptr(ur), _ptr(depth),
                                                 self.kp_cap, C.byref(n)))
        return ur[:n.value], depth[:n.value]

    def device_results(self):
        v = DeviceView()
        self.check(lib().slamgpu_device_results(self.h, C.byref(v)))
        return v

    @property
    def record_bytes(self):
        """Bytes of one per-frame result record (include/slamgpu.h)."""
        return lib().slamgpu_frame_record_bytes(self.h)

    def pack_frame_records_device(self, first, n, d_dst, stream=None):
        """Frames [first, first + n) of the last frontend call -> n records at d_dst."""
        self.check(lib().slamgpu_pack_frame_records_device(self.h, first, n, _ptr(d_dst),
                                                           C.c_void_p(stream or 0)))

    # ---- batched device path (torch CUDA tensors or raw device pointers) ----
    def make_vo_queries_device(self, d_poses, blocks, d_queries, d_q_start, d_q_count, n_frames,
                               stream=None):
        self.check(lib().slamgpu_make_vo_queries_device(
            self.h, _ptr(d_poses), blocks, _ptr(d_queries), _ptr(d_q_start), _ptr(d_q_count),
            n_frames, C.c_void_p(stream or 0)))

    def search_by_projection_frame_device(self, d_queries, total_queries, d_q_start, d_q_count,
                                          max_queries, d_poses, d_map_point, d_blocked, mp_stride,
                                          d_nmatches, n_frames, stream=None):
        self.check(lib().slamgpu_search_by_projection_frame_device(
            self.h, _ptr(d_queries), total_queries, _ptr(d_q_start), _ptr(d_q_count), max_queries,
            _ptr(d_poses), _ptr(d_map_point), _ptr(d_blocked), mp_stride, _ptr(d_nmatches),
            n_frames, C.c_void_p(stream or 0)))

    def search_by_projection_reloc_device(self, d_queries, total_queries, d_q_start, d_q_count,
                                          max_queries, d_poses, d_map_point, d_blocked, mp_stride,
                                          d_nmatches, n_frames, stream=None):
        """slamgpu_search_by_projection_reloc_device: RELOC_QUERY / RELOC_POSE records, one pose
        per frame; d_blocked = "the slot holds a map point". Never allocates or synchronises."""
        self.check(lib().slamgpu_search_by_projection_reloc_device(
            self.h, _ptr(d_queries), total_queries, _ptr(d_q_start), _ptr(d_q_count), max_queries,
            _ptr(d_poses), _ptr(d_map_point), _ptr(d_blocked), mp_stride, _ptr(d_nmatches),
            n_frames, C.c_void_p(stream or 0)))

    def search_for_initialization_device(self, d_queries, total_queries, d_q_start, d_q_count,
                                         max_queries, d_params, d_prev_matched, d_matches12,
                                         d_nmatches, n_frames, stream=None):
        """slamgpu_search_for_initialization_device: INIT_QUERY records, one INIT_SEARCH record
        per frame; d_prev_matched ([.][2] float32) and d_matches12 (int32) are parallel to
        d_queries. Never allocates or synchronises."""
        self.check(lib().slamgpu_search_for_initialization_device(
            self.h, _ptr(d_queries), total_queries, _ptr(d_q_start), _ptr(d_q_count), max_queries,
            _ptr(d_params), _ptr(d_prev_matched), _ptr(d_matches12), _ptr(d_nmatches), n_frames,
            C.c_void_p(stream or 0)))

    def set_extract_fork(self, on):
        """Level 0's FAST beside the pyramid on a side stream (True, the default) or after it
        (False: a timing pass then sees each kernel alone)."""
        self.check(lib().slamgpu_set_extract_fork(self.h, 1 if on else 0))

    def timing_start(self, kernel="*", max_launches=8192):
        self.check(lib().slamgpu_timing_start(self.h, kernel.encode(), max_launches))

    def timing_stop(self, stream=None):
        self.check(lib().slamgpu_timing_stop(self.h, C.c_void_p(stream or 0)))

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_int()
        self.check(lib().slamgpu_timing_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def search_by_projection_frame(self, frame, queries, pose, map_point, blocked):
        queries = np.ascontiguousarray(queries, dtype=F2F_QUERY_DTYPE)
        pose = np.ascontiguousarray(np.atleast_1d(pose), dtype=F2F_POSE_DTYPE)
        assert map_point.dtype == np.int32 and blocked.dtype == np.uint8
        nm = C.c_int()
        self.check(lib().slamgpu_search_by_projection_frame(
            self.h, frame, _ptr(queries), len(queries), _ptr(pose), _ptr(map_point),
            _ptr(blocked), len(map_point), C.byref(nm)))
        return nm.value

    def search_by_projection_mps(self, frame, queries, nnratio, th, map_point, blocked):
        queries = np.ascontiguousarray(queries, dtype=MPS_QUERY_DTYPE)
        assert map_point.dtype == np.int32 and blocked.dtype == np.uint8
        nm = C.c_int()
        self.check(lib().slamgpu_search_by_projection_mps(
            self.h, frame, _ptr(queries), len(queries), nnratio, th, _ptr(map_point),
            _ptr(blocked), len(map_point), C.byref(nm)))
        return nm.value

    def search_by_projection_reloc(self, frame, queries, pose, map_point, blocked):
        """slamgpu_search_by_projection_reloc on frame `frame`: map_point (int32 per keypoint,
        -1 = none) is in/out, blocked (uint8) returns as map_point >= 0. Returns nmatches."""
        queries = np.ascontiguousarray(queries, dtype=RELOC_QUERY_DTYPE)
        pose = np.ascontiguousarray(np.atleast_1d(pose), dtype=RELOC_POSE_DTYPE)
        assert map_point.dtype == np.int32 and blocked.dtype == np.uint8
        assert len(map_point) == len(blocked)
        nm = C.c_int()
        self.check(lib().slamgpu_search_by_projection_reloc(
            self.h, frame, _ptr(queries), len(queries), _ptr(pose), _ptr(map_point),
            _ptr(blocked), len(map_point), C.byref(nm)))
        return nm.value


    def search_for_initialization(self, frame, queries, params, prev_matched):
        """slamgpu_search_for_initialization with F2 = frame `frame`: queries are INIT_QUERY
        records of all F1 keypoints, params one INIT_SEARCH record, prev_matched ([n1][2] float32)
        is updated in place. Returns (nmatches, matches12 as int32[n1])."""
        queries = np.ascontiguousarray(queries, dtype=INIT_QUERY_DTYPE)
        params = np.ascontiguousarray(np.atleast_1d(params), dtype=INIT_SEARCH_DTYPE)
        assert prev_matched.dtype == np.float32 and prev_matched.flags.c_contiguous
        assert prev_matched.shape == (len(queries), 2)
        m12 = np.full(len(queries), -1, np.int32)
        nm = C.c_int()
        self.check(lib().slamgpu_search_for_initialization(
            self.h, frame, _ptr(queries), len(queries), _ptr(params), _ptr(prev_matched),
            _ptr(m12), C.byref(nm)))
        return nm.value, m12


def init_queries(keys, desc):
    """INIT_QUERY records of a frame's undistorted keypoints (KP_DTYPE) and descriptors."""
    q = np.zeros(len(keys), INIT_QUERY_DTYPE)
    q["angle"] = keys["angle"]
    q["octave"] = keys["octave"]
    q["desc"] = np.asarray(desc, np.uint8).reshape(-1, 32)
    return q


def init_search(nnratio, window_size, check_ori):
    p = np.zeros(1, INIT_SEARCH_DTYPE)
    p["nnratio"], p["window_size"], p["check_ori"] = nnratio, window_size, 1 if check_ori else 0
    return p


def _io_check(rc, what):
    if rc != 0:
        raise SlamGpuError(f"{what} ({rc}): {lib().slamgpu_io_last_error().decode()}")


def png_decode(data: bytes):
    """slamgpu_png_decode: an in-memory PNG -> uint8 array (h, w) or (h, w, c), channels in
    cv::imread(IMREAD_UNCHANGED) order (include/slamgpu_io.h)."""
    buf = np.frombuffer(data, np.uint8)
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    _io_check(lib().slamgpu_png_info(_ptr(buf), buf.size, C.byref(w), C.byref(h), C.byref(c)),
              "slamgpu_png_info")
    out = np.zeros((h.value, w.value * c.value), np.uint8)
    _io_check(lib().slamgpu_png_decode(_ptr(buf), buf.size, _ptr(out), out.strides[0], out.size,
                                       C.byref(w), C.byref(h), C.byref(c)), "slamgpu_png_decode")
    return out if c.value == 1 else out.reshape(h.value, w.value, c.value)


def imread_png(path: str):
    """cv::imread(path, CV_LOAD_IMAGE_UNCHANGED) of a PNG file (main_stereo.cpp:105-106)."""
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    p = path.encode()
    _io_check(lib().slamgpu_imread_png(p, None, 0, 0, C.byref(w), C.byref(h), C.byref(c)),
              "slamgpu_imread_png")
    out = np.zeros((h.value, w.value * c.value), np.uint8)
    _io_check(lib().slamgpu_imread_png(p, _ptr(out), out.strides[0], out.size, C.byref(w),
                                       C.byref(h), C.byref(c)), "slamgpu_imread_png")
    return out if c.value == 1 else out.reshape(h.value, w.value, c.value)


def kitti_load_images(kitti_path: str):
    """LoadKittiImages (main_stereo.cpp:16-49): (left paths, right paths, timestamps)."""
    n = C.c_int()
    p = kitti_path.encode()
    _io_check(lib().slamgpu_kitti_load_images(p, None, 0, C.byref(n)), "slamgpu_kitti_load_images")
    ts = np.zeros(n.value, np.float64)
    _io_check(lib().slamgpu_kitti_load_images(p, _ptr(ts), n.value, C.byref(n)),
              "slamgpu_kitti_load_images")
    paths = {2: [], 3: []}
    buf = C.create_string_buffer(len(p) + 64)
    for cam in (2, 3):
        for i in range(n.value):
            _io_check(lib().slamgpu_kitti_image_path(p, cam, i, buf, len(buf)),
                      "slamgpu_kitti_image_path")
            paths[cam].append(buf.value.decode())
    return paths[2], paths[3], ts


def undistort_points(cam, dist_coef, xy):
    """cv::undistortPoints(xy, ., K, DistCoef, noArray(), K) (host entry point)."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dist_coef, np.float32)
    out = np.zeros_like(xy)
    cm = Camera(*cam)
    rc = lib().slamgpu_undistort_points(C.byref(cm), _ptr(d), d.size, _ptr(xy), _ptr(out),
                                        len(xy))
    if rc != 0:
        raise SlamGpuError(f"slamgpu_undistort_points: {rc}")
    return out


def undistort_keypoints_device(cam, dist_coef, d_in, in_stride, d_counts, counts_stride, d_out,
                               out_stride, n_sets, max_kps, stream=None):
    """Batched device Frame::UndistortKeyPoints over n_sets keypoint sets (torch tensors or
    device pointers)."""
    d = np.ascontiguousarray(dist_coef, np.float32)
    cm = Camera(*cam)
    rc = lib().slamgpu_undistort_keypoints_device(C.byref(cm), _ptr(d), d.size, _ptr(d_in),
                                                  in_stride, _ptr(d_counts), counts_stride,
                                                  _ptr(d_out), out_stride, n_sets, max_kps,
                                                  C.c_void_p(stream or 0))
    if rc != 0:
        raise SlamGpuError(f"slamgpu_undistort_keypoints_device: {rc}")


class ORBextractor:
    """Reference-shaped ORBextractor (orb_extractor.h:25-93) on the MI355X path.

    The device context is sized per image size, so it is created on the first Compute() and
    re-created if the image size changes."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0):
        self.args = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        self.nlevels = nlevels
        self.scaleFactor = scaleFactor
        self.device = device
        self.ctx = None

    def _ctx(self, cols, rows):
        if self.ctx is None or (self.ctx.cols, self.ctx.rows) != (cols, rows):
            n, s, l, ini, mn = self.args
            self.ctx = Context(cols, rows, n, s, l, ini, mn, max_frames=1, device=self.device)
        return self.ctx

    def Compute(self, image, mask=None):
        """Returns (keypoints[N] as KP_DTYPE, descriptors N x 32 u8); empty image -> None."""
        image = np.asarray(image)
        if image.size == 0:
            return None
        assert image.dtype == np.uint8 and image.ndim == 2
        return self._ctx(image.shape[1], image.shape[0]).extract(image)

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.scaleFactor

    def _tables(self):
        return (self.ctx or Context(256, 256, *self.args, max_frames=1)).scale_tables()

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def GetImagePyramid(self):
        return [self.ctx.pyramid_level(0, l) for l in range(self.nlevels)]


def reloc_pose(Tcw, th, orb_dist, check_ori):
    """RELOC_POSE record of a 4x4 camera pose: Rcw, tcw and Ow = -Rcw.t() * tcw (products and sum
    in double, one rounding to float: slamgpu_adapter::reloc_camera_center)."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    p = np.zeros(1, RELOC_POSE_DTYPE)
    p["Rcw"] = T[:3, :3].reshape(-1)
    p["tcw"] = T[:3, 3]
    for k in range(3):
        p["Ow"][0, k] = -(float(T[0, k]) * float(T[0, 3]) + float(T[1, k]) * float(T[1, 3]) +
                          float(T[2, k]) * float(T[2, 3]))
    p["th"], p["orb_dist"], p["check_ori"] = th, int(orb_dist), int(bool(check_ori))
    return p


def reloc_queries(kf, already_found, Tcw, th, orb_dist, check_ori):
    """The keyframe's GetMapPointMatches() in keypoint order as RELOC_QUERY records (skip = no
    point, or in already_found) and the RELOC_POSE record."""
    mps = np.asarray(kf.map_points, np.int64)
    q = np.zeros(len(mps), RELOC_QUERY_DTYPE)
    q["kf_angle"] = np.asarray(kf.keypoints)["angle"]
    found = set(int(i) for i in already_found)
    for i, m in enumerate(mps):
        m = int(m)
        if m < 0 or m in found:
            q["skip"][i] = 1
            continue
        xyz, max_dist, min_dist, desc = kf.points[m]
        q["xyz"][i], q["max_dist"][i], q["min_dist"][i], q["desc"][i] = xyz, max_dist, min_dist, desc
        q["mp_id"][i] = m
    return q, reloc_pose(Tcw, th, orb_dist, check_ori)


class OrbMatcher:
    """Reference-shaped OrbMatcher (orb_matcher.h:14-119) for the per-frame searches."""
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        return lib().slamgpu_descriptor_distance(_ptr(a), _ptr(b))

    def SearchByBoW(self, kf, F):
        """SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (orb_matcher.cpp:133-262).
        kf: .descriptors, .keypoints, .feature_vec (bow.FeatureVector), .map_points (map point id
        per keypoint, -1 = none; a bad point counts as none); F: .descriptors, .keypoints,
        .feature_vec. Returns (nmatches, vpMapPointMatches as ids per F keypoint, -1 = none)."""
        from . import bow
        mps = np.asarray(kf.map_points, np.int64)
        nm, m = bow.search_by_bow(kf.descriptors, kf.keypoints, mps >= 0, kf.feature_vec,
                                  F.descriptors, F.keypoints, F.feature_vec, kf_kf=False,
                                  nnratio=self.mfNNratio, check_ori=self.mbCheckOrientation)
        out = np.full(len(F.descriptors), -1, np.int64)
        sel = m >= 0
        out[m[sel]] = mps[sel]
        return nm, out

    def SearchByBoWKeyFrames(self, kf1, kf2):
        """SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (orb_matcher.cpp:499-632).
        Returns (nmatches, vpMatches12 as kf2 map point ids per kf1 keypoint, -1 = none)."""
        from . import bow
        mp1 = np.asarray(kf1.map_points, np.int64)
        mp2 = np.asarray(kf2.map_points, np.int64)
        nm, m = bow.search_by_bow(kf1.descriptors, kf1.keypoints, mp1 >= 0, kf1.feature_vec,
                                  kf2.descriptors, kf2.keypoints, kf2.feature_vec,
                                  b_valid=mp2 >= 0, kf_kf=True, nnratio=self.mfNNratio,
                                  check_ori=self.mbCheckOrientation)
        out = np.full(len(kf1.descriptors), -1, np.int64)
        sel = m >= 0
        out[sel] = mp2[m[sel]]
        return nm, out


    def SearchForTriangulation(self, kf1, kf2, F12, cam, levels, bOnlyStereo=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
        (orb_matcher.cpp:634-802). kf: .keypoints, .descriptors, .u_right, .map_points (-1 =
        none), .feature_vec, .Tcw. Returns (nmatches, vMatchedPairs as an (n, 2) array)."""
        from . import kfmatch as K
        a = K.host_kf(kf1.keypoints, kf1.descriptors, kf1.u_right, kf1.Tcw,
                      np.asarray(kf1.map_points) >= 0, kf1.feature_vec)
        b = K.host_kf(kf2.keypoints, kf2.descriptors, kf2.u_right, kf2.Tcw,
                      np.asarray(kf2.map_points) >= 0, kf2.feature_vec)
        nm, m = K.search_for_triangulation(a, b, F12, cam, levels, bOnlyStereo,
                                           self.mbCheckOrientation)
        i = np.nonzero(m >= 0)[0]
        return nm, np.stack([i, m[i]], 1)

    def Fuse(self, kf, points, th, cam, levels, grid):
        """Fuse(pKF, vpMapPoints, th) (orb_matcher.cpp:804-954): the per-point candidate search
        on the device; returns (nfused, best_idx) -- kfmatch.fuse_apply walks it as the
        reference does."""
        from . import kfmatch as K
        k = K.host_kf(kf.keypoints, kf.descriptors, kf.u_right, kf.Tcw)
        nf, bi, _ = K.fuse(k, points, th, cam, levels, grid)
        return nf, bi

    def SearchBySim3(self, kf1, kf2, vpMatches12, s12, R12, t12, th, cam, levels, grid):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (orb_matcher.cpp:1081-1310).
        kf: .keypoints, .descriptors, .Tcw, .map_points (id per feature, -1 = none or bad),
        .mp_records (one FUSE_POINT record per feature). vpMatches12: kf2 map point id per kf1
        feature (-1 = none), updated in place where both directions agree. Returns nFound."""
        from . import kfmatch as K
        mp1, mp2 = np.asarray(kf1.map_points, np.int64), np.asarray(kf2.map_points, np.int64)
        m12 = np.asarray(vpMatches12)
        already1 = m12 >= 0
        already2 = np.zeros(len(mp2), bool)
        # GetIndexInKeyFrame(pKF2) of the points already matched (:1116-1126)
        pos2 = {int(m): i for i, m in enumerate(mp2) if m >= 0}
        for m in m12[already1]:
            if int(m) in pos2:
                already2[pos2[int(m)]] = True

        def host(kf):
            T = np.asarray(kf.Tcw, np.float32)
            return K.host_kf_pose(kf.keypoints, kf.descriptors, T[:3, :3], T[:3, 3],
                                  K.camera_center(T))

        def records(kf, mps):
            r = np.ascontiguousarray(kf.mp_records).view(K.FUSE_POINT_DTYPE).copy()
            r["skip"] = (r["skip"] != 0) | (mps < 0)
            return r
        nf, match12, _, _ = K.search_by_sim3(host(kf1), host(kf2), records(kf1, mp1),
                                             records(kf2, mp2), already1, already2,
                                             K.relative_sim3(s12, R12, t12), th, cam, levels, grid)
        sel = match12 >= 0
        vpMatches12[sel] = mp2[match12[sel]]
        return nf

    def SearchByProjectionSim3(self, kf, Scw, points, vpMatched, th, cam, levels, grid,
                               point_ids=None):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (orb_matcher.cpp:384-497).
        points: FUSE_POINT records (skip = isBad() or already in vpMatched); vpMatched: map point
        id per keypoint (-1 = none), updated in place with point_ids[i] (default i) of the
        claiming point. Returns nmatches."""
        from . import kfmatch as K
        k = K.host_kf_pose(kf.keypoints, kf.descriptors, *K.decompose_scw(Scw))
        nm, kp_point, _ = K.search_by_projection_sim3(k, points, np.asarray(vpMatched) >= 0, th,
                                                      cam, levels, grid)
        sel = kp_point >= 0
        ids = np.arange(len(points)) if point_ids is None else np.asarray(point_ids)
        vpMatched[sel] = ids[kp_point[sel]]
        return nm

    def SearchByProjectionReloc(self, ctx, frame, kf, already_found, th, ORBdist, Tcw,
                                vpMapPoints):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
        (orb_matcher.cpp:1455-1582) on frame `frame` of `ctx`'s last frame call.
        kf: .keypoints (undistorted, for the angles), .map_points (map point id per keypoint, -1 =
        none or bad), .points (dict id -> (xyz, max_dist, min_dist, desc[32])); already_found: ids
        of sAlreadyFound; Tcw: the frame's 4x4 pose; vpMapPoints: the frame's map point id per
        keypoint (int32, -1 = none), updated in place. Returns nmatches."""
        q, pose = reloc_queries(kf, already_found, Tcw, th, ORBdist, self.mbCheckOrientation)
        blocked = np.zeros(len(vpMapPoints), np.uint8)
        return ctx.search_by_projection_reloc(frame, q, pose, vpMapPoints, blocked)

    def SearchForInitialization(self, ctx, frame, F1, vbPrevMatched, windowSize=10):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
        (orb_matcher.cpp:264-382) with F2 = frame `frame` of `ctx`'s last frame call.
        F1: .keypoints (undistorted, KP_DTYPE) and .descriptors of the initial frame;
        vbPrevMatched: float32 [n1][2], updated in place. Returns (nmatches, vnMatches12)."""
        q = init_queries(F1.keypoints, F1.descriptors)
        p = init_search(self.mfNNratio, int(windowSize), self.mbCheckOrientation)
        return ctx.search_for_initialization(frame, q, p, vbPrevMatched)

    def FuseSim3(self, kf, Scw, points, th, cam, levels, grid):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (orb_matcher.cpp:956-1079): the per-point
        candidate search on the device; returns (nfused, best_idx) -- kfmatch.fuse_sim3_apply
        does the reference's tail (vpReplacePoint / AddObservation) over it."""
        from . import kfmatch as K
        k = K.host_kf_pose(kf.keypoints, kf.descriptors, *K.decompose_scw(Scw))
        nf, bi, _ = K.fuse_sim3(k, points, th, cam, levels, grid)
        return nf, bi


def _opt_check(rc):
    if rc != 0:
        raise SlamGpuError(f"slamgpu optimizer error {rc}: "
                           f"{lib().slamgpu_optimizer_last_error().decode()}")


class Optimizer:
    """The reference's Optimizer (src/optimizer/optimizer.h:13-50) for the hot path.

    PoseOptimization takes the frame's correspondences as POSE_EDGE_DTYPE records (map point
    world position, undistorted keypoint, right coordinate or -1, octave) instead of a Frame&:
    the caller's Frame -> edge gather is optimizer.cpp:239-309 without the g2o objects."""

    @staticmethod
    def PoseOptimization(edges, Tcw, cam, inv_sigma2):
        """Optimizer::PoseOptimization (optimizer.cpp:209-411). Returns (n_inliers, Tcw', outlier):
        the reference's return value, the optimised pose (f32 4x4; the input pose when fewer
        than 3 edges) and Frame::mvbOutlier for the edges."""
        edges = np.ascontiguousarray(edges, dtype=POSE_EDGE_DTYPE)
        T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(4, 4)).copy()
        isig = np.ascontiguousarray(inv_sigma2, np.float32)
        outl = np.zeros(len(edges), np.uint8)
        n_inl = C.c_int()
        _opt_check(lib().slamgpu_pose_optimization(C.byref(Camera(*cam)), _ptr(isig), len(isig),
                                                   _ptr(edges), len(edges), _ptr(T), _ptr(outl),
                                                   C.byref(n_inl)))
        return n_inl.value, T, outl.astype(bool)

    @staticmethod
    def LocalBundleAdjustment(kf_Tcw, kf_mode, points, point_obs_start, obs, cam, inv_sigma2,
                              stop_flag=False):
        """Optimizer::LocalBundleAdjustment (optimizer.cpp:413-716) on the gathered graph.
        kf_mode per keyframe: 0 local, 1 local fixed (id 0), 2 fixed camera; observations
        grouped by point (CSR point_obs_start). stop_flag: a bool, or a ctypes.c_bool that
        another thread may raise mid-run (the reference's bool* stop_flag). Returns (kf_Tcw',
        points', erase, lm_iterations); erase marks the reference's vToErase observations."""
        kf = np.ascontiguousarray(np.asarray(kf_Tcw, np.float32).reshape(-1, 4, 4)).copy()
        mode = np.ascontiguousarray(kf_mode, np.uint8)
        pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3)).copy()
        start = np.ascontiguousarray(point_obs_start, np.int32)
        ob = np.ascontiguousarray(obs, dtype=BA_OBS_DTYPE)
        isig = np.ascontiguousarray(inv_sigma2, np.float32)
        erase = np.zeros(max(len(ob), 1), np.uint8)
        its = C.c_int()
        # a ctypes.c_bool stays live: another thread may raise it while the call runs
        stop = stop_flag if isinstance(stop_flag, C.c_bool) else C.c_bool(bool(stop_flag))
        _opt_check(lib().slamgpu_local_bundle_adjustment(
            C.byref(Camera(*cam)), _ptr(isig), len(isig), _ptr(kf), _ptr(mode), len(mode),
            _ptr(pts), len(pts), _ptr(start), _ptr(ob), C.byref(stop), _ptr(erase),
            C.byref(its)))
        return kf, pts, erase[:len(ob)].astype(bool), its.value

    @staticmethod
    def OptimizeSim3(matches, S12, K1, K2, inv_sigma2_1, inv_sigma2_2, th2=10.0, fix_scale=False):
        """Optimizer::OptimizeSim3 (optimizer.cpp:962-1152) on the gathered correspondences
        (SIM3_MATCH_DTYPE: both points in their cameras' frames, both undistorted keypoints and
        octaves). S12: the g2o::Sim3 as (qx, qy, qz, qw, tx, ty, tz, s). Returns (n_inliers,
        S12', inlier): the reference's return value, the optimised Sim3 (the input one on the
        early return) and False where the reference nulls vpMatches1."""
        K1, K2, i1, i2 = _sim3_args(K1, K2, inv_sigma2_1, inv_sigma2_2)
        m = np.ascontiguousarray(matches, dtype=SIM3_MATCH_DTYPE)
        S = np.ascontiguousarray(S12, np.float64).copy()
        inl = np.zeros(max(len(m), 1), np.uint8)
        n_in = C.c_int()
        _opt_check(lib().slamgpu_optimize_sim3(_ptr(K1), _ptr(K2), _ptr(i1), _ptr(i2), len(i1),
                                               _ptr(m), len(m), float(th2), int(bool(fix_scale)),
                                               _ptr(S), _ptr(inl), C.byref(n_in)))
        return n_in.value, S, inl[:len(m)].astype(bool)

    @staticmethod
    def OptimizeEssentialGraph(Scw, fixed, edges, fix_scale=True, n_iterations=20, points=None,
                               point_ref=None):
        """Optimizer::OptimizeEssentialGraph (optimizer.cpp:718-960) on the gathered graph:
        Scw [n][8] the vertices' vScw (keyframe id order), fixed [n] (1 for the loop keyframe),
        edges SIM3_EDGE_DTYPE in the reference's insertion order. points [m][3] / point_ref [m]
        (optional): map points and the keyframe index that corrects each. Returns (Scw' [n][8]
        the optimised CorrectedSiw, Tcw' [n][4][4] f32 [R t/s], points' or None,
        lm_iterations)."""
        S = np.ascontiguousarray(np.asarray(Scw, np.float64).reshape(-1, 8)).copy()
        fx = np.ascontiguousarray(fixed, np.uint8)
        E = np.ascontiguousarray(edges, dtype=SIM3_EDGE_DTYPE)
        T = np.zeros((max(len(S), 1), 4, 4), np.float32)
        P = None if points is None else \
            np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3)).copy()
        ref = None if points is None else np.ascontiguousarray(point_ref, np.int32)
        its = C.c_int()
        _opt_check(lib().slamgpu_optimize_essential_graph(
            len(S), _ptr(S), _ptr(fx), _ptr(E), len(E), int(bool(fix_scale)), int(n_iterations),
            _ptr(T), _ptr(P), _ptr(ref), 0 if P is None else len(P), C.byref(its)))
        return S, T[:len(S)], P, its.value

    @staticmethod
    def BundleAdjustment(kf_Tcw, kf_mode, points, point_obs_start, obs, cam, inv_sigma2,
                         n_iterations=10, robust=True, stop_flag=False):
        """Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (optimizer.cpp:18-207) on the
        gathered graph: kf_mode 1 for the keyframe with id 0 (fixed), 0 for the others. Returns
        (kf_Tcw', points', lm_iterations)."""
        kf = np.ascontiguousarray(np.asarray(kf_Tcw, np.float32).reshape(-1, 4, 4)).copy()
        mode = np.ascontiguousarray(kf_mode, np.uint8)
        pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3)).copy()
        start = np.ascontiguousarray(point_obs_start, np.int32)
        ob = np.ascontiguousarray(obs, dtype=BA_OBS_DTYPE)
        isig = np.ascontiguousarray(inv_sigma2, np.float32)
        its = C.c_int()
        stop = stop_flag if isinstance(stop_flag, C.c_bool) else C.c_bool(bool(stop_flag))
        _opt_check(lib().slamgpu_global_bundle_adjustment(
            C.byref(Camera(*cam)), _ptr(isig), len(isig), _ptr(kf), _ptr(mode), len(mode),
            _ptr(pts), len(pts), _ptr(start), _ptr(ob), int(n_iterations), int(bool(robust)),
            C.byref(stop), C.byref(its)))
        return kf, pts, its.value


def _sim3_args(K1, K2, inv_sigma2_1, inv_sigma2_2):
    K1 = np.ascontiguousarray(np.asarray(K1, np.float32)[:4])
    K2 = np.ascontiguousarray(np.asarray(K2, np.float32)[:4])
    i1 = np.ascontiguousarray(inv_sigma2_1, np.float32)
    i2 = np.ascontiguousarray(inv_sigma2_2, np.float32)
    if len(i1) != len(i2):
        raise ValueError("both keyframes need the same number of levels")
    return K1, K2, i1, i2


def optimize_sim3_device(K1, K2, inv_sigma2_1, inv_sigma2_2, d_matches, d_match_start,
                         n_problems, d_S12, d_inlier, d_n_inliers, th2=10.0, fix_scale=False,
                         d_lm_iterations=None, stream=None):
    """slamgpu_optimize_sim3_device: OptimizeSim3 for a batch of loop candidates in HBM."""
    K1, K2, i1, i2 = _sim3_args(K1, K2, inv_sigma2_1, inv_sigma2_2)
    _opt_check(lib().slamgpu_optimize_sim3_device(
        _ptr(K1), _ptr(K2), _ptr(i1), _ptr(i2), len(i1), _ptr(d_matches), _ptr(d_match_start),
        n_problems, float(th2), int(bool(fix_scale)), _ptr(d_S12), _ptr(d_inlier),
        _ptr(d_n_inliers), _ptr(d_lm_iterations), C.c_void_p(stream) if stream else None))


def _s3_check(rc):
    if rc != 0:
        raise SlamGpuError(f"slamgpu sim3solver error {rc}: "
                           f"{lib().slamgpu_sim3solver_last_error().decode()}")


def sim3_ransac_device(K1, K2, sigma2_1, sigma2_2, d_matches, n_matches_total, d_draws,
                       n_draws_total, d_jobs, n_jobs, max_n, max_its, d_hyp, d_inlier_bits,
                       d_events, d_n_events, stream=None):
    """slamgpu_sim3_ransac_device: the whole RANSAC schedule of a batch of loop candidates in HBM
    (jobs SIM3_RANSAC_JOB_DTYPE; hyp [n_jobs][max_its] SIM3_HYP_DTYPE; inlier_bits
    [n_jobs][max_its][ceil(max_n / 64)] int64/uint64; events [n_jobs][max_its], n_events [n_jobs]
    int32). sigma2_*: level_sigma_sq, not the inverse."""
    K1, K2, s1, s2 = _sim3_args(K1, K2, sigma2_1, sigma2_2)
    _s3_check(lib().slamgpu_sim3_ransac_device(
        _ptr(K1), _ptr(K2), _ptr(s1), _ptr(s2), len(s1), _ptr(d_matches), int(n_matches_total),
        _ptr(d_draws), int(n_draws_total), _ptr(d_jobs), int(n_jobs), int(max_n), int(max_its),
        _ptr(d_hyp), _ptr(d_inlier_bits), _ptr(d_events), _ptr(d_n_events),
        C.c_void_p(stream) if stream else None))


def sim3_ransac(matches, draws, n_its, min_inliers, fix_scale, K1, K2, sigma2_1, sigma2_2):
    """slamgpu_sim3_ransac (synchronous, one candidate): returns (hyp[n_its] SIM3_HYP_DTYPE,
    inlier_bits[n_its][ceil(n / 64)] uint64, events[n_events])."""
    K1, K2, s1, s2 = _sim3_args(K1, K2, sigma2_1, sigma2_2)
    m = np.ascontiguousarray(matches, dtype=SIM3_MATCH_DTYPE)
    d = np.ascontiguousarray(draws, np.int32).reshape(-1)
    n, rows = len(m), max(int(n_its), 1)
    if len(d) < 3 * int(n_its):
        raise ValueError("three draws per iteration are needed")
    hyp = np.zeros(rows, SIM3_HYP_DTYPE)
    bits = np.zeros((rows, max((n + 63) // 64, 1)), np.uint64)
    events = np.zeros(rows, np.int32)
    ne = C.c_int()
    _s3_check(lib().slamgpu_sim3_ransac(_ptr(K1), _ptr(K2), _ptr(s1), _ptr(s2), len(s1), _ptr(m), n,
                                        _ptr(d), int(n_its), int(min_inliers),
                                        int(bool(fix_scale)), _ptr(hyp), _ptr(bits), _ptr(events),
                                        C.byref(ne)))
    return hyp[:n_its], bits[:n_its], events[:ne.value].copy()


def sim3_ransac_iterations(n, probability=0.99, min_inliers=6, max_its=300):
    """The effective mRansacMaxIts of Sim3Solver::SetRansacParameters (sim3solver.cpp:127-137):
    float epsilon, double log / pow, N == minInliers -> 1, max(1, min(...)). A quotient that is
    not a positive int (epsilon >= 1 or 0) converts to INT_MIN in the reference's build: 1."""
    import math
    if min_inliers == n:
        return max(1, min(1, int(max_its)))
    if n <= 0:
        return 1
    eps = float(np.float32(np.float32(min_inliers) / np.float32(n)))
    try:
        its = math.ceil(math.log(1 - probability) / math.log(1 - eps ** 3))
    except (ValueError, ZeroDivisionError, OverflowError):
        return 1
    if not 1 <= its <= 2147483647:
        return 1
    return max(1, min(its, int(max_its)))


_libc = None


def reference_random_int(lo, hi):
    """DUtils::Random::RandomInt (DUtils/Random.cpp:47-50) on the C library's rand()."""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
    d = hi - lo + 1
    return int((_libc.rand() / (2147483647 + 1.0)) * d) + lo


class Sim3Solver:
    """The reference's Sim3Solver (src/solvers/sim3solver.h) over gathered correspondences
    (SIM3_MATCH_DTYPE as Optimizer.OptimizeSim3 takes them; indices1 = mvnIndices1, the pKF1
    feature of each, n1 = mN1 = len(vpMatched12)). SetRansacParameters draws the WHOLE schedule
    with random_int(min, max) -- in the order the reference would consume the draws for this
    solver alone -- and evaluates it in one synchronous device call; iterate / find replay
    sim3solver.cpp:142-217 over the per-hypothesis counts and events without touching the points
    again. The constructor only records the reference's default parameters (0.99, 6, 300): they
    are evaluated by the first iterate if SetRansacParameters was never called."""

    def __init__(self, matches, K1, K2, sigma2_1, sigma2_2, fix_scale=True, indices1=None,
                 n1=None, random_int=None):
        self.matches = np.ascontiguousarray(matches, dtype=SIM3_MATCH_DTYPE)
        self.N = len(self.matches)
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = self.N if n1 is None else int(n1)
        self._cam = (K1, K2, sigma2_1, sigma2_2)
        self.fix_scale = bool(fix_scale)
        self.random_int = random_int or reference_random_int
        self._params = (0.99, 6, 300)
        self._evaluated = False
        self.mnIterations = 0
        self.last_k = -1

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self._params = (probability, minInliers, maxIterations)
        self.mRansacMinInliers = int(minInliers)
        self.mRansacMaxIts = sim3_ransac_iterations(self.N, probability, minInliers, maxIterations)
        self.mnIterations = 0
        self._evaluated = True
        self.draws = np.zeros((self.mRansacMaxIts, 3), np.int32)
        self.hyp = self.bits = self.events = None
        if self.N < self.mRansacMinInliers or self.N < 3:
            return  # iterate returns at once (:151-154): nothing is drawn
        if self.mRansacMaxIts > SIM3_RANSAC_MAX_ITS:
            raise SlamGpuError(f"maxIterations above {SIM3_RANSAC_MAX_ITS}")
        for k in range(self.mRansacMaxIts):
            for i in range(3):
                self.draws[k, i] = self.random_int(0, self.N - 1 - i)
        self.hyp, self.bits, self.events = sim3_ransac(
            self.matches, self.draws, self.mRansacMaxIts, self.mRansacMinInliers, self.fix_scale,
            *self._cam)

    def _scatter(self, k):
        vb = np.zeros(self.mN1, bool)
        row = np.unpackbits(self.bits[k].view(np.uint8), bitorder="little")[:self.N].astype(bool)
        vb[self.indices1[row]] = True
        return vb

    def _T12(self, k):
        h = self.hyp[k]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.float32(h["s12"]) * h["R12"].reshape(3, 3)
        T[:3, 3] = h["t12"]
        return T

    def iterate(self, nIterations):
        """Returns (T12 4x4 f32 or None, bNoMore, vbInliers[mN1], nInliers)."""
        if not self._evaluated:
            self.SetRansacParameters(*self._params)
        vb = np.zeros(self.mN1, bool)
        self.last_k = -1
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        if self.hyp is None:
            raise SlamGpuError("fewer than 3 correspondences")
        start = self.mnIterations
        end = min(self.mRansacMaxIts, start + max(int(nIterations), 0))
        j = int(np.searchsorted(self.events, start))
        if j < len(self.events) and self.events[j] < end:
            k = int(self.events[j])
            self.mnIterations = k + 1
            self.last_k = k
            return self._T12(k), False, self._scatter(k), int(self.hyp["n_inliers"][k])
        self.mnIterations = end
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self):
        """Returns (T12 or None, vbInliers12, nInliers)."""
        if not self._evaluated:
            self.SetRansacParameters(*self._params)
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def _best(self):
        """The iteration mBest* hold: the last one, among those run, that reached the running
        maximum (the >= of :186); None before the first."""
        if not self._evaluated or self.hyp is None or self.mnIterations == 0:
            return None
        c = self.hyp["n_inliers"][:self.mnIterations]
        return int(len(c) - 1 - np.argmax(c[::-1]))

    def GetEstimatedRotation(self):
        k = self._best()
        return None if k is None else self.hyp["R12"][k].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        k = self._best()
        return None if k is None else self.hyp["t12"][k].copy()

    def GetEstimatedScale(self):
        k = self._best()
        return None if k is None else float(self.hyp["s12"][k])


def _pnp_check(rc):
    if rc != 0:
        raise SlamGpuError(f"slamgpu pnpsolver error {rc}: "
                           f"{lib().slamgpu_pnpsolver_last_error().decode()}")


def _pnp_args(K, sigma2):
    K = np.ascontiguousarray(K, np.float32).reshape(-1)
    if len(K) != 4:
        raise ValueError("K = (fx, fy, cx, cy)")
    return K, np.ascontiguousarray(sigma2, np.float32).reshape(-1)


def pnp_ransac_device(K, sigma2, th2, d_matches, n_matches_total, d_draws, n_draws_total, d_jobs,
                      n_jobs, max_n, max_its, d_hyp, d_inlier_bits, d_refined, d_refined_bits,
                      d_events, d_n_events, stream=None):
    """slamgpu_pnp_ransac_device: the whole RANSAC EPnP schedule of a batch of relocalisation
    candidates in HBM (matches PNP_MATCH_DTYPE; jobs PNP_JOB_DTYPE; hyp and refined
    [n_jobs][max_its] PNP_HYP_DTYPE; inlier_bits and refined_bits
    [n_jobs][max_its][ceil(max_n / 64)] int64/uint64; events [n_jobs][max_its], n_events [n_jobs]
    int32). sigma2: level_sigma_sq, not the inverse."""
    K, s = _pnp_args(K, sigma2)
    _pnp_check(lib().slamgpu_pnp_ransac_device(
        _ptr(K), _ptr(s), len(s), float(th2), _ptr(d_matches), int(n_matches_total), _ptr(d_draws),
        int(n_draws_total), _ptr(d_jobs), int(n_jobs), int(max_n), int(max_its), _ptr(d_hyp),
        _ptr(d_inlier_bits), _ptr(d_refined), _ptr(d_refined_bits), _ptr(d_events),
        _ptr(d_n_events), C.c_void_p(stream) if stream else None))


def pnp_ransac(matches, draws, n_its, min_inliers, K, sigma2, th2=5.991):
    """slamgpu_pnp_ransac (synchronous, one candidate): returns (hyp[n_its] PNP_HYP_DTYPE,
    inlier_bits[n_its][ceil(n / 64)] uint64, refined[n_its], refined_bits[n_its][...],
    events[n_events])."""
    K, s = _pnp_args(K, sigma2)
    m = np.ascontiguousarray(matches, dtype=PNP_MATCH_DTYPE)
    d = np.ascontiguousarray(draws, np.int32).reshape(-1)
    n, rows = len(m), max(int(n_its), 1)
    if len(d) < 4 * int(n_its):
        raise ValueError("four draws per iteration are needed")
    words = max((n + 63) // 64, 1)
    hyp, refined = np.zeros(rows, PNP_HYP_DTYPE), np.zeros(rows, PNP_HYP_DTYPE)
    bits, rbits = np.zeros((rows, words), np.uint64), np.zeros((rows, words), np.uint64)
    events = np.zeros(rows, np.int32)
    ne = C.c_int()
    _pnp_check(lib().slamgpu_pnp_ransac(_ptr(K), _ptr(s), len(s), float(th2), _ptr(m), n, _ptr(d),
                                        int(n_its), int(min_inliers), _ptr(hyp), _ptr(bits),
                                        _ptr(refined), _ptr(rbits), _ptr(events), C.byref(ne)))
    return hyp[:n_its], bits[:n_its], refined[:n_its], rbits[:n_its], events[:ne.value].copy()


def pnp_ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                          epsilon=0.4):
    """The effective (mRansacMinInliers, mRansacMaxIts) of PnPsolver::SetRansacParameters
    (pnp_solver.cpp:87-105): int(N * float epsilon), the two lower bounds, the float epsilon
    raised to minInliers / N, pow(epsilon, 3) and log in double, N == minInliers -> 1. A quotient
    that is not a positive int converts to INT_MIN in the reference's build: 1."""
    import math
    if minSet != 4:
        raise SlamGpuError(f"PnPsolver: minSet {minSet} is not supported, the sample is 4 points")
    eps = np.float32(epsilon)
    n_min = max(int(np.float32(N) * eps), int(minInliers), int(minSet))
    if N > 0 and eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        return n_min, max(1, min(1, int(maxIterations)))
    try:
        its = math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3))
    except (ValueError, ZeroDivisionError, OverflowError):
        return n_min, 1
    if not 1 <= its <= 2147483647:
        return n_min, 1
    return n_min, max(1, min(its, int(maxIterations)))


class PnPsolver:
    """The reference's PnPsolver (src/solvers/pnp_solver.h) over gathered correspondences
    (PNP_MATCH_DTYPE; indices = mvKeyPointIndices, the frame keypoint of each; n_kp =
    len(vpMapPointMatches) for the scatter). SetRansacParameters draws the WHOLE schedule with
    random_int(min, max) -- in the order the reference would consume the draws for this solver
    alone -- and evaluates it in one synchronous device call; iterate / find replay
    pnp_solver.cpp:112-211 over the counts, the running bests, the refined rows and the events.
    The loop of :135 runs while mnIterations < mRansacMaxIts OR the call's own count < nIterations:
    a call that starts near the end runs past the schedule, so the solver appends draws and
    evaluates the longer schedule again (the prefix is the same draws, hence the same rows). The
    constructor only records the reference's default parameters: they are evaluated by the first
    iterate if SetRansacParameters was never called."""

    def __init__(self, matches, K, sigma2, indices=None, n_kp=None, random_int=None):
        self.matches = np.ascontiguousarray(matches, dtype=PNP_MATCH_DTYPE)
        self.N = len(self.matches)
        self.indices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self.n_kp = self.N if n_kp is None else int(n_kp)
        self._cam = (K, sigma2)
        self.random_int = random_int or reference_random_int
        self._params = (0.99, 8, 300, 4, 0.4, 5.991)
        self._evaluated = False
        self.mnIterations = 0
        self.device_calls = 0

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                            epsilon=0.4, th2=5.991):
        self._params = (probability, minInliers, maxIterations, minSet, epsilon, th2)
        self.mRansacMinInliers, self.mRansacMaxIts = pnp_ransac_parameters(
            self.N, probability, minInliers, maxIterations, minSet, epsilon)
        self.th2 = float(th2)
        self.mnIterations = 0
        self._evaluated = True
        self.draws = np.zeros((0, 4), np.int32)
        self.hyp = self.bits = self.refined = self.refined_bits = self.events = None
        if self.N < self.mRansacMinInliers:
            return  # iterate returns at once (:126-130): nothing is drawn
        self._extend(self.mRansacMaxIts)

    def _extend(self, n_its):
        """Draws up to n_its iterations and evaluates the schedule."""
        if n_its > PNP_RANSAC_MAX_ITS:
            raise SlamGpuError(f"PnPsolver: {n_its} iterations > PNP_RANSAC_MAX_ITS "
                               f"({PNP_RANSAC_MAX_ITS})")
        more = np.zeros((n_its - len(self.draws), 4), np.int32)
        for k in range(len(more)):
            for i in range(4):
                more[k, i] = self.random_int(0, self.N - 1 - i)
        self.draws = np.concatenate([self.draws, more])
        self.hyp, self.bits, self.refined, self.refined_bits, self.events = pnp_ransac(
            self.matches, self.draws, n_its, self.mRansacMinInliers, *self._cam, self.th2)
        self.device_calls += 1

    def _scatter(self, row):
        vb = np.zeros(self.n_kp, bool)
        on = np.unpackbits(row.view(np.uint8), bitorder="little")[:self.N].astype(bool)
        vb[self.indices[on]] = True
        return vb

    @staticmethod
    def _Tcw(h):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = h["Rcw"].reshape(3, 3)
        T[:3, 3] = h["tcw"]
        return T

    def iterate(self, nIterations):
        """Returns (Tcw 4x4 f32 or None, bNoMore, vbInliers[n_kp], nInliers)."""
        if not self._evaluated:
            self.SetRansacParameters(*self._params)
        vb = np.zeros(self.n_kp, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        start = self.mnIterations
        end = max(self.mRansacMaxIts, start + max(int(nIterations), 0))  # the || of :135
        while True:
            have = len(self.draws)
            j = int(np.searchsorted(self.events, start))
            if j < len(self.events) and self.events[j] < end:
                k = int(self.events[j])
                b = int(self.hyp["best"][k])
                self.mnIterations = k + 1
                return (self._Tcw(self.refined[b]), False, self._scatter(self.refined_bits[b]),
                        int(self.refined["n_inliers"][b]))
            if have >= end:
                break
            self._extend(end)
        self.mnIterations = end  # >= mRansacMaxIts >= 1: bNoMore (:194-196)
        b = int(self.hyp["best"][end - 1])
        if b >= 0:  # mnBestInliers >= mRansacMinInliers (:197)
            return (self._Tcw(self.hyp[b]), True, self._scatter(self.bits[b]),
                    int(self.hyp["n_inliers"][b]))
        return None, True, vb, 0

    def find(self):
        """Returns (Tcw or None, vbInliers, nInliers)."""
        if not self._evaluated:
            self.SetRansacParameters(*self._params)
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n


def _init_check(rc):
    if rc != 0:
        raise SlamGpuError(f"slamgpu initializer error {rc}: "
                           f"{lib().slamgpu_initializer_last_error().decode()}")


def init_ransac_device(d_keys1, d_matches12, n_keys1_total, d_keys2, n_keys2_total, d_draws,
                       n_draws_total, d_jobs, n_jobs, max_n1, max_its, d_hyp, d_bits, d_result,
                       d_pairs, d_motion, d_good_bits, d_p3d, stream=None):
    """slamgpu_init_ransac_device: the monocular Initializer of a batch of frame pairs in HBM
    (keys float32 [n][2]; matches12 int32; jobs INIT_JOB_DTYPE; hyp [n_jobs][2][max_its]
    INIT_HYP_DTYPE; bits [n_jobs][2][max_its][ceil(max_n1 / 64)] uint64; result [n_jobs]
    INIT_RESULT_DTYPE; pairs [n_jobs][max_n1][2] int32; motion [n_jobs][8] INIT_MOTION_DTYPE;
    good_bits [n_jobs][8][words] uint64; p3d [n_jobs][8][max_n1][3] float32)."""
    _init_check(lib().slamgpu_init_ransac_device(
        _ptr(d_keys1), _ptr(d_matches12), int(n_keys1_total), _ptr(d_keys2), int(n_keys2_total),
        _ptr(d_draws), int(n_draws_total), _ptr(d_jobs), int(n_jobs), int(max_n1), int(max_its),
        _ptr(d_hyp), _ptr(d_bits), _ptr(d_result), _ptr(d_pairs), _ptr(d_motion),
        _ptr(d_good_bits), _ptr(d_p3d), C.c_void_p(stream) if stream else None))


def init_ransac(keys1, keys2, matches12, K, sigma, draws, n_its):
    """slamgpu_init_ransac (synchronous, one pair of frames): returns (hyp[2][n_its]
    INIT_HYP_DTYPE, bits[2][n_its][ceil(n1 / 64)] uint64, result INIT_RESULT_DTYPE record,
    pairs[N][2], motion[n_motions] INIT_MOTION_DTYPE, good_bits[n_motions][words],
    p3d[n_motions][n1][3])."""
    k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
    m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    K = np.ascontiguousarray(K, np.float32).reshape(-1)
    d = np.ascontiguousarray(draws, np.int32).reshape(-1)
    if len(K) != 4:
        raise ValueError("K = (fx, fy, cx, cy)")
    if len(m) != len(k1):
        raise ValueError("one matches12 entry per key of frame 1")
    if len(d) < 8 * int(n_its):
        raise ValueError("eight draws per iteration are needed")
    n1, rows = len(k1), max(int(n_its), 1)
    words = max((n1 + 63) // 64, 1)
    hyp = np.zeros((2, rows), INIT_HYP_DTYPE)
    bits = np.zeros((2, rows, words), np.uint64)
    result = np.zeros(1, INIT_RESULT_DTYPE)
    pairs = np.zeros((max(n1, 1), 2), np.int32)
    motion = np.zeros(INIT_MAX_MOTIONS, INIT_MOTION_DTYPE)
    good = np.zeros((INIT_MAX_MOTIONS, words), np.uint64)
    p3d = np.zeros((INIT_MAX_MOTIONS, max(n1, 1), 3), np.float32)
    _init_check(lib().slamgpu_init_ransac(_ptr(k1), _ptr(m), n1, _ptr(k2), len(k2), _ptr(K),
                                          float(sigma), _ptr(d), int(n_its), _ptr(hyp), _ptr(bits),
                                          _ptr(result), _ptr(pairs), _ptr(motion), _ptr(good),
                                          _ptr(p3d)))
    r = result[0]
    nm = int(r["n_motions"])
    return hyp, bits, r, pairs[:int(r["n"])], motion[:nm], good[:nm], p3d[:nm, :n1]


_seeded_once = False


def seed_rand_once(seed):
    """DUtils::Random::SeedRandOnce(int) (DUtils/Random.cpp:38-45): srand(seed) the first time
    in the process."""
    global _libc, _seeded_once
    if not _seeded_once:
        if _libc is None:
            _libc = C.CDLL(None)
        _libc.srand(int(seed))
        _seeded_once = True


class Initializer:
    """The reference's Initializer (src/util/initializer.h): keys1 = the reference frame's
    undistorted keypoint positions [n1][2], K = (fx, fy, cx, cy). Initialize draws the schedule
    with random_int(min, max) as initializer.cpp:60-77 does (SeedRandOnce(0) first when the
    generator is the default rand()), evaluates it in ONE synchronous device call and replays
    :92-98 and the tails of ReconstructH / ReconstructF on the host."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, random_int=None):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        self.K = np.ascontiguousarray(K, np.float32).reshape(-1)
        self.sigma = float(sigma)
        self.iterations = int(iterations)
        self._default_rand = random_int is None
        self.random_int = random_int or reference_random_int
        self.device_calls = 0

    def Initialize(self, keys2, vMatches12, minParallax=1.0, minTriangulated=50):
        """Returns (ok, R21 3x3 f32, t21 f32[3], vP3D f32[n1][3], vbTriangulated bool[n1]); the
        last four are None when ok is False."""
        m = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        n1 = len(self.keys1)
        N = int((m >= 0).sum())
        if self._default_rand:
            seed_rand_once(0)
        draws = np.zeros((self.iterations, 8), np.int32)
        for k in range(self.iterations):
            for j in range(8):
                draws[k, j] = self.random_int(0, N - 1 - j)
        hyp, bits, r, pairs, motion, good, p3d = init_ransac(
            self.keys1, keys2, m, self.K, self.sigma, draws, self.iterations)
        self.device_calls += 1
        self.result, self.hyp, self.motion = r, hyp, motion
        fail = (False, None, None, None, None)
        model, nm = int(r["model"]), len(motion)
        b = int(r["best"][model])
        if b < 0 or nm == 0:  # FindFundamental's empty mask, or the early return of :601
            return fail
        Nin = int(np.unpackbits(bits[model, b].view(np.uint8), bitorder="little")[:N].sum())
        ng = motion["n_good"].astype(np.int64)
        cosv = motion["cos_parallax"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            parallax = np.where(ng > 0, np.float32(np.arccos(cosv) * 180 / np.pi),
                                np.float32(0)).astype(np.float32)
        minParallax = np.float32(minParallax)
        if model == 1:  # ReconstructF :495-565
            maxGood = int(ng.max())
            nMinGood = max(int(0.9 * Nin), minTriangulated)
            nsimilar = int((ng > 0.7 * maxGood).sum())
            if maxGood < nMinGood or nsimilar > 1:
                return fail
            i = int(np.argmax(ng == maxGood))
            if not parallax[i] > minParallax:
                return fail
        else:  # ReconstructH :693-735
            bestGood = secondBestGood = 0
            i, bestParallax = -1, np.float32(-1)
            for j in range(nm):
                if ng[j] > bestGood:
                    secondBestGood, bestGood, i, bestParallax = bestGood, int(ng[j]), j, parallax[j]
                elif ng[j] > secondBestGood:
                    secondBestGood = int(ng[j])
            if not (secondBestGood < 0.75 * bestGood and bestParallax >= minParallax
                    and bestGood > minTriangulated and bestGood > 0.9 * Nin):
                return fail
        vb = np.unpackbits(good[i].view(np.uint8), bitorder="little")[:n1].astype(bool)
        return (True, motion["R"][i].reshape(3, 3).copy(), motion["t"][i].copy(), p3d[i].copy(),
                vb)


def pose_optimization_device(cam, inv_sigma2, d_edges, d_edge_start, n_frames, d_Tcw, d_outlier,
                             d_n_inliers, d_lm_iterations=None, stream=None):
    """slamgpu_pose_optimization_device: PoseOptimization for a batch of frames in HBM."""
    isig = np.ascontiguousarray(inv_sigma2, np.float32)
    _opt_check(lib().slamgpu_pose_optimization_device(
        C.byref(Camera(*cam)), _ptr(isig), len(isig), _ptr(d_edges), _ptr(d_edge_start), n_frames,
        _ptr(d_Tcw), _ptr(d_outlier), _ptr(d_n_inliers), _ptr(d_lm_iterations),
        C.c_void_p(stream) if stream else None))


def local_ba_workspace_bytes(total_kf, total_points, total_obs):
    return int(lib().slamgpu_local_ba_workspace_bytes(total_kf, total_points, total_obs))


def local_bundle_adjustment_device(cam, inv_sigma2, d_problems, n_problems, d_kf_Tcw, d_kf_mode,
                                   d_points, d_point_obs_start, d_obs, d_erase, d_status,
                                   d_workspace, total_kf, total_points, total_obs,
                                   d_stop_flag=None, stream=None):
    """slamgpu_local_bundle_adjustment_device: LocalBundleAdjustment for a batch of problems."""
    isig = np.ascontiguousarray(inv_sigma2, np.float32)
    _opt_check(lib().slamgpu_local_bundle_adjustment_device(
        C.byref(Camera(*cam)), _ptr(isig), len(isig), _ptr(d_problems), n_problems,
        _ptr(d_kf_Tcw), _ptr(d_kf_mode), _ptr(d_points), _ptr(d_point_obs_start), _ptr(d_obs),
        _ptr(d_erase), _ptr(d_status), _ptr(d_workspace),
        int(d_workspace.numel() * d_workspace.element_size()), total_kf, total_points, total_obs,
        _ptr(d_stop_flag), C.c_void_p(stream) if stream else None))


def local_ba_linearize_device(cam, inv_sigma2, d_problems, n_problems, d_kf_Tcw, d_kf_mode,
                              d_points, d_point_obs_start, d_obs, out, d_status, d_workspace,
                              total_kf, total_points, total_obs, stream=None):
    """slamgpu_local_ba_linearize_device. `out`: dict of device tensors chi2, hpl, hll, bl, hpp,
    bp, chi (float64)."""
    isig = np.ascontiguousarray(inv_sigma2, np.float32)
    lin = BaLinear(*[int(out[n].data_ptr()) for n in ("chi2", "hpl", "hll", "bl", "hpp", "bp",
                                                      "chi")])
    _opt_check(lib().slamgpu_local_ba_linearize_device(
        C.byref(Camera(*cam)), _ptr(isig), len(isig), _ptr(d_problems), n_problems,
        _ptr(d_kf_Tcw), _ptr(d_kf_mode), _ptr(d_points), _ptr(d_point_obs_start), _ptr(d_obs),
        C.byref(lin), _ptr(d_status), _ptr(d_workspace),
        int(d_workspace.numel() * d_workspace.element_size()), total_kf, total_points, total_obs,
        C.c_void_p(stream) if stream else None))
