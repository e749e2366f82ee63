"""ctypes binding of libvo_hip.so (include/vo_hip.h).

There is no CPU fallback: if the library is missing, or no GPU is present when a
context is created, the caller gets an exception, never a silent slow path.
"""
import ctypes as C
import atexit
import os
import threading
import weakref

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvo_hip.so")

VO_OK, VO_EINVAL, VO_ENOMEM, VO_EHIP, VO_ECAPACITY, VO_ETRACKING = 0, -1, -2, -3, -4, -5
_CODES = {VO_EINVAL: "VO_EINVAL", VO_ENOMEM: "VO_ENOMEM", VO_EHIP: "VO_EHIP", VO_ECAPACITY: "VO_ECAPACITY",
          VO_ETRACKING: "VO_ETRACKING"}

# kernel ids (vo_hip.h)
K_HARRIS_RESPONSE, K_NMS_CANDIDATES, K_NMS_THRESHOLD, K_NMS_COMPACT, K_NMS_SELECT = 0, 1, 2, 3, 4
K_PATCH_DESC, K_PYR_DOWN, K_KLT_TRACK, K_DLT, K_P3P_SOLVE, K_P3P_SCORE, K_REPROJ, K_MATCH = 5, 6, 7, 8, 9, 10, 11, 12
K_SHI_TOMASI_CHAIN = 27
K_WINDOW_BA, K_WINDOW_BUILD = 28, 29          # vo_window_ba_dev's solver; vo_window_from_tracks_dev, both launches
K_TWOVIEW_HYP, K_TWOVIEW_SCORE = 30, 31      # f8_hyp_kernel / e5_hyp_kernel and f_score_kernel / e5_score_kernel
K_WINDOW_STRUCTURE = 32                       # vo_window_structure_dev, both launches
K_LOOP_RECORD, K_LOOP_JOIN, K_LOOP_WRITE = 33, 34, 35     # vo_structure_loop_post's three kernels
K_BRIEF_DESCRIBE, K_HAMMING_KNN2 = 36, 37                 # vo_brief_describe_dev / vo_hamming_knn2_dev
K_COUNT = 38


class VoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_CODES.get(code, "VO_E?"), code, msg))
        self.code = code


_lib = None
_lib_lock = threading.Lock()


class Pcg64(C.Structure):
    """NumPy PCG64 bit-generator state (vo_pcg64)."""
    _fields_ = [("state_hi", C.c_uint64), ("state_lo", C.c_uint64), ("inc_hi", C.c_uint64), ("inc_lo", C.c_uint64),
                ("has_uint32", C.c_uint32), ("uinteger", C.c_uint32)]

    @classmethod
    def from_generator(cls, gen):
        st = gen.bit_generator.state
        assert st["bit_generator"] == "PCG64"
        s, inc = st["state"]["state"], st["state"]["inc"]
        m = (1 << 64) - 1
        return cls(s >> 64, s & m, inc >> 64, inc & m, st["has_uint32"], st["uinteger"])

    def to_generator(self, gen):
        st = gen.bit_generator.state
        st["state"]["state"] = (self.state_hi << 64) | self.state_lo
        st["state"]["inc"] = (self.inc_hi << 64) | self.inc_lo
        st["has_uint32"] = int(self.has_uint32)
        st["uinteger"] = int(self.uinteger)
        gen.bit_generator.state = st


class RansacState(C.Structure):
    _fields_ = [("outlier_ratio", C.c_double), ("confidence", C.c_double), ("max_iterations", C.c_int64),
                ("n_iterations", C.c_int64), ("s", C.c_int32), ("adaptive", C.c_int32)]


class PipelineConfig(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_frames", C.c_int32),
                ("n_keypoints", C.c_int32), ("harris_patch", C.c_int32), ("nms_radius", C.c_int32),
                ("harris_kappa", C.c_double),
                ("klt_win", C.c_int32), ("klt_max_level", C.c_int32), ("klt_max_iter", C.c_int32), ("hyp", C.c_int32),
                ("klt_eps", C.c_double), ("klt_min_eig", C.c_double), ("klt_err_threshold", C.c_double),
                ("p3p_thr_sq", C.c_double), ("ransac_outlier_ratio", C.c_double), ("ransac_confidence", C.c_double),
                ("ransac_max_iterations", C.c_int64),
                ("K", C.c_double * 9), ("Kinv", C.c_double * 9), ("refine_iters", C.c_int32), ("feature_cap", C.c_int32),
                ("bearing_threshold", C.c_double), ("redetect_fraction", C.c_double),
                ("debug_fault_every", C.c_int32), ("redetect_start_pose", C.c_int32), ("detect_margin", C.c_double),
                ("debug_never_detect", C.c_int32), ("detect_losses", C.c_double), ("sequences", C.c_int32),
                ("tracker_mode", C.c_int32), ("sift_cap", C.c_int32), ("track_ids", C.c_int32),
                ("match_ratio", C.c_double),
                ("detector", C.c_int32), ("st_block", C.c_int32), ("st_quality", C.c_double),
                ("st_min_distance", C.c_double)]


class StepResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("n_tracked", C.c_int32), ("n_inliers", C.c_int32),
                ("best_index", C.c_int32), ("hyp_valid", C.c_int32), ("ransac_iterations", C.c_int64),
                ("draws_consumed", C.c_int32), ("refine_iterations", C.c_int32),
                ("R_refined", C.c_double * 9), ("t_refined", C.c_double * 3), ("refine_cost", C.c_double),
                ("n_features_in", C.c_int32), ("redetected", C.c_int32), ("n_triangulated", C.c_int32),
                ("n_candidates", C.c_int32), ("n_dropped", C.c_int32), ("n_landmarks", C.c_int32),
                ("fault", C.c_int32), ("recovered", C.c_int32), ("detector_ran", C.c_int32), ("reserved", C.c_int32),
                ("raw_pos", C.c_uint64), ("T_wc", C.c_double * 12),
                ("ts", C.c_uint64 * 8), ("seq_head", C.c_uint32), ("seq_tail", C.c_uint32)]

    def pose_world_cam(self):
        """State.curr_pose after the step: camera-to-world, 4x4."""
        return np.vstack([np.array(self.T_wc).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])

    @property
    def idle(self):
        """The record of an idle lane (vo_pipeline_set_active_seq): nothing was computed for it."""
        return self.n_features_in == -1


class BootstrapParams(C.Structure):
    """vo_bootstrap_params: 0 in a field = its default (klt_max_level: -1)."""
    _fields_ = [("max_corners", C.c_int32), ("quality", C.c_double), ("min_distance", C.c_double), ("block", C.c_int32),
                ("klt_win", C.c_int32), ("klt_max_level", C.c_int32), ("threshold_px", C.c_double),
                ("outlier_ratio", C.c_double), ("confidence", C.c_double), ("max_iterations", C.c_int32),
                ("route", C.c_int32)]


class BootstrapResult(C.Structure):
    """vo_bootstrap_result."""
    _fields_ = [("n_corners", C.c_int32), ("n_tracked", C.c_int32), ("n_ransac_inliers", C.c_int32),
                ("n_landmarks", C.c_int32), ("n_features", C.c_int32), ("reserved", C.c_int32),
                ("ransac_iterations", C.c_int64), ("M", C.c_double * 12), ("bytes_h2d", C.c_int64),
                ("bytes_d2h", C.c_int64)]

    seq, status = 0, 0          # Pipeline.bootstrap_lanes: the lane and its VO_E* code (0 = bootstrapped)

    def relative_pose(self):
        """M: camera a -> camera b, (3, 4), |t| = 1."""
        return np.array(self.M).reshape(3, 4)


class BaParams(C.Structure):
    """vo_ba_params: 0 in a field = its default (max_iter 10, max_trials 2 * max_iter, n_fixed 2, squared loss,
    lambda0 1e-3, step_tol 1e-10)."""
    _fields_ = [("max_iter", C.c_int32), ("max_trials", C.c_int32), ("n_fixed", C.c_int32), ("reserved", C.c_int32),
                ("huber_px", C.c_double), ("lambda0", C.c_double), ("step_tol", C.c_double)]


class BaResult(C.Structure):
    """vo_ba_result.  status: 0 converged, 1 max_iter, 2 max_trials, 3 lambda beyond 1e12, 4 refused."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("n_obs", C.c_int32),
                ("cost0", C.c_double), ("cost", C.c_double), ("lam", C.c_double)]


BA_RESULT = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("trials", "<i4"), ("n_obs", "<i4"), ("cost0", "<f8"),
                      ("cost", "<f8"), ("lam", "<f8")])       # the same 40 bytes as a NumPy row


def ba_params(n_fixed=0, huber_px=0.0, max_iter=0, max_trials=0, lambda0=0.0, step_tol=0.0):
    return BaParams(int(max_iter), int(max_trials), int(n_fixed), 0, float(huber_px), float(lambda0), float(step_tol))


class StructureParams(C.Structure):
    """vo_structure_params: 0 in a field = its default (max_iter 10, max_trials 2 * max_iter, squared loss, lambda0 1e-3,
    step_tol 1e-10, f_tol 1e-9, no residual gate, no parallax gate)."""
    _fields_ = [("max_iter", C.c_int32), ("max_trials", C.c_int32), ("huber_px", C.c_double), ("lambda0", C.c_double),
                ("step_tol", C.c_double), ("f_tol", C.c_double), ("gate_px", C.c_double), ("min_parallax", C.c_double)]


# vo_structure_result (per landmark; status as BA_RESULT's, kept: X is the refined point) and vo_structure_summary (per
# window) as NumPy rows: the same 48 and 32 bytes
STRUCTURE_RESULT = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("trials", "<i4"), ("n_obs", "<i4"), ("cost0", "<f8"),
                             ("cost", "<f8"), ("min_cos", "<f8"), ("kept", "<i4"), ("reserved", "<i4")])
STRUCTURE_SUMMARY = np.dtype([("L", "<i4"), ("n_refused", "<i4"), ("n_kept", "<i4"), ("max_iterations", "<i4"),
                              ("cost0", "<f8"), ("cost", "<f8")])


# vo_structure_loop_entry (per lane and post of a vo.landmarks.StructureLoop): 24 bytes of int32, then the summary
STRUCTURE_LOOP_ENTRY = np.dtype([("step", "<i4"), ("full", "<i4"), ("L", "<i4"), ("M", "<i4"), ("flags", "<i4"), ("n_written", "<i4"),
                                 ("summary", STRUCTURE_SUMMARY)])


class StructureLoopConfig(C.Structure):
    """vo_structure_loop_config."""
    _fields_ = [("window", C.c_int32), ("L_cap", C.c_int32), ("M_cap", C.c_int32), ("feedback", C.c_int32),
                ("params", StructureParams)]


def structure_params(huber_px=0.0, max_iter=0, max_trials=0, lambda0=0.0, step_tol=0.0, f_tol=0.0, gate_px=0.0,
                     min_parallax=0.0):
    return StructureParams(int(max_iter), int(max_trials), float(huber_px), float(lambda0), float(step_tol), float(f_tol),
                           float(gate_px), float(min_parallax))


_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
_SIGS = {
    "vo_create": (_i, [_i, _vp, C.POINTER(_vp)]),
    "vo_destroy": (None, [_vp]),
    "vo_last_error": (C.c_char_p, [_vp]),
    "vo_version": (_i, []),
    "vo_sync": (_i, [_vp]),
    "vo_stream": (_vp, [_vp]),
    "vo_dev_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "vo_dev_free": (_i, [_vp, _vp]),
    "vo_dev_upload": (_i, [_vp, _vp, _vp, _sz]),
    "vo_dev_download": (_i, [_vp, _vp, _vp, _sz]),
    "vo_prof_enable": (_i, [_vp, _i]),
    "vo_prof_set_sampling": (_i, [_vp, _i]),
    "vo_prof_disable": (_i, [_vp]),
    "vo_prof_read": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(C.c_int64)]),
    "vo_prof_reset": (_i, [_vp]),
    "vo_kernel_name": (C.c_char_p, [_i]),
    "vo_harris_response": (_i, [_vp, _vp, _i, _i, _i, _d, _vp]),
    "vo_harris_keypoints": (_i, [_vp, _vp, _i, _i, _i, _d, _i, _i, _vp, _vp]),
    "vo_nms_keypoints": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vo_harris_keypoints_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _i, _i, _vp, _vp]),
    "vo_harris_response_dev": (_i, [_vp, _vp, _i, _i, _i, _d, _vp]),
    "vo_nms_keypoints_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vo_patch_descriptors": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "vo_patch_descriptors_dev": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "vo_klt_num_levels": (_i, [_i, _i, _i, _i]),
    "vo_pyramid_bytes": (_sz, [_i, _i, _i]),
    "vo_pyr_down": (_i, [_vp, _vp, _i, _i, _vp]),
    "vo_pyramid_build_dev": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vo_klt_track": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp]),
    "vo_klt_track_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _d, _d, _vp, _vp, _vp]),
    "vo_klt_track_fb": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "vo_klt_track_fb_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "vo_triangulate_dlt": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "vo_triangulate_dlt_dev": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "vo_p3p_hypotheses": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "vo_p3p_hypotheses_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "vo_reproj_inliers": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _d, _vp, _vp]),
    "vo_reproj_inliers_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _d, _vp, _vp]),
    "vo_refine_pose": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(_d)]),
    "vo_refine_pose_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "vo_match_knn2_ratio": (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _vp, _vp]),
    "vo_knn2_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "vo_match_knn2": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, C.POINTER(_i)]),
    "vo_match_last_path": (_i, [_vp]),
    "vo_brief_describe": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "vo_brief_describe_dev": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "vo_brief_pattern": (_i, [_vp]),
    "vo_match_hamming_knn2": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "vo_hamming_knn2_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "vo_brief_describe_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp]),
    "vo_match_hamming_batch_dev": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp, _i, _i, _i, _i, _d, _i, _vp, _vp]),
    "vo_match_hamming_ratio": (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _i, _vp, _vp]),
    "vo_fast_score": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vo_fast_keypoints": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vo_fast_keypoints_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vo_fast_keypoints_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    "vo_good_features": (_i, [_vp, _vp, _i, _i, _vp, _i, _d, _d, _i, _vp, _vp]),
    "vo_min_eigen_map": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vo_good_features_capacity": (_i, [_i, _i, _i]),
    "vo_good_features_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _vp, _sz, _i, _d, _d, _i, _vp, _sz, _vp, _vp, _vp]),
    "vo_good_features_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _i, _vp, _vp]),
    "vo_sift": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "vo_sift_capacity": (_i, [_i, _i]),
    "vo_sift_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "vo_sift_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "vo_sift_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vo_sift_all_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "vo_harris_subpix_capacity": (_i, [_i, _i]),
    "vo_harris_subpix_batch_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp,
                                        _vp]),
    "vo_harris_subpix_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "vo_harris_subpix_corners": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "vo_fundamental_hypotheses": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _d, _vp, _vp, _vp]),
    "vo_fundamental_fit": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp]),
    "vo_fundamental_ransac": (_i, [_vp, _vp, _vp, _i, _i, _i, _d, _d, _d, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_essential_hypotheses": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "vo_essential_ransac": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _d, _d, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "vo_rng_raw32_device": (_i, [_vp, _vp, _i, _vp]),
    "vo_rng_choice8_from_raw": (_i, [_vp, _i, _vp, _vp]),
    "vo_essential_decompose": (_i, [_vp, _vp, _vp]),
    "vo_relative_pose": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_comm_unique_id": (_i, [_vp, _vp]),
    "vo_comm_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "vo_comm_destroy": (None, [_vp]),
    "vo_comm_world": (_i, [_vp]),
    "vo_allgather_state_dev": (_i, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "vo_allgather_state": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "vo_rng_choice": (_i, [_vp, _i, _i, _i, _vp]),
    "vo_ransac_num_iterations": (C.c_int64, [_d, _d, _i]),
    "vo_ransac_replay": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "vo_record_seal": (None, [_vp, C.c_uint]),
    "vo_record_check": (_i, [_vp, C.c_uint]),
    "vo_pipeline_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "vo_pipeline_set_descriptors": (_i, [_vp, _vp, _i]),
    "vo_pipeline_set_descriptors_seq": (_i, [_vp, _i, _vp, _i]),
    "vo_pipeline_get_descriptors_seq": (_i, [_vp, _i, _vp, _vp]),
    "vo_pipeline_checkpoint": (_i, [_vp]),
    "vo_pipeline_rewind": (_i, [_vp]),
    "vo_pipeline_destroy": (None, [_vp]),
    "vo_pipeline_release_cached": (None, []),
    "vo_pipeline_release_cached_at_exit": (_i, []),
    "vo_pipeline_set_frame": (_i, [_vp, _i, _vp]),
    "vo_pipeline_seed": (_i, [_vp, _vp]),
    "vo_pipeline_get_rng": (_i, [_vp, _vp]),
    "vo_pipeline_set_state": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "vo_pipeline_feature_cap": (_i, [_vp]),
    "vo_pipeline_get_state": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_pipeline_get_detection": (_i, [_vp, _vp]),
    "vo_pipeline_get_detection_seq": (_i, [_vp, _i, _vp, _vp]),
    "vo_pipeline_step": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_submit": (_i, [_vp, _i, _i]),
    "vo_pipeline_collect": (_i, [_vp, _vp]),
    "vo_pipeline_bookkeeping": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "vo_pipeline_export_state_post": (_i, [_vp, _vp, _i, _vp]),
    "vo_pipeline_export_state_join": (_i, [_vp, _vp]),
    "vo_pipeline_prof_read": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(C.c_int64)]),
    "vo_pipeline_prof_reset": (_i, [_vp]),
    "vo_pipeline_ransac_bound": (C.c_int64, [_vp, _d]),
    "vo_pipeline_sequences": (_i, [_vp]),
    "vo_pipeline_set_frame_seq": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_set_frame_pinned": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_frame_uploaded": (_i, [_vp, _i, _i]),
    "vo_pipeline_prepare": (_i, [_vp, _i]),
    "vo_pipeline_set_klt_fb": (_i, [_vp, _d]),
    "vo_pipeline_get_klt_fb": (_i, [_vp, _vp]),
    "vo_pipeline_set_fast_brief": (_i, [_vp, _i, _i, _i]),
    "vo_pipeline_get_fast_brief": (_i, [_vp, _vp, _vp, _vp]),
    "vo_host_alloc": (_i, [_vp, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vo_host_free": (_i, [_vp, _vp]),
    "vo_gray_from_bgr": (_i, [_vp, _vp, _i, _i, _vp]),
    "vo_undistort_image": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "vo_pipeline_set_distortion_seq": (_i, [_vp, _i, _vp, _vp]),
    "vo_pipeline_set_frame_bgr_seq": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_set_frame_bgr_pinned": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_get_frame_seq": (_i, [_vp, _i, _i, _vp]),
    "vo_pipeline_set_state_seq": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "vo_pipeline_get_state_seq": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_pipeline_get_rng_seq": (_i, [_vp, _i, _vp]),
    "vo_pipeline_collect_all": (_i, [_vp, _vp]),
    "vo_pipeline_export_state_post_seq": (_i, [_vp, _i, _vp, _i, _vp]),
    "vo_pipeline_tracks_record_bytes": (_sz, [_i]),
    "vo_pipeline_get_track_ids_seq": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "vo_pipeline_set_track_ids_seq": (_i, [_vp, _i, _vp, _vp, _i, C.c_int32]),
    "vo_pipeline_export_tracks_post_seq": (_i, [_vp, _i, _vp, _i, _vp]),
    "vo_pipeline_set_camera_seq": (_i, [_vp, _i, _vp, _vp]),
    "vo_pipeline_set_active_seq": (_i, [_vp, _i, _i]),
    "vo_pipeline_restart_seq": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "vo_pipeline_bootstrap_seq": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "vo_pipeline_bootstrap": (_i, [_vp, _i, _i, _vp, _vp]),
    "vo_pipeline_bootstrap_lanes": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "vo_bootstrap_default_rng": (None, [_vp]),
    "vo_window_ba_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "vo_window_ba_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_window_ba": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_window_from_tracks_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_window_structure_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_window_structure": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_pipeline_update_landmarks_seq": (_i, [_vp, _i, _i, _vp, _vp]),
    "vo_structure_loop_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "vo_structure_loop_post": (_i, [_vp, _vp]),
    "vo_structure_loop_posts": (_i, [_vp]),
    "vo_structure_loop_reset_seq": (_i, [_vp, _i]),
    "vo_structure_loop_poll": (_i, [_vp, _i, _i, _vp]),
    "vo_structure_loop_download_seq": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vo_structure_loop_destroy": (_i, [_vp]),
}


# entry points libvo_hip.so exports without their being part of the C ABI of include/vo_hip.h (csrc/vo_internal.h)
_INTERNAL_SIGS = {
    "vo_knn2_u8_batch_dev": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp, _i, _i, _i, _i, _vp, _vp]),
    "vo_match_u8_batch_dev": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp, _i, _i, _i, _d, _vp, _vp, _i]),
}

MATCH_PATH_FLOAT, MATCH_PATH_BYTE_DOT, MATCH_PATH_MFMA = 0, 1, 2      # vo_match_knn2's *path (vo_hip.h)


def distortion_coefficients(dist):
    """(k1, k2, p1, p2, k3) as five float64; None: zeros; four coefficients: k3 = 0.  The model has no more."""
    d = np.zeros(5, np.float64) if dist is None else np.asarray(dist, np.float64).reshape(-1)
    if d.size > 5:
        raise ValueError("%d distortion coefficients: the model is (k1, k2, p1, p2, k3), five at most (four: k3 = 0)" % d.size)
    if d.size not in (4, 5):
        raise ValueError("%d distortion coefficients: the model takes (k1, k2, p1, p2) or (k1, k2, p1, p2, k3)" % d.size)
    return np.ascontiguousarray(np.concatenate((d, np.zeros(5 - d.size))))


def lib_path():
    return _LIB_PATH


def load():
    """Load libvo_hip.so; raises if it has not been built (see __graft_entry__.build)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise ImportError(
                    "libvo_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (there is no CPU fallback)" % _LIB_PATH)
            lib = C.CDLL(_LIB_PATH)
            for name, (res, args) in list(_SIGS.items()) + list(_INTERNAL_SIGS.items()):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


class Context:
    """One HIP stream + device workspace (vo_ctx).  Not thread-safe."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.vo_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != VO_OK:
            raise VoError(rc, "vo_create(device=%d) failed: no usable MI355X/HIP device (no CPU fallback)" % device)
        self._h = h
        self.device = device
        self._pipelines = weakref.WeakSet()      # pipelines built on this context: closed before it is
        self._pinned_ranges = []                 # live pinned_empty allocations: (first byte, one past the last, owner)

    def close(self):
        if getattr(self, "_h", None):
            for p in list(self._pipelines):
                p.close()
            self._lib.vo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != VO_OK:
            raise VoError(rc, self._lib.vo_last_error(self._h).decode("utf-8", "replace"))

    # ---- plumbing ----
    def sync(self):
        self._chk(self._lib.vo_sync(self._h))

    @property
    def stream(self):
        return self._lib.vo_stream(self._h)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._lib.vo_dev_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def free(self, p):
        self._chk(self._lib.vo_dev_free(self._h, C.c_void_p(p)))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self._lib.vo_dev_upload(self._h, C.c_void_p(dptr), _ptr(arr), arr.nbytes))

    def download(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._chk(self._lib.vo_dev_download(self._h, _ptr(out), C.c_void_p(dptr), out.nbytes))
        return out

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 1))
        self.upload(p, arr)
        return p

    def prof_enable(self, kernel_id=-1):
        self._chk(self._lib.vo_prof_enable(self._h, int(kernel_id)))

    def prof_set_sampling(self, every):
        self._chk(self._lib.vo_prof_set_sampling(self._h, int(every)))

    def prof_disable(self):
        self._chk(self._lib.vo_prof_disable(self._h))

    def prof_reset(self):
        self._chk(self._lib.vo_prof_reset(self._h))

    def prof_read(self, kernel_id):
        ms, n = C.c_double(), C.c_int64()
        self._chk(self._lib.vo_prof_read(self._h, int(kernel_id), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_name(self, kernel_id):
        return self._lib.vo_kernel_name(int(kernel_id)).decode()

    # ---- Harris / NMS / descriptors (host arrays) ----
    def harris_response(self, img, patch=9, kappa=0.09):
        img = _c(img, np.uint8)
        assert img.ndim == 2
        H, W = img.shape
        out = np.empty((H, W), np.float64)
        self._chk(self._lib.vo_harris_response(self._h, _ptr(img), H, W, int(patch), float(kappa), _ptr(out)))
        return out

    def harris_keypoints(self, img, patch=9, kappa=0.09, num_keypoints=1000, r=5, want_scores=False):
        img = _c(img, np.uint8)
        assert img.ndim == 2
        H, W = img.shape
        kp = np.empty((num_keypoints, 2), np.float64)
        sc = np.empty((H, W), np.float64) if want_scores else None
        self._chk(self._lib.vo_harris_keypoints(self._h, _ptr(img), H, W, int(patch), float(kappa),
                                                int(num_keypoints), int(r), _ptr(kp), _ptr(sc)))
        return (kp, sc) if want_scores else kp

    def harris_keypoints_batch(self, imgs, patch=9, kappa=0.09, num_keypoints=1000, r=5, want_scores=False):
        """(S, H, W) uint8 -> (S, N, 2) keypoints [, (S, H, W) score maps]: S frames in one set of launches."""
        imgs = _c(imgs, np.uint8)
        assert imgs.ndim == 3
        S, H, W = imgs.shape
        kp = np.empty((S, num_keypoints, 2), np.float64)
        sc = np.empty((S, H, W), np.float64) if want_scores else None
        self._chk(self._lib.vo_harris_keypoints_batch(self._h, _ptr(imgs), S, H, W, int(patch), float(kappa),
                                                      int(num_keypoints), int(r), _ptr(kp), _ptr(sc)))
        return (kp, sc) if want_scores else kp

    def nms_keypoints(self, scores, num_keypoints, r):
        scores = _c(scores, np.float64)
        H, W = scores.shape
        kp = np.empty((num_keypoints, 2), np.float64)
        self._chk(self._lib.vo_nms_keypoints(self._h, _ptr(scores), H, W, int(num_keypoints), int(r), _ptr(kp)))
        return kp

    def patch_descriptors(self, img, kp_xy, r=9):
        img = _c(img, np.uint8)
        kp = _c(np.asarray(kp_xy).reshape(-1, 2), np.float64)
        H, W = img.shape
        n = kp.shape[0]
        d = (2 * r + 1) ** 2
        out = np.empty((n, d), np.float64)
        self._chk(self._lib.vo_patch_descriptors(self._h, _ptr(img), H, W, _ptr(kp), n, int(r), _ptr(out)))
        return out

    # ---- matching / corners ----
    def match_knn2_ratio(self, q, t, ratio):
        q, t = np.asarray(q), np.asarray(t)
        if len(q) == 0 or len(t) == 0:
            return np.empty((0, 2), np.int64)
        q = _c(q.reshape(len(q), -1), np.float32)
        t = _c(t.reshape(len(t), -1), np.float32)
        assert q.shape[1] == t.shape[1]
        pairs = np.empty((max(q.shape[0], 1), 2), np.int32)
        n = C.c_int32(0)
        self._chk(self._lib.vo_match_knn2_ratio(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0],
                                                max(q.shape[1], 1), float(ratio), _ptr(pairs), C.byref(n)))
        return pairs[: n.value].astype(np.int64)

    def match_knn2(self, q, t):
        """The two nearest train rows of every query (vo_match_knn2): (best (nq, 2) int32, -1 where absent; d2 (nq, 2)
        float64 squared distances, 0.0 where absent; path: the kernel that made them, MATCH_PATH_FLOAT / _BYTE_DOT / _MFMA,
        -1 when q or t is empty)."""
        q, t = np.asarray(q), np.asarray(t)
        if len(q) == 0 or len(t) == 0:                      # (no distance is computed: the rows' length does not matter)
            q, t = np.zeros((len(q), 1), np.float32), np.zeros((len(t), 1), np.float32)
        else:
            q, t = _c(q.reshape(len(q), -1), np.float32), _c(t.reshape(len(t), -1), np.float32)
        assert q.shape[1] == t.shape[1]
        best = np.empty((q.shape[0], 2), np.int32)
        d2 = np.empty((q.shape[0], 2), np.float64)
        path = C.c_int(-1)
        self._chk(self._lib.vo_match_knn2(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], q.shape[1],
                                          _ptr(best), _ptr(d2), C.byref(path)))
        return best, d2, path.value

    def match_last_path(self):
        """The kernel the last match_knn2_ratio / match_knn2 call of this context kept (vo_match_last_path); -1: none ran."""
        return int(self._lib.vo_match_last_path(self._h))

    # ---- BRIEF-256 and Hamming matching (csrc/brief.hip) ----
    def brief_describe(self, img, kp_xy, oriented=False, want_bins=False):
        """(N, 32) uint8 BRIEF-256 descriptors of the keypoints (vo_brief_describe), rows index-aligned with kp_xy;
        with want_bins also the (N,) uint8 orientation bins (all 0 unless oriented)."""
        img = _c(img, np.uint8)
        assert img.ndim == 2
        kp = _c(np.asarray(kp_xy).reshape(-1, 2), np.float64)
        H, W = img.shape
        n = kp.shape[0]
        desc = np.empty((n, 32), np.uint8)
        bins = np.empty((n,), np.uint8) if want_bins else None
        self._chk(self._lib.vo_brief_describe(self._h, _ptr(img), H, W, _ptr(kp), n, 1 if oriented else 0, _ptr(desc),
                                              _ptr(bins)))
        return (desc, bins) if want_bins else desc

    def brief_describe_dev(self, d_img, H, W, d_kp, N, oriented, d_desc, d_bin=None):
        self._chk(self._lib.vo_brief_describe_dev(self._h, C.c_void_p(d_img), int(H), int(W), C.c_void_p(d_kp), int(N),
                                                  1 if oriented else 0, C.c_void_p(d_desc), C.c_void_p(d_bin)))

    def brief_describe_batch_dev(self, d_imgs, img_stride, S, H, W, d_kp_xy, xy_stride, d_n, N, oriented, d_desc, desc_stride,
                                 d_bin=None):
        """vo_brief_describe_batch_dev on device pointers (alloc / to_device): image q describes its first
        min(max(d_n[q], 0), N) rows; enqueued on the context's stream, nothing read back."""
        self._chk(self._lib.vo_brief_describe_batch_dev(self._h, C.c_void_p(d_imgs), int(img_stride), int(S), int(H), int(W),
                                                        C.c_void_p(d_kp_xy), int(xy_stride), C.c_void_p(d_n), int(N),
                                                        1 if oriented else 0, C.c_void_p(d_desc), int(desc_stride),
                                                        C.c_void_p(d_bin) if d_bin else None))

    def brief_pattern(self):
        """The (30, 256, 4) int8 table (ax, ay, bx, by) the library was built with (vo_brief_pattern)."""
        out = np.empty((30, 256, 4), np.int8)
        rc = self._lib.vo_brief_pattern(_ptr(out))
        if rc != VO_OK:
            raise VoError(rc, "vo_brief_pattern failed")
        return out

    @staticmethod
    def _byte_rows(q, t):
        q, t = np.asarray(q), np.asarray(t)
        if len(q) == 0 or len(t) == 0:                      # (no distance is computed: the rows' length does not matter)
            return np.zeros((len(q), 4), np.uint8), np.zeros((len(t), 4), np.uint8)
        q, t = _c(q.reshape(len(q), -1), np.uint8), _c(t.reshape(len(t), -1), np.uint8)
        assert q.shape[1] == t.shape[1]
        return q, t

    def match_hamming_knn2(self, q, t):
        """The two train rows nearest to every query under (Hamming distance, train index) (vo_match_hamming_knn2): best
        (nq, 2) int32, -1 where absent; dist (nq, 2) int32, 0 where absent.  Rows are uint8, a multiple of 4 in 4 .. 64 long."""
        q, t = self._byte_rows(q, t)
        best = np.empty((q.shape[0], 2), np.int32)
        dist = np.empty((q.shape[0], 2), np.int32)
        self._chk(self._lib.vo_match_hamming_knn2(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], q.shape[1],
                                                  _ptr(best), _ptr(dist)))
        return best, dist

    def hamming_knn2_dev(self, d_q, nq, d_t, nt, row_bytes, d_best, d_dist):
        self._chk(self._lib.vo_hamming_knn2_dev(self._h, C.c_void_p(d_q), int(nq), C.c_void_p(d_t), int(nt), int(row_bytes),
                                                C.c_void_p(d_best), C.c_void_p(d_dist)))

    def match_hamming_batch_dev(self, d_q, q_stride, d_nq, nq_stride, cap_q, d_t, t_stride, d_nt, nt_stride, cap_t, S, row_bytes,
                                ratio, max_dist, d_pairs, d_npairs):
        """vo_match_hamming_batch_dev on device pointers: match_hamming_ratio's rule for S sequences whose counts lie in
        device memory, enqueued on the context's stream."""
        self._chk(self._lib.vo_match_hamming_batch_dev(self._h, C.c_void_p(d_q), int(q_stride), C.c_void_p(d_nq), int(nq_stride),
                                                       int(cap_q), C.c_void_p(d_t), int(t_stride), C.c_void_p(d_nt),
                                                       int(nt_stride), int(cap_t), int(S), int(row_bytes), float(ratio),
                                                       int(max_dist), C.c_void_p(d_pairs), C.c_void_p(d_npairs)))

    def match_hamming_ratio(self, q, t, ratio, max_dist=-1):
        """(n, 2) int64 pairs (query, train) in query order: ratio test on the Hamming distances, the distance limit
        (max_dist >= 0) and first-come uniqueness (vo_match_hamming_ratio)."""
        if len(q) == 0 or len(t) == 0:
            return np.empty((0, 2), np.int64)
        q, t = self._byte_rows(q, t)
        pairs = np.empty((q.shape[0], 2), np.int32)
        n = C.c_int32(0)
        self._chk(self._lib.vo_match_hamming_ratio(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], q.shape[1],
                                                   float(ratio), int(max_dist), _ptr(pairs), C.byref(n)))
        return pairs[: n.value].astype(np.int64)

    # ---- FAST-9 corners (csrc/fast.hip) ----
    def fast_score(self, img, threshold=20):
        """The (H, W) uint8 FAST-9 score map (vo_fast_score): s(p) where p is a corner, 0 elsewhere."""
        img = _c(img, np.uint8)
        assert img.ndim == 2
        H, W = img.shape
        out = np.empty((H, W), np.uint8)
        self._chk(self._lib.vo_fast_score(self._h, _ptr(img), H, W, int(threshold), _ptr(out)))
        return out

    def fast_keypoints(self, img, threshold=20, num_keypoints=1000, nonmax=True, want_scores=False):
        """(n, 2) float64 (x, y) of the n = min(num_keypoints, survivors) strongest FAST-9 corners in the order (score
        descending, index ascending) (vo_fast_keypoints); with want_scores also their (n,) uint8 scores."""
        img = _c(img, np.uint8)
        assert img.ndim == 2
        H, W = img.shape
        kp = np.empty((int(num_keypoints), 2), np.float64)
        sc = np.empty((int(num_keypoints),), np.uint8) if want_scores else None
        n = C.c_int32(0)
        self._chk(self._lib.vo_fast_keypoints(self._h, _ptr(img), H, W, int(threshold), 1 if nonmax else 0,
                                              int(num_keypoints), _ptr(kp), _ptr(sc), C.byref(n)))
        return (kp[: n.value].copy(), sc[: n.value].copy()) if want_scores else kp[: n.value].copy()

    def fast_keypoints_batch(self, imgs, threshold=20, num_keypoints=1000, nonmax=True, want_scores=False):
        """FAST-9 corners of S images of one size in one set of launches (vo_fast_keypoints_batch): `imgs` is an (S, H, W)
        uint8 array or a list of equal-shape 2-D arrays.  Returns a list of S items, each what fast_keypoints(image, ...)
        returns."""
        imgs, _ = self._image_stack("fast_keypoints_batch", imgs)
        S, H, W = imgs.shape
        N = int(num_keypoints)
        kp = np.empty((S, max(N, 0), 2), np.float64)
        sc = np.empty((S, max(N, 0)), np.uint8) if want_scores else None
        n = np.zeros(S, np.int32)
        self._chk(self._lib.vo_fast_keypoints_batch(self._h, _ptr(imgs), S, H, W, int(threshold), 1 if nonmax else 0, N,
                                                    _ptr(kp), _ptr(sc), _ptr(n)))
        if want_scores:
            return [(kp[q, : n[q]].copy(), sc[q, : n[q]].copy()) for q in range(S)]
        return [kp[q, : n[q]].copy() for q in range(S)]

    def fast_keypoints_batch_dev(self, d_imgs, img_stride, S, H, W, d_kp_xy, xy_stride, d_n, threshold=20, num_keypoints=1000,
                                 nonmax=True, d_kp_score=None, d_total=None):
        """vo_fast_keypoints_batch_dev on device pointers (alloc / to_device): enqueued on the context's stream, nothing
        read back."""
        def vp(p):
            return C.c_void_p(p) if p else None
        self._chk(self._lib.vo_fast_keypoints_batch_dev(self._h, vp(d_imgs), int(img_stride), int(S), int(H), int(W),
                                                        int(threshold), 1 if nonmax else 0, int(num_keypoints), vp(d_kp_xy),
                                                        int(xy_stride), vp(d_kp_score), vp(d_n), vp(d_total)))

    def knn2_u8_batch_dev(self, d_q, q_stride, d_nq, nq_stride, cap_q, d_t, t_stride, d_nt, nt_stride, cap_t, S, row_bytes,
                          d_best, d_d2):
        """vo_knn2_u8_batch_dev (csrc/vo_internal.h) on device pointers (to_device / alloc): the frame pipeline's 2-NN lists of
        S sequences, enqueued on the context's stream."""
        self._chk(self._lib.vo_knn2_u8_batch_dev(self._h, C.c_void_p(d_q), int(q_stride), C.c_void_p(d_nq), int(nq_stride),
                                                 int(cap_q), C.c_void_p(d_t), int(t_stride), C.c_void_p(d_nt), int(nt_stride),
                                                 int(cap_t), int(S), int(row_bytes), C.c_void_p(d_best), C.c_void_p(d_d2)))

    def match_u8_batch_dev(self, d_q, q_stride, d_nq, nq_stride, cap_q, d_t, t_stride, d_nt, nt_stride, cap_t, S, ratio,
                           d_pairs, d_npairs, row_bytes):
        """vo_match_u8_batch_dev (csrc/vo_internal.h) on device pointers: the frame pipeline's matcher for S sequences,
        enqueued on the context's stream."""
        self._chk(self._lib.vo_match_u8_batch_dev(self._h, C.c_void_p(d_q), int(q_stride), C.c_void_p(d_nq), int(nq_stride),
                                                  int(cap_q), C.c_void_p(d_t), int(t_stride), C.c_void_p(d_nt), int(nt_stride),
                                                  int(cap_t), int(S), float(ratio), C.c_void_p(d_pairs), C.c_void_p(d_npairs),
                                                  int(row_bytes)))

    # ---- window bundle adjustment (csrc/window_ba.hip) ----
    def window_ba(self, K, poses, X, lm_start, obs_slot, obs_xy, counts, n_fixed=0, huber_px=0.0, max_iter=0, max_trials=0,
                  lambda0=0.0, step_tol=0.0):
        """vo_window_ba on host arrays: S windows of W slots in strided arrays -- K (S, 3, 3) or (3, 3) for all, poses
        (S, W, 12) world -> camera (R row-major, then t), X (S, L_cap, 3), lm_start (S, L_cap + 1), obs_slot (S, M_cap),
        obs_xy (S, M_cap, 2), counts (S, 2) = each window's (L, M).  Returns (poses, X, results): the refined copies and a
        (S,) record array (dtype BA_RESULT).  The parameters: 0 = the default of vo_ba_params."""
        poses = np.array(poses, np.float64, order="C")
        if poses.ndim != 3 or poses.shape[2] != 12:
            raise ValueError("window_ba: poses must be (S, W, 12), got %s" % (poses.shape,))
        S, W = poses.shape[:2]
        X = np.array(X, np.float64, order="C")
        lm_start, obs_slot = _c(lm_start, np.int32), _c(obs_slot, np.int32)
        obs_xy = _c(obs_xy, np.float64)
        if X.ndim != 3 or X.shape[0] != S or X.shape[2] != 3 or X.shape[1] < 1:
            raise ValueError("window_ba: X must be (S, L_cap >= 1, 3), got %s" % (X.shape,))
        L_cap = X.shape[1]
        if lm_start.shape != (S, L_cap + 1):
            raise ValueError("window_ba: lm_start must be (S, L_cap + 1) = %s, got %s" % ((S, L_cap + 1), lm_start.shape))
        if obs_slot.ndim != 2 or obs_slot.shape[0] != S or obs_slot.shape[1] < 1 or obs_xy.shape != obs_slot.shape + (2,):
            raise ValueError("window_ba: obs_slot must be (S, M_cap >= 1) and obs_xy (S, M_cap, 2), got %s and %s"
                             % (obs_slot.shape, obs_xy.shape))
        M_cap = obs_slot.shape[1]
        K = np.asarray(K, np.float64)
        K = _c(np.broadcast_to(K.reshape(-1, 3, 3), (S, 3, 3)) if K.size == 9 else K.reshape(S, 3, 3), np.float64)
        cnt = np.zeros((S, 4), np.int32)
        cnt[:, :2] = np.asarray(counts).reshape(S, -1)[:, :2]
        prm = ba_params(n_fixed, huber_px, max_iter, max_trials, lambda0, step_tol)
        res = np.zeros(S, BA_RESULT)
        self._chk(self._lib.vo_window_ba(self._h, S, W, L_cap, M_cap, _ptr(cnt), _ptr(K), _ptr(poses), _ptr(X), _ptr(lm_start),
                                         _ptr(obs_slot), _ptr(obs_xy), C.byref(prm), _ptr(res)))
        return poses, X, res

    def window_ba_dev(self, S, W, L_cap, M_cap, d_counts, d_K, d_poses, d_X, d_lm_start, d_obs_slot, d_obs_xy, d_results,
                      **params):
        """vo_window_ba_dev on device pointers (alloc / to_device), enqueued on the context's stream: S windows solved in
        place, one BA_RESULT row each at d_results.  params: ba_params' keywords."""
        prm = ba_params(**params)
        self._chk(self._lib.vo_window_ba_dev(self._h, int(S), int(W), int(L_cap), int(M_cap), C.c_void_p(d_counts),
                                             C.c_void_p(d_K), C.c_void_p(d_poses), C.c_void_p(d_X), C.c_void_p(d_lm_start),
                                             C.c_void_p(d_obs_slot), C.c_void_p(d_obs_xy), C.byref(prm), C.c_void_p(d_results)))

    def window_ba_workspace_bytes(self, S, W, L_cap, M_cap):
        return int(self._lib.vo_window_ba_workspace_bytes(int(S), int(W), int(L_cap), int(M_cap)))

    def window_from_tracks(self, d_records, cap, L_cap, M_cap, d_head, d_lm_start, d_obs_slot, d_obs_xy, d_X, d_lm_id):
        """vo_window_from_tracks_dev: the window of the W = len(d_records) observation records (device pointers, oldest
        first, as Pipeline.export_tracks_post wrote them with capacity `cap`) into device arrays -- d_head 4 int32
        {L, M, flags, 0}, d_lm_start L_cap + 1 int32, d_obs_slot M_cap int32, d_obs_xy 2 M_cap float64, d_X 3 L_cap float64,
        d_lm_id L_cap int32.  Enqueued on the context's stream."""
        recs = (C.c_void_p * len(d_records))(*[int(d) for d in d_records])
        self._chk(self._lib.vo_window_from_tracks_dev(self._h, len(d_records), recs, int(cap), int(L_cap), int(M_cap),
                                                      C.c_void_p(d_head), C.c_void_p(d_lm_start), C.c_void_p(d_obs_slot),
                                                      C.c_void_p(d_obs_xy), C.c_void_p(d_X), C.c_void_p(d_lm_id)))

    # ---- window structure refinement (csrc/window_structure.hip) ----
    def window_structure(self, K, poses, X, lm_start, obs_slot, obs_xy, counts, **params):
        """vo_window_structure on host arrays, laid out as window_ba's: every pose held, each landmark refined on its own.
        Returns (X, results, summary): the refined copy (a landmark that is refused or not kept keeps its bits), an
        (S, L_cap) record array (dtype STRUCTURE_RESULT; rows beyond a window's L are zero) and an (S,) one (dtype
        STRUCTURE_SUMMARY).  params: structure_params' keywords, 0 = the default of vo_structure_params."""
        poses = _c(poses, np.float64)
        if poses.ndim != 3 or poses.shape[2] != 12:
            raise ValueError("window_structure: poses must be (S, W, 12), got %s" % (poses.shape,))
        S, W = poses.shape[:2]
        X = np.array(X, np.float64, order="C")
        lm_start, obs_slot = _c(lm_start, np.int32), _c(obs_slot, np.int32)
        obs_xy = _c(obs_xy, np.float64)
        if X.ndim != 3 or X.shape[0] != S or X.shape[2] != 3 or X.shape[1] < 1:
            raise ValueError("window_structure: X must be (S, L_cap >= 1, 3), got %s" % (X.shape,))
        L_cap = X.shape[1]
        if lm_start.shape != (S, L_cap + 1):
            raise ValueError("window_structure: lm_start must be (S, L_cap + 1) = %s, got %s" % ((S, L_cap + 1), lm_start.shape))
        if obs_slot.ndim != 2 or obs_slot.shape[0] != S or obs_slot.shape[1] < 1 or obs_xy.shape != obs_slot.shape + (2,):
            raise ValueError("window_structure: obs_slot must be (S, M_cap >= 1) and obs_xy (S, M_cap, 2), got %s and %s"
                             % (obs_slot.shape, obs_xy.shape))
        M_cap = obs_slot.shape[1]
        K = np.asarray(K, np.float64)
        K = _c(np.broadcast_to(K.reshape(-1, 3, 3), (S, 3, 3)) if K.size == 9 else K.reshape(S, 3, 3), np.float64)
        cnt = np.zeros((S, 4), np.int32)
        cnt[:, :2] = np.asarray(counts).reshape(S, -1)[:, :2]
        prm = structure_params(**params)
        res, summ = np.zeros((S, L_cap), STRUCTURE_RESULT), np.zeros(S, STRUCTURE_SUMMARY)
        self._chk(self._lib.vo_window_structure(self._h, S, W, L_cap, M_cap, _ptr(cnt), _ptr(K), _ptr(poses), _ptr(X),
                                                _ptr(lm_start), _ptr(obs_slot), _ptr(obs_xy), C.byref(prm), _ptr(res), _ptr(summ)))
        return X, res, summ

    def window_structure_dev(self, S, W, L_cap, M_cap, d_counts, d_K, d_poses, d_X, d_lm_start, d_obs_slot, d_obs_xy,
                             d_results, d_summary, **params):
        """vo_window_structure_dev on device pointers, enqueued on the context's stream: the landmarks of S windows refined
        in place, STRUCTURE_RESULT rows at d_results + L_cap q, one STRUCTURE_SUMMARY row per window at d_summary."""
        prm = structure_params(**params)
        self._chk(self._lib.vo_window_structure_dev(self._h, int(S), int(W), int(L_cap), int(M_cap), C.c_void_p(d_counts),
                                                    C.c_void_p(d_K), C.c_void_p(d_poses), C.c_void_p(d_X), C.c_void_p(d_lm_start),
                                                    C.c_void_p(d_obs_slot), C.c_void_p(d_obs_xy), C.byref(prm),
                                                    C.c_void_p(d_results), C.c_void_p(d_summary)))

    # ---- frame ingest (csrc/ingest.hip) ----
    def gray_from_bgr(self, bgr):
        """(H, W, 3) uint8, channels B, G, R -> (H, W) uint8: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
        bgr = _c(bgr, np.uint8)
        assert bgr.ndim == 3 and bgr.shape[2] == 3
        H, W = bgr.shape[:2]
        out = np.empty((H, W), np.uint8)
        self._chk(self._lib.vo_gray_from_bgr(self._h, _ptr(bgr), H, W, _ptr(out)))
        return out

    def undistort_image(self, img, K, dist, K_raw=None):
        """(H, W) uint8 of a camera with intrinsics K_raw (None: K) and distortion dist = (k1, k2, p1, p2[, k3]) -> the
        image of the pinhole camera K (vo_undistort_image: 1/32-pixel bilinear taps, zero border)."""
        img = _c(img, np.uint8)
        assert img.ndim == 2
        H, W = img.shape
        K = _c(np.asarray(K, np.float64).reshape(3, 3), np.float64)
        Kr = None if K_raw is None else _c(np.asarray(K_raw, np.float64).reshape(3, 3), np.float64)
        d = distortion_coefficients(dist)
        out = np.empty((H, W), np.uint8)
        self._chk(self._lib.vo_undistort_image(self._h, _ptr(img), H, W, _ptr(K), _ptr(d), _ptr(Kr), _ptr(out)))
        return out

    def pinned_empty(self, shape, dtype=np.uint8):
        """A NumPy array in pinned host memory (vo_host_alloc): what Pipeline.set_frame(..., pinned=True) uploads from
        without a staging copy.  The memory lives as long as the array (and every view of it) does."""
        shape = tuple(int(v) for v in np.atleast_1d(shape))
        dt = np.dtype(dtype)
        nbytes = max(int(np.prod(shape)) * dt.itemsize, 1)
        q = C.c_void_p()
        self._chk(self._lib.vo_host_alloc(self._h, nbytes, C.byref(q)))
        buf = (C.c_uint8 * nbytes).from_address(q.value)
        arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        lib, addr = self._lib, q.value
        weakref.finalize(buf, lambda: lib.vo_host_free(None, C.c_void_p(addr)))     # (the context may be gone by then)
        arr.flags.writeable = True
        self._pinned_ranges.append((addr, addr + nbytes, weakref.ref(buf)))
        return arr

    def is_pinned(self, arr):
        """True when arr's bytes lie inside a live pinned_empty allocation of this context."""
        a = arr.__array_interface__["data"][0]
        b = a + arr.nbytes
        self._pinned_ranges = [r for r in self._pinned_ranges if r[2]() is not None]
        return any(lo <= a and b <= hi for lo, hi, _ in self._pinned_ranges)

    def good_features(self, img, mask=None, max_corners=500, quality=0.01, min_distance=8, block_size=7):
        img = _c(img, np.uint8)
        H, W = img.shape
        m = None if mask is None else _c(mask, np.uint8)
        cap = max_corners if max_corners > 0 else (H * W + 3) // 4 + 64     # (the C side's candidate capacity)
        xy = np.empty((cap, 2), np.float32)
        n = C.c_int32(0)
        self._chk(self._lib.vo_good_features(self._h, _ptr(img), H, W, _ptr(m), int(max_corners), float(quality),
                                             float(min_distance), int(block_size), _ptr(xy), C.byref(n)))
        return xy[: n.value].copy()

    def good_features_capacity(self, H, W, max_corners):
        """Rows per image the outputs of the batched forms must hold (vo_good_features_capacity)."""
        return int(self._lib.vo_good_features_capacity(int(H), int(W), int(max_corners)))

    @staticmethod
    def _image_stack(what, images, masks=None):
        shapes = {np.shape(a) for a in images}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2:
            raise ValueError("%s: images must be 2-D and of one shape, got %s" % (what, sorted(shapes)))
        imgs = _c(np.stack([np.asarray(a) for a in images]), np.uint8)
        if masks is None:
            return imgs, None
        if len(masks) != len(imgs):
            raise ValueError("%s: %d masks for %d images" % (what, len(masks), len(imgs)))
        if all(m is None for m in masks):
            return imgs, None
        full = np.full(imgs.shape[1:], 255, np.uint8)                # (no mask = every pixel allowed)
        ms = [full if m is None else np.asarray(m) for m in masks]
        if any(m.shape != imgs.shape[1:] for m in ms):
            raise ValueError("%s: a mask's shape differs from the images' %s" % (what, imgs.shape[1:]))
        return imgs, _c(np.stack(ms), np.uint8)

    def good_features_batch(self, imgs, masks=None, max_corners=500, quality=0.01, min_distance=8, block_size=7):
        """Shi-Tomasi corners of S images of one size in one set of launches (vo_good_features_batch): `imgs` is an
        (S, H, W) uint8 array or a list of equal-shape 2-D arrays, `masks` None or one mask (or None) per image.  Returns a
        list of S (n_q, 2) float32 arrays, each what good_features(image, mask, ...) returns."""
        imgs, m = self._image_stack("good_features_batch", imgs, masks)
        S, H, W = imgs.shape
        rows = self.good_features_capacity(H, W, max_corners)
        xy = np.empty((S, rows, 2), np.float32)
        n = np.zeros(S, np.int32)
        self._chk(self._lib.vo_good_features_batch(self._h, _ptr(imgs), _ptr(m), S, H, W, int(max_corners), float(quality),
                                                   float(min_distance), int(block_size), _ptr(xy), _ptr(n)))
        return [xy[q, : n[q]].copy() for q in range(S)]

    def good_features_batch_dev(self, d_imgs, img_stride, S, H, W, d_xy, xy_stride, d_n, d_masks=None, mask_stride=0,
                                max_corners=500, quality=0.01, min_distance=8, block_size=7, d_over=None, d_info=None):
        """vo_good_features_batch_dev on device pointers (dev_alloc): enqueued on the context's stream, nothing read back."""
        def vp(p):
            return C.c_void_p(p) if p else None
        self._chk(self._lib.vo_good_features_batch_dev(self._h, vp(d_imgs), int(img_stride), int(S), int(H), int(W),
                                                       vp(d_masks), int(mask_stride), int(max_corners), float(quality),
                                                       float(min_distance), int(block_size), vp(d_xy), int(xy_stride),
                                                       vp(d_n), vp(d_over), vp(d_info)))

    def sift(self, img, cap=None):
        """(kp (n, 6) float32: x, y, size, angle, response, octave; desc (n, 128) float32).
        cap=None keeps every keypoint, as cv2.SIFT_create() does; an integer keeps the strongest `cap`."""
        img = _c(img, np.uint8)
        H, W = img.shape
        rows = int(cap) if cap else self._lib.vo_sift_capacity(H, W)
        kp = np.empty((rows, 6), np.float32)
        desc = np.empty((rows, 128), np.float32)
        n = C.c_int32(0)
        self._chk(self._lib.vo_sift(self._h, _ptr(img), H, W, int(cap) if cap else 0, _ptr(kp), _ptr(desc), C.byref(n)))
        return kp[: n.value].copy(), desc[: n.value].copy()

    def sift_batch(self, images, cap=None):
        """SIFT on S images of one size in one set of launches (vo_sift_batch): `images` is an (S, H, W) uint8 array or a
        list of equal-shape 2-D arrays.  Returns a list of S (kp, desc) pairs, each what sift(image, cap) returns."""
        shapes = {np.shape(a) for a in images}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2:
            raise ValueError("sift_batch: images must be 2-D and of one shape, got %s" % sorted(shapes))
        imgs = _c(np.stack([np.asarray(a) for a in images]), np.uint8)
        S, H, W = imgs.shape
        rows = int(cap) if cap else self._lib.vo_sift_capacity(H, W)
        kp = np.empty((S, rows, 6), np.float32)
        desc = np.empty((S, rows, 128), np.float32)
        n = np.zeros(S, np.int32)
        self._chk(self._lib.vo_sift_batch(self._h, _ptr(imgs), S, H, W, int(cap) if cap else 0, _ptr(kp), _ptr(desc),
                                          _ptr(n)))
        return [(kp[q, : n[q]].copy(), desc[q, : n[q]].copy()) for q in range(S)]

    def min_eigen_map(self, img, block_size=7):
        img = _c(img, np.uint8)
        H, W = img.shape
        out = np.empty((H, W), np.float32)
        self._chk(self._lib.vo_min_eigen_map(self._h, _ptr(img), H, W, int(block_size), _ptr(out)))
        return out

    # ---- Harris + sub-pixel refinement (klt.py:99-112) ----
    @staticmethod
    def _subpix_criteria(criteria):
        """(type, count, epsilon) -> (max_iter, eps) as cornerSubPix resolves them: without COUNT 100 iterations,
        without EPS no epsilon; the count is clamped to 1..100."""
        kind, count, epsilon = criteria
        max_iter = min(max(int(count), 1), 100) if kind & 1 else 100
        eps = max(float(epsilon), 0.0) if kind & 2 else 0.0
        return max_iter, eps

    def harris_subpix_corners(self, img, block_size=2, ksize=3, k=0.04, rel_threshold=0.01, win=(5, 5),
                              criteria=(3, 100, 0.001), stages=False):
        """cornerHarris -> dilate -> threshold -> connected-component centroids -> cornerSubPix on the device
        (vo_harris_subpix_corners): (n, 2) float32 corners, row 0 the background's.  stages=True also returns a dict of
        the stage outputs: response (H, W) float32, labels (H, W) int32, centroids (n, 2) float64."""
        img = _c(img, np.uint8)
        if img.ndim != 2:
            raise ValueError("harris_subpix_corners: img must be 2-D, got shape %s" % (img.shape,))
        H, W = img.shape
        max_iter, eps = self._subpix_criteria(criteria)
        cap = self._lib.vo_harris_subpix_capacity(H, W)
        xy = np.empty((cap, 2), np.float32)
        n = C.c_int32(0)
        resp = np.empty((H, W), np.float32) if stages else None
        labels = np.empty((H, W), np.int32) if stages else None
        cen = np.empty((cap, 2), np.float64) if stages else None
        self._chk(self._lib.vo_harris_subpix_corners(self._h, _ptr(img), H, W, int(block_size), int(ksize), float(k),
                                                     float(rel_threshold), int(win[0]), int(win[1]), max_iter, eps,
                                                     _ptr(xy), C.byref(n), _ptr(resp), _ptr(labels), _ptr(cen)))
        pts = xy[: n.value].copy()
        return (pts, dict(response=resp, labels=labels, centroids=cen[: n.value].copy())) if stages else pts

    def harris_subpix_corners_batch(self, images, block_size=2, ksize=3, k=0.04, rel_threshold=0.01, win=(5, 5),
                                    criteria=(3, 100, 0.001), stages=False):
        """harris_subpix_corners on S images of one size in one set of launches (vo_harris_subpix_batch): `images` is an
        (S, H, W) uint8 array or a list of equal-shape 2-D arrays.  Returns a list of S results, each what
        harris_subpix_corners(image, ...) returns."""
        shapes = {np.shape(a) for a in images}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2:
            raise ValueError("harris_subpix_corners_batch: images must be 2-D and of one shape, got %s" % sorted(shapes))
        imgs = _c(np.stack([np.asarray(a) for a in images]), np.uint8)
        S, H, W = imgs.shape
        max_iter, eps = self._subpix_criteria(criteria)
        cap = self._lib.vo_harris_subpix_capacity(H, W)
        xy = np.empty((S, cap, 2), np.float32)
        n = np.zeros(S, np.int32)
        resp = np.empty((S, H, W), np.float32) if stages else None
        labels = np.empty((S, H, W), np.int32) if stages else None
        cen = np.empty((S, cap, 2), np.float64) if stages else None
        self._chk(self._lib.vo_harris_subpix_batch(self._h, _ptr(imgs), S, H, W, int(block_size), int(ksize), float(k),
                                                   float(rel_threshold), int(win[0]), int(win[1]), max_iter, eps,
                                                   _ptr(xy), _ptr(n), _ptr(resp), _ptr(labels), _ptr(cen)))
        if not stages:
            return [xy[q, : n[q]].copy() for q in range(S)]
        return [(xy[q, : n[q]].copy(), dict(response=resp[q], labels=labels[q], centroids=cen[q, : n[q]].copy()))
                for q in range(S)]

    def harris_subpix_capacity(self, H, W):
        return self._lib.vo_harris_subpix_capacity(int(H), int(W))

    def harris_subpix_batch_dev(self, d_imgs, img_stride, S, H, W, d_xy, xy_stride, d_n, block_size=2, ksize=3, k=0.04,
                                rel_threshold=0.01, win=(5, 5), criteria=(3, 100, 0.001), d_response=None, d_labels=None,
                                d_centroids=None):
        """vo_harris_subpix_batch_dev: enqueued on the context's stream; the stage outputs may be None."""
        max_iter, eps = self._subpix_criteria(criteria)
        self._chk(self._lib.vo_harris_subpix_batch_dev(
            self._h, C.c_void_p(d_imgs), int(img_stride), int(S), int(H), int(W), int(block_size), int(ksize), float(k),
            float(rel_threshold), int(win[0]), int(win[1]), max_iter, eps, C.c_void_p(d_xy), int(xy_stride),
            C.c_void_p(d_n), C.c_void_p(d_response), C.c_void_p(d_labels), C.c_void_p(d_centroids)))

    # ---- KLT ----
    def klt_num_levels(self, H, W, win, max_level):
        return self._lib.vo_klt_num_levels(int(H), int(W), int(win), int(max_level))

    def pyramid_bytes(self, H, W, n_levels):
        return self._lib.vo_pyramid_bytes(int(H), int(W), int(n_levels))

    def pyr_down(self, img):
        img = _c(img, np.uint8)
        H, W = img.shape
        out = np.empty(((H + 1) // 2, (W + 1) // 2), np.uint8)
        self._chk(self._lib.vo_pyr_down(self._h, _ptr(img), H, W, _ptr(out)))
        return out

    def klt_track(self, prev, nxt, prev_xy, win=17, max_level=2, max_iter=10, eps=0.03, min_eig=1e-4):
        prev = _c(prev, np.uint8)
        nxt = _c(nxt, np.uint8)
        assert prev.shape == nxt.shape and prev.ndim == 2
        H, W = prev.shape
        pts = _c(np.asarray(prev_xy).reshape(-1, 2), np.float32)
        n = pts.shape[0]
        out = np.empty((n, 2), np.float32)
        status = np.empty(n, np.uint8)
        err = np.empty(n, np.float32)
        self._chk(self._lib.vo_klt_track(self._h, _ptr(prev), _ptr(nxt), H, W, _ptr(pts), n, int(win), int(max_level),
                                         int(max_iter), float(eps), float(min_eig), _ptr(out), _ptr(status), _ptr(err)))
        return out, status, err

    def klt_track_fb(self, prev, nxt, prev_xy, win=17, max_level=2, max_iter=10, eps=0.03, min_eig=1e-4, fb_max=1.0):
        """klt_track with the forward-backward check (vo_klt_track_fb): next_pts and err are the forward call's; fb is
        the squared round-trip distance in px^2 (+inf where either pass failed); status = forward & backward &
        (fb <= fb_max^2).  fb_max > 0 pixels, +inf allowed."""
        prev = _c(prev, np.uint8)
        nxt = _c(nxt, np.uint8)
        assert prev.shape == nxt.shape and prev.ndim == 2
        H, W = prev.shape
        pts = _c(np.asarray(prev_xy).reshape(-1, 2), np.float32)
        n = pts.shape[0]
        out = np.empty((n, 2), np.float32)
        status = np.empty(n, np.uint8)
        err = np.empty(n, np.float32)
        fb = np.empty(n, np.float32)
        self._chk(self._lib.vo_klt_track_fb(self._h, _ptr(prev), _ptr(nxt), H, W, _ptr(pts), n, int(win), int(max_level),
                                            int(max_iter), float(eps), float(min_eig), float(fb_max), _ptr(out),
                                            _ptr(status), _ptr(err), _ptr(fb)))
        return out, status, err, fb

    # ---- DLT ----
    def triangulate_dlt(self, x1, x2, C1, C2):
        x1 = _c(np.asarray(x1).reshape(-1, 2), np.float64)
        x2 = _c(np.asarray(x2).reshape(-1, 2), np.float64)
        n = x1.shape[0]
        C1 = _c(C1, np.float64)
        C2 = _c(C2, np.float64).reshape(3, 4)
        per_point = 1 if C1.ndim == 3 else 0
        assert C1.shape[-2:] == (3, 4) and (not per_point or C1.shape[0] == n)
        X = np.empty((n, 3), np.float64)
        self._chk(self._lib.vo_triangulate_dlt(self._h, _ptr(x1), _ptr(x2), n, _ptr(C1), per_point, _ptr(C2), _ptr(X)))
        return X

    # ---- two-view bootstrap ----
    def fundamental_hypotheses(self, p1, p2, samples, threshold, normalize_samples=False, error_kind=0, want_masks=False):
        """8-point F of every sample (samples (Hyp, 8)) and its inlier count over all correspondences:
        (F (Hyp, 3, 3), counts (Hyp,)[, masks (Hyp, N) bool]).  error_kind 0: (p2^T F p1)^2; 1: squared epipolar distance."""
        p1 = _c(np.asarray(p1).reshape(-1, 2), np.float64)
        p2 = _c(np.asarray(p2).reshape(-1, 2), np.float64)
        samples = _c(np.asarray(samples).reshape(-1, 8), np.int32)
        n, h = p1.shape[0], samples.shape[0]
        F = np.empty((h, 3, 3), np.float64)
        counts = np.empty(h, np.int32)
        words = (n + 63) // 64
        masks = np.empty((h, words), np.uint64) if want_masks else None
        self._chk(self._lib.vo_fundamental_hypotheses(self._h, _ptr(p1), _ptr(p2), n, _ptr(samples), h,
                                                      int(bool(normalize_samples)), int(error_kind), float(threshold),
                                                      _ptr(F), _ptr(counts), _ptr(masks)))
        if want_masks == "packed":          # (rows of 64-bit words; Context.unpack_mask(row, n) opens one)
            return F, counts, masks
        if want_masks:
            bits = np.unpackbits(masks.view(np.uint8).reshape(h, words * 8), axis=1, bitorder="little")[:, :n]
            return F, counts, bits.astype(bool)
        return F, counts

    @staticmethod
    def unpack_mask(row, n):
        return np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")[:n].astype(bool)

    def fundamental_fit(self, p1, p2, mask=None, normalize=True):
        """The 8-point fit over all (masked) correspondences: F (3, 3)."""
        p1 = _c(np.asarray(p1).reshape(-1, 2), np.float64)
        p2 = _c(np.asarray(p2).reshape(-1, 2), np.float64)
        m = None if mask is None else _c(np.asarray(mask).reshape(-1), np.uint8)
        F = np.empty((3, 3), np.float64)
        self._chk(self._lib.vo_fundamental_fit(self._h, _ptr(p1), _ptr(p2), p1.shape[0], _ptr(m), int(bool(normalize)), _ptr(F)))
        return F

    def fundamental_ransac(self, p1, p2, threshold, rng, normalize_samples=False, error_kind=0, outlier_ratio=0.9,
                           confidence=0.999, max_iterations=2000):
        """The 8-point RANSAC loop and its closing fit in one call, sampler and accept / adapt rule on the device
        (vo_fundamental_ransac): (F (3, 3), inlier mask (N,) bool, info) with info = {"iterations", "best_count",
        "finished_by_host"}.  rng: a Pcg64 (advanced in place by what the loop consumed) or a NumPy Generator (likewise).
        max_iterations: None / np.inf = unbounded (the host sampler's loop)."""
        p1 = _c(np.asarray(p1).reshape(-1, 2), np.float64)
        p2 = _c(np.asarray(p2).reshape(-1, 2), np.float64)
        n = p1.shape[0]
        pcg = rng if isinstance(rng, Pcg64) else Pcg64.from_generator(rng)
        budget = -1 if max_iterations is None or max_iterations == np.inf else int(max_iterations)
        F = np.empty((3, 3), np.float64)
        mask = np.zeros(n, np.uint8)
        it, best, host = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.vo_fundamental_ransac(self._h, _ptr(p1), _ptr(p2), n, int(bool(normalize_samples)), int(error_kind),
                                                  float(threshold), float(outlier_ratio), float(confidence), budget,
                                                  C.byref(pcg), _ptr(F), _ptr(mask), C.byref(it), C.byref(best), C.byref(host)))
        if not isinstance(rng, Pcg64):
            pcg.to_generator(rng)
        return F, mask.astype(bool), {"iterations": int(it.value), "best_count": int(best.value),
                                      "finished_by_host": int(host.value)}

    # ---- calibrated two-view bootstrap ----
    def essential_hypotheses(self, x1, x2, K1, K2, samples, threshold, error_kind=1, want_masks=False):
        """Every real five-point E of every sample (samples (Hyp, 5)) and its inlier count over all correspondences, scored
        as F = K2^-T E K1^-1 in pixels (vo_essential_hypotheses): (E (Hyp, 10, 3, 3), n_sol (Hyp,), counts (Hyp, 10),
        best_sol (Hyp,)[, masks (Hyp, 10, N) bool]).  error_kind 0: (p2^T F p1)^2; 1: squared epipolar distance.
        want_masks="packed": rows of 64-bit words (Context.unpack_mask(row, n) opens one)."""
        x1 = _c(np.asarray(x1).reshape(-1, 2), np.float64)
        x2 = _c(np.asarray(x2).reshape(-1, 2), np.float64)
        K1 = _c(np.asarray(K1).reshape(3, 3), np.float64)
        K2 = _c(np.asarray(K2).reshape(3, 3), np.float64)
        samples = _c(np.asarray(samples).reshape(-1, 5), np.int32)
        n, h = x1.shape[0], samples.shape[0]
        E = np.empty((h, 10, 3, 3), np.float64)
        n_sol = np.empty(h, np.int32)
        counts = np.empty((h, 10), np.int32)
        best_sol = np.empty(h, np.int32)
        words = (n + 63) // 64
        masks = np.empty((h, 10, words), np.uint64) if want_masks else None
        self._chk(self._lib.vo_essential_hypotheses(self._h, _ptr(x1), _ptr(x2), n, _ptr(K1), _ptr(K2), _ptr(samples), h,
                                                    int(error_kind), float(threshold), _ptr(E), _ptr(n_sol), _ptr(counts),
                                                    _ptr(best_sol), _ptr(masks)))
        if want_masks == "packed":
            return E, n_sol, counts, best_sol, masks
        if want_masks:
            bits = np.unpackbits(masks.view(np.uint8).reshape(h, 10, words * 8), axis=2, bitorder="little")[:, :, :n]
            return E, n_sol, counts, best_sol, bits.astype(bool)
        return E, n_sol, counts, best_sol

    def essential_ransac(self, x1, x2, K1, K2, threshold, rng, error_kind=1, outlier_ratio=0.9, confidence=0.999,
                         max_iterations=2000):
        """The five-point RANSAC loop in one call (vo_essential_ransac): (E (3, 3), inlier mask (N,) bool, info) with
        info = {"iterations", "best_count"}; E is the accepted minimal-sample model, there is no closing fit.  rng: a Pcg64
        (advanced in place by what the loop consumed) or a NumPy Generator (likewise).  max_iterations: None / np.inf =
        unbounded."""
        x1 = _c(np.asarray(x1).reshape(-1, 2), np.float64)
        x2 = _c(np.asarray(x2).reshape(-1, 2), np.float64)
        K1 = _c(np.asarray(K1).reshape(3, 3), np.float64)
        K2 = _c(np.asarray(K2).reshape(3, 3), np.float64)
        n = x1.shape[0]
        pcg = rng if isinstance(rng, Pcg64) else Pcg64.from_generator(rng)
        budget = -1 if max_iterations is None or max_iterations == np.inf else int(max_iterations)
        E = np.empty((3, 3), np.float64)
        mask = np.zeros(n, np.uint8)
        it, best = C.c_int64(0), C.c_int32(0)
        rc = self._lib.vo_essential_ransac(self._h, _ptr(x1), _ptr(x2), n, _ptr(K1), _ptr(K2), int(error_kind), float(threshold),
                                           float(outlier_ratio), float(confidence), budget, C.byref(pcg), _ptr(E), _ptr(mask),
                                           C.byref(it), C.byref(best))
        if not isinstance(rng, Pcg64) and rc != VO_EINVAL:
            pcg.to_generator(rng)
        self._chk(rc)
        return E, mask.astype(bool), {"iterations": int(it.value), "best_count": int(best.value)}

    def rng_raw32_device(self, pcg, count):
        """The next `count` 32-bit outputs of `pcg` (a Pcg64, advanced in place) made by the device's fill kernel."""
        out = np.empty(int(count), np.uint32)
        self._chk(self._lib.vo_rng_raw32_device(self._h, C.byref(pcg), int(count), _ptr(out)))
        return out

    def essential_decompose(self, E):
        E = _c(np.asarray(E).reshape(3, 3), np.float64)
        M4 = np.empty((4, 3, 4), np.float64)
        self._chk(self._lib.vo_essential_decompose(self._h, _ptr(E), _ptr(M4)))
        return M4

    def relative_pose(self, x1, x2, K1, K2, F, inliers=None):
        """(M (3, 4), X (N, 3), mask (N,) bool, M4 (4, 3, 4)): the cheirality vote over the four decompositions of
        E = K2^T F K1 and the winner's triangulation of all correspondences."""
        x1 = _c(np.asarray(x1).reshape(-1, 2), np.float64)
        x2 = _c(np.asarray(x2).reshape(-1, 2), np.float64)
        K1 = _c(np.asarray(K1).reshape(3, 3), np.float64)
        K2 = _c(np.asarray(K2).reshape(3, 3), np.float64)
        F = _c(np.asarray(F).reshape(3, 3), np.float64)
        inl = None if inliers is None else _c(np.asarray(inliers).reshape(-1), np.uint8)
        n = x1.shape[0]
        M, X, mask, M4 = np.empty((3, 4)), np.empty((n, 3)), np.empty(n, np.uint8), np.empty((4, 3, 4))
        self._chk(self._lib.vo_relative_pose(self._h, _ptr(x1), _ptr(x2), n, _ptr(inl), _ptr(K1), _ptr(K2), _ptr(F), _ptr(M),
                                             _ptr(X), _ptr(mask), _ptr(M4)))
        return M, X, mask.astype(bool), M4

    # ---- P3P ----
    def p3p_hypotheses(self, X, x, K, samples, thr_sq, want_masks=False):
        X = _c(np.asarray(X).reshape(-1, 3), np.float64)
        x = _c(np.asarray(x).reshape(-1, 2), np.float64)
        K = _c(K, np.float64).reshape(3, 3)
        samples = _c(np.asarray(samples).reshape(-1, 4), np.int32)
        n, h = X.shape[0], samples.shape[0]
        R = np.empty((h, 3, 3), np.float64)
        t = np.empty((h, 3), np.float64)
        valid = np.empty(h, np.uint8)
        counts = np.empty(h, np.int32)
        words = (n + 63) // 64
        masks = np.empty((h, words), np.uint64) if want_masks else None
        self._chk(self._lib.vo_p3p_hypotheses(self._h, _ptr(X), _ptr(x), n, _ptr(K), _ptr(samples), h, float(thr_sq),
                                              _ptr(R), _ptr(t), _ptr(valid), _ptr(counts), _ptr(masks)))
        if want_masks:
            bits = np.unpackbits(masks.view(np.uint8).reshape(h, words * 8), axis=1, bitorder="little")[:, :n]
            return R, t, valid, counts, bits.astype(bool)
        return R, t, valid, counts

    def refine_pose(self, X, x, K, R0, t0, inlier_mask=None, max_iter=20):
        """Least-squares pose from (R0, t0) over the (masked) correspondences: (R, t (3,), iterations, cost)
        -- the minimiser p3p.py:188-213 asks SciPy for (vo_refine_pose)."""
        X = _c(np.asarray(X).reshape(-1, 3), np.float64)
        x = _c(np.asarray(x).reshape(-1, 2), np.float64)
        K = _c(K, np.float64)
        R0 = _c(np.asarray(R0).reshape(3, 3), np.float64)
        t0 = _c(np.asarray(t0).reshape(3), np.float64)
        m = None if inlier_mask is None else _c(np.asarray(inlier_mask).reshape(-1), np.uint8)
        R, t = np.empty((3, 3)), np.empty(3)
        it, cost = C.c_int32(), C.c_double()
        self._chk(self._lib.vo_refine_pose(self._h, _ptr(X), _ptr(x), len(X), _ptr(K), _ptr(m), _ptr(R0), _ptr(t0),
                                           int(max_iter), _ptr(R), _ptr(t), C.byref(it), C.byref(cost)))
        return R, t, it.value, cost.value

    def reproj_inliers(self, X, x, K, R, t, thr_sq, want_err=False):
        X = _c(np.asarray(X).reshape(-1, 3), np.float64)
        x = _c(np.asarray(x).reshape(-1, 2), np.float64)
        K = _c(K, np.float64).reshape(3, 3)
        R = _c(R, np.float64).reshape(3, 3)
        t = _c(np.asarray(t).reshape(3), np.float64)
        n = X.shape[0]
        mask = np.empty(n, np.uint8)
        err = np.empty(n, np.float64) if want_err else None
        self._chk(self._lib.vo_reproj_inliers(self._h, _ptr(X), _ptr(x), n, _ptr(K), _ptr(R), _ptr(t), float(thr_sq),
                                              _ptr(mask), _ptr(err)))
        return (mask.astype(bool), err) if want_err else mask.astype(bool)

    # ---- device-pointer variants (async on the context's stream) ----
    def pyramid_build_dev(self, d_img, H, W, n_levels, d_pyr):
        self._chk(self._lib.vo_pyramid_build_dev(self._h, C.c_void_p(d_img), H, W, int(n_levels), C.c_void_p(d_pyr)))

    def klt_track_dev(self, d_prev, d_prev_pyr, d_next, d_next_pyr, H, W, n_levels, d_prev_xy, N, win, max_iter, eps,
                      min_eig, d_next_xy, d_status, d_err):
        self._chk(self._lib.vo_klt_track_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_prev_pyr), C.c_void_p(d_next),
                                             C.c_void_p(d_next_pyr), H, W, int(n_levels), C.c_void_p(d_prev_xy), int(N),
                                             int(win), int(max_iter), float(eps), float(min_eig),
                                             C.c_void_p(d_next_xy), C.c_void_p(d_status), C.c_void_p(d_err)))

    def klt_track_fb_dev(self, d_prev, d_prev_pyr, d_next, d_next_pyr, H, W, n_levels, d_prev_xy, N, win, max_iter, eps,
                         min_eig, fb_max, d_next_xy, d_status, d_err, d_fb):
        self._chk(self._lib.vo_klt_track_fb_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_prev_pyr), C.c_void_p(d_next),
                                                C.c_void_p(d_next_pyr), H, W, int(n_levels), C.c_void_p(d_prev_xy), int(N),
                                                int(win), int(max_iter), float(eps), float(min_eig), float(fb_max),
                                                C.c_void_p(d_next_xy), C.c_void_p(d_status), C.c_void_p(d_err),
                                                C.c_void_p(d_fb)))

    def triangulate_dlt_dev(self, d_x1, d_x2, n, d_C1, per_point, d_C2, d_X):
        self._chk(self._lib.vo_triangulate_dlt_dev(self._h, C.c_void_p(d_x1), C.c_void_p(d_x2), int(n),
                                                   C.c_void_p(d_C1), int(per_point), C.c_void_p(d_C2), C.c_void_p(d_X)))

    def p3p_hypotheses_dev(self, d_X, d_x, N, K, d_samples, Hyp, thr_sq, d_R, d_t, d_valid, d_counts, d_masks):
        K = _c(K, np.float64).reshape(3, 3)
        self._chk(self._lib.vo_p3p_hypotheses_dev(self._h, C.c_void_p(d_X), C.c_void_p(d_x), int(N), _ptr(K),
                                                  C.c_void_p(d_samples), int(Hyp), float(thr_sq), C.c_void_p(d_R),
                                                  C.c_void_p(d_t), C.c_void_p(d_valid), C.c_void_p(d_counts),
                                                  C.c_void_p(d_masks)))

    def reproj_inliers_dev(self, d_X, d_x, N, K, d_Rt, thr_sq, d_mask, d_err):
        K = _c(K, np.float64).reshape(3, 3)
        self._chk(self._lib.vo_reproj_inliers_dev(self._h, C.c_void_p(d_X), C.c_void_p(d_x), int(N), _ptr(K),
                                                  C.c_void_p(d_Rt), float(thr_sq), C.c_void_p(d_mask), C.c_void_p(d_err)))

    def refine_pose_dev(self, d_X, d_x, N, K, d_mask, d_Rt0, max_iter, d_out14):
        """vo_refine_pose_dev: d_mask (N bytes) may be None; d_Rt0 = R0 then t0 (12 doubles); d_out14 receives R, t,
        iterations, cost."""
        K = _c(K, np.float64).reshape(3, 3)
        self._chk(self._lib.vo_refine_pose_dev(self._h, C.c_void_p(d_X), C.c_void_p(d_x), int(N), _ptr(K),
                                               C.c_void_p(d_mask), C.c_void_p(d_Rt0), int(max_iter), C.c_void_p(d_out14)))

    def harris_response_dev(self, d_img, H, W, patch, kappa, d_scores):
        self._chk(self._lib.vo_harris_response_dev(self._h, C.c_void_p(d_img), H, W, int(patch), float(kappa),
                                                   C.c_void_p(d_scores)))

    def nms_keypoints_dev(self, d_scores, H, W, N, r, d_kp):
        self._chk(self._lib.vo_nms_keypoints_dev(self._h, C.c_void_p(d_scores), H, W, int(N), int(r),
                                                 C.c_void_p(d_kp)))

    def patch_descriptors_dev(self, d_img, H, W, d_kp, N, r, d_desc):
        self._chk(self._lib.vo_patch_descriptors_dev(self._h, C.c_void_p(d_img), H, W, C.c_void_p(d_kp), int(N),
                                                     int(r), C.c_void_p(d_desc)))

    def sift_all_batch_dev(self, d_imgs, img_stride, S, H, W, rows, d_kp, kp_stride, d_desc, d_desc_u8, desc_stride, d_n,
                           d_over=None):
        """Every SIFT keypoint of S images on the device (vo_sift_all_batch_dev); d_desc / d_desc_u8 / d_over may be
        None.  Image q's count lands in d_n[q], 0 when d_over[q] != 0 (1: list overflow, 2: more than `rows`)."""
        self._chk(self._lib.vo_sift_all_batch_dev(self._h, C.c_void_p(d_imgs), int(img_stride), int(S), H, W, int(rows),
                                                  C.c_void_p(d_kp), int(kp_stride), C.c_void_p(d_desc),
                                                  C.c_void_p(d_desc_u8), int(desc_stride), C.c_void_p(d_n),
                                                  C.c_void_p(d_over)))


class Comm:
    """RCCL communicator of the shared-map exchange for hosts without torch.distributed (vo_comm_*): rank 0 makes the
    id (`Comm.unique_id(ctx)`, 128 bytes) and hands it to the other ranks by its own means; every rank then constructs
    Comm(ctx, world, rank, id)."""

    @staticmethod
    def unique_id(ctx):
        buf = C.create_string_buffer(128)
        ctx._chk(ctx._lib.vo_comm_unique_id(ctx._h, buf))
        return buf.raw

    def __init__(self, ctx, world, rank, uid):
        assert len(uid) == 128
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        h = C.c_void_p()
        ctx._chk(ctx._lib.vo_comm_create(ctx._h, self.world, self.rank, C.c_char_p(uid), C.byref(h)))
        self._h = h

    def allgather_state(self, T_cw, landmarks, cap):
        """One record per rank, host arrays, synchronous: (world, 17 + 3 cap) float64."""
        T = _c(np.asarray(T_cw).reshape(16), np.float64)
        lm = _c(np.asarray(landmarks).reshape(-1, 3), np.float64)
        out = np.empty((self.world, 17 + 3 * int(cap)), np.float64)
        self.ctx._chk(self.ctx._lib.vo_allgather_state(self.ctx._h, self._h, _ptr(T), _ptr(lm), lm.shape[0], int(cap), _ptr(out)))
        return out

    def allgather_dev(self, d_records, doubles_per_rank, d_all, stream=None):
        self.ctx._chk(self.ctx._lib.vo_allgather_state_dev(self.ctx._h, self._h, C.c_void_p(d_records), int(doubles_per_rank),
                                                           C.c_void_p(d_all), C.c_void_p(stream or 0)))

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.vo_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rng_choice(pcg, pop, s, count):
    """`count` draws of Generator.choice(arange(pop), replace=False, size=s); advances `pcg` (host only)."""
    out = np.empty((count, s), np.int32)
    rc = load().vo_rng_choice(C.byref(pcg), int(pop), int(s), int(count), _ptr(out))
    if rc != VO_OK:
        raise VoError(rc, "vo_rng_choice(pop=%d, s=%d)" % (pop, s))
    return out


def rng_choice8_from_raw(raw, pop):
    """One Generator.choice(pop, 8, replace=False) from the 15 generator outputs it consumes when no draw is rejected:
    (sample (8,) int32, possibly_rejected).  pop >= 9 (host only)."""
    raw = _c(np.asarray(raw).reshape(15), np.uint32)
    out = np.empty(8, np.int32)
    flag = C.c_int(0)
    rc = load().vo_rng_choice8_from_raw(_ptr(raw), int(pop), _ptr(out), C.byref(flag))
    if rc != VO_OK:
        raise VoError(rc, "vo_rng_choice8_from_raw(pop=%d)" % pop)
    return out, int(flag.value)


def ransac_num_iterations(confidence, outlier_ratio, s):
    return int(load().vo_ransac_num_iterations(float(confidence), float(outlier_ratio), int(s)))


from vo._pipeline import Pipeline  # noqa: E402,F401  (device-resident frame loop, vo_pipeline_*)


_default_ctx = None


def release_cached():
    """vo_pipeline_release_cached: destroy the side streams / workspace kept from closed pipelines."""
    if _lib is not None:
        _lib.vo_pipeline_release_cached()


def _release_cached_at_exit():
    if _lib is not None and _lib.vo_pipeline_release_cached_at_exit():
        _lib.vo_pipeline_release_cached()


atexit.register(_release_cached_at_exit)        # (before the interpreter and the HIP runtime are torn down)


def set_default_context(ctx):
    """Make `ctx` the context the drop-in classes use when none is passed to them."""
    global _default_ctx
    _default_ctx = ctx


def default_context():
    """Process-wide context on the device selected by LOCAL_RANK (or device 0)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("VO_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _default_ctx
