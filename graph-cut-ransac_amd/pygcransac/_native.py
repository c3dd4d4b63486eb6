"""ctypes view of the engine's C ABI (include/gcr.h).

The shared library ``libgcr.so`` is built in-tree next to this file (see
``graph-cut-ransac_amd/csrc/Makefile``).  Importing this module fails loudly if
it is missing: there is no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GCR_LIB selects an alternative in-tree build of the same engine (the
# diagnostic libgcr_stamps.so of tools/stamp_probe.py)
LIB_PATH = os.path.join(_HERE, os.environ.get("GCR_LIB", "libgcr.so"))

GCR_OK = 0
GCR_EINVAL = -22
GCR_ENODEV = -19
SOLVER_SCALE3, SOLVER_SCALE3_ORIGINAL, SOLVER_SIFT22, SOLVER_HOMOGRAPHY4, SOLVER_FUNDAMENTAL7 = 0, 1, 2, 3, 4
SOLVER_ESSENTIAL5 = 5    # problems of this kind come from gcr_problem_create_essential
SOLVER_ESSENTIAL3_GRAVITY = 6   # ... from gcr_problem_create_gravity_essential
SOLVER_HOMOGRAPHY2_SIFT = 7     # ... from gcr_problem_create_sift_homography
FLAG_NO_LO = 1
FLAG_GUIDED_STOP = 2     # guided sampling only: the adaptive stop on the inlier mass (csrc/guided_stop.h)
FLAG_PROSAC_STOP = 4     # PROSAC sampling only: the adaptive stop on the best-ranked prefix (csrc/prosac_stop.h)


class Params(C.Structure):
    _fields_ = [
        ("scale_residual_thresh", C.c_double),
        ("orientation_residual_thresh", C.c_double),
        ("spatial_coherence_weight", C.c_double),
        ("min_iteration_number", C.c_uint64),
        ("max_iteration_number", C.c_uint64),
        ("max_local_optimization_number", C.c_uint64),
        ("confidence", C.c_double),
        ("seed", C.c_uint64),
        ("batch_slots", C.c_uint32),
        ("flags", C.c_uint32),
        ("cell_size", C.c_double * 4),      # H / F neighbourhood grid (x1, y1, x2, y2)
        ("cell_number", C.c_uint32),        # cells along every axis, 0 = empty grid
        ("reserved", C.c_uint32),
    ]


class RectModel(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("x0", "y0", "s", "h7", "h8", "alpha", "phi")]


class Stats(C.Structure):
    _fields_ = [
        ("iteration_number", C.c_uint64),
        ("local_optimization_number", C.c_uint64),
        ("graph_cut_number", C.c_uint64),
        ("slots", C.c_uint64),
        ("hypotheses", C.c_uint64),
        ("hypotheses_computed", C.c_uint64),
        ("lo_models", C.c_uint64),
        ("launches", C.c_uint64),
        ("score", C.c_double),
        ("ms_setup", C.c_double),
        ("ms_generate", C.c_double),
        ("ms_score", C.c_double),
        ("ms_replay", C.c_double),
        ("ms_lo", C.c_double),
        ("ms_refit", C.c_double),
        ("ms_total", C.c_double),
        ("ms_score_kernel", C.c_double),
        ("ms_lo_lists", C.c_double),
        ("ms_lo_fit", C.c_double),
        ("ms_lo_score", C.c_double),
        ("ms_refit_fit", C.c_double),
        ("prefetched_chunks", C.c_uint64),
        ("exact_models", C.c_uint64),
        ("exact_pairs", C.c_uint64),
        ("exact_flips", C.c_uint64),
        ("ms_exact", C.c_double),
        ("near_ties", C.c_uint64),
        ("near_tie_flips", C.c_uint64),
        ("lo_refolds", C.c_uint64),
        ("chunk_msac_lists", C.c_uint64),
    ]

    def as_dict(self):
        # one read of the whole struct through a numpy record (ints and floats
        # as getattr would give them), not 30-odd ctypes attribute reads
        return dict(zip(_STATS_NAMES, np.frombuffer(self, dtype=_STATS_DT)[0].tolist()))


_STATS_DT = np.dtype(Stats)
_STATS_NAMES = _STATS_DT.names


class BatchResult(C.Structure):
    _fields_ = [
        ("models", C.c_uint64),
        ("iterations", C.c_uint64),
        ("best_slot", C.c_int64),
        ("best_score", C.c_double),
        ("best_inliers", C.c_uint64 * 2),
        ("best_model", RectModel),
    ]


class BatchItem(C.Structure):
    _fields_ = [
        ("solver", C.c_int),
        ("f0", C.POINTER(C.c_double)),
        ("n0", C.c_size_t),
        ("f1", C.POINTER(C.c_double)),
        ("n1", C.c_size_t),
        ("params", Params),
        ("mask0_out", C.POINTER(C.c_uint8)),
        ("mask1_out", C.POINTER(C.c_uint8)),
        ("H_out", C.c_double * 9),
        ("model_out", RectModel),
        ("stats_out", Stats),
        ("result", C.c_int),
    ]


class MatchOptions(C.Structure):
    """gcr_match_options: the front-end rule of the descriptor-set entries"""
    _fields_ = [
        ("has_ratio", C.c_int),
        ("rr", C.c_double),
        ("mutual", C.c_int),
        ("has_max_distance", C.c_int),
        ("max_distance", C.c_double),
    ]


class ManyResult(C.Structure):
    """gcr_many_result: one problem's record of gcr_verify_many"""
    _fields_ = [
        ("models", C.c_uint64),
        ("iterations", C.c_uint64),
        ("best_slot", C.c_int64),
        ("best_hypothesis", C.c_uint32),
        ("best_inliers", C.c_uint32),
        ("best_score", C.c_double),
        ("best_model", C.c_double * 9),
    ]


MANY_DT = np.dtype(ManyResult)


# int (*)(void* user, const void* send, void* recv, size_t bytes)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"pygcransac: HIP engine library not found at {LIB_PATH}; build it with "
            "`make -C graph-cut-ransac_amd/csrc` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    dp, u8p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    vp = C.c_void_p
    L.gcr_last_error.restype = C.c_char_p
    L.gcr_abi_version.restype = C.c_int
    L.gcr_device_count.restype = C.c_int
    L.gcr_kernel_build_id.restype = C.c_char_p
    L.gcr_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.gcr_synchronize.argtypes = [vp]
    L.gcr_destroy.argtypes = [vp]
    L.gcr_destroy.restype = None
    L.gcr_default_params.argtypes = [C.POINTER(Params)]
    L.gcr_default_params.restype = None
    # the public entry points take their arrays as plain addresses (c_void_p
    # also accepts typed pointers): the wrappers pass ndarray.ctypes.data,
    # a third of their per-call Python cost otherwise
    L.gcr_rect_scale_only.argtypes = [vp, vp, C.c_size_t, C.POINTER(Params), C.c_int, vp, vp,
                                      C.POINTER(RectModel), C.POINTER(Stats)]
    L.gcr_rect_sift.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(Params), vp, vp, vp,
                                C.POINTER(RectModel), C.POINTER(Stats)]
    L.gcr_problem_create.argtypes = [vp, C.c_int, dp, C.c_size_t, dp, C.c_size_t, C.POINTER(vp)]
    L.gcr_problem_destroy.argtypes = [vp]
    L.gcr_problem_destroy.restype = None
    L.gcr_problem_run.argtypes = [vp, C.POINTER(Params), u8p, u8p, dp, C.POINTER(RectModel), C.POINTER(Stats)]
    L.gcr_problem_run_sharded.argtypes = [vp, C.POINTER(Params), C.c_int, C.c_int, ALLGATHER_FN, vp, u8p, u8p, dp,
                                          C.POINTER(RectModel), C.POINTER(Stats)]
    L.gcr_comm_unique_id.argtypes = [u8p]
    L.gcr_comm_create.argtypes = [vp, C.c_int, C.c_int, u8p, C.POINTER(vp)]
    L.gcr_comm_destroy.argtypes = [vp]
    L.gcr_comm_destroy.restype = None
    L.gcr_problem_run_comm.argtypes = [vp, C.POINTER(Params), vp, u8p, u8p, dp, C.POINTER(RectModel),
                                       C.POINTER(Stats)]
    L.gcr_solve_batch.argtypes = [C.c_int, C.POINTER(BatchItem), C.c_size_t, C.c_int]
    L.gcr_problem_verify_batch.argtypes = [vp, C.POINTER(Params), C.c_uint64, C.c_uint32, C.POINTER(BatchResult),
                                           C.POINTER(Stats)]
    L.gcr_problem_verify_batches.argtypes = [vp, C.POINTER(Params), C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.POINTER(BatchResult), C.POINTER(Stats)]
    L.gcr_debug_generate.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, u8p, C.POINTER(RectModel)]
    L.gcr_debug_score.argtypes = [vp, C.POINTER(Params), C.POINTER(RectModel), C.c_uint32, u32p, u32p, dp, dp, dp]
    L.gcr_debug_verify_slots.argtypes = [vp, C.POINTER(Params), C.c_uint64, C.c_uint32, u8p, u32p, u32p, dp, dp, dp]
    L.gcr_debug_verify_bound.argtypes = [vp, C.POINTER(Params), C.c_uint64, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
    L.gcr_debug_verify_bound_live.argtypes = [vp, C.POINTER(Params), C.c_uint64, C.c_uint32, C.c_uint32, u32p]
    L.gcr_debug_score_less.argtypes = [vp, C.POINTER(Params), C.POINTER(RectModel), C.POINTER(RectModel)]
    L.gcr_debug_exchange_log.argtypes = [C.POINTER(C.c_uint64), C.c_size_t]
    L.gcr_debug_exchange_log.restype = C.c_size_t
    L.gcr_debug_mask.argtypes = [vp, C.POINTER(Params), C.POINTER(RectModel), C.c_int, C.c_int, u8p]
    L.gcr_host_log.argtypes = [C.c_double]
    L.gcr_host_log.restype = C.c_double
    L.gcr_host_pow_m3.argtypes = [C.c_double]
    L.gcr_host_pow_m3.restype = C.c_double
    L.gcr_host_atan2.argtypes = [C.c_double, C.c_double]
    L.gcr_host_atan2.restype = C.c_double
    L.gcr_host_math.argtypes = [C.c_int, C.c_double, C.c_double]
    L.gcr_host_math.restype = C.c_double
    L.gcr_host_sample.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                  C.c_uint32, u32p]
    L.gcr_debug_math.argtypes = [vp, C.c_int, dp, dp, C.c_size_t, dp]
    L.gcr_measure_hbm.argtypes = [vp, C.c_size_t, C.c_int, dp]
    L.gcr_warp_perspective.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, vp, C.c_int,
                                       C.c_int]
    L.gcr_host_fit_nonminimal.argtypes = [C.c_int, dp, C.c_size_t, dp, C.c_size_t, u32p, C.c_size_t, u32p,
                                          C.c_size_t, C.POINTER(RectModel)]
    L.gcr_debug_fit_nonminimal.argtypes = [vp, u32p, C.c_size_t, u32p, C.c_size_t, C.c_int, C.POINTER(RectModel)]
    L.gcr_find_homography.argtypes = [vp, vp, C.c_size_t, C.POINTER(Params), vp, vp, C.POINTER(Stats)]
    L.gcr_debug_generate_h.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, u8p, dp]
    L.gcr_debug_score_h.argtypes = [vp, C.POINTER(Params), dp, C.c_uint32, u32p, dp, dp]
    L.gcr_debug_mask_h.argtypes = [vp, C.POINTER(Params), dp, C.c_int, u8p]
    L.gcr_host_fit_h.argtypes = [dp, C.c_size_t, u32p, C.c_size_t, dp]
    L.gcr_find_fundamental_matrix.argtypes = L.gcr_find_homography.argtypes
    L.gcr_host_fit_f.argtypes = L.gcr_host_fit_h.argtypes
    # guided (importance) sampling: gcr_problem_set_probabilities, the guided
    # one-shot entries and their host / debug hooks
    L.gcr_problem_set_probabilities.argtypes = [vp, vp, C.c_size_t]
    L.gcr_find_homography_guided.argtypes = [vp, vp, C.c_size_t, vp, C.POINTER(Params), vp, vp, C.POINTER(Stats)]
    L.gcr_find_fundamental_matrix_guided.argtypes = L.gcr_find_homography_guided.argtypes
    L.gcr_host_sample_guided.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                         C.c_uint32, u32p]
    L.gcr_host_guided_index.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint64, u32p]
    L.gcr_host_check_probabilities.argtypes = [vp, C.c_size_t, C.c_uint32]
    L.gcr_debug_sample_h.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u32p]
    L.gcr_measure_generate_h.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, dp]
    L.gcr_host_solve_minimal.argtypes = [C.c_int, dp, C.c_size_t, u32p, dp, u32p]
    # the guided stop (GCR_FLAG_GUIDED_STOP): its host definition and its kernel alone
    u64p = C.POINTER(C.c_uint64)
    L.gcr_host_guided_quanta.argtypes = [vp, C.c_size_t, C.c_uint32, u64p, u64p]
    L.gcr_host_guided_iterations.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, u64p]
    L.gcr_debug_inlier_mass_h.argtypes = [vp, C.POINTER(Params), dp, C.c_uint32, u32p, u64p]
    # PROSAC sampling (csrc/prosac.h): gcr_problem_set_prosac and its host definition
    L.gcr_problem_set_prosac.argtypes = [vp, C.c_uint64]
    L.gcr_host_prosac_growth.argtypes = [C.c_size_t, C.c_uint32, C.c_uint64, u64p]
    L.gcr_host_prosac_pool.argtypes = [C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, u32p]
    L.gcr_host_sample_prosac.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint64,
                                         u32p]
    # the PROSAC stop (GCR_FLAG_PROSAC_STOP, csrc/prosac_stop.h): its host definition and its kernel alone
    u8p = C.POINTER(C.c_uint8)
    L.gcr_host_prosac_stop_tables.argtypes = [C.c_size_t, C.c_uint32, C.c_uint64, C.c_double, u32p, dp]
    L.gcr_host_prosac_stop.argtypes = [u8p, C.c_size_t, C.c_uint32, u32p, dp, u32p, u32p]
    L.gcr_host_prosac_stop_number.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, u64p]
    L.gcr_debug_prosac_stop_h.argtypes = [vp, C.POINTER(Params), dp, C.c_uint32, u32p, u32p, u32p]
    # NAPSAC sampling (csrc/napsac.h): gcr_problem_set_napsac and its host definition
    L.gcr_problem_set_napsac.argtypes = [vp, dp, C.c_uint64]
    L.gcr_host_napsac_layers.argtypes = [dp, C.c_size_t, dp, u32p, u32p, u32p, u32p]
    L.gcr_host_sample_napsac.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, dp, C.c_size_t, C.c_uint32, dp,
                                         C.c_uint64, u32p]
    L.gcr_host_samples_napsac.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, dp, C.c_size_t, C.c_uint32,
                                          dp, C.c_uint64, u32p]
    L.gcr_host_generate_napsac.argtypes = [C.c_int, dp, dp, dp, dp, dp, C.c_size_t, dp, C.c_uint64, C.c_uint64,
                                           C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint8), dp]
    # essential matrix (csrc/ess.h): pixel rows + calibration matrices
    L.gcr_find_essential_matrix.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.POINTER(Params), vp, vp,
                                            C.POINTER(Stats)]
    L.gcr_problem_create_essential.argtypes = [vp, vp, C.c_size_t, vp, vp, C.POINTER(vp)]
    L.gcr_host_fit_e.argtypes = L.gcr_host_fit_h.argtypes
    L.gcr_host_generate_e.argtypes = [vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, vp, vp]
    L.gcr_host_essential_normalise.argtypes = [vp, C.c_size_t, vp, vp, C.c_double, vp, dp]
    # essential matrix with known gravity (csrc/grav.h): ... + the two gravity-alignment rotations
    L.gcr_find_gravity_essential_matrix.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(Params), vp, vp,
                                                    C.POINTER(Stats)]
    L.gcr_problem_create_gravity_essential.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.POINTER(vp)]
    L.gcr_host_check_gravity.argtypes = [vp, vp]
    L.gcr_host_solve_g3.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, u32p]
    L.gcr_host_fit_g.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]
    L.gcr_host_generate_g.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, vp, vp]
    # homography from two SIFT correspondences (csrc/sifth.h): rows + N x 4 SIFT columns (q1, q2, alpha1, alpha2)
    L.gcr_find_homography_sift.argtypes = [vp, vp, vp, C.c_size_t, vp, C.POINTER(Params), vp, vp, C.POINTER(Stats)]
    L.gcr_problem_create_sift_homography.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(vp)]
    L.gcr_host_check_sift.argtypes = [vp, C.c_size_t]
    L.gcr_host_solve_s2.argtypes = [vp, vp, C.c_size_t, vp, vp, u32p]
    L.gcr_host_generate_s.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, vp, vp]
    # descriptor matching (csrc/match.h): uint8 descriptors in, idx / dist / idx2 / dist2 (uint32) out
    L.gcr_match_descriptors.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, vp, vp, vp, vp, dp]
    L.gcr_host_match_descriptors.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_int, vp, vp, vp, vp]
    # guided matching (csrc/match_geo.h): positions, kind, model, squared bound, direction
    L.gcr_match_descriptors_guided.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, vp,
                                               C.c_double, C.c_int, vp, vp, vp, vp, dp]
    L.gcr_host_match_descriptors_guided.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, vp,
                                                    C.c_double, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gcr_match_tiling.argtypes = [u32p]
    L.gcr_match_tiling.restype = None
    # resident descriptor sets (csrc/match_sets.h): matches (uint32 pairs) and ratios (doubles) out
    mop, szp = C.POINTER(MatchOptions), C.POINTER(C.c_size_t)
    L.gcr_descriptors_create.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, C.POINTER(vp)]
    L.gcr_descriptors_destroy.argtypes = [vp]
    L.gcr_descriptors_destroy.restype = None
    L.gcr_descriptors_info.argtypes = [vp, szp, u32p, C.POINTER(C.c_int)]
    L.gcr_match_sets.argtypes = [vp, vp, vp, mop, vp, vp, C.c_size_t, szp, vp]
    L.gcr_match_sets_guided.argtypes = [vp, vp, vp, C.c_int, vp, C.c_double, mop, vp, vp, C.c_size_t, szp, vp]
    L.gcr_match_set_pairs.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, mop, vp, vp, vp, vp, vp]
    L.gcr_host_match_select.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, mop, vp, vp,
                                        C.c_size_t, szp]
    L.gcr_match_select_tiling.argtypes = [u32p]
    L.gcr_match_select_tiling.restype = None
    L.gcr_debug_match_workspace.argtypes = [vp, C.POINTER(C.c_uint64)]
    # k nearest neighbours (csrc/match_knn.h): idx / dist (uint32, n1 x k) out
    L.gcr_knn_descriptors.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, dp]
    L.gcr_host_knn_descriptors.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, vp, vp]
    L.gcr_knn_sets.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, dp]
    # many small problems per call (csrc/verify_many.h): packed rows, offsets (uint64), thresholds, seeds in;
    # gcr_many_result records and the packed masks out
    mrp = C.POINTER(ManyResult)
    L.gcr_verify_many.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, vp, vp, C.c_uint32, mrp, vp, dp]
    L.gcr_host_verify_many.argtypes = [C.c_int, vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_int, mrp, vp]
    L.gcr_host_grid_edges.argtypes = [dp, C.c_size_t, C.c_int, dp, C.c_uint64, u32p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]
    L.gcr_host_bk_energy.argtypes = [C.c_size_t, dp, u32p, dp, C.c_size_t, u8p]
    L.gcr_host_labeling.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, dp, C.c_int, dp, C.c_uint64, u8p]
    L.gcr_host_weighted_mode.argtypes = [dp, dp, C.c_size_t, C.c_double]
    L.gcr_host_weighted_mode.restype = C.c_double
    L.gcr_host_homography.argtypes = [C.POINTER(RectModel), dp]
    L.gcr_host_homography.restype = None
    L.gcr_host_residuals.argtypes = [C.c_int, C.c_int, dp, C.c_size_t, C.POINTER(RectModel), C.c_int, dp]
    L.gcr_host_residuals.restype = C.c_int
    return L


lib = _load()

_ctx_lock = threading.Lock()
_contexts: dict[int, int] = {}


def default_device() -> int:
    for var in ("GCR_DEVICE", "LOCAL_RANK"):
        if var in os.environ:
            try:
                return int(os.environ[var])
            except ValueError:
                pass
    return 0


def context(device: int | None = None) -> int:
    """Per-device engine context (created lazily, kept for the process)."""
    dev = default_device() if device is None else int(device)
    with _ctx_lock:
        h = _contexts.get(dev)
        if h is None:
            out = C.c_void_p()
            rc = lib.gcr_create(dev, C.byref(out))
            check(rc)
            h = out.value
            _contexts[dev] = h
        return h


def last_error() -> str:
    msg = lib.gcr_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int) -> int:
    if rc >= 0:
        return rc
    msg = last_error() or f"engine error {rc}"
    if rc == GCR_EINVAL:
        raise ValueError(msg)
    raise RuntimeError(msg)


def default_params() -> Params:
    p = Params()
    lib.gcr_default_params(C.byref(p))
    return p


def exchange_log():
    """The collective events of the calling thread's last summary replay
    (GCR_EXCHANGE_LOG=1; gcr_debug_exchange_log): a list of (kind, chunk,
    flags, arg) tuples -- kind 1 chunk issue (flags: set | ahead << 1, arg:
    slots), 2 re-summary (flags: set | locate << 1, arg: owner + 1 | from_pos
    << 16), 3 chunk collected."""
    n = lib.gcr_debug_exchange_log(None, 0)
    buf = (C.c_uint64 * max(n, 1))()
    lib.gcr_debug_exchange_log(buf, n)
    w = list(buf)[:n]
    return [tuple(w[i:i + 4]) for i in range(0, n, 4)]
