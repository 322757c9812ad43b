"""ctypes binding of the C-ABI in include/lgs_hip.h (liblgs_hip.so).

This is plumbing for tests and bench.py: every compute call goes through the
HIP library.  There is no CPU fallback -- if liblgs_hip.so is missing or no
device is present, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblgs_hip.so")

LGS_OK = 0
LGS_OPT_GUARD_EPS = 1
LGS_OPT_FORCE_DENSE = 2
LGS_OPT_INJECT_INDEX = 3
LGS_OPT_GUARD_CAP = 4
LGS_OPT_PROFILE = 5
LGS_OPT_PROFILE_MASK = 7
LGS_OPT_SPIN_SYNC = 8
LGS_OPT_SUPER_PRUNE = 9
LGS_OPT_LANES_MIN_BATCH = 11
LGS_OPT_RAY_CHUNK_KEYS = 13
LGS_OPT_POISON_WS = 15   # diagnostics only
LGS_OPT_SKIP_MASK = 10   # diagnostics only
LGS_OPT_LINSOLVE_SPLIT = 17
LGS_OPT_HANDOFF_SPIN_US = 18
LGS_OPT_PEER_COPY = 19
LGS_OPT_PRUNE_MIN_SUPER = 21
LGS_OPT_COOP_TILES = 22
LGS_OPT_SORT_BARRIER_US = 23
LGS_OPT_FINE_STAGED = 24
LGS_OPT_SMALL_WINDOW = 25
LGS_OPT_POST_RECORDS = 26
LGS_OPT_FUSED_PLANES = 27
LGS_OPT_PRIORITY_TAIL = 28
LGS_OPT_HV_FULL = 29
LGS_OPT_SPLIT_CHUNKS = 30
LGS_OPT_DEVICE_HITS = 31
LGS_OPT_SEED_WIDE = 32
LGS_OPT_ZERO_TILES = 33
LGS_OPT_DEVICE_TIMING = 34   # correlative chunks' kernels timed on the device (s_memrealtime spans)
LGS_OPT_LEAN_PROJECT = 35    # batched chunks: only superblock bases projected; consumers form their rows
LGS_OPT_PGCG_GRID_NODES = 36  # lgs_pg_cg_solve: node count from which the solve runs over many workgroups
LGS_OPT_FAST_ROWS = 37       # lean batches: certified fast hit-point cells in the superblock pass (0: exact chain)
LGS_OPT_HV_INZERO = 38       # k_super_hv: threads whose inputs the precompute found all +0 load nothing (0: all load)
KERNEL_IDS = ["k_project", "k_coarse", "k_seed", "k_select", "k_fine", "k_replay", "k_cost", "k_precompute",
              "k_linsolve", "k_ray_emit", "k_ray_apply", "k_super", "k_super_planes", "k_bb_score",
              "k_bb_expand", "k_coarse_aux", "k_match_small", "k_gs_score",
              "k_cost_sq", "k_cost_gx"]   # lgs_ctx_kernel_stats order
# kernels with a statistics slot past the list above (not part of the profile / skip masks built from it)
MORE_KERNEL_IDS = ["k_loop_search"]
LGS_OPT_LOOP_SEARCH_MIN_PAIRS = 39  # lgs_loop_search_nearest: hint x position pairs below which the host loop runs (0: always the device)
LGS_OPT_LOOP_SEARCH_GROUP = 40      # tests: walk positions per workgroup group of the search (0: chosen per call)
LGS_OPT_LIST_ORDER = 42             # work-list batches: the list superblock-major, angles ascending (k_keep_ord; 0: k_keep's atomics)
LGS_OPT_LIST_PAIRS = 43             # work-list batches: two blocks per lane, 16-byte gathers (k_coarse_list_p; 0: k_coarse_list_c)
LGS_OPT_SELECT_LIST = 41            # work-list batches: largest K selected from the kept-superblock list (k_select_list; 0: never)


class Pose2D(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("theta", C.c_double)]

    def tuple(self):
        return (self.x, self.y, self.theta)


class ScanHost(C.Structure):
    _fields_ = [
        ("ranges", C.POINTER(C.c_double)),
        ("angles", C.POINTER(C.c_double)),
        ("n", C.c_int),
        ("rel_sensor_pose", Pose2D),
        ("min_range", C.c_double),
        ("max_range", C.c_double),
    ]


class RtcsmParams(C.Structure):
    _fields_ = [
        ("low_resolution", C.c_int),
        ("range_x", C.c_double),
        ("range_y", C.c_double),
        ("range_theta", C.c_double),
        ("scan_range_max", C.c_double),
    ]


class CostGEParams(C.Structure):
    _fields_ = [
        ("usable_range_min", C.c_double),
        ("usable_range_max", C.c_double),
        ("hit_and_missed_dist", C.c_double),
        ("occupancy_threshold", C.c_double),
        ("kernel_size", C.c_int),
        ("scaling_factor", C.c_double),
        ("standard_deviation", C.c_double),
    ]


class RtcsmSummary(C.Structure):
    _fields_ = [
        ("pose_found", C.c_int),
        ("normalized_cost", C.c_double),
        ("initial_pose", Pose2D),
        ("estimated_pose", Pose2D),
        ("covariance", C.c_double * 9),
        ("score_max", C.c_double),
        ("score_threshold", C.c_double),
        ("best_win", C.c_int * 3),
        ("win", C.c_int * 3),
        ("steps", C.c_double * 3),
        ("best_sensor_pose", Pose2D),
        ("coarse_blocks", C.c_int64),
        ("fine_blocks", C.c_int64),
        ("guard_hits", C.c_int),
        ("fixups", C.c_int),
        ("slow_path", C.c_int),
    ]


class BBParams(C.Structure):
    """lgs_bb_params: ScanMatcherBranchBound ctor (nodeHeightMax, rangeX/Y/Theta,
    scanRangeMax) + ScorePixelAccurate (usableRangeMin/Max)."""
    _fields_ = [("node_height_max", C.c_int), ("range_x", C.c_double), ("range_y", C.c_double),
                ("range_theta", C.c_double), ("scan_range_max", C.c_double),
                ("score_usable_range_min", C.c_double), ("score_usable_range_max", C.c_double)]


class GSParams(C.Structure):
    """lgs_gs_params: ScanMatcherGridSearch ctor (rangeX/Y/Theta, stepX/Y/Theta)
    + ScorePixelAccurate (usableRangeMin/Max)."""
    _fields_ = [("range_x", C.c_double), ("range_y", C.c_double), ("range_theta", C.c_double),
                ("step_x", C.c_double), ("step_y", C.c_double), ("step_theta", C.c_double),
                ("score_usable_range_min", C.c_double), ("score_usable_range_max", C.c_double)]


class HCParams(C.Structure):
    """lgs_hc_params: ScanMatcherHillClimbing ctor (linearStep, angularStep,
    maxIterations, maxNumOfRefinements)."""
    _fields_ = [("linear_step", C.c_double), ("angular_step", C.c_double), ("max_iterations", C.c_int),
                ("max_num_of_refinements", C.c_int)]


class HCSummary(C.Structure):
    """lgs_hc_summary: ScanMatchingSummary, then the walk's diagnostics."""
    _fields_ = [("pose_found", C.c_int), ("normalized_cost", C.c_double), ("initial_pose", Pose2D),
                ("estimated_pose", Pose2D), ("covariance", C.c_double * 9), ("best_sensor_pose", Pose2D),
                ("min_cost", C.c_double), ("final_linear_step", C.c_double), ("final_angular_step", C.c_double),
                ("num_iterations", C.c_int), ("num_refinements", C.c_int), ("passes", C.c_int),
                ("cost_evals", C.c_int)]


class CostSQParams(C.Structure):
    """lgs_cost_sq_params: CostSquareError ctor (usableRangeMin, usableRangeMax)."""
    _fields_ = [("usable_range_min", C.c_double), ("usable_range_max", C.c_double)]


LGS_COST_GREEDY_ENDPOINT = 0
LGS_COST_SQUARE_ERROR = 1
LGS_COST_GREEDY_ENDPOINT_EXACT = 2   # the greedy-endpoint cost of `ge`, bit for bit


class CostSpec(C.Structure):
    """lgs_cost_spec: the cost function of a `_cost` entry point (kind selects ge or sq)."""
    _fields_ = [("kind", C.c_int), ("ge", CostGEParams), ("sq", CostSQParams)]


def cost_spec(cost, exact: bool = False) -> "CostSpec":
    """the CostSpec of a CostGEParams or a CostSQParams; exact=True (greedy
    endpoint only) selects the bit-exact kind LGS_COST_GREEDY_ENDPOINT_EXACT"""
    if exact:
        if not isinstance(cost, CostGEParams):
            raise TypeError("exact=True takes a CostGEParams")
        return CostSpec(LGS_COST_GREEDY_ENDPOINT_EXACT, cost, CostSQParams())
    if isinstance(cost, CostSpec):
        return cost
    if isinstance(cost, CostSQParams):
        return CostSpec(LGS_COST_SQUARE_ERROR, CostGEParams(), cost)
    if isinstance(cost, CostGEParams):
        return CostSpec(LGS_COST_GREEDY_ENDPOINT, cost, CostSQParams())
    raise TypeError(f"cost must be CostGEParams, CostSQParams or CostSpec, not {type(cost).__name__}")


def _is_ge(cost) -> bool:
    """a CostGEParams keeps calling the greedy-endpoint entry points"""
    return isinstance(cost, CostGEParams)


class BuilderParams(C.Structure):
    _fields_ = [("usable_range_min", C.c_double), ("usable_range_max", C.c_double),
                ("prob_hit", C.c_double), ("prob_miss", C.c_double)]


class MapGeometry(C.Structure):
    _fields_ = [("resolution", C.c_double), ("patch_size", C.c_int), ("num_patches_x", C.c_int),
                ("num_patches_y", C.c_int), ("num_cells_x", C.c_int), ("num_cells_y", C.c_int),
                ("min_x", C.c_double), ("min_y", C.c_double)]

    def dict(self):
        return dict(w=self.num_cells_x, h=self.num_cells_y, min_x=self.min_x, min_y=self.min_y,
                    npx=self.num_patches_x, npy=self.num_patches_y)

    def res(self):
        return self.resolution


class LinsolveParams(C.Structure):
    """lgs_linsolve_params: ScanMatcherLinearSolver ctor order, then CostSquareError's usable range."""
    _fields_ = [("num_iterations_max", C.c_int), ("convergence_threshold", C.c_double),
                ("usable_range_min", C.c_double), ("usable_range_max", C.c_double),
                ("translation_regularizer", C.c_double), ("rotation_regularizer", C.c_double),
                ("cost_usable_range_min", C.c_double), ("cost_usable_range_max", C.c_double)]


class LinsolveSummary(C.Structure):
    _fields_ = [("pose_found", C.c_int), ("iterations", C.c_int), ("normalized_cost", C.c_double),
                ("initial_pose", Pose2D), ("estimated_pose", Pose2D), ("covariance", C.c_double * 9),
                ("sensor_pose", Pose2D), ("best_sensor_pose", Pose2D), ("cost", C.c_double)]


class IcpParams(C.Structure):
    """lgs_icp_params: the point-to-line ICP matcher."""
    _fields_ = [("num_iterations_max", C.c_int), ("convergence_threshold", C.c_double),
                ("usable_range_min", C.c_double), ("usable_range_max", C.c_double),
                ("translation_regularizer", C.c_double), ("rotation_regularizer", C.c_double),
                ("max_correspondence_dist", C.c_double), ("max_segment_length", C.c_double)]


class IcpSummary(C.Structure):
    _fields_ = [("pose_found", C.c_int), ("iterations", C.c_int), ("num_pairs", C.c_int), ("initial_pairs", C.c_int),
                ("normalized_cost", C.c_double), ("initial_pose", Pose2D), ("estimated_pose", Pose2D),
                ("covariance", C.c_double * 9), ("sensor_pose", Pose2D), ("best_sensor_pose", Pose2D),
                ("cost", C.c_double), ("pair_cost", C.c_double), ("initial_cost", C.c_double),
                ("hessian", C.c_double * 9), ("rhs", C.c_double * 3)]


class LoopSearchHint(C.Structure):
    """lgs_loop_search_hint: one LoopSearchHint of the nearest-node loop searcher."""
    _fields_ = [("latest_node_idx", C.c_int), ("latest_local_map_idx", C.c_int), ("num_maps", C.c_int),
                ("pad_", C.c_int), ("accum_travel_dist", C.c_double)]


class LoopSearchParams(C.Structure):
    """lgs_loop_search_params: LoopSearcherNearest's constructor arguments."""
    _fields_ = [("travel_dist_threshold", C.c_double), ("node_dist_threshold", C.c_double),
                ("num_candidate_nodes", C.c_int), ("pad_", C.c_int)]


class LoopSearchResult(C.Structure):
    _fields_ = [("found", C.c_int), ("local_map_idx", C.c_int), ("local_map_node_idx", C.c_int),
                ("node_idx_min", C.c_int), ("node_idx_max", C.c_int), ("walked", C.c_int), ("dist_sq", C.c_double)]


class LoopSearchMapBest(C.Structure):
    _fields_ = [("node_idx", C.c_int), ("pad_", C.c_int), ("dist_sq", C.c_double)]


class LoopQuery(C.Structure):
    _fields_ = [("map", C.c_void_p), ("coarse", C.c_void_p), ("local_map_node_pose", Pose2D),
                ("local_map_node_index", C.c_int), ("first_candidate", C.c_int), ("num_candidates", C.c_int)]


class LoopCandidate(C.Structure):
    _fields_ = [("scan", C.c_void_p), ("node_pose", Pose2D), ("node_index", C.c_int), ("pad", C.c_int)]


class LoopResult(C.Structure):
    _fields_ = [("found", C.c_int), ("start_node_index", C.c_int), ("end_node_index", C.c_int), ("pad", C.c_int),
                ("relative_pose", Pose2D), ("start_node_pose", Pose2D), ("estimated_pose", Pose2D),
                ("covariance", C.c_double * 9), ("score", C.c_double), ("normalized_cost", C.c_double)]


LOOP_RESULT_DOUBLES = 22   # sizeof(lgs_loop_result) / 8


class LoopRefineGate(C.Structure):
    """lgs_loop_refine_gate: what an ICP refinement of a loop record must meet."""
    _fields_ = [("min_pairs", C.c_int), ("max_normalized_cost", C.c_double), ("max_translation", C.c_double),
                ("max_rotation", C.c_double)]


class IcpWindow(C.Structure):
    """lgs_icp_window: the lattice of start poses of the ICP loop detector:
    2 * half + 1 poses per axis around a centre, theta outermost and x innermost."""
    _fields_ = [("half_x", C.c_int), ("half_y", C.c_int), ("half_theta", C.c_int), ("step_xy", C.c_double),
                ("step_theta", C.c_double)]

    @property
    def shape(self):
        """(nt, ny, nx)"""
        return 2 * self.half_theta + 1, 2 * self.half_y + 1, 2 * self.half_x + 1

    def pose(self, centre, p: int):
        """the robot pose of lattice index p around `centre` (the centre index gives the centre itself)"""
        nt, ny, nx = self.shape
        ix, iy, it = p % nx, (p // nx) % ny, p // (nx * ny)
        f = lambda c, i, h, step: float(c) if i == h else float(c) + float(i - h) * step
        return (f(centre[0], ix, self.half_x, self.step_xy), f(centre[1], iy, self.half_y, self.step_xy),
                f(centre[2], it, self.half_theta, self.step_theta))


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("algo_bytes", C.c_double), ("dispatch_ms", C.c_double)]


# (name, restype, argtypes) for every symbol of include/lgs_hip.h
_P = C.c_void_p
class PgEdge(C.Structure):
    """lgs_pg_edge (the layout of lgs_io.h's lgs_pose_graph_edge)"""
    _fields_ = [("start_node_index", C.c_int), ("end_node_index", C.c_int), ("relative_pose", Pose2D),
                ("information", C.c_double * 9)]


class PgLmParams(C.Structure):
    _fields_ = [("num_iterations_max", C.c_int), ("error_tolerance", C.c_double), ("loss_kind", C.c_int),
                ("loss_scale", C.c_double)]


def pg_edges(edges):
    """edges: [(start, end, (x, y, theta), info 3x3)] -> a PgEdge array"""
    arr = (PgEdge * max(1, len(edges)))()
    for k, (s, e, z, info) in enumerate(edges):
        arr[k].start_node_index, arr[k].end_node_index = s, e
        arr[k].relative_pose = Pose2D(*z)
        arr[k].information[:] = [float(v) for v in np.asarray(info, dtype=np.float64).reshape(9)]
    return arr


_PROTOS = [
    ("lgs_abi_version", C.c_int, []),
    ("lgs_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("lgs_ctx_destroy", None, [_P]),
    ("lgs_ctx_last_error", C.c_char_p, [_P]),
    ("lgs_ctx_synchronize", C.c_int, [_P]),
    ("lgs_ctx_stream", _P, [_P]),
    ("lgs_ctx_set_option", C.c_int, [_P, C.c_int, C.c_double]),
    ("lgs_ctx_kernel_stats", C.c_int, [_P, C.POINTER(KernelStat), C.c_int]),
    ("lgs_ctx_reset_stats", C.c_int, [_P]),
    ("lgs_ctx_match_counters", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("lgs_grid_create", C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(_P)]),
    ("lgs_grid_wrap", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(_P)]),
    ("lgs_grid_destroy", None, [_P]),
    ("lgs_grid_upload", C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    ("lgs_grid_upload_patches", C.c_int, [_P, _P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("lgs_grid_download", C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    ("lgs_grid_fill", C.c_int, [_P, _P, C.c_double]),
    ("lgs_grid_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("lgs_grid_device_ptr", _P, [_P]),
    ("lgs_grid_precompute_max", C.c_int, [_P, _P, C.c_int, _P]),
    ("lgs_scan_create", C.c_int, [_P, C.POINTER(ScanHost), C.POINTER(_P)]),
    ("lgs_scan_destroy", None, [_P]),
    ("lgs_rtcsm_optimize_pose", C.c_int, [_P, _P, _P, C.POINTER(RtcsmParams), C.POINTER(CostGEParams), _P,
                                          Pose2D, C.c_double, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_query", C.c_int, [_P, _P, C.POINTER(RtcsmParams), C.POINTER(CostGEParams), _P,
                                                Pose2D, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_query_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(RtcsmParams),
                                                      C.POINTER(CostGEParams), C.POINTER(_P), C.POINTER(Pose2D),
                                                      C.c_int, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_batch", C.c_int, [_P, _P, _P, C.POINTER(RtcsmParams), C.POINTER(CostGEParams),
                                                C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.c_double,
                                                C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_dense_scores", C.c_int, [_P, _P, _P, C.POINTER(RtcsmParams), _P, Pose2D,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("lgs_cost_greedy_endpoint", C.c_int, [_P, _P, C.POINTER(CostGEParams), _P, Pose2D,
                                           C.POINTER(C.c_double)]),
    ("lgs_scan_get", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("lgs_scan_interpolate", C.c_int, [_P, _P, C.c_double, C.c_double, C.POINTER(_P)]),
    ("lgs_map_create", C.c_int, [_P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                 C.POINTER(_P)]),
    ("lgs_map_destroy", None, [_P]),
    ("lgs_map_get_geometry", C.c_int, [_P, C.POINTER(MapGeometry)]),
    ("lgs_map_grid", C.c_int, [_P, C.POINTER(_P)]),
    ("lgs_map_update_scan", C.c_int, [_P, _P, _P, Pose2D, C.POINTER(BuilderParams)]),
    ("lgs_map_construct_from_scans", C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(Pose2D), C.c_int,
                                               C.POINTER(BuilderParams)]),
    ("lgs_map_append_scan", C.c_int, [_P, _P, _P, C.POINTER(_P), C.POINTER(Pose2D), C.c_int,
                                      C.POINTER(BuilderParams)]),
    ("lgs_maps_construct_from_scans", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                C.c_int, C.POINTER(_P), C.POINTER(Pose2D), C.c_int,
                                                C.POINTER(BuilderParams)]),
    ("lgs_map_construct_global", C.c_int, [_P, C.c_double, C.c_int, C.POINTER(_P), C.POINTER(Pose2D), C.c_int,
                                           C.POINTER(BuilderParams), C.POINTER(_P)]),
    ("lgs_map_render_gray", C.c_int, [_P, _P, C.POINTER(C.c_uint8)]),
    ("lgs_map_render_gray_region", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_uint8)]),
    ("lgs_map_download_patches", C.c_int, [_P, _P, C.POINTER(C.c_uint8)]),
    ("lgs_map_actual_size", C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("lgs_map_download", C.c_int, [_P, _P, C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32)]),
    ("lgs_grid_precompute_pyramid", C.c_int, [_P, _P, C.c_int, C.POINTER(_P)]),
    ("lgs_bb_optimize_pose_batch", C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(BBParams), C.POINTER(CostGEParams),
                                             C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.c_double,
                                             C.POINTER(RtcsmSummary)]),
    ("lgs_bb_optimize_pose_query", C.c_int, [_P, _P, C.POINTER(BBParams), C.POINTER(CostGEParams), _P, Pose2D,
                                             C.POINTER(RtcsmSummary)]),
    ("lgs_loop_detect_bb", C.c_int, [_P, C.POINTER(BBParams), C.POINTER(CostGEParams), C.c_double,
                                     C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                     C.POINTER(LoopResult)]),
    ("lgs_gs_steps", C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_double), C.c_int]),
    ("lgs_gs_optimize_pose_batch", C.c_int, [_P, _P, C.POINTER(GSParams), C.POINTER(CostGEParams), C.POINTER(_P),
                                             C.POINTER(Pose2D), C.c_int, C.c_double, C.POINTER(RtcsmSummary)]),
    ("lgs_gs_optimize_pose_query", C.c_int, [_P, _P, C.POINTER(GSParams), C.POINTER(CostGEParams), _P, Pose2D,
                                             C.POINTER(RtcsmSummary)]),
    ("lgs_gs_dense_scores", C.c_int, [_P, _P, C.POINTER(GSParams), _P, Pose2D, C.POINTER(C.c_double),
                                      C.c_longlong]),
    ("lgs_loop_detect_gs", C.c_int, [_P, C.POINTER(GSParams), C.POINTER(CostGEParams), C.c_double,
                                     C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                     C.POINTER(LoopResult)]),
    ("lgs_hc_term_table", C.c_int, [C.POINTER(CostGEParams), C.c_double, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.c_int]),
    ("lgs_hc_optimize_pose_query", C.c_int, [_P, _P, C.POINTER(HCParams), C.POINTER(CostGEParams), _P, Pose2D,
                                             C.POINTER(HCSummary)]),
    ("lgs_hc_optimize_pose_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(HCParams), C.POINTER(CostGEParams),
                                             C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.POINTER(HCSummary)]),
    ("lgs_hc_trace", C.c_int, [_P, _P, C.POINTER(HCParams), C.POINTER(CostGEParams), _P, Pose2D,
                               C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]),
    ("lgs_cost_ge_exact", C.c_int, [_P, _P, C.POINTER(CostGEParams), _P, C.POINTER(Pose2D), C.c_int,
                                    C.POINTER(C.c_double)]),
    ("lgs_loop_detect_rtcsm", C.c_int, [_P, C.POINTER(RtcsmParams), C.POINTER(CostGEParams), C.c_double,
                                        C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                        C.POINTER(LoopResult)]),
    ("lgs_loop_detect_rtcsm_multi", C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(RtcsmParams),
                                              C.POINTER(CostGEParams), C.c_double, C.POINTER(LoopQuery), C.c_int,
                                              C.POINTER(LoopCandidate), C.c_int, C.POINTER(LoopResult)]),
    ("lgs_cost_spec_size", C.c_size_t, []),
    ("lgs_rtcsm_optimize_pose_cost", C.c_int, [_P, _P, _P, C.POINTER(RtcsmParams), C.POINTER(CostSpec), _P,
                                               Pose2D, C.c_double, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_query_cost", C.c_int, [_P, _P, C.POINTER(RtcsmParams), C.POINTER(CostSpec), _P,
                                                     Pose2D, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_query_batch_cost", C.c_int, [_P, C.POINTER(_P), C.POINTER(RtcsmParams),
                                                           C.POINTER(CostSpec), C.POINTER(_P), C.POINTER(Pose2D),
                                                           C.c_int, C.POINTER(RtcsmSummary)]),
    ("lgs_rtcsm_optimize_pose_batch_cost", C.c_int, [_P, _P, _P, C.POINTER(RtcsmParams), C.POINTER(CostSpec),
                                                     C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.c_double,
                                                     C.POINTER(RtcsmSummary)]),
    ("lgs_bb_optimize_pose_batch_cost", C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(BBParams), C.POINTER(CostSpec),
                                                  C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.c_double,
                                                  C.POINTER(RtcsmSummary)]),
    ("lgs_bb_optimize_pose_query_cost", C.c_int, [_P, _P, C.POINTER(BBParams), C.POINTER(CostSpec), _P, Pose2D,
                                                  C.POINTER(RtcsmSummary)]),
    ("lgs_gs_optimize_pose_batch_cost", C.c_int, [_P, _P, C.POINTER(GSParams), C.POINTER(CostSpec), C.POINTER(_P),
                                                  C.POINTER(Pose2D), C.c_int, C.c_double,
                                                  C.POINTER(RtcsmSummary)]),
    ("lgs_gs_optimize_pose_query_cost", C.c_int, [_P, _P, C.POINTER(GSParams), C.POINTER(CostSpec), _P, Pose2D,
                                                  C.POINTER(RtcsmSummary)]),
    ("lgs_loop_detect_rtcsm_cost", C.c_int, [_P, C.POINTER(RtcsmParams), C.POINTER(CostSpec), C.c_double,
                                             C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                             C.POINTER(LoopResult)]),
    ("lgs_loop_detect_rtcsm_multi_cost", C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(RtcsmParams),
                                                   C.POINTER(CostSpec), C.c_double, C.POINTER(LoopQuery), C.c_int,
                                                   C.POINTER(LoopCandidate), C.c_int, C.POINTER(LoopResult)]),
    ("lgs_loop_detect_bb_cost", C.c_int, [_P, C.POINTER(BBParams), C.POINTER(CostSpec), C.c_double,
                                          C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                          C.POINTER(LoopResult)]),
    ("lgs_loop_detect_gs_cost", C.c_int, [_P, C.POINTER(GSParams), C.POINTER(CostSpec), C.c_double,
                                          C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                          C.POINTER(LoopResult)]),
    ("lgs_loop_shard_bounds", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("lgs_loop_records_allgather", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(LoopResult),
                                             C.POINTER(LoopResult)]),
    ("lgs_rccl_unique_id", C.c_int, [C.POINTER(C.c_ubyte)]),
    ("lgs_rccl_comm_init", C.c_int, [_P, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(_P)]),
    ("lgs_rccl_comm_destroy", C.c_int, [_P]),
    ("lgs_linsolve_optimize_pose", C.c_int, [_P, _P, C.POINTER(LinsolveParams), _P, Pose2D,
                                             C.POINTER(LinsolveSummary), C.POINTER(C.c_double)]),
    ("lgs_linsolve_optimize_pose_batch", C.c_int, [_P, _P, C.POINTER(LinsolveParams), C.POINTER(_P),
                                                   C.POINTER(Pose2D), C.c_int, C.POINTER(LinsolveSummary)]),
    ("lgs_cost_square_error", C.c_int, [_P, _P, C.c_double, C.c_double, _P, Pose2D, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    ("lgs_cost_square_error_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(CostSQParams), C.POINTER(_P),
                                              C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double)]),
    ("lgs_summaries_apply_cost_sq", C.c_int, [_P, C.POINTER(_P), C.POINTER(CostSQParams), C.POINTER(_P),
                                              C.POINTER(RtcsmSummary), C.c_int]),
    ("lgs_cost_ge_exact_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(CostGEParams), C.POINTER(_P),
                                          C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
    ("lgs_summaries_apply_cost_ge_exact", C.c_int, [_P, C.POINTER(_P), C.POINTER(CostGEParams), C.POINTER(_P),
                                                    C.POINTER(RtcsmSummary), C.c_int]),
    ("lgs_hc_sq_optimize_pose_query", C.c_int, [_P, _P, C.POINTER(HCParams), C.POINTER(CostSQParams), _P, Pose2D,
                                                C.POINTER(HCSummary)]),
    ("lgs_hc_sq_optimize_pose_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(HCParams), C.POINTER(CostSQParams),
                                                C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.POINTER(HCSummary)]),
    ("lgs_hc_sq_trace", C.c_int, [_P, _P, C.POINTER(HCParams), C.POINTER(CostSQParams), _P, Pose2D,
                                  C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]),
    ("lgs_pg_cg_solve", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                  C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("lgs_pg_cg_stats", C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                  C.POINTER(C.c_longlong)]),
    ("lgs_pg_lm_optimize", C.c_int, [_P, C.POINTER(PgLmParams), C.POINTER(C.c_double), C.POINTER(Pose2D), C.c_int, _P,
                                     C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    ("lgs_pg_lm_linearize", C.c_int, [_P, C.c_int, C.c_double, C.c_double, C.POINTER(Pose2D), C.c_int, _P, C.c_int,
                                      C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("lgs_pg_lm_stats", C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                  C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("lgs_icp_params_size", C.c_size_t, []),
    ("lgs_icp_summary_size", C.c_size_t, []),
    ("lgs_icp_optimize_pose", C.c_int, [_P, _P, Pose2D, _P, Pose2D, C.POINTER(IcpParams), C.POINTER(IcpSummary),
                                        C.POINTER(C.c_double)]),
    ("lgs_icp_optimize_pose_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(Pose2D), C.POINTER(_P), C.POINTER(Pose2D),
                                              C.c_int, C.POINTER(IcpParams), C.POINTER(IcpSummary)]),
    ("lgs_icp_pairs", C.c_int, [_P, _P, Pose2D, _P, Pose2D, C.POINTER(IcpParams), C.POINTER(C.c_int),
                                C.POINTER(C.c_double)]),
    ("lgs_icp_ref_create", C.c_int, [_P, C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.POINTER(IcpParams),
                                     C.POINTER(_P)]),
    ("lgs_icp_ref_destroy", None, [_P]),
    ("lgs_icp_ref_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("lgs_icp_ref_optimize_pose", C.c_int, [_P, _P, _P, Pose2D, C.POINTER(IcpParams), C.POINTER(IcpSummary),
                                            C.POINTER(C.c_double)]),
    ("lgs_icp_ref_optimize_pose_batch", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(Pose2D), C.c_int,
                                                  C.POINTER(IcpParams), C.POINTER(IcpSummary)]),
    ("lgs_icp_ref_pairs", C.c_int, [_P, _P, _P, Pose2D, C.POINTER(IcpParams), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_double)]),
    ("lgs_icp_ref_set_create", C.c_int, [_P, C.POINTER(_P), C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.c_int, C.POINTER(IcpParams), C.POINTER(_P)]),
    ("lgs_icp_ref_set_destroy", None, [_P]),
    ("lgs_icp_ref_set_size", C.c_int, [_P]),
    ("lgs_icp_ref_set_ref", _P, [_P, C.c_int]),
    ("lgs_icp_ref_set_stats", C.c_int, [_P] + [C.POINTER(C.c_longlong)] * 7),
    ("lgs_icp_ref_set_last_build_ms", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("lgs_loop_refine_icp", C.c_int, [_P, C.POINTER(_P), C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                      C.POINTER(IcpParams), C.POINTER(LoopRefineGate), C.POINTER(LoopResult),
                                      C.POINTER(C.c_int), C.POINTER(IcpSummary)]),
    ("lgs_icp_window_size", C.c_size_t, []),
    ("lgs_icp_ref_window_scores", C.c_int, [_P, _P, _P, Pose2D, C.POINTER(IcpWindow), C.POINTER(IcpParams),
                                            C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("lgs_loop_detect_icp", C.c_int, [_P, C.POINTER(_P), C.POINTER(LoopQuery), C.c_int, C.POINTER(LoopCandidate), C.c_int,
                                      C.POINTER(IcpParams), C.POINTER(IcpWindow), C.POINTER(LoopRefineGate),
                                      C.POINTER(LoopResult), C.POINTER(C.c_int), C.POINTER(IcpSummary)]),
    ("lgs_icp_window_stats", C.c_int, [_P] + [C.POINTER(C.c_longlong)] * 4),
    ("lgs_loop_graph_create", C.c_int, [_P, C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                        C.POINTER(_P)]),
    ("lgs_loop_graph_destroy", None, [_P]),
    ("lgs_loop_graph_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_double)]),
    ("lgs_loop_graph_travel", C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
    ("lgs_loop_search_nearest", C.c_int, [_P, C.POINTER(LoopSearchParams), _P, C.c_int, _P, _P]),
    ("lgs_loop_search_nearest_host", C.c_int, [C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.c_int, C.POINTER(LoopSearchParams), _P, C.c_int, _P, _P]),
    ("lgs_pg_accum_travel_dist", C.c_int, [C.POINTER(Pose2D), C.c_int, C.POINTER(C.c_double)]),
    ("lgs_loop_search_stats", C.c_int, [_P, C.POINTER(C.c_longlong)]),
    ("lgs_debug_keysort", C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_int]),
    ("lgs_debug_map_rebuilds", C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("lgs_debug_copy_counters", C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("lgs_debug_offset_checks", C.c_int, [_P, C.c_int, C.POINTER(C.c_ulonglong)]),
    ("lgs_debug_item_buffer", C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("lgs_debug_libm", C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
]

SYMBOLS = [p[0] for p in _PROTOS]

# the loop searcher's records as numpy rows (the layouts of the structs above)
LOOP_HINT_DTYPE = np.dtype([("latest_node_idx", "<i4"), ("latest_local_map_idx", "<i4"), ("num_maps", "<i4"),
                            ("pad_", "<i4"), ("accum_travel_dist", "<f8")])
LOOP_RESULT_DTYPE = np.dtype([("found", "<i4"), ("local_map_idx", "<i4"), ("local_map_node_idx", "<i4"),
                              ("node_idx_min", "<i4"), ("node_idx_max", "<i4"), ("walked", "<i4"), ("dist_sq", "<f8")])
LOOP_MAP_BEST_DTYPE = np.dtype([("node_idx", "<i4"), ("pad_", "<i4"), ("dist_sq", "<f8")])


def loop_hints(latest_node_idx, latest_local_map_idx, num_maps, accum_travel_dist) -> np.ndarray:
    """lgs_loop_search_hint rows from four equally long sequences (scalars broadcast)"""
    a = np.broadcast_arrays(np.asarray(latest_node_idx), np.asarray(latest_local_map_idx), np.asarray(num_maps),
                            np.asarray(accum_travel_dist, dtype=np.float64))
    h = np.zeros(a[0].size, dtype=LOOP_HINT_DTYPE)
    h["latest_node_idx"], h["latest_local_map_idx"], h["num_maps"] = a[0].ravel(), a[1].ravel(), a[2].ravel()
    h["accum_travel_dist"] = a[3].ravel()
    return h


def _loop_snapshot(poses, idx_min, idx_max):
    p = np.ascontiguousarray(poses, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ValueError("poses: n x 2 (x, y) or n x 3 (x, y, theta)")
    if p.shape[1] == 2:
        p = np.ascontiguousarray(np.hstack([p, np.zeros((len(p), 1))]))
    lo, hi = np.ascontiguousarray(idx_min, dtype=np.int32), np.ascontiguousarray(idx_max, dtype=np.int32)
    if lo.shape != hi.shape or lo.ndim != 1:
        raise ValueError("idx_min, idx_max: two equally long index lists")
    return p, lo, hi


def _loop_hint_rows(hints) -> np.ndarray:
    h = np.ascontiguousarray(hints)
    if h.dtype != LOOP_HINT_DTYPE:
        raise ValueError("hints: rows of LOOP_HINT_DTYPE (abi.loop_hints)")
    return h


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def loop_search_host(poses, idx_min, idx_max, params: "LoopSearchParams", hints, per_map: bool = False):
    """lgs_loop_search_nearest_host: the reference's loop per hint, no device.
    Returns the records (LOOP_RESULT_DTYPE rows), with per_map also the q x m
    table (LOOP_MAP_BEST_DTYPE); raises LgsError on bad arguments."""
    lib = load()
    p, lo, hi = _loop_snapshot(poses, idx_min, idx_max)
    h = _loop_hint_rows(hints)
    q, m = len(h), len(lo)
    res = np.zeros(q, dtype=LOOP_RESULT_DTYPE)
    tab = np.zeros((q, m), dtype=LOOP_MAP_BEST_DTYPE) if per_map else None
    rc = lib.lgs_loop_search_nearest_host(p.ctypes.data_as(C.POINTER(Pose2D)), len(p), _iptr(lo), _iptr(hi), m,
                                          C.byref(params), h.ctypes.data, q, res.ctypes.data,
                                          tab.ctypes.data if per_map else None)
    if rc != LGS_OK:
        err = LgsError(f"loop_search_host: status {rc}")
        err.status = rc
        raise err
    return (res, tab) if per_map else res


def accum_travel_dist(poses) -> float:
    """lgs_pg_accum_travel_dist: GridMapBuilder::UpdateAccumTravelDist over all nodes (host)"""
    lib = load()
    p, _, _ = _loop_snapshot(poses, [], [])
    out = C.c_double()
    rc = lib.lgs_pg_accum_travel_dist(p.ctypes.data_as(C.POINTER(Pose2D)), len(p), C.byref(out))
    if rc != LGS_OK:
        err = LgsError(f"accum_travel_dist: status {rc}")
        err.status = rc
        raise err
    return out.value

_lib: Optional[C.CDLL] = None


def load(path: str = None) -> C.CDLL:
    """Load liblgs_hip.so and bind prototypes.  Raises if missing (no fallback).
    LGS_LIB overrides the path (A/B builds of the same library, tools/ab_build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("LGS_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"HIP extension missing: {path} (run __graft_entry__.build())")
    lib = C.CDLL(path)
    for name, res, args in _PROTOS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def gs_steps(rng: float, step: float) -> np.ndarray:
    """lgs_gs_steps: the window values of one grid-search axis (host only, no
    device); raises LgsError on bad arguments."""
    lib = load()
    n = lib.lgs_gs_steps(float(rng), float(step), None, 0)
    if n < 0:
        raise LgsError(f"gs_steps: status {-n}")
    out = np.zeros(n)
    lib.lgs_gs_steps(float(rng), float(step), dptr(out) if n else None, n)
    return out


def hc_term_table(cost: "CostGEParams", res: float):
    """lgs_hc_term_table: (sq, term), the squared distances of the kernel
    offsets and of the start offset and exp(-0.5 * sq / variance) of each
    (host only, no device); raises LgsError on bad arguments."""
    lib = load()
    n = lib.lgs_hc_term_table(C.byref(cost), float(res), None, None, 0)
    if n < 0:
        raise LgsError(f"hc_term_table: status {-n}")
    sq, term = np.zeros(n), np.zeros(n)
    lib.lgs_hc_term_table(C.byref(cost), float(res), dptr(sq), dptr(term), n)
    return sq, term


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


class LgsError(RuntimeError):
    pass


class Context:
    """One lgs_ctx: a device + HIP stream + scratch arena."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _P()
        rc = self.lib.lgs_ctx_create(device, C.byref(h))
        if rc != LGS_OK:
            raise LgsError(f"lgs_ctx_create(device={device}) failed with status {rc}")
        self.h = h
        # A/B runs: LGS_CTX_OPTIONS="ID=VALUE,ID=VALUE" applied to every new context
        for kv in filter(None, os.environ.get("LGS_CTX_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            self.set_option(int(k), float(v))

    def check(self, rc: int, what: str):
        if rc != LGS_OK:
            msg = self.lib.lgs_ctx_last_error(self.h)
            err = LgsError(f"{what}: status {rc}: {msg.decode() if msg else ''}")
            err.status = rc   # the LGS_ERR_* code
            raise err

    def set_option(self, opt: int, value: float):
        self.check(self.lib.lgs_ctx_set_option(self.h, opt, float(value)), "set_option")

    def kernel_stats(self) -> dict:
        """{name: dict(launches, total_ms, algo_bytes)} since the last reset."""
        cap = len(KERNEL_IDS) + len(MORE_KERNEL_IDS)
        buf = (KernelStat * cap)()
        n = self.lib.lgs_ctx_kernel_stats(self.h, buf, cap)
        if n < 0:
            self.check(-n, "kernel_stats")
        return {buf[i].name.decode(): dict(launches=buf[i].launches, total_ms=buf[i].total_ms,
                                           algo_bytes=buf[i].algo_bytes, dispatch_ms=buf[i].dispatch_ms)
                for i in range(n)}

    def reset_stats(self):
        self.check(self.lib.lgs_ctx_reset_stats(self.h), "reset_stats")

    def match_counters(self) -> dict:
        """matches / coarse blocks scored / dense coarse blocks / pruned matches
        since the last reset_stats (lgs_ctx_match_counters)"""
        buf = (C.c_int64 * 4)()
        self.check(self.lib.lgs_ctx_match_counters(self.h, buf), "match_counters")
        return dict(matches=buf[0], coarse_blocks=buf[1], coarse_blocks_dense=buf[2], pruned=buf[3])

    def synchronize(self):
        self.check(self.lib.lgs_ctx_synchronize(self.h), "synchronize")

    def close(self):
        if getattr(self, "h", None):
            self.lib.lgs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- grids ----
    def grid(self, w: int, h: int, min_x: float, min_y: float, res: float) -> "Grid":
        g = _P()
        self.check(self.lib.lgs_grid_create(self.h, w, h, min_x, min_y, res, C.byref(g)), "grid_create")
        return Grid(self, g, w, h, min_x, min_y, res)

    def grid_from_array(self, cells: np.ndarray, min_x: float, min_y: float, res: float) -> "Grid":
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        h, w = cells.shape
        g = self.grid(w, h, min_x, min_y, res)
        g.upload(cells)
        return g

    def grid_from_patches(self, patches, npx: int, npy: int, patch_size: int, min_x: float, min_y: float,
                          res: float, cell_bytes: int = 16, value_offset: int = 8,
                          into: Optional["Grid"] = None) -> "Grid":
        """lgs_grid_upload_patches: `patches` is a row-major list (py * npx + px)
        of host arrays holding patch_size^2 cells of cell_bytes bytes each (the
        fp64 value at value_offset), or None for an unallocated patch."""
        g = into or self.grid(npx * patch_size, npy * patch_size, min_x, min_y, res)
        keep = [None if p is None else np.ascontiguousarray(p) for p in patches]
        for p in keep:
            if p is not None and p.nbytes != patch_size * patch_size * cell_bytes:
                raise ValueError("patch array size does not match patch_size^2 * cell_bytes")
        table = (_P * max(1, len(keep)))(*[None if p is None else p.ctypes.data for p in keep])
        self.check(self.lib.lgs_grid_upload_patches(self.h, g.h, table, npx, npy, patch_size, cell_bytes,
                                                    value_offset), "grid_upload_patches")
        return g

    def wrap_device(self, ptr: int, w: int, h: int, min_x: float, min_y: float, res: float) -> "Grid":
        g = _P()
        self.check(self.lib.lgs_grid_wrap(self.h, _P(ptr), w, h, min_x, min_y, res, C.byref(g)), "grid_wrap")
        return Grid(self, g, w, h, min_x, min_y, res, owned=False)

    def precompute_max(self, src: "Grid", win: int, out: Optional["Grid"] = None) -> "Grid":
        if out is None:
            out = self.grid(src.w, src.hgt, src.min_x, src.min_y, src.res)
        self.check(self.lib.lgs_grid_precompute_max(self.h, src.h, int(win), out.h), "precompute_max")
        return out

    # ---- scans ----
    def scan(self, ranges, angles, rel_pose=(0.0, 0.0, 0.0), min_range=0.0, max_range=30.0) -> "Scan":
        r = np.ascontiguousarray(ranges, dtype=np.float64)
        a = np.ascontiguousarray(angles, dtype=np.float64)
        hs = ScanHost(dptr(r), dptr(a), len(r), Pose2D(*rel_pose), min_range, max_range)
        s = _P()
        self.check(self.lib.lgs_scan_create(self.h, C.byref(hs), C.byref(s)), "scan_create")
        return Scan(self, s, r, a, rel_pose, min_range, max_range)

    def interpolate(self, scan: "Scan", dist_scans: float = 0.05, dist_threshold_empty: float = 0.25) -> "Scan":
        """ScanInterpolator::Interpolate: a new device scan (launcher defaults 0.05 / 0.25)."""
        s = _P()
        self.check(self.lib.lgs_scan_interpolate(self.h, scan.h, dist_scans, dist_threshold_empty, C.byref(s)),
                   "scan_interpolate")
        n = C.c_int()
        self.check(self.lib.lgs_scan_get(s, C.byref(n), None, None), "scan_get")
        r, a = np.zeros(n.value), np.zeros(n.value)
        self.check(self.lib.lgs_scan_get(s, C.byref(n), dptr(r), dptr(a)), "scan_get")
        return Scan(self, s, r, a, scan.rel_pose, scan.min_range, scan.max_range)

    # ---- matcher ----
    def _call_cost(self, name: str, args: list, i: int):
        """lgs_<name> with args[i], a CostGEParams, passed by reference; any
        other cost goes to lgs_<name>_cost as its CostSpec.  Raises unless LGS_OK."""
        cost = args[i]
        if not _is_ge(cost):
            name, cost = name + "_cost", cost_spec(cost)
        args[i] = C.byref(cost)
        self.check(getattr(self.lib, "lgs_" + name)(*args), name)

    def optimize_pose(self, grid, coarse, params: RtcsmParams, cost: CostGEParams, scan, init,
                      thr: float) -> RtcsmSummary:
        """cost: a CostGEParams (the greedy-endpoint entry point) or a CostSQParams / CostSpec (its `_cost` twin);
        the same holds for every matcher and loop-detector method below"""
        out = RtcsmSummary()
        self._call_cost("rtcsm_optimize_pose", [self.h, grid.h, coarse.h, C.byref(params), cost, scan.h,
                                                Pose2D(*init), float(thr), C.byref(out)], 4)
        return out

    def optimize_pose_query(self, grid, params: RtcsmParams, cost: CostGEParams, scan, init) -> RtcsmSummary:
        out = RtcsmSummary()
        self._call_cost("rtcsm_optimize_pose_query", [self.h, grid.h, C.byref(params), cost, scan.h, Pose2D(*init),
                                                      C.byref(out)], 3)
        return out

    def optimize_pose_query_batch(self, grids, params: RtcsmParams, cost: CostGEParams, scans, inits):
        """n independent OptimizePose(query) calls as one batched pipeline;
        grids: one map per query (or a single map for all)."""
        n = len(scans)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        garr = (_P * n)(*[g.h for g in grids])
        sarr = (_P * n)(*[s.h for s in scans])
        poses = (Pose2D * n)(*[Pose2D(*p) for p in inits])
        out = (RtcsmSummary * n)()
        self._call_cost("rtcsm_optimize_pose_query_batch", [self.h, garr, C.byref(params), cost, sarr, poses, n, out], 3)
        return list(out)

    def optimize_pose_batch(self, grid, coarse, params, cost, scans: Sequence["Scan"], inits, thr: float):
        n = len(scans)
        arr = (_P * n)(*[s.h for s in scans])
        poses = (Pose2D * n)(*[Pose2D(*p) for p in inits])
        out = (RtcsmSummary * n)()
        self._call_cost("rtcsm_optimize_pose_batch", [self.h, grid.h, coarse.h, C.byref(params), cost, arr, poses, n,
                                                      float(thr), out], 4)
        return list(out)

    def dense_scores(self, grid, coarse, params, scan, init):
        dims = (C.c_int * 7)()
        self.check(self.lib.lgs_rtcsm_dense_scores(self.h, grid.h, coarse.h, C.byref(params), scan.h,
                                                   Pose2D(*init), None, None, dims), "dense_scores(dims)")
        wx, wy, wt, ncx, ncy, nfx, nfy = list(dims)
        T = 2 * wt + 1
        cs = np.zeros((T, ncx, ncy))
        fs = np.zeros((T, nfx, nfy))
        self.check(self.lib.lgs_rtcsm_dense_scores(self.h, grid.h, coarse.h, C.byref(params), scan.h,
                                                   Pose2D(*init), dptr(cs), dptr(fs), dims), "dense_scores")
        return list(dims), cs, fs

    # ---- loop-closure batch ----
    @staticmethod
    def _loop_arrays(queries, candidates, coarse: bool):
        """the (LoopQuery, LoopCandidate, LoopResult) arrays of a loop batch;
        coarse: pass a query's coarse grid on (else the detector ignores it)"""
        qs = (LoopQuery * max(1, len(queries)))()
        for i, (m, c, pose, idx, first, cnt) in enumerate(queries):
            qs[i] = LoopQuery(m.h, c.h if coarse and c is not None else None, Pose2D(*pose), idx, first, cnt)
        cs = (LoopCandidate * max(1, len(candidates)))()
        for i, (s, pose, idx) in enumerate(candidates):
            cs[i] = LoopCandidate(s.h, Pose2D(*pose), idx, 0)
        return qs, cs, (LoopResult * max(1, len(candidates)))()

    def loop_detect(self, params: RtcsmParams, cost: CostGEParams, thr: float, queries, candidates,
                    shards: Sequence["Context"] = ()):
        """queries: [(map Grid, coarse Grid|None, node_pose, node_index, first, count)];
        candidates: [(Scan, node_pose, node_index)] -> ctypes LoopResult array (one per candidate).
        shards: further contexts (GPUs) to split the candidates over
        (lgs_loop_detect_rtcsm_multi; this context is shard 0)."""
        qs, cs, out = self._loop_arrays(queries, candidates, True)
        tail = [C.byref(params), cost, float(thr), qs, len(queries), cs, len(candidates), out]
        if shards:
            hs = (_P * (1 + len(shards)))(self.h, *[c.h for c in shards])
            self._call_cost("loop_detect_rtcsm_multi", [hs, len(hs)] + tail, 3)
        else:
            self._call_cost("loop_detect_rtcsm", [self.h] + tail, 2)
        return out

    # ---- the loop batch over several processes (RCCL) ----
    def rccl_comm(self, world: int = 1, rank: int = 0, unique_id: Optional[bytes] = None):
        """An ncclComm_t of `world` ranks on this context's device (lgs_rccl_comm_init);
        unique_id: the 128 bytes of lgs_rccl_unique_id, made on one rank (new if None)."""
        if unique_id is None:
            buf = (C.c_ubyte * 128)()
            self.check(self.lib.lgs_rccl_unique_id(buf), "rccl_unique_id")
        else:
            buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        comm = _P()
        self.check(self.lib.lgs_rccl_comm_init(self.h, buf, world, rank, C.byref(comm)), "rccl_comm_init")
        return comm

    def rccl_comm_destroy(self, comm):
        self.check(self.lib.lgs_rccl_comm_destroy(comm), "rccl_comm_destroy")

    def loop_records_allgather(self, comm, rank: int, world: int, n: int, local):
        """lgs_loop_records_allgather: this rank's block of LoopResult records ->
        all n records in candidate order."""
        cnt = len(local)
        loc = (LoopResult * max(1, cnt))(*local) if cnt else (LoopResult * 1)()
        out = (LoopResult * max(1, n))()
        self.check(self.lib.lgs_loop_records_allgather(self.h, comm, rank, world, n, loc, out),
                   "loop_records_allgather")
        return out

    # ---- branch-and-bound matcher ----
    def precompute_pyramid(self, src: "Grid", node_height_max: int):
        """PrecomputeGridMaps: [window-max grid with window 2^h for h = 0..H]"""
        out = [self.grid(src.w, src.hgt, src.min_x, src.min_y, src.res) for _ in range(node_height_max + 1)]
        arr = (_P * len(out))(*[g.h for g in out])
        self.check(self.lib.lgs_grid_precompute_pyramid(self.h, src.h, int(node_height_max), arr),
                   "grid_precompute_pyramid")
        return out

    def bb_optimize_pose_batch(self, grid, pyramid, params: "BBParams", cost: CostGEParams, scans, inits,
                               thr: float):
        n = len(scans)
        parr = (_P * len(pyramid))(*[g.h for g in pyramid])
        sarr = (_P * n)(*[s.h for s in scans])
        poses = (Pose2D * n)(*[Pose2D(*p) for p in inits])
        out = (RtcsmSummary * max(1, n))()
        self._call_cost("bb_optimize_pose_batch", [self.h, grid.h, parr, C.byref(params), cost, sarr, poses, n,
                                                   float(thr), out], 4)
        return list(out)[:n]

    def bb_optimize_pose_query(self, grid, params: "BBParams", cost: CostGEParams, scan, init) -> RtcsmSummary:
        out = RtcsmSummary()
        self._call_cost("bb_optimize_pose_query", [self.h, grid.h, C.byref(params), cost, scan.h, Pose2D(*init),
                                                   C.byref(out)], 3)
        return out

    def loop_detect_bb(self, params: "BBParams", cost: CostGEParams, thr: float, queries, candidates):
        """as loop_detect, with LoopDetectorBranchBound (the coarse entry of a query is ignored)"""
        qs, cs, out = self._loop_arrays(queries, candidates, False)
        self._call_cost("loop_detect_bb", [self.h, C.byref(params), cost, float(thr), qs, len(queries), cs,
                                           len(candidates), out], 2)
        return out

    # ---- exhaustive grid-search matcher ----
    def gs_optimize_pose_batch(self, grid, params: "GSParams", cost: CostGEParams, scans, inits, thr: float):
        n = len(scans)
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in inits])
        out = (RtcsmSummary * max(1, n))()
        self._call_cost("gs_optimize_pose_batch", [self.h, grid.h, C.byref(params), cost, sarr, poses, n, float(thr),
                                                   out], 3)
        return list(out)[:n]

    def gs_optimize_pose_query(self, grid, params: "GSParams", cost: CostGEParams, scan, init) -> RtcsmSummary:
        out = RtcsmSummary()
        self._call_cost("gs_optimize_pose_query", [self.h, grid.h, C.byref(params), cost, scan.h, Pose2D(*init),
                                                   C.byref(out)], 3)
        return out

    def gs_dense_scores(self, grid, params: "GSParams", scan, init) -> np.ndarray:
        """every pose's score, [ny, nx, nt] (the reference's loop order)"""
        nx, ny, nt = (len(gs_steps(r, s)) for r, s in ((params.range_x, params.step_x),
                                                        (params.range_y, params.step_y),
                                                        (params.range_theta, params.step_theta)))
        out = np.zeros((ny, nx, nt))
        self.check(self.lib.lgs_gs_dense_scores(self.h, grid.h, C.byref(params), scan.h, Pose2D(*init), dptr(out),
                                                out.size), "gs_dense_scores")
        return out

    def loop_detect_gs(self, params: "GSParams", cost: CostGEParams, thr: float, queries, candidates):
        """as loop_detect, with LoopDetectorGridSearch (the coarse entry of a query is ignored)"""
        qs, cs, out = self._loop_arrays(queries, candidates, False)
        self._call_cost("loop_detect_gs", [self.h, C.byref(params), cost, float(thr), qs, len(queries), cs,
                                           len(candidates), out], 2)
        return out

    # ---- hill-climbing matcher ----
    def hc_optimize_pose_query(self, grid, params: "HCParams", cost: CostGEParams, scan, init) -> "HCSummary":
        out = HCSummary()
        self.check(self.lib.lgs_hc_optimize_pose_query(self.h, grid.h, C.byref(params), C.byref(cost), scan.h,
                                                       Pose2D(*init), C.byref(out)), "hc_optimize_pose_query")
        return out

    def hc_optimize_pose_batch(self, grids, params: "HCParams", cost: CostGEParams, scans, inits):
        """n independent matches, one launch per chunk; grids: one map per
        match (or a single map for all)"""
        n = len(scans)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in inits])
        out = (HCSummary * max(1, n))()
        self.check(self.lib.lgs_hc_optimize_pose_batch(self.h, garr, C.byref(params), C.byref(cost), sarr, poses, n,
                                                       out), "hc_optimize_pose_batch")
        return list(out)[:n]

    def hc_trace(self, grid, params: "HCParams", cost: CostGEParams, scan, init):
        """(moves, costs): the accepted move (or -1) and minCost of every pass"""
        cap = max(1, params.max_iterations)
        moves = np.zeros(cap, dtype=np.int32)
        costs = np.zeros(cap)
        n = self.lib.lgs_hc_trace(self.h, grid.h, C.byref(params), C.byref(cost), scan.h, Pose2D(*init),
                                  moves.ctypes.data_as(C.POINTER(C.c_int)), dptr(costs), cap)
        if n < 0:
            self.check(-n, "hc_trace")
        return moves[:n].copy(), costs[:n].copy()

    def cost_ge_exact(self, grid, cost: CostGEParams, scan, poses) -> np.ndarray:
        """the greedy-endpoint cost at every sensor pose, bit-exact"""
        n = len(poses)
        parr = (Pose2D * max(1, n))(*[Pose2D(*p) for p in poses])
        out = np.zeros(max(1, n))
        self.check(self.lib.lgs_cost_ge_exact(self.h, grid.h, C.byref(cost), scan.h, parr, n, dptr(out)),
                   "cost_ge_exact")
        return out[:n]

    # ---- Gauss-Newton refine (K4) ----
    def linsolve(self, grid, params: LinsolveParams, scan, init, trajectory: bool = False):
        """ScanMatcherLinearSolver::OptimizePose; returns the summary and, with
        trajectory=True, [(x, y, theta, cost)] after every OptimizeStep."""
        out = LinsolveSummary()
        traj = np.zeros(4 * max(1, params.num_iterations_max)) if trajectory else None
        self.check(self.lib.lgs_linsolve_optimize_pose(self.h, grid.h, C.byref(params), scan.h, Pose2D(*init),
                                                       C.byref(out), dptr(traj) if trajectory else None),
                   "linsolve_optimize_pose")
        if trajectory:
            return out, [tuple(traj[4 * k: 4 * k + 4]) for k in range(out.iterations)]
        return out

    def linsolve_batch(self, grid, params: LinsolveParams, scans, inits):
        n = len(scans)
        arr = (_P * n)(*[s.h for s in scans])
        poses = (Pose2D * n)(*[Pose2D(*p) for p in inits])
        out = (LinsolveSummary * n)()
        self.check(self.lib.lgs_linsolve_optimize_pose_batch(self.h, grid.h, C.byref(params), arr, poses, n, out),
                   "linsolve_optimize_pose_batch")
        return list(out)

    # ---- point-to-line ICP (scan against scan) ----
    def icp(self, ref_scan, ref_pose, scan, init, params: "IcpParams", trajectory: bool = False):
        """lgs_icp_optimize_pose; returns the summary and, with trajectory=True,
        [(x, y, theta, cost, pairs)] after every step."""
        out = IcpSummary()
        traj = np.zeros(5 * max(1, params.num_iterations_max)) if trajectory else None
        self.check(self.lib.lgs_icp_optimize_pose(self.h, ref_scan.h, Pose2D(*ref_pose), scan.h, Pose2D(*init),
                                                  C.byref(params), C.byref(out), dptr(traj) if trajectory else None),
                   "icp_optimize_pose")
        if trajectory:
            return out, [tuple(traj[5 * k: 5 * k + 5]) for k in range(out.iterations)]
        return out

    def icp_batch(self, ref_scans, ref_poses, scans, inits, params: "IcpParams"):
        n = len(scans)
        rarr = (_P * max(1, n))(*[s.h for s in ref_scans])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        rposes = (Pose2D * max(1, n))(*[Pose2D(*p) for p in ref_poses])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in inits])
        out = (IcpSummary * max(1, n))()
        self.check(self.lib.lgs_icp_optimize_pose_batch(self.h, rarr, rposes, sarr, poses, n, C.byref(params), out),
                   "icp_optimize_pose_batch")
        return list(out)[:n]

    def icp_pairs(self, ref_scan, ref_pose, scan, sensor_pose, params: "IcpParams"):
        """lgs_icp_pairs: (index, residual) per beam of `scan` at a sensor pose;
        index is the paired reference beam, -1 rejected, -2 unusable."""
        n = len(scan.ranges)
        index = np.zeros(n, dtype=np.int32)
        residual = np.zeros(n)
        self.check(self.lib.lgs_icp_pairs(self.h, ref_scan.h, Pose2D(*ref_pose), scan.h, Pose2D(*sensor_pose),
                                          C.byref(params), index.ctypes.data_as(C.POINTER(C.c_int)), dptr(residual)),
                   "icp_pairs")
        return index, residual

    def icp_ref(self, scans, poses, params: "IcpParams") -> "IcpRef":
        """lgs_icp_ref_create: a set of reference scans at robot poses as one
        table behind a grid; the scans may be closed afterwards."""
        n = len(scans)
        arr = (_P * max(1, n))(*[s.h for s in scans])
        ps = (Pose2D * max(1, n))(*[Pose2D(*p) for p in poses])
        h = _P()
        self.check(self.lib.lgs_icp_ref_create(self.h, arr, ps, n, C.byref(params), C.byref(h)), "icp_ref_create")
        return IcpRef(self, h)

    def icp_ref_set(self, scans, poses, idx_min, idx_max, params: "IcpParams") -> "IcpRefSet":
        """lgs_icp_ref_set_create: one reference per inclusive node range
        idx_min[i] .. idx_max[i] of (scans, poses), all built in one pass
        (DESIGN.md 4.5d); reference i equals icp_ref(scans[lo:hi + 1], poses[lo:hi + 1])."""
        n, m = len(scans), len(idx_min)
        arr = (_P * max(1, n))(*[s.h for s in scans])
        ps = (Pose2D * max(1, n))(*[Pose2D(*p) for p in poses])
        lo = (C.c_int * max(1, m))(*[int(v) for v in idx_min])
        hi = (C.c_int * max(1, m))(*[int(v) for v in idx_max])
        h = _P()
        self.check(self.lib.lgs_icp_ref_set_create(self.h, arr, ps, n, lo, hi, m, C.byref(params), C.byref(h)),
                   "icp_ref_set_create")
        return IcpRefSet(self, h)

    IcpRefSetStats = namedtuple("IcpRefSetStats", "builds table_launches count_launches scan_launches "
                                                  "scatter_launches build_syncs refine_launches")

    def icp_ref_set_stats(self):
        """lgs_icp_ref_set_stats: this context's counters of set builds and refine launches"""
        v = [C.c_longlong() for _ in range(7)]
        self.check(self.lib.lgs_icp_ref_set_stats(self.h, *[C.byref(x) for x in v]), "icp_ref_set_stats")
        return Context.IcpRefSetStats(*[x.value for x in v])

    def icp_ref_set_last_build_ms(self):
        """lgs_icp_ref_set_last_build_ms: (table pass, grids) of the last set build, host clock"""
        a, b = C.c_double(), C.c_double()
        self.check(self.lib.lgs_icp_ref_set_last_build_ms(self.h, C.byref(a), C.byref(b)), "icp_ref_set_last_build_ms")
        return a.value, b.value

    def loop_refine_icp(self, refs, queries, candidates, params: "IcpParams", gate: "LoopRefineGate", results):
        """lgs_loop_refine_icp: refs[q] is query q's IcpRef; queries and candidates as loop_detect takes them
        (a query's map and coarse grid may be None); results: a ctypes LoopResult array, refined in place.
        Returns (refined flags, [IcpSummary] per candidate)."""
        n = len(candidates)
        qs = (LoopQuery * max(1, len(queries)))()
        for i, (m, c, pose, idx, first, cnt) in enumerate(queries):
            qs[i] = LoopQuery(m.h if m is not None else None, None, Pose2D(*pose), idx, first, cnt)
        cs = (LoopCandidate * max(1, n))()
        for i, (s, pose, idx) in enumerate(candidates):
            cs[i] = LoopCandidate(s.h, Pose2D(*pose), idx, 0)
        rarr = (_P * max(1, len(refs)))(*[r.h for r in refs])
        refined = (C.c_int * max(1, n))()
        sums = (IcpSummary * max(1, n))()
        self.check(self.lib.lgs_loop_refine_icp(self.h, rarr, qs, len(queries), cs, n, C.byref(params), C.byref(gate),
                                                results, refined, sums), "loop_refine_icp")
        return list(refined)[:n], list(sums)[:n]

    def icp_window_scores(self, ref: "IcpRef", scan, centre, window: "IcpWindow", params: "IcpParams"):
        """lgs_icp_ref_window_scores: (cost float64, pairs int32), each shaped [nt, ny, nx]: what
        ref.refine(scan, window.pose(centre, p), params) reports as initial_cost / initial_pairs"""
        shape = window.shape
        cost, pairs = np.zeros(shape), np.zeros(shape, dtype=np.int32)
        self.check(self.lib.lgs_icp_ref_window_scores(self.h, ref.h, scan.h, Pose2D(*centre), C.byref(window),
                                                      C.byref(params), dptr(cost),
                                                      pairs.ctypes.data_as(C.POINTER(C.c_int))), "icp_ref_window_scores")
        return cost, pairs

    def loop_detect_icp(self, refs, queries, candidates, params: "IcpParams", window: "IcpWindow",
                        gate: "LoopRefineGate"):
        """lgs_loop_detect_icp: refs[q] is query q's IcpRef; queries and candidates as loop_refine_icp takes them.
        Returns (ctypes LoopResult array, [best lattice index] and [IcpSummary] per candidate)."""
        n = len(candidates)
        qs = (LoopQuery * max(1, len(queries)))()
        for i, (m, c, pose, idx, first, cnt) in enumerate(queries):
            qs[i] = LoopQuery(m.h if m is not None else None, None, Pose2D(*pose), idx, first, cnt)
        cs = (LoopCandidate * max(1, n))()
        for i, (s, pose, idx) in enumerate(candidates):
            cs[i] = LoopCandidate(s.h, Pose2D(*pose), idx, 0)
        rarr = (_P * max(1, len(refs)))(*[r.h for r in refs])
        out = (LoopResult * max(1, n))()
        best = (C.c_int * max(1, n))()
        sums = (IcpSummary * max(1, n))()
        self.check(self.lib.lgs_loop_detect_icp(self.h, rarr, qs, len(queries), cs, n, C.byref(params), C.byref(window),
                                                C.byref(gate), out, best, sums), "loop_detect_icp")
        return out, list(best)[:n], list(sums)[:n]

    IcpWindowStats = namedtuple("IcpWindowStats", "calls score_launches syncs refine_launches")

    def icp_window_stats(self):
        """lgs_icp_window_stats: this context's counters of window searches"""
        v = [C.c_longlong() for _ in range(4)]
        self.check(self.lib.lgs_icp_window_stats(self.h, *[C.byref(x) for x in v]), "icp_window_stats")
        return Context.IcpWindowStats(*[x.value for x in v])

    def loop_graph(self, poses, idx_min, idx_max) -> "LoopGraph":
        """lgs_loop_graph_create: a graph snapshot (poses n x 2 or n x 3, the
        maps' inclusive node ranges) for the nearest-node loop searcher
        (DESIGN.md 4.6g); the walk and its travel chain go to the device once."""
        p, lo, hi = _loop_snapshot(poses, idx_min, idx_max)
        h = _P()
        self.check(self.lib.lgs_loop_graph_create(self.h, p.ctypes.data_as(C.POINTER(Pose2D)), len(p), _iptr(lo),
                                                  _iptr(hi), len(lo), C.byref(h)), "loop_graph_create")
        return LoopGraph(self, h, len(lo))

    def loop_search_stats(self) -> dict:
        """lgs_loop_search_stats: searches of this context that ran the kernels / the host loop"""
        v = (C.c_longlong * 4)()
        self.check(self.lib.lgs_loop_search_stats(self.h, v), "loop_search_stats")
        return dict(device_calls=v[0], host_calls=v[1], launches=v[2], pairs=v[3])

    def cost_square_error(self, grid, umin: float, umax: float, scan, sensor_pose, covariance: bool = False):
        v = C.c_double()
        cov = (C.c_double * 9)() if covariance else None
        self.check(self.lib.lgs_cost_square_error(self.h, grid.h, umin, umax, scan.h, Pose2D(*sensor_pose),
                                                  C.byref(v), cov), "cost_square_error")
        return (v.value, list(cov)) if covariance else v.value

    # ---- CostSquareError for every matcher ----
    def cost_square_error_batch(self, grids, cost: "CostSQParams", scans, sensor_poses, covariance: bool = False):
        """Cost and, with covariance=True, ComputeCovariance of item j at
        sensor_poses[j] on grids[j] with scans[j] (a single grid or scan
        serves every item): costs [n], or (costs, covariances [n, 9])"""
        n = len(sensor_poses)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        if not isinstance(scans, (list, tuple)):
            scans = [scans] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in sensor_poses])
        out = np.zeros(max(1, n))
        cov = np.zeros((max(1, n), 9)) if covariance else None
        self.check(self.lib.lgs_cost_square_error_batch(self.h, garr, C.byref(cost), sarr, poses, n, dptr(out),
                                                        dptr(cov) if covariance else None),
                   "cost_square_error_batch")
        return (out[:n], cov[:n]) if covariance else out[:n]

    def summaries_apply_cost_sq(self, grids, cost: "CostSQParams", scans, summaries):
        """the summaries of rtcsm / bb / gs matches as a matcher constructed
        with CostSquareError returns them: normalized cost and covariance at
        best_sensor_pose replaced, every other field kept.  Returns new copies."""
        n = len(summaries)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        arr = (RtcsmSummary * max(1, n))()
        for k, s in enumerate(summaries):
            C.memmove(C.byref(arr, k * C.sizeof(RtcsmSummary)), C.byref(s), C.sizeof(RtcsmSummary))
        self.check(self.lib.lgs_summaries_apply_cost_sq(self.h, garr, C.byref(cost), sarr, arr, n),
                   "summaries_apply_cost_sq")
        return list(arr)[:n]

    # ---- the greedy-endpoint cost bit for bit, for the search matchers ----
    def cost_ge_exact_batch(self, grids, cost: "CostGEParams", scans, sensor_poses, covariance: bool = False):
        """CostGreedyEndpoint::Cost and, with covariance=True, ComputeCovariance
        of item j at sensor_poses[j] on grids[j] with scans[j] (a single grid
        or scan serves every item), the reference's bytes: costs [n], or
        (costs, covariances [n, 9])"""
        n = len(sensor_poses)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        if not isinstance(scans, (list, tuple)):
            scans = [scans] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in sensor_poses])
        out = np.zeros(max(1, n))
        cov = np.zeros((max(1, n), 9)) if covariance else None
        self.check(self.lib.lgs_cost_ge_exact_batch(self.h, garr, C.byref(cost), sarr, poses, n, dptr(out),
                                                    dptr(cov) if covariance else None),
                   "cost_ge_exact_batch")
        return (out[:n], cov[:n]) if covariance else out[:n]

    def summaries_apply_cost_ge_exact(self, grids, cost: "CostGEParams", scans, summaries):
        """the summaries of rtcsm / bb / gs matches as LGS_COST_GREEDY_ENDPOINT_EXACT
        returns them: normalized cost and covariance at best_sensor_pose replaced
        by the reference's bytes, every other field kept.  Returns new copies."""
        n = len(summaries)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        arr = (RtcsmSummary * max(1, n))()
        for k, s in enumerate(summaries):
            C.memmove(C.byref(arr, k * C.sizeof(RtcsmSummary)), C.byref(s), C.sizeof(RtcsmSummary))
        self.check(self.lib.lgs_summaries_apply_cost_ge_exact(self.h, garr, C.byref(cost), sarr, arr, n),
                   "summaries_apply_cost_ge_exact")
        return list(arr)[:n]

    def hc_sq_optimize_pose_query(self, grid, params: "HCParams", cost: "CostSQParams", scan, init) -> "HCSummary":
        out = HCSummary()
        self.check(self.lib.lgs_hc_sq_optimize_pose_query(self.h, grid.h, C.byref(params), C.byref(cost), scan.h,
                                                          Pose2D(*init), C.byref(out)), "hc_sq_optimize_pose_query")
        return out

    def hc_sq_optimize_pose_batch(self, grids, params: "HCParams", cost: "CostSQParams", scans, inits):
        """n independent matches; grids: one map per match (or a single map
        for all), of any size and resolution"""
        n = len(scans)
        if not isinstance(grids, (list, tuple)):
            grids = [grids] * n
        garr = (_P * max(1, n))(*[g.h for g in grids])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in inits])
        out = (HCSummary * max(1, n))()
        self.check(self.lib.lgs_hc_sq_optimize_pose_batch(self.h, garr, C.byref(params), C.byref(cost), sarr, poses,
                                                          n, out), "hc_sq_optimize_pose_batch")
        return list(out)[:n]

    def hc_sq_trace(self, grid, params: "HCParams", cost: "CostSQParams", scan, init):
        """(moves, costs): the accepted move (or -1) and minCost of every pass"""
        cap = max(1, params.max_iterations)
        moves = np.zeros(cap, dtype=np.int32)
        costs = np.zeros(cap)
        n = self.lib.lgs_hc_sq_trace(self.h, grid.h, C.byref(params), C.byref(cost), scan.h, Pose2D(*init),
                                     moves.ctypes.data_as(C.POINTER(C.c_int)), dptr(costs), cap)
        if n < 0:
            self.check(-n, "hc_sq_trace")
        return moves[:n].copy(), costs[:n].copy()

    # ---- occupancy maps (K3) ----
    def pg_cg_solve(self, diag, pairs, off, rhs, tolerance: float = 0.0, max_iterations: int = 0):
        """lgs_pg_cg_solve: H x = rhs of a pose-graph LM step by Jacobi-preconditioned
        CG on the device.  diag [n, 3, 3], pairs [p, 2] (a < b, unique), off
        [p, 3, 3] (block (a, b)), rhs [3n] -> (x [3n], passes, last |r|^2)"""
        diag = np.ascontiguousarray(diag, dtype=np.float64).reshape(-1, 9)
        n = diag.shape[0]
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        off = np.ascontiguousarray(off, dtype=np.float64).reshape(-1, 9)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
        assert off.shape[0] == pairs.shape[0] and rhs.shape[0] == 3 * n
        x = np.zeros(3 * max(n, 1))
        it, res = C.c_int(), C.c_double()
        npairs = pairs.shape[0]
        self.check(self.lib.lgs_pg_cg_solve(self.h, n, dptr(diag), npairs,
                                            pairs.ctypes.data_as(C.POINTER(C.c_int)) if npairs else None,
                                            dptr(off) if npairs else None, dptr(rhs), float(tolerance),
                                            int(max_iterations), dptr(x), C.byref(it), C.byref(res)), "pg_cg_solve")
        return x[:3 * n], it.value, res.value

    def pg_cg_stats(self) -> dict:
        """lgs_pg_cg_stats: solves, CG passes, block patterns built and multi-workgroup solves on this context"""
        a, b, c, d = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        self.check(self.lib.lgs_pg_cg_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "pg_cg_stats")
        return dict(solves=a.value, iterations=b.value, patterns=c.value, grid_solves=d.value)

    def pg_lm_optimize(self, poses, edges, iters: int = 10, tol: float = 1e-3, lam: float = 1e-4, loss: int = 0,
                       scale: float = 1.0):
        """lgs_pg_lm_optimize: PoseGraphOptimizerLM::Optimize with the graph resident on
        the device.  poses [n, 3]; edges [(start, end, (x, y, theta), info 3x3)] or
        a pg_edges() array -> (poses [n, 3], LM steps, total error, lambda after, CG passes)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        n = poses.shape[0]
        out = poses.copy()
        earr, m = (edges, len(edges)) if isinstance(edges, C.Array) else (pg_edges(edges), len(edges))
        prm = PgLmParams(int(iters), float(tol), int(loss), float(scale))
        lam_io, it, tot, passes = C.c_double(lam), C.c_int(), C.c_double(), C.c_longlong()
        self.check(self.lib.lgs_pg_lm_optimize(self.h, C.byref(prm), C.byref(lam_io),
                                               out.ctypes.data_as(C.POINTER(Pose2D)) if n else None, n,
                                               C.cast(earr, _P) if m else None, m, C.byref(it), C.byref(tot),
                                               C.byref(passes)), "pg_lm_optimize")
        return out, it.value, tot.value, lam_io.value, passes.value

    def pg_lm_linearize(self, poses, edges, lam: float = 1e-4, loss: int = 0, scale: float = 1.0):
        """lgs_pg_lm_linearize: the device's H and right-hand side of one LM step ->
        (diag [n, 3, 3], pairs [p, 2] in first-appearance order, off [p, 3, 3], rhs [3n])"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        n = poses.shape[0]
        earr, m = (edges, len(edges)) if isinstance(edges, C.Array) else (pg_edges(edges), len(edges))
        diag, rhs = np.zeros((max(n, 1), 3, 3)), np.zeros(3 * max(n, 1))
        pairs, off = np.zeros((max(m, 1), 2), dtype=np.int32), np.zeros((max(m, 1), 3, 3))
        npairs = C.c_int()
        self.check(self.lib.lgs_pg_lm_linearize(self.h, int(loss), float(scale), float(lam),
                                                poses.ctypes.data_as(C.POINTER(Pose2D)) if n else None, n,
                                                C.cast(earr, _P) if m else None, m, dptr(diag), C.byref(npairs),
                                                pairs.ctypes.data_as(C.POINTER(C.c_int)), dptr(off), dptr(rhs)),
                   "pg_lm_linearize")
        return diag[:n], pairs[:npairs.value].copy(), off[:npairs.value].copy(), rhs[:3 * n]

    def pg_lm_stats(self) -> dict:
        """lgs_pg_lm_stats: resident Optimize calls, LM steps, pose uploads and downloads, incidence-list builds"""
        v = [C.c_longlong() for _ in range(5)]
        self.check(self.lib.lgs_pg_lm_stats(self.h, *[C.byref(x) for x in v]), "pg_lm_stats")
        return dict(zip(("optimizes", "steps", "pose_uploads", "pose_downloads", "incidence_builds"),
                        [x.value for x in v]))

    def map(self, res: float, patch_size: int, ncx: int, ncy: int, center=(0.0, 0.0)) -> "Map":
        h = _P()
        self.check(self.lib.lgs_map_create(self.h, res, patch_size, ncx, ncy, center[0], center[1],
                                           C.byref(h)), "map_create")
        return Map(self, h)

    def construct_maps(self, maps, ranges, scans, poses, bp: "BuilderParams"):
        """GridMapBuilder::AfterLoopClosure's rebuild: maps[i] from pose-graph
        nodes ranges[i] = (idx_min, idx_max) inclusive; node k = (scans[k], poses[k])."""
        nm, n = len(maps), len(scans)
        mh = (_P * nm)(*[m.h for m in maps])
        lo = (C.c_int * nm)(*[int(a) for a, _ in ranges])
        hi = (C.c_int * nm)(*[int(b) for _, b in ranges])
        arr = (_P * n)(*[s.h for s in scans])
        ps = (Pose2D * n)(*[Pose2D(*p) for p in poses])
        self.check(self.lib.lgs_maps_construct_from_scans(self.h, mh, lo, hi, nm, arr, ps, n, C.byref(bp)),
                   "maps_construct_from_scans")

    def construct_global_map(self, res: float, patch_size: int, scans, poses, bp: "BuilderParams") -> "Map":
        """GridMapBuilder::ConstructGlobalMap: a new map from all nodes."""
        n = len(scans)
        arr = (_P * n)(*[s.h for s in scans])
        ps = (Pose2D * n)(*[Pose2D(*p) for p in poses])
        h = _P()
        self.check(self.lib.lgs_map_construct_global(self.h, res, patch_size, arr, ps, n, C.byref(bp), C.byref(h)),
                   "map_construct_global")
        return Map(self, h)

    DEBUG_BUFFERS = {"sbound": (0, np.float64), "part_c": (1, np.float64), "part_k": (2, np.int64),
                     "L": (3, np.float64), "tedge": (4, np.int32), "cbase": (5, np.int32), "idx": (6, np.int32),
                     "cscore": (7, np.float64), "planes": (8, np.float64), "super": (9, np.float16),
                     "hv_inmask": (10, np.uint64), "hv_outmask": (11, np.uint64),
                     # the selection: list [nseg, 1024], segcnt [nseg], [nsel, dlist...], [1 = k_select_list wrote it]
                     "sel_list": (12, np.int32), "sel_segcnt": (13, np.int32), "sel_dense": (14, np.int32),
                     "sel_by_list": (15, np.int32),
                     # cflag [K]; the work list: entries t << 6 | sb, [entries, edge angles, ...], edge angles
                     "cflag": (16, np.uint8), "wl_sbl": (17, np.int32), "wl_cnt": (18, np.int32),
                     "wl_al": (19, np.int32)}

    def debug_buffer(self, name: str, item: int = 0) -> np.ndarray:
        """Diagnostics: an intermediate buffer of one item of the last
        correlative batch (lgs_debug_item_buffer); "L" = [Lp, pad x7, Lc0..Lc3]."""
        which, dt = self.DEBUG_BUFFERS[name]
        n = C.c_size_t()
        self.check(self.lib.lgs_debug_item_buffer(self.h, item, which, None, 0, C.byref(n)), "debug_item_buffer")
        out = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
        self.check(self.lib.lgs_debug_item_buffer(self.h, item, which, out.ctypes.data_as(_P), out.nbytes,
                                                  C.byref(n)),
                   "debug_item_buffer")
        return out

    def debug_libm(self, op: int, x) -> np.ndarray:
        """Diagnostics: the device's glibc sincos (op 0, rows of (sin, cos)) or
        pow(x, 3.0) (op 1) on the GPU, or the device's sqrt(x) (op 2) and
        fmod(x, 2 pi) (op 3) (lgs_debug_libm)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros((len(x), 2) if op == 0 else len(x), dtype=np.float64)
        self.check(self.lib.lgs_debug_libm(self.h, op, x.ctypes.data_as(_P), len(x), out.ctypes.data_as(_P)),
                   "debug_libm")
        return out

    def copy_counters(self) -> dict:
        """Diagnostics: cross-context map copies made onto this context by
        lgs_loop_detect_rtcsm_multi (lgs_debug_copy_counters)."""
        a, b = C.c_longlong(), C.c_longlong()
        self.check(self.lib.lgs_debug_copy_counters(self.h, C.byref(a), C.byref(b)), "debug_copy_counters")
        return {"direct": a.value, "staged": b.value}

    def offset_checks(self, reset: bool = True) -> dict:
        """Checked build only (liblgs_hip_checked.so): plane-offset checks and
        violations of the correlative consumers since the last reset
        (lgs_debug_offset_checks); raises in the product build."""
        out = (C.c_ulonglong * 4)()
        self.check(self.lib.lgs_debug_offset_checks(self.h, 1 if reset else 0, out), "debug_offset_checks")
        return {"checked": out[0], "violations": out[1], "first": out[2], "first_base": out[3]}

    def debug_keysort(self, keys, lo: int, bits: int) -> np.ndarray:
        """Diagnostics: the K3 stable radix sort (csrc/k_sort.hip) of host u32
        keys on bits [lo, lo + bits) (lgs_debug_keysort)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        out = np.zeros_like(k)
        self.check(self.lib.lgs_debug_keysort(self.h, k.ctypes.data_as(_P), out.ctypes.data_as(_P), len(k), lo, bits),
                   "debug_keysort")
        return out

    def cost_greedy_endpoint(self, grid, cost: CostGEParams, scan, pose) -> float:
        v = C.c_double()
        self.check(self.lib.lgs_cost_greedy_endpoint(self.h, grid.h, C.byref(cost), scan.h, Pose2D(*pose),
                                                     C.byref(v)), "cost_greedy_endpoint")
        return v.value


class Grid:
    def __init__(self, ctx: Context, h, w, hh, min_x, min_y, res, owned=True, map_view=None):
        self.ctx, self.h = ctx, h
        self.map_view = map_view      # owning Map for lgs_map_grid views (handle not ours)
        self.w, self.hgt = w, hh
        self.min_x, self.min_y, self.res = min_x, min_y, res
        self.owned = owned

    def upload(self, cells: np.ndarray):
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        assert cells.shape == (self.hgt, self.w)
        self.ctx.check(self.ctx.lib.lgs_grid_upload(self.ctx.h, self.h, dptr(cells)), "grid_upload")

    def download(self) -> np.ndarray:
        out = np.zeros((self.hgt, self.w))
        self.ctx.check(self.ctx.lib.lgs_grid_download(self.ctx.h, self.h, dptr(out)), "grid_download")
        return out

    def device_ptr(self) -> int:
        return self.ctx.lib.lgs_grid_device_ptr(self.h)

    def close(self):
        if self.h:
            if self.map_view is None:
                self.ctx.lib.lgs_grid_destroy(self.h)  # frees the handle; cells only if owned
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Map:
    """lgs_map: GridMap<BinaryBayesGridCell<double>> with device-resident cells."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def geometry(self) -> dict:
        g = MapGeometry()
        self.ctx.check(self.ctx.lib.lgs_map_get_geometry(self.h, C.byref(g)), "map_geometry")
        return g.dict()

    def grid(self) -> "Grid":
        """Non-owning grid view (valid until the next geometry change)."""
        gh = _P()
        self.ctx.check(self.ctx.lib.lgs_map_grid(self.h, C.byref(gh)), "map_grid")
        mg = MapGeometry()
        self.ctx.check(self.ctx.lib.lgs_map_get_geometry(self.h, C.byref(mg)), "map_geometry")
        return Grid(self.ctx, gh, mg.num_cells_x, mg.num_cells_y, mg.min_x, mg.min_y, mg.resolution,
                    owned=False, map_view=self)

    def update_scan(self, scan: "Scan", robot_pose, bp: BuilderParams):
        self.ctx.check(self.ctx.lib.lgs_map_update_scan(self.ctx.h, self.h, scan.h, Pose2D(*robot_pose),
                                                        C.byref(bp)), "map_update_scan")

    def construct(self, scans, poses, bp: BuilderParams):
        n = len(scans)
        arr = (_P * n)(*[s.h for s in scans])
        ps = (Pose2D * n)(*[Pose2D(*p) for p in poses])
        self.ctx.check(self.ctx.lib.lgs_map_construct_from_scans(self.ctx.h, self.h, arr, ps, n, C.byref(bp)),
                       "map_construct_from_scans")

    def append_scan(self, latest: "Map", scans, poses, bp: BuilderParams):
        """GridMapBuilder::AppendScan: scans[-1] inserted into this (local) map,
        `latest` rebuilt from all of `scans` (lgs_map_append_scan)."""
        n = len(scans)
        arr = (_P * n)(*[s.h for s in scans])
        ps = (Pose2D * n)(*[Pose2D(*p) for p in poses])
        self.ctx.check(self.ctx.lib.lgs_map_append_scan(self.ctx.h, self.h, latest.h, arr, ps, n, C.byref(bp)),
                       "map_append_scan")

    def rebuilds(self) -> dict:
        """Diagnostics: incremental and full latest-map rebuilds of this map
        (lgs_debug_map_rebuilds)."""
        a, b = C.c_longlong(), C.c_longlong()
        self.ctx.check(self.ctx.lib.lgs_debug_map_rebuilds(self.h, C.byref(a), C.byref(b)), "debug_map_rebuilds")
        return {"incremental": a.value, "full": b.value}

    def render_gray(self) -> np.ndarray:
        """MapSaver::DrawMap gray image (rows flipped up-down), uint8 [h, w]."""
        g = self.geometry()
        img = np.zeros((g["h"], g["w"]), dtype=np.uint8)
        if img.size:
            self.ctx.check(self.ctx.lib.lgs_map_render_gray(self.ctx.h, self.h,
                                                            img.ctypes.data_as(C.POINTER(C.c_uint8))),
                           "map_render_gray")
        return img

    def render_gray_region(self, x0, y0, w, h, flip=True) -> np.ndarray:
        """DrawMap of the w x h cells at (x0, y0), uint8 [h, w] (lgs_map_render_gray_region)."""
        img = np.zeros((h, w), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.lgs_map_render_gray_region(self.ctx.h, self.h, x0, y0, w, h, int(flip),
                                                               img.ctypes.data_as(C.POINTER(C.c_uint8))),
                       "map_render_gray_region")
        return img

    def patches(self) -> np.ndarray:
        """Patch::IsAllocated per patch, uint8 [npy, npx]."""
        g = self.geometry()
        f = np.zeros((g["npy"], g["npx"]), dtype=np.uint8)
        if f.size:
            self.ctx.check(self.ctx.lib.lgs_map_download_patches(self.ctx.h, self.h,
                                                                 f.ctypes.data_as(C.POINTER(C.c_uint8))),
                           "map_download_patches")
        return f

    def actual_size(self):
        """GridMap::ComputeActualMapSize -> (allocated patches, 12 ints)."""
        n = C.c_int()
        out = (C.c_int * 12)()
        self.ctx.check(self.ctx.lib.lgs_map_actual_size(self.ctx.h, self.h, C.byref(n), out), "map_actual_size")
        return n.value, list(out)

    def download(self):
        g = self.geometry()
        cells = np.zeros((g["h"], g["w"]))
        hits = np.zeros((g["h"], g["w"]), dtype=np.uint32)
        misses = np.zeros((g["h"], g["w"]), dtype=np.uint32)
        self.ctx.check(self.ctx.lib.lgs_map_download(self.ctx.h, self.h, dptr(cells),
                                                     hits.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     misses.ctypes.data_as(C.POINTER(C.c_uint32))),
                       "map_download")
        return cells, hits, misses

    def close(self):
        if self.h:
            self.ctx.lib.lgs_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IcpRef:
    """lgs_icp_ref: the reference of the multi-scan point-to-line ICP."""
    RefInfo = namedtuple("RefInfo", "n_refs entries lines cells_x cells_y cell_size")

    def __init__(self, ctx, h, borrowed: bool = False):
        self.ctx, self.h = ctx, h
        self.borrowed = borrowed   # a member of an IcpRefSet: close() leaves it to the set

    def info(self):
        v = [C.c_int() for _ in range(5)]
        c = C.c_double()
        self.ctx.check(self.ctx.lib.lgs_icp_ref_info(self.h, *[C.byref(x) for x in v], C.byref(c)), "icp_ref_info")
        return IcpRef.RefInfo(*[x.value for x in v], c.value)

    def refine(self, scan, init, params: "IcpParams", trajectory: bool = False):
        """lgs_icp_ref_optimize_pose; as Context.icp"""
        out = IcpSummary()
        traj = np.zeros(5 * max(1, params.num_iterations_max)) if trajectory else None
        self.ctx.check(self.ctx.lib.lgs_icp_ref_optimize_pose(self.ctx.h, self.h, scan.h, Pose2D(*init), C.byref(params),
                                                              C.byref(out), dptr(traj) if trajectory else None),
                       "icp_ref_optimize_pose")
        if trajectory:
            return out, [tuple(traj[5 * k: 5 * k + 5]) for k in range(out.iterations)]
        return out

    def refine_batch(self, scans, inits, params: "IcpParams", refs=None):
        """lgs_icp_ref_optimize_pose_batch: item j is scans[j] from inits[j]
        against refs[j] (default: this reference for every item)"""
        n = len(scans)
        ctx = self.ctx
        refs = [self] * n if refs is None else refs
        rarr = (_P * max(1, n))(*[r.h for r in refs])
        sarr = (_P * max(1, n))(*[s.h for s in scans])
        poses = (Pose2D * max(1, n))(*[Pose2D(*p) for p in inits])
        out = (IcpSummary * max(1, n))()
        ctx.check(ctx.lib.lgs_icp_ref_optimize_pose_batch(ctx.h, rarr, sarr, poses, n, C.byref(params), out),
                  "icp_ref_optimize_pose_batch")
        return list(out)[:n]

    def pairs(self, scan, sensor_pose, params: "IcpParams"):
        """lgs_icp_ref_pairs: (reference scan, its beam, residual) per beam of `scan`"""
        n = len(scan.ranges)
        k, j = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        residual = np.zeros(n)
        ip = C.POINTER(C.c_int)
        self.ctx.check(self.ctx.lib.lgs_icp_ref_pairs(self.ctx.h, self.h, scan.h, Pose2D(*sensor_pose), C.byref(params),
                                                      k.ctypes.data_as(ip), j.ctypes.data_as(ip), dptr(residual)),
                       "icp_ref_pairs")
        return k, j, residual

    def close(self):
        if self.h and not self.borrowed:
            self.ctx.lib.lgs_icp_ref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IcpRefSet:
    """lgs_icp_ref_set: one IcpRef per local map, built in one pass; set[i] is a
    view that lives as long as the set and whose close() does nothing."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        self.n = ctx.lib.lgs_icp_ref_set_size(h)

    def __len__(self):
        return self.n

    def __getitem__(self, i) -> "IcpRef":
        if not self.h:
            raise ValueError("the reference set is closed")
        if not -self.n <= i < self.n:
            raise IndexError(i)
        return IcpRef(self.ctx, _P(self.ctx.lib.lgs_icp_ref_set_ref(self.h, i % self.n)), borrowed=True)

    def close(self):
        if self.h:
            self.ctx.lib.lgs_icp_ref_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoopGraph:
    """lgs_loop_graph: a graph snapshot of the nearest-node loop searcher."""
    GraphInfo = namedtuple("GraphInfo", "n m positions walk_travel")

    def __init__(self, ctx, h, m):
        self.ctx, self.h, self.m = ctx, h, m

    def info(self):
        v = [C.c_int() for _ in range(3)]
        t = C.c_double()
        self.ctx.check(self.ctx.lib.lgs_loop_graph_info(self.h, *[C.byref(x) for x in v], C.byref(t)), "loop_graph_info")
        return LoopGraph.GraphInfo(*[x.value for x in v], t.value)

    def travel(self) -> np.ndarray:
        """lgs_loop_graph_travel: travel[p] after every walk position"""
        out = np.zeros(self.info().positions)
        self.ctx.check(self.ctx.lib.lgs_loop_graph_travel(self.h, dptr(out), len(out)), "loop_graph_travel")
        return out

    def search(self, params: "LoopSearchParams", hints, per_map: bool = False):
        """lgs_loop_search_nearest: the records (LOOP_RESULT_DTYPE rows) of the
        hints (abi.loop_hints), with per_map also the q x m table"""
        h = _loop_hint_rows(hints)
        q = len(h)
        res = np.zeros(q, dtype=LOOP_RESULT_DTYPE)
        tab = np.zeros((q, self.m), dtype=LOOP_MAP_BEST_DTYPE) if per_map else None
        self.ctx.check(self.ctx.lib.lgs_loop_search_nearest(self.h, C.byref(params), h.ctypes.data, q, res.ctypes.data,
                                                            tab.ctypes.data if per_map else None),
                       "loop_search_nearest")
        return (res, tab) if per_map else res

    def close(self):
        if self.h:
            self.ctx.lib.lgs_loop_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scan:
    def __init__(self, ctx, h, ranges, angles, rel_pose, min_range, max_range):
        self.ctx, self.h = ctx, h
        self.ranges, self.angles = ranges, angles
        self.rel_pose, self.min_range, self.max_range = rel_pose, min_range, max_range

    def close(self):
        if self.h:
            self.ctx.lib.lgs_scan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
