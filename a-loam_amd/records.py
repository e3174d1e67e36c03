"""The records and enumerators of include/aloam_mi355x.h, each declared once, in the header's order.

A record is a ctypes.Structure; record_dtype() makes the numpy dtype of the same bytes from it, so a record that grows is changed in one
place.  This module imports ctypes and numpy only and never loads the library: binding.py re-exports all of it, and the numpy models
(posegraph.py, atlas.py, graph_records.py) take their dtypes from here.  tests/test_abi_records.py holds every class, dtype and constant
against what a C compiler makes of the header.
"""
from __future__ import annotations

import ctypes as C

import numpy as np


def record_dtype(cls):
    """The numpy dtype of a ctypes.Structure: names from _fields_, offsets from the field descriptors, itemsize from ctypes.sizeof; a
    nested Structure becomes a nested dtype, an array (of arrays) a sub-array of one shape."""
    def of(t):
        shape = ()
        while issubclass(t, C.Array):
            shape, t = shape + (t._length_,), t._type_
        base = record_dtype(t) if issubclass(t, C.Structure) else np.dtype(t)
        return (base, shape) if shape else base
    names = [n for n, _ in cls._fields_]
    return np.dtype({"names": names, "formats": [of(t) for _, t in cls._fields_], "offsets": [getattr(cls, n).offset for n in names],
                     "itemsize": C.sizeof(cls)})


E_ARG, E_SCAN_LINES, E_EMPTY, E_CAPACITY, E_HIP, E_STATE = -1, -2, -3, -4, -5, -6


class AloamConfig(C.Structure):
    _fields_ = [("n_scans", C.c_int), ("min_range", C.c_float), ("ring_from_field", C.c_int), ("batch", C.c_int),
                ("max_points", C.c_int), ("max_ring_points", C.c_int), ("device", C.c_int), ("lm_max_iterations", C.c_int),
                ("outer_iterations", C.c_int), ("distortion", C.c_int)]


CLOUD_FULL, CLOUD_SHARP, CLOUD_LESS_SHARP, CLOUD_FLAT, CLOUD_LESS_FLAT, CLOUD_CORNER_LAST, CLOUD_SURF_LAST = range(7)


class AloamOdomStats(C.Structure):
    _fields_ = [("corner_corr", C.c_int * 2), ("plane_corr", C.c_int * 2), ("lm_iterations", C.c_int * 2),
                ("lm_successful", C.c_int * 2), ("initial_cost", C.c_double * 2), ("final_cost", C.c_double * 2),
                ("termination", C.c_int * 2)]


STAGE_REGISTRATION, STAGE_ODOMETRY, STAGE_MAPPING, STAGE_ALL = 1, 2, 4, 7
RANGE_COLUMN_MAJOR, RANGE_ROW_MAJOR = 0, 1


class AloamRangeDecoder(C.Structure):
    """aloam_range_decoder: how a 16-bit range image becomes points (a-loam_amd/range_input.py holds the definition)."""
    _fields_ = [("rows", C.c_int), ("n_az", C.c_int), ("order", C.c_int), ("range_scale", C.c_float),
                ("az_x", C.POINTER(C.c_float)), ("az_y", C.POINTER(C.c_float)), ("cos_el", C.POINTER(C.c_float)), ("sin_el", C.POINTER(C.c_float)),
                ("range_off", C.POINTER(C.c_float)), ("z_off", C.POINTER(C.c_float)), ("az_off", C.POINTER(C.c_int)), ("ring_id", C.POINTER(C.c_int))]


def range_decoder_struct(dec):
    """The C struct of a range_input.RangeDecoder (or anything with its fields); the second value keeps the arrays it points to alive."""
    keep = {k: np.ascontiguousarray(getattr(dec, k), dtype=np.float32) for k in ("az_x", "az_y", "cos_el", "sin_el", "range_off", "z_off")}
    keep.update({k: np.ascontiguousarray(getattr(dec, k), dtype=np.int32) for k in ("az_off", "ring_id")})
    d = AloamRangeDecoder(int(dec.rows), int(dec.n_az), int(dec.order), float(dec.range_scale))
    for k, a in keep.items():
        setattr(d, k, a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_int)))
    return d, keep


MAP_REGISTERED, MAP_CORNER_STACK, MAP_SURF_STACK, MAP_SURROUND, MAP_FULL = 2, 3, 4, 5, 6


class AloamPoseRecord(C.Structure):
    _fields_ = [("q_w", C.c_double * 4), ("t_w", C.c_double * 3), ("q_last_curr", C.c_double * 4), ("t_last_curr", C.c_double * 3),
                ("map_q_w", C.c_double * 4), ("map_t_w", C.c_double * 3), ("q_wmap_wodom", C.c_double * 4), ("t_wmap_wodom", C.c_double * 3),
                ("inited", C.c_int), ("map_frames", C.c_int), ("pad", C.c_int * 2)]


EXPORT_MAP, EXPORT_MAX_IDS = 16, 12                 # export ids: CLOUD_* or EXPORT_MAP + MAP_*


class AloamMapCorrection(C.Structure):
    """One candidate map <- odometry correction (aloam_map_correction, 64 bytes)."""
    _fields_ = [("q_wmap_wodom", C.c_double * 4), ("t_wmap_wodom", C.c_double * 3), ("pad", C.c_double)]


class AloamMapScore(C.Structure):
    """What one pose counts against a bucketed target: a (sequence, candidate) pair, a node of a loop search (aloam_map_score, 32 bytes)."""
    _fields_ = [("corner_factors", C.c_int), ("surf_factors", C.c_int), ("corner_found", C.c_int), ("surf_found", C.c_int), ("cost", C.c_double), ("pad", C.c_int * 2)]


MAP_CORRECTION_DTYPE = record_dtype(AloamMapCorrection)
MAP_SCORE_DTYPE = record_dtype(AloamMapScore)


def map_corrections(q, t):
    """Candidates as the C ABI takes them: q [K, 4] (x, y, z, w) and t [K, 3] -> structured array [K] of MAP_CORRECTION_DTYPE."""
    q, t = np.asarray(q, np.float64).reshape(-1, 4), np.asarray(t, np.float64).reshape(-1, 3)
    assert len(q) == len(t)
    c = np.zeros(len(q), MAP_CORRECTION_DTYPE)
    c["q_wmap_wodom"], c["t_wmap_wodom"] = q, t
    return c


class AloamMapTile(C.Structure):
    """One cube of one class with absolute cube coordinates (aloam_map_tile, 32 bytes)."""
    _fields_ = [("cube", C.c_int * 3), ("feature_class", C.c_int), ("count", C.c_int), ("frame", C.c_int), ("first_point", C.c_longlong)]


MAP_TILE_DTYPE = record_dtype(AloamMapTile)
PLACE_RINGS, PLACE_SECTORS = 20, 60


class AloamPlace(C.Structure):
    """One stored place (aloam_place, 4880 bytes): the 60 x 20 sector-major cells of its descriptor and the tag."""
    _fields_ = [("cells", (C.c_float * 20) * 60), ("q", C.c_double * 4), ("t", C.c_double * 3), ("slot", C.c_int), ("frame", C.c_int),
                ("n_points", C.c_int), ("pad", C.c_int * 3)]


class AloamPlaceMatch(C.Structure):
    """One result of aloam_places_match (aloam_place_match, 16 bytes)."""
    _fields_ = [("entry", C.c_int), ("shift", C.c_int), ("distance", C.c_float), ("pad", C.c_int)]


PLACE_DTYPE = record_dtype(AloamPlace)
PLACE_MATCH_DTYPE = record_dtype(AloamPlaceMatch)
SEQ_RECORD_MAGIC, SEQ_RECORD_VERSION = 0x51534C41, 1
SEQ_PART_ODOMETRY, SEQ_PART_MAP = 1, 2


class AloamSeqRecordHeader(C.Structure):
    """The first 128 bytes of a sequence record (aloam_seq_record_header)."""
    _fields_ = [("magic", C.c_uint), ("version", C.c_uint), ("bytes", C.c_longlong), ("parts", C.c_int), ("n_scans", C.c_int),
                ("ring_from_field", C.c_int), ("min_range_bits", C.c_uint), ("distortion", C.c_int), ("lm_max_iterations", C.c_int),
                ("outer_iterations", C.c_int), ("sum_order", C.c_int), ("line_res_bits", C.c_uint), ("plane_res_bits", C.c_uint),
                ("inited", C.c_int), ("n_corner_last", C.c_int), ("n_surf_last", C.c_int), ("n_cubes", C.c_int * 2),
                ("map_points", C.c_int * 2), ("err_events", C.c_int), ("seq_meta_bytes", C.c_int), ("odom_bytes", C.c_int),
                ("map_seq_bytes", C.c_int), ("pad", C.c_int * 6)]


INFO_ODOMETRY, INFO_MAPPING = 0, 1
INFO_OK, INFO_NONE, INFO_NO_FACTORS, INFO_SINGULAR = 0, 1, 2, 3


class AloamPoseInformation(C.Structure):
    """The information matrix of one solve (aloam_pose_information, 1048 bytes); a-loam_amd/information.py holds the definition.  The
    header's flat row-major matrices are declared 2-D here."""
    _fields_ = [("info", (C.c_double * 6) * 6), ("eigenvalues", C.c_double * 6), ("eigenvectors", (C.c_double * 6) * 6),
                ("trans_info", (C.c_double * 3) * 3), ("trans_eigenvalues", C.c_double * 3), ("trans_eigenvectors", (C.c_double * 3) * 3),
                ("rot_info", (C.c_double * 3) * 3), ("rot_eigenvalues", C.c_double * 3), ("rot_eigenvectors", (C.c_double * 3) * 3),
                ("gradient", C.c_double * 6), ("cost", C.c_double), ("n_line", C.c_int), ("n_plane", C.c_int), ("rows", C.c_int),
                ("status", C.c_int), ("frame", C.c_int), ("pad", C.c_int * 3)]


POSE_INFORMATION_DTYPE = record_dtype(AloamPoseInformation)
GRAPH_EDGE_ROBUST = 1
GRAPH_OK, GRAPH_NO_EDGES, GRAPH_FAILED = 0, 1, 2


class AloamGraphNode(C.Structure):
    """One keyframe of a pose graph (aloam_graph_node, 128 bytes); a-loam_amd/posegraph.py holds the definitions of this section."""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("q_opt", C.c_double * 4), ("t_opt", C.c_double * 3), ("frame", C.c_int),
                ("pad", C.c_int * 3)]


class AloamGraphEdge(C.Structure):
    """One edge (aloam_graph_edge, 240 bytes): i = -1 is an anchor; info is the upper triangle, row-major."""
    _fields_ = [("seq", C.c_int), ("i", C.c_int), ("j", C.c_int), ("flags", C.c_int), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("info", C.c_double * 21)]


class AloamGraphOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("pcg_max_iterations", C.c_int), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("pcg_tolerance", C.c_double), ("huber_delta", C.c_double)]


class AloamGraphResult(C.Structure):
    """The outcome of one sequence's solve (aloam_graph_result, 64 bytes)."""
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("lm_iterations", C.c_int), ("accepted_steps", C.c_int),
                ("pcg_iterations", C.c_int), ("nodes", C.c_int), ("edges", C.c_int), ("pad", C.c_int), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("gradient_max", C.c_double), ("reserved", C.c_double)]


GRAPH_NODE_DTYPE = record_dtype(AloamGraphNode)
GRAPH_EDGE_DTYPE = record_dtype(AloamGraphEdge)
GRAPH_RESULT_DTYPE = record_dtype(AloamGraphResult)
GRAPH_POSE_ENTERED, GRAPH_POSE_OPTIMIZED = 0, 1


class AloamGraphMapRequest(C.Structure):
    """Nodes [first, first + count) of one sequence at the entered or the optimised poses (aloam_graph_map_request, 16 bytes)."""
    _fields_ = [("seq", C.c_int), ("first", C.c_int), ("count", C.c_int), ("pose", C.c_int)]


class AloamGraphMapStats(C.Structure):
    """What aloam_graph_export_map made of one request (aloam_graph_map_stats, 32 bytes)."""
    _fields_ = [("tiles", C.c_int * 2), ("points", C.c_int * 2), ("raw_points", C.c_int * 2), ("outside", C.c_int), ("written", C.c_int)]


GRAPH_MAP_REQUEST_DTYPE = record_dtype(AloamGraphMapRequest)
GRAPH_MAP_STATS_DTYPE = record_dtype(AloamGraphMapStats)
GRAPH_APPLY_POSE, GRAPH_APPLY_MAP = 1, 2
GRAPH_APPLIED, GRAPH_APPLY_NO_NODES, GRAPH_APPLY_NO_ROOM = 0, 1, 2


class AloamGraphApplyRequest(C.Structure):
    """The map of nodes [first, first + count) of one sequence carried into its live state (aloam_graph_apply_request, 16 bytes)."""
    _fields_ = [("seq", C.c_int), ("first", C.c_int), ("count", C.c_int), ("flags", C.c_int)]


class AloamGraphApplyResult(C.Structure):
    """What aloam_graph_apply did to one sequence (aloam_graph_apply_result, 104 bytes)."""
    _fields_ = [("status", C.c_int), ("nodes", C.c_int), ("cen", C.c_int * 3), ("cubes", C.c_int * 2), ("points", C.c_int * 2),
                ("raw_points", C.c_int * 2), ("outside_window", C.c_int), ("q_corr", C.c_double * 4), ("t_corr", C.c_double * 3)]


GRAPH_APPLY_REQUEST_DTYPE = record_dtype(AloamGraphApplyRequest)
GRAPH_APPLY_RESULT_DTYPE = record_dtype(AloamGraphApplyResult)
LOOP_OK, LOOP_NO_CLOUDS, LOOP_TARGET_TOO_SMALL, LOOP_TOO_LARGE, LOOP_SOLVE_FAILED = 0, 1, 2, 3, 4


class AloamGraphLoopRequest(C.Structure):
    """Node j registered against nodes [first, first + count) in the frame of node i (aloam_graph_loop_request, 96 bytes)."""
    _fields_ = [("seq", C.c_int), ("i", C.c_int), ("j", C.c_int), ("first", C.c_int), ("count", C.c_int), ("pose", C.c_int), ("pad", C.c_int * 2),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("reserved", C.c_double)]


class AloamGraphLoopOptions(C.Structure):
    _fields_ = [("outer_iterations", C.c_int), ("lm_max_iterations", C.c_int)]


class AloamGraphLoopResult(C.Structure):
    """The measured loop edge of one request (aloam_graph_loop_result, 448 bytes); a-loam_amd/loopreg.py holds the definitions."""
    _fields_ = [("status", C.c_int), ("n_line", C.c_int), ("n_plane", C.c_int), ("lm_iterations", C.c_int), ("lm_termination", C.c_int), ("pad", C.c_int),
                ("target_points", C.c_int * 2), ("target_raw", C.c_int * 2), ("source_points", C.c_int * 2), ("cost", C.c_double),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("info", C.c_double * 21), ("info_left", C.c_double * 21)]


class AloamGraphLoopSearch(C.Structure):
    """The pose grid around every request's guess (aloam_graph_loop_search, 32 bytes)."""
    _fields_ = [("radius_m", C.c_double), ("step_m", C.c_double), ("yaw_deg", C.c_double), ("yaw_step_deg", C.c_double)]


class AloamGraphLoopSearchResult(C.Structure):
    """The node a searched registration started from (aloam_graph_loop_search_result, 160 bytes); a-loam_amd/loopreg.py holds the definitions."""
    _fields_ = [("status", C.c_int), ("nodes", C.c_int), ("best", C.c_int), ("ix", C.c_int), ("iy", C.c_int), ("iyaw", C.c_int), ("pad", C.c_int * 2),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("reserved", C.c_double), ("best_score", AloamMapScore), ("guess_score", AloamMapScore)]


GRAPH_LOOP_REQUEST_DTYPE = record_dtype(AloamGraphLoopRequest)
GRAPH_LOOP_RESULT_DTYPE = record_dtype(AloamGraphLoopResult)
GRAPH_LOOP_SEARCH_DTYPE = record_dtype(AloamGraphLoopSearch)
GRAPH_LOOP_SEARCH_RESULT_DTYPE = record_dtype(AloamGraphLoopSearchResult)
GRAPH_MARGINAL_MEASURED, GRAPH_MARGINAL_AT_ESTIMATE = 0, 1
GRAPH_MARGINAL_OK, GRAPH_MARGINAL_NO_EDGES, GRAPH_MARGINAL_NOT_CONVERGED, GRAPH_MARGINAL_FAILED = 0, 1, 2, 3


class AloamGraphMarginalRequest(C.Structure):
    """A candidate edge whose residual covariance and chi-square are wanted (aloam_graph_marginal_request, 248 bytes)."""
    _fields_ = [("edge", AloamGraphEdge), ("mode", C.c_int), ("pad", C.c_int)]


class AloamGraphMarginalOptions(C.Structure):
    _fields_ = [("pcg_max_iterations", C.c_int), ("pad", C.c_int), ("pcg_tolerance", C.c_double), ("huber_delta", C.c_double)]


class AloamGraphMarginalResult(C.Structure):
    """Sigma_r, s_edge and chi2 of one request (aloam_graph_marginal_result, 440 bytes); a-loam_amd/posegraph.py marginals() holds the
    definitions.  The header's flat row-major cov is declared 6 x 6 here."""
    _fields_ = [("status", C.c_int), ("mode", C.c_int), ("seq", C.c_int), ("i", C.c_int), ("j", C.c_int), ("pcg_iterations", C.c_int), ("nodes", C.c_int),
                ("edges", C.c_int), ("chi2", C.c_double), ("s_edge", C.c_double), ("r", C.c_double * 6), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("cov", (C.c_double * 6) * 6)]


GRAPH_MARGINAL_REQUEST_DTYPE = record_dtype(AloamGraphMarginalRequest)
GRAPH_MARGINAL_RESULT_DTYPE = record_dtype(AloamGraphMarginalResult)
GRAPH_RECORD_MAGIC, GRAPH_RECORD_VERSION = 0x52474C41, 1
GRAPH_PART_GRAPH, GRAPH_PART_KEYFRAMES = 1, 2


class AloamGraphRecordHeader(C.Structure):
    """The first 128 bytes of a graph record (aloam_graph_record_header)."""
    _fields_ = [("magic", C.c_uint), ("version", C.c_uint), ("bytes", C.c_longlong), ("parts", C.c_int), ("nodes", C.c_int), ("edges", C.c_int),
                ("kf_points", C.c_int * 2), ("seq", C.c_int), ("line_res_bits", C.c_uint), ("plane_res_bits", C.c_uint), ("node_bytes", C.c_int),
                ("edge_bytes", C.c_int), ("desc_bytes", C.c_int), ("point_bytes", C.c_int), ("pad", C.c_int * 16)]


GRAPH_RECORD_HEADER_DTYPE = record_dtype(AloamGraphRecordHeader)


class AloamGraphRobustOptions(C.Structure):
    """The outer loop of aloam_graph_optimize_robust (aloam_graph_robust_options, 32 bytes)."""
    _fields_ = [("max_outer_iterations", C.c_int), ("pad", C.c_int), ("inlier_chi2", C.c_double), ("mu_step", C.c_double), ("reserved", C.c_double)]


class AloamGraphRobustResult(C.Structure):
    """The outcome of one sequence's robust solve (aloam_graph_robust_result, 128 bytes); a-loam_amd/posegraph.py optimize_robust() holds the definitions."""
    _fields_ = [("solve", AloamGraphResult), ("outer_iterations", C.c_int), ("robust_edges", C.c_int), ("inliers", C.c_int), ("outliers", C.c_int),
                ("mu", C.c_double), ("s_max", C.c_double), ("truncated_cost", C.c_double), ("reserved", C.c_double * 3)]


GRAPH_ROBUST_RESULT_DTYPE = record_dtype(AloamGraphRobustResult)
