"""Loop edges measured by registering keyframe clouds: the numpy model of aloam_graph_register_loops (include/aloam_mi355x.h, "loop edges
measured on the device").

A request (seq, i, j, first, count, pose, guess) registers the clouds of node j against a local target made of the clouds of nodes
first .. first + count - 1 of the same sequence, moved into the frame of node i, and returns the edge (i, j, Z, info):

    target_cloud(q, t, clouds, i, first, count, leaves, voxel_filter)   the two filtered target clouds, bit for bit what the device builds
    edge_information(info_left, q_z)                                     the registration's left-tangent information in the edge's tangent
    guess_from_match(...)                                                the guess of Z a place match stands for
    edge_from_result(result, seq, i, j)                                  the aloam_graph_edge of a result record
    search_grid(q_g, t_g, radius_m, step_m, yaw_deg, yaw_step_deg)       the pose grid aloam_graph_search_loops scores around a guess
    search_best(scores, centre)                                          the node it takes
    room_sample(rng, ...), sensor_cloud(world, q, t, rng)                the hand-made scene the tests and tools/loop_register_rate.py share

The registration itself (association, fits, Levenberg-Marquardt) is the mapping step's; tests/loopreg_model.py composes it from the
oracle's pieces.  Everything here is float64 numpy on the host.
"""
from __future__ import annotations

import math

import numpy as np

from . import places
from .atlas import associate_to_map
from .relocalize import grid_axes
from .posegraph import EDGE_ROBUST, MARGINAL_MEASURED, MARGINAL_REQUEST_DTYPE, compose, info_full, info_upper, inverse, make_edges, qrot, relative_pose, rotmat
from .posegraph import LINK_REQUEST_DTYPE, POSE_OPTIMIZED, make_links

LOOP_OK, LOOP_NO_CLOUDS, LOOP_TARGET_TOO_SMALL, LOOP_TOO_LARGE, LOOP_SOLVE_FAILED = 0, 1, 2, 3, 4
GATE_CORNER, GATE_SURF = 10, 50                  # the filtered targets must hold MORE points than these (src/laserMapping.cpp:554)


def target_poses(q, t, i, first, count):
    """T_k = X_i^-1 o X_k of nodes first .. first + count - 1, as the header defines a relative pose: q_d = conj(q_i) q_k,
    t_d = conj(q_i) (t_k - t_i), every operation a separately rounded f64 operation.  Node i goes through the same arithmetic."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    return [relative_pose(q[i], t[i], q[k], t[k]) for k in range(first, first + count)]


def target_cloud(q, t, clouds, i, first, count, leaves, voxel_filter):
    """The filtered target (corner, surf) of a request, in the frame of node i.  q [K, 4], t [K, 3]: the poses of the sequence's nodes
    (entered or optimised, as the request says); clouds[k] = (corner, surf): node k's sensor-frame clouds, float32 [n, 4].  Per class the
    points of the target nodes in node order, then point order, each through associate_to_map(p, T_k) (f64 rotation and translation,
    stored to f32, intensity kept); the class's whole cloud is then filtered once with voxel_filter(points, leaves[class]), the caller's
    input-order pcl::VoxelGrid."""
    poses = target_poses(q, t, i, first, count)
    out = []
    for cls in (0, 1):
        parts = [associate_to_map(clouds[first + k][cls], *poses[k]) for k in range(count) if len(clouds[first + k][cls])]
        raw = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
        out.append(np.asarray(voxel_filter(raw, leaves[cls]), np.float32).reshape(-1, 4) if len(raw) else raw)
    return out[0], out[1]


def gate(target_corner, target_surf):
    return len(target_corner) > GATE_CORNER and len(target_surf) > GATE_SURF


def edge_information(info_left, q_z):
    """The information of the edge (i, j, Z) from the registration's.  The registration's tangent is a LEFT perturbation of Z
    (q <- exp(theta / 2) q, t <- t + dt); the graph's residual r = (2 q_E.xyz, t_E), E = Z^-1 o X_i^-1 o X_j, is a RIGHT perturbation
    (q_Z <- q_Z exp(phi / 2), t_Z <- t_Z + R_Z tau).  So theta = R_Z phi, dt = R_Z tau and info = T^T info_left T with
    T = blockdiag(R_Z, R_Z).  info_left: [6, 6] or its upper triangle [21]; returns the same shape."""
    a = np.asarray(info_left, np.float64)
    full = a if a.shape[-1] == 6 else info_full(a)
    R = rotmat(np.asarray(q_z, np.float64))
    T = np.zeros((6, 6))
    T[:3, :3] = R
    T[3:, 3:] = R
    out = T.T @ (full @ T)
    out = 0.5 * (out + out.T)
    return out if a.shape[-1] == 6 else info_upper(out)


def guess_from_match(q_i, t_i, place_q, place_t, shift, odom_q, odom_t):
    """The guess of Z a place match stands for: places.guess_from_match gives the correction C that carries the sweep's odometry pose to
    the stored place's pose turned by the match's yaw shift (in the frame the nodes live in); Z = X_i^-1 o C o X_odom."""
    qc, tc = places.guess_from_match(place_q, place_t, shift, odom_q, odom_t)
    qm, tm = compose(qc, tc, np.asarray(odom_q, np.float64), np.asarray(odom_t, np.float64))
    qz, tz = relative_pose(q_i, t_i, qm, tm)
    return qz / np.linalg.norm(qz), tz


def edge_from_result(result, seq, i, j, robust=True):
    """The aloam_graph_edge (posegraph.EDGE_DTYPE, one element) of an ALOAM_LOOP_OK result record; None for every other status.  Whether
    an OK edge is a good loop is the caller's decision, from the counts, the cost and the information: hence robust by default."""
    if int(result["status"]) != LOOP_OK:
        return None
    q = np.asarray(result["q"], np.float64)
    return make_edges(seq, i, j, (q / np.linalg.norm(q))[None], np.asarray(result["t"], np.float64)[None], np.asarray(result["info"], np.float64)[None], robust)


def request_from_result(result, i, j, seq):
    """The request of aloam_graph_marginals (posegraph.MARGINAL_REQUEST_DTYPE, one element, MEASURED) for an ALOAM_LOOP_OK result record: the
    edge edge_from_result would enter, held against the graph first (its chi2 against posegraph.chi2_gate()).  None for every other status."""
    e = edge_from_result(result, seq, i, j, robust=False)
    if e is None:
        return None
    r = np.zeros(1, MARGINAL_REQUEST_DTYPE)
    r["edge"], r["mode"] = e, MARGINAL_MEASURED
    return r


def link_request(seq_i, i, first, count, seq_j, j, q, t, pose=POSE_OPTIMIZED):
    """The aloam_graph_link_request (posegraph.LINK_REQUEST_DTYPE, one element) that registers node j of seq_j against nodes
    [first, first + count) of seq_i in the frame of node i, from the guess (q, t) of Z."""
    r = np.zeros(1, LINK_REQUEST_DTYPE)
    r["seq_i"], r["i"], r["first"], r["count"], r["seq_j"], r["j"], r["pose"] = int(seq_i), int(i), int(first), int(count), int(seq_j), int(j), int(pose)
    r["q"], r["t"] = np.asarray(q, np.float64), np.asarray(t, np.float64)
    return r


def link_from_result(result, seq_i, i, seq_j, j, robust=True):
    """The aloam_graph_link (posegraph.LINK_DTYPE, one element) of an ALOAM_LOOP_OK result record of aloam_graph_register_links /
    aloam_graph_search_links; None for every other status.  Its info is the result's right-tangent `info`, which is what a link wants.
    Whether an OK link is a good one is the caller's decision: hence robust by default."""
    if int(result["status"]) != LOOP_OK:
        return None
    q = np.asarray(result["q"], np.float64)
    return make_links(seq_i, i, seq_j, j, (q / np.linalg.norm(q))[None], np.asarray(result["t"], np.float64)[None], np.asarray(result["info"], np.float64)[None], robust)


SEARCH_MAX_YAW, SEARCH_MAX_NODES = 31, 1 << 14   # yaw steps to either side, nodes of one grid (aloam_graph_search_loops)


def search_grid(q_g, t_g, radius_m, step_m, yaw_deg, yaw_step_deg):
    """The grid of aloam_graph_search_loops around the guess (q_g, t_g) of Z, the pose of node j in the frame of node i: (q [K, 4], t [K, 3],
    nodes [K, 3] int = ix, iy, iyaw).  The axes are relocalize.grid_axes; K = (2a + 1)(2m + 1)^2, yaw outermost, then y, then x, as
    relocalize.correction_grid orders them.  Node (ix, iy, iyaw) turns the guess by dyaw = iyaw * yaw_step_deg about the z axis of node i's
    frame through the guessed sensor position, then shifts it by (ix * step_m, iy * step_m, 0): q_c = dq q_g (Hamilton product, evaluated
    left to right as the device's quat_mul) with dq = (0, 0, sin h, cos h), h = (dyaw * (pi / 180)) / 2, t_c = t_g + (dx, dy, 0); every
    operation a separately rounded f64 operation.  iyaw == 0 keeps q_g itself and a zero index keeps its coordinate: the centre node is the
    guess bit for bit.  math.sin / math.cos are the C library's, which is what the host side of the call fills its table with."""
    q_g, t_g = np.asarray(q_g, np.float64), np.asarray(t_g, np.float64)
    lin, yaw = grid_axes(radius_m, step_m, yaw_deg, yaw_step_deg)
    m, a = (len(lin) - 1) // 2, (len(yaw) - 1) // 2
    if a > SEARCH_MAX_YAW or not 1 <= len(yaw) * len(lin) * len(lin) <= SEARCH_MAX_NODES:
        raise ValueError("a search grid has at most 31 yaw steps to either side and 2^14 nodes")
    step_m, yaw_step_deg = float(step_m), float(yaw_step_deg)
    qs, ts, nodes = [], [], []
    for iyaw in range(-a, a + 1):
        if iyaw == 0:
            q = q_g.copy()
        else:
            h = ((float(iyaw) * yaw_step_deg) * (math.pi / 180.0)) / 2
            d = (0.0, 0.0, math.sin(h), math.cos(h))
            b = [float(v) for v in q_g]
            q = np.array([d[3] * b[0] + d[0] * b[3] + d[1] * b[2] - d[2] * b[1],
                          d[3] * b[1] + d[1] * b[3] + d[2] * b[0] - d[0] * b[2],
                          d[3] * b[2] + d[2] * b[3] + d[0] * b[1] - d[1] * b[0],
                          d[3] * b[3] - d[0] * b[0] - d[1] * b[1] - d[2] * b[2]])
        for iy in range(-m, m + 1):
            for ix in range(-m, m + 1):
                t = t_g.copy()
                if ix != 0:
                    t[0] = t[0] + float(ix) * step_m
                if iy != 0:
                    t[1] = t[1] + float(iy) * step_m
                qs.append(q); ts.append(t); nodes.append((ix, iy, iyaw))
    return np.array(qs), np.array(ts), np.array(nodes, np.int64).reshape(-1, 3)


def search_best(scores, centre):
    """The node aloam_graph_search_loops takes: the ranking of aloam_score_map_corrections - most corner_factors + surf_factors, then the
    lower cost (NaN ranks as +infinity), then the lower index - and, when even the winner has no factor, the centre node (the guess; index
    0 is a corner of the grid).  scores: a structured array or a sequence of mappings with the fields of aloam_map_score."""
    def key(c):
        cost = float(scores[c]["cost"])
        return (-(int(scores[c]["corner_factors"]) + int(scores[c]["surf_factors"])), cost if cost == cost else math.inf, c)
    w = min(range(len(scores)), key=key)
    return w if int(scores[w]["corner_factors"]) + int(scores[w]["surf_factors"]) > 0 else int(centre)


def room_sample(rng, n_corner=300, n_surf=1500):
    """A random sample, in world coordinates (corner [n, 3], surf [m, 3], float64), of the room the loop-registration tests and
    tools/loop_register_rate.py share: a floor (x -5 .. 15, y -6 .. 6), two perpendicular walls (y = 6 and x = 15, 3 m high), four vertical
    poles and the walls' top edges; about 0.5 m between the surf samples, 0.15 m along the lines at the default sizes."""
    u = rng.uniform
    nf = (n_surf * 3) // 5
    nw = (n_surf - nf) * 5 // 8
    floor = np.stack([u(-5, 15, nf), u(-6, 6, nf), np.zeros(nf)], 1)
    w1 = np.stack([u(-5, 15, nw), np.full(nw, 6.0), u(0, 3, nw)], 1)
    w2 = np.stack([np.full(n_surf - nf - nw, 15.0), u(-6, 6, n_surf - nf - nw), u(0, 3, n_surf - nf - nw)], 1)
    surf = np.concatenate([floor, w1, w2])
    npole = n_corner // 10
    poles = [np.stack([np.full(npole, x), np.full(npole, y), u(0, 3, npole)], 1) for x, y in ((0.0, -4.0), (4.0, 3.0), (9.0, -2.0), (12.0, 4.0))]
    ne = n_corner - 4 * npole
    e1 = np.stack([u(-5, 15, ne * 5 // 8), np.full(ne * 5 // 8, 6.0), np.full(ne * 5 // 8, 3.0)], 1)
    e2 = np.stack([np.full(ne - ne * 5 // 8, 15.0), u(-6, 6, ne - ne * 5 // 8), np.full(ne - ne * 5 // 8, 3.0)], 1)
    return np.concatenate(poles + [e1, e2]), surf


def sensor_cloud(world_xyz, q, t, rng):
    """X^-1 of world points as a float32 cloud [n, 4]; the intensity is a non-decreasing ring id (0 .. 15), as a sweep's clouds have it."""
    qi, ti = inverse(np.asarray(q, np.float64), np.asarray(t, np.float64))
    p = np.zeros((len(world_xyz), 4), np.float32)
    if len(world_xyz):
        p[:, :3] = (qrot(qi, np.asarray(world_xyz, np.float64)) + ti).astype(np.float32)
        p[:, 3] = np.sort(rng.integers(0, 16, len(world_xyz)))
    return p


__all__ = ["EDGE_ROBUST", "LOOP_OK", "LOOP_NO_CLOUDS", "LOOP_TARGET_TOO_SMALL", "LOOP_TOO_LARGE", "LOOP_SOLVE_FAILED", "target_poses", "target_cloud",
           "gate", "edge_information", "guess_from_match", "edge_from_result", "search_grid", "search_best", "room_sample", "sensor_cloud"]
