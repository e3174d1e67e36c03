"""The pose-grid search of aloam_graph_search_loops as a numpy model: the grid and the ranking are a-loam_amd/loopreg.py's (search_grid,
search_best), a node's score is relocalize_model.score_one at the node's pose taken as `parameters` directly (a slot has no odometry
frame), and the registration that follows is loopreg_model.register started from the best node.  score_one applies the gate itself."""
import importlib

import numpy as np

import loopreg_model
import relocalize_model

KEYS = ("corner_factors", "surf_factors", "corner_found", "surf_found", "cost")
DEFAULT_GRID = (3.0, 0.5, 12.5, 2.5)               # aloam_graph_loop_default_search


def _loopreg():
    return importlib.import_module("a-loam_amd.loopreg")


def _clouds(src_corner, src_surf, tgt_corner, tgt_surf):
    return (np.asarray(src_corner, np.float32).reshape(-1, 4), np.asarray(src_surf, np.float32).reshape(-1, 4),
            np.ascontiguousarray(tgt_corner, np.float32), np.ascontiguousarray(tgt_surf, np.float32))


def score_nodes(src_corner, src_surf, tgt_corner, tgt_surf, q, t, only=None):
    """The aloam_map_score of every node (q [K, 4], t [K, 3]) as a list of dicts; `only`: the node indices to score (the others are None)."""
    sc, ss, tc, ts = _clouds(src_corner, src_surf, tgt_corner, tgt_surf)
    out = [None] * len(q)
    for c in (range(len(q)) if only is None else only):
        out[c] = dict(zip(KEYS, relocalize_model.score_one(sc, ss, tc, ts, np.concatenate([q[c], t[c]]))))
    return out


def node_bounds(src_corner, src_surf, tgt_corner, tgt_surf, q, t):
    """(lower, upper) of corner_factors + surf_factors of every node, from relocalize_model.factor_bounds (numpy's batched fits): [K, 2]."""
    sc, ss, tc, ts = _clouds(src_corner, src_surf, tgt_corner, tgt_surf)
    if not _loopreg().gate(tc, ts):
        return np.zeros((len(q), 2), np.int64)
    return np.array([relocalize_model.factor_bounds(sc, ss, tc, ts, np.concatenate([q[c], t[c]]))[:2] for c in range(len(q))], np.int64).reshape(-1, 2)


def best_node(src_corner, src_surf, tgt_corner, tgt_surf, q, t, centre):
    """loopreg.search_best(score_nodes(...), centre) without fitting every node, in the manner of relocalize_model.best_model: only the
    nodes whose upper bound reaches the largest lower bound can win, and only those go through score_one.  The nodes are visited in
    descending order of the points found for every 8th source point, so that the largest lower bound is met early (the order changes the
    work, not the result).  When no node can have a factor the centre node is taken.  Returns (index, its score, nodes fitted exactly)."""
    sc, ss, tc, ts = _clouds(src_corner, src_surf, tgt_corner, tgt_surf)
    pars = [np.concatenate([q[c], t[c]]) for c in range(len(q))]
    score = lambda c: dict(zip(KEYS, relocalize_model.score_one(sc, ss, tc, ts, pars[c])))
    if not _loopreg().gate(tc, ts):
        return int(centre), score(centre), 1
    rough = [len(relocalize_model._neighbours(sc[::8], tc, p)) + len(relocalize_model._neighbours(ss[::8], ts, p)) for p in pars]
    floor, upper = 0, {}
    for c in sorted(range(len(pars)), key=lambda c: (-rough[c], c)):
        lo, upper[c], _ = relocalize_model.factor_bounds(sc, ss, tc, ts, pars[c], floor)
        floor = max(floor, lo)
    alive = sorted(c for c, hi in upper.items() if hi >= max(floor, 1))
    if not alive:
        return int(centre), score(centre), 1
    scores = [score(c) for c in alive]
    w = relocalize_model.best_of(scores)
    if scores[w]["corner_factors"] + scores[w]["surf_factors"] == 0:
        return int(centre), score(centre), len(alive) + 1
    return alive[w], scores[w], len(alive)


def far_guess(fx, shift, dyaw_deg):
    """The truth of the fixture's request turned by quat_z(dyaw) and shifted: a guess well outside the registration's basin."""
    P = importlib.import_module("a-loam_amd.posegraph")
    (_, _), (qt, tt) = loopreg_model.request_of(fx)
    q = P.qmul(loopreg_model.quat_z(np.radians(dyaw_deg)), qt)
    return q / np.linalg.norm(q), np.asarray(tt, np.float64) + np.asarray(shift, np.float64)


FAR_GUESSES = (((2.2, -1.6, 0.08), 11.0), ((-2.7, 2.3, -0.05), -9.0))
