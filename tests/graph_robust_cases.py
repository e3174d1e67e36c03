"""What the tests of the robust pose-graph solve share (posegraph.optimize_robust, aloam_graph_optimize_robust): the two
graphs with false loops, the model's solves of them (computed once and kept), the margin condition that makes the device's discrete
decisions the model's, and the assertions the host emulation and the GPU hold a result to.

Case A: drifted_laps(7, 60, 2), its two loops flagged, with false_loops(g, 3, 107): 18 outer iterations, weights [1, 1, 0, 0, 0]; over
all iterations no flagged s comes closer than 2.7 % to lo or hi.
Case B: drifted_laps(1, 300, 2) with false_loops(g, 6, 101): more nodes than a workgroup has threads, 14 outer iterations, weights
[1, 1, 0 x 6], closest approach 0.3 %.  Its model loop takes twelve seconds even with chain_pcg, so what the GPU test needs of it is
recorded (tests/golden/graph_robust_case_b.npy, written by `PYTHONPATH=. python tests/graph_robust_cases.py`), as posegraph_cases records scipy's
answer; test_graph_robust_model.py checks the record against the model."""
import functools
import os

import numpy as np

import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg

GOLDEN_B = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_robust_case_b.npy")
C2, MU_STEP = 22.46, 1.4
MARGIN = 1e-6                        # every flagged s stays this far (relative) from both thresholds at every outer iteration
RESULT_DTYPE = np.dtype([("solve", [("status", np.int32), ("termination", np.int32), ("lm_iterations", np.int32), ("accepted_steps", np.int32),
                                    ("pcg_iterations", np.int32), ("nodes", np.int32), ("edges", np.int32), ("pad", np.int32),
                                    ("initial_cost", np.float64), ("final_cost", np.float64), ("gradient_max", np.float64), ("reserved", np.float64)]),
                         ("outer_iterations", np.int32), ("robust_edges", np.int32), ("inliers", np.int32), ("outliers", np.int32),
                         ("mu", np.float64), ("s_max", np.float64), ("truncated_cost", np.float64), ("reserved", np.float64, 3)])


def with_false_loops(laps, n_false, seed):
    """A drifted_laps graph as a case of posegraph_cases (q, t, odom, extra, edges, ...): its loops flagged robust, then the false loops;
    `inliers` holds the edges without the false loops."""
    g = pg.drifted_laps(*laps)
    loop = g["loop"].copy()
    loop["flags"] = pg.EDGE_ROBUST
    extra = np.concatenate([loop, pg.false_loops(g, n_false, seed)])
    return dict(g, extra=extra, edges=np.concatenate([g["odom"], extra]), inliers=np.concatenate([g["odom"], loop]), n_false=n_false,
                max_nodes=len(g["q"]), max_edges=len(g["odom"]) + len(extra) + 1)


@functools.lru_cache(maxsize=None)
def case_a():
    return with_false_loops((7, 60, 2), 3, 107)


@functools.lru_cache(maxsize=None)
def case_b():
    return with_false_loops((1, 300, 2), 6, 101)


@functools.lru_cache(maxsize=None)
def clean_case():
    """drifted_laps(4, 40, 2) with its loops flagged and no false loop: GNC runs (the loops' entry residuals are large) and rejects nothing."""
    return with_false_loops((4, 40, 2), 0, 0)


def margin(trace):
    """The closest relative approach of a flagged s to lo or hi over the outer iterations of a model trace."""
    return min(min(np.abs(s["s"] - s["lo"]).min() / s["lo"], np.abs(s["s"] - s["hi"]).min() / s["hi"]) for s in trace if len(s["s"]) and s["mu"] > 0)


_MODEL = {}


def model(case, solve=None, **robust):
    """The model's robust solve of a case from its entered poses, kept: dict(q, t, res, trace, margin)."""
    key = (case["edges"].tobytes(), case["q"].tobytes(), solve is not None, tuple(sorted(robust.items())))
    if key not in _MODEL:
        trace = []
        q, t, res = pg.optimize_robust(case["q"], case["t"], case["edges"], trace=trace, solve=pg.chain_solver(OPTIONS["pcg_tolerance"], OPTIONS["pcg_max_iterations"]) if solve else None,
                                       **dict(dict(inlier_chi2=C2, mu_step=MU_STEP), **robust), **OPTIONS)
        _MODEL[key] = dict(q=q, t=t, res=res, trace=trace, margin=margin(trace) if res["mu"] > 0 else np.inf)
    return _MODEL[key]


@functools.lru_cache(maxsize=None)
def inlier_solve(name):
    """posegraph.optimize (A: dense steps; B: chain_pcg) of the case without its false loops, flags cleared: what GNC should end at."""
    case = dict(a=case_a, b=case_b)[name]()
    e = case["inliers"].copy()
    e["flags"] = 0
    q, t, res = (pg.optimize if name == "a" else pg.chain_pcg)(case["q"], case["t"], e, **OPTIONS)
    assert res["status"] == 0
    return q, t


def record_b():
    """The record of the model on case B: rows 0 .. N - 1 hold q | t; then one row (outer_iterations, inliers, outliers, s_max, mu, margin,
    0); then the weights of the flagged edges, seven to a row, padded with -1."""
    a = np.load(GOLDEN_B)
    N = len(case_b()["q"])
    head = a[N]
    w = a[N + 1:].ravel()
    return dict(q=a[:N, :4], t=a[:N, 4:], outer_iterations=int(head[0]), inliers=int(head[1]), outliers=int(head[2]), s_max=float(head[3]), mu=float(head[4]),
                margin=float(head[5]), weights=w[w >= 0])


def as_dict(res):
    """A device result (RESULT_DTYPE scalar) with the fields of `solve` at the top level, as the model's dict."""
    d = {k: res["solve"][k].item() for k in res["solve"].dtype.names}
    d.update({k: res[k].item() for k in ("outer_iterations", "robust_edges", "inliers", "outliers", "mu", "s_max", "truncated_cost")})
    return d


def check_against_model(what, case, res, weights, out, want, inlier=None):
    """A layer's robust solve of `case` from its entered poses (`res`: as_dict; `weights`: its row, one per edge; `out`: the nodes afterwards)
    against `want`, the model's (dict with q, t, outer_iterations, inliers, outliers, s_max, weights of the flagged edges), and the
    inlier-only solve: the discrete outcome exactly, s_max to 1e-9, mu recomputed from the layer's own s_max to 1e-12, the poses within
    8 eps_ref of both, final_cost against posegraph.cost at the exported poses with the final weights."""
    edges = case["edges"]
    flagged = (edges["flags"] & pg.EDGE_ROBUST) != 0
    eps = pc.eps_ref()
    dev = pg.pose_difference(out["q_opt"], out["t_opt"], want["q"], want["t"])
    dev_in = pg.pose_difference(out["q_opt"], out["t_opt"], *inlier) if inlier is not None else 0.0
    mu = C2 / (2.0 * res["s_max"] - C2) * MU_STEP ** (res["outer_iterations"] - 1)
    c = pg.cost(out["q_opt"], out["t_opt"], pg.weighted_edges(edges, weights))
    print(f"{what}: outer {res['outer_iterations']} inliers {res['inliers']} outliers {res['outliers']} weights {weights[flagged].tolist()}; LM {res['lm_iterations']} accepted "
          f"{res['accepted_steps']} PCG {res['pcg_iterations']} termination {res['termination']}; s_max {res['s_max']:.17g} (model {want['s_max']:.17g}); mu {res['mu']:.17g} "
          f"(recomputed {mu:.17g}); poses against the model {dev:.3e}, against the inlier-only solve {dev_in:.3e} (tolerance {8 * eps:.3e}); final_cost {res['final_cost']:.17g} "
          f"(posegraph.cost {c:.17g}); truncated_cost {res['truncated_cost']:.17g}")
    assert res["status"] == 0 and (res["nodes"], res["edges"], res["robust_edges"]) == (len(case["q"]), len(edges), int(flagged.sum()))
    assert (res["outer_iterations"], res["inliers"], res["outliers"]) == (want["outer_iterations"], want["inliers"], want["outliers"])
    assert weights.shape == (len(edges),) and (weights[~flagged] == 1.0).all() and weights[flagged].tolist() == list(want["weights"])
    assert abs(res["s_max"] - want["s_max"]) <= 1e-9 * want["s_max"]
    assert abs(res["mu"] - mu) <= 1e-12 * mu
    assert dev <= 8 * eps and dev_in <= 8 * eps
    assert abs(res["final_cost"] - c) <= 8 * eps * max(1.0, c)
    assert res["lm_iterations"] > 0 and res["pcg_iterations"] > 0 and res["accepted_steps"] > 0
    assert all(pc.bits_equal(out[f], v) for f, v in (("q", case["q"]), ("t", case["t"])))
    return dev


def want_of(m):
    """The model() dict as check_against_model takes it."""
    r = m["res"]
    return dict(q=m["q"], t=m["t"], outer_iterations=r["outer_iterations"], inliers=r["inliers"], outliers=r["outliers"], s_max=r["s_max"],
                weights=[tr for tr in m["trace"]][-1]["weights"].tolist())


if __name__ == "__main__":          # records the model's solve of case B
    m = model(case_b(), solve=True)
    r, w = m["res"], m["trace"][-1]["weights"]
    rows = -np.ones((-(-len(w) // 7), 7))
    rows.ravel()[:len(w)] = w
    np.save(GOLDEN_B, np.vstack([np.hstack([m["q"], m["t"]]), [r["outer_iterations"], r["inliers"], r["outliers"], r["s_max"], r["mu"], m["margin"], 0], rows]))
    print(f"{GOLDEN_B}: outer {r['outer_iterations']}, weights {w.tolist()}, margin {m['margin']:.3e}, s_max {r['s_max']:.17g}")
