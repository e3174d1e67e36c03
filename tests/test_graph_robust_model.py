"""posegraph.optimize_robust, the numpy definition of aloam_graph_optimize_robust (no GPU): GNC-TLS on the graphs with false loops of
graph_robust_cases.py ends at the solve of the inlier edges alone where Huber does not; the margin condition the device tests rest on; the
paths of the definition (a clean graph, the skip branch, an empty R, a non-finite edge, the cap); the weight formula at its two ends; and
the record of case B against the model."""
import numpy as np
import pytest

import graph_robust_cases as rc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg


def test_false_loops_is_seeded_and_flagged():
    g = pg.drifted_laps(7, 60, 2)
    f = pg.false_loops(g, 3, 107)
    assert f.dtype == pg.EDGE_DTYPE and len(f) == 3 and (f["flags"] == pg.EDGE_ROBUST).all() and f.tobytes() == pg.false_loops(g, 3, 107).tobytes()
    assert (f["i"] >= 0).all() and (f["i"] < 30).all() and (f["j"] - f["i"] >= 15).all() and (f["j"] - f["i"] < 30).all() and (f["j"] < 60).all()
    assert pc.bits_equal(f["info"], np.tile(pg.info_upper(g["info"]), (3, 1)))
    zq, zt = pg.relative_pose(g["q_true"][f["i"]], g["t_true"][f["i"]], g["q_true"][f["j"]], g["t_true"][f["j"]])
    off = np.abs(f["t"] - zt)
    assert off.max() <= 8.0 and np.linalg.norm(f["t"] - zt, axis=1).min() > 1.0 and np.abs(np.linalg.norm(f["q"], axis=1) - 1).max() < 1e-15
    assert len(pg.false_loops(g, 0, 1)) == 0


def test_case_a_rejects_the_false_loops_where_huber_is_pulled_away():
    case = rc.case_a()
    m = rc.model(case)
    res, flagged = m["res"], case["edges"]["flags"] != 0
    qi, ti = rc.inlier_solve("a")
    dev = pg.pose_difference(m["q"], m["t"], qi, ti)
    qh, th, _ = pg.optimize(case["q"], case["t"], case["edges"], **OPTIONS)
    huber = float(np.linalg.norm(th - ti, axis=1).max())
    print(f"case A: outer {res['outer_iterations']}, weights {res['weights'][flagged].tolist()}, margin {m['margin']:.3e}; against the inlier-only solve {dev:.3e} "
          f"(tolerance {8 * pc.eps_ref():.3e}); the Huber solve ends {huber:.2f} m from it; ATE robust {pg.ate(m['t'], case['t_true']):.2f} m, Huber {pg.ate(th, case['t_true']):.2f} m")
    assert res["status"] == 0 and res["outer_iterations"] == 18 and res["weights"][flagged].tolist() == [1, 1, 0, 0, 0] and (res["weights"][~flagged] == 1).all()
    assert (res["robust_edges"], res["inliers"], res["outliers"]) == (5, 2, 3)
    assert m["margin"] >= rc.MARGIN and m["margin"] > 0.02                   # 2.7 %: the device's discrete decisions must be the model's
    assert dev <= 8 * pc.eps_ref()
    assert huber > 1.0                                                       # the fixture bites
    assert abs(res["mu"] - rc.C2 / (2 * res["s_max"] - rc.C2) * rc.MU_STEP ** 17) <= 1e-12 * res["mu"]
    assert abs(res["final_cost"] - pg.cost(m["q"], m["t"], pg.weighted_edges(case["edges"], res["weights"]))) <= 1e-9 * res["final_cost"]
    s = pg.edge_chi2(m["q"], m["t"], case["edges"])
    assert abs(res["truncated_cost"] - 0.5 * (s[~flagged].sum() + np.minimum(s[flagged], rc.C2).sum())) <= 1e-12 * res["truncated_cost"]
    assert abs(res["initial_cost"] - 0.5 * pg.edge_chi2(case["q"], case["t"], case["edges"]).sum()) <= 1e-12 * res["initial_cost"]
    assert res["lm_iterations"] == sum(tr["solve"]["lm_iterations"] for tr in m["trace"]) and res["termination"] == m["trace"][-1]["solve"]["termination"]
    assert [tr["mu"] for tr in m["trace"]] == sorted(tr["mu"] for tr in m["trace"]) and len(m["trace"]) == 18


def test_the_record_of_case_b_is_the_models():
    """Case B by chain_pcg, as recorded for the GPU test: 14 outer iterations, weights [1, 1, 0 x 6], margin 0.3 %."""
    case, rec = rc.case_b(), rc.record_b()
    m = rc.model(case, solve=True)
    assert (rec["outer_iterations"], rec["inliers"], rec["outliers"]) == (m["res"]["outer_iterations"], m["res"]["inliers"], m["res"]["outliers"]) == (14, 2, 6)
    assert rec["weights"].tolist() == m["trace"][-1]["weights"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert rec["s_max"] == m["res"]["s_max"] and abs(rec["mu"] - m["res"]["mu"]) <= 1e-15 and rec["margin"] == m["margin"] >= 1e-3
    assert pg.pose_difference(rec["q"], rec["t"], m["q"], m["t"]) <= 1e-12
    assert pg.pose_difference(m["q"], m["t"], *rc.inlier_solve("b")) <= 8 * pc.eps_ref()


def test_a_clean_graph_keeps_every_edge():
    case = rc.clean_case()
    m = rc.model(case)
    plain = case["edges"].copy(); plain["flags"] = 0
    q, t, _ = pg.optimize(case["q"], case["t"], plain, **OPTIONS)
    assert m["res"]["status"] == 0 and (m["res"]["weights"] == 1).all() and (m["res"]["inliers"], m["res"]["outliers"]) == (2, 0)
    assert m["res"]["outer_iterations"] > 1 and m["res"]["mu"] > 0           # GNC ran: the loops' entry residuals are far beyond c2
    assert pg.pose_difference(m["q"], m["t"], q, t) <= 8 * pc.eps_ref()


def test_skip_empty_failure_and_cap():
    case = rc.clean_case()
    flagged = case["edges"]["flags"] != 0
    s = pg.edge_chi2(case["q"], case["t"], case["edges"])[flagged]
    plain = case["edges"].copy(); plain["flags"] = 0
    q0, t0, r0 = pg.optimize(case["q"], case["t"], plain, **OPTIONS)
    # the skip branch: 2 s_max - c2 <= 0
    q, t, res = pg.optimize_robust(case["q"], case["t"], case["edges"], inlier_chi2=2.0 * s.max(), **OPTIONS)
    assert (res["status"], res["outer_iterations"], res["mu"], res["inliers"], res["outliers"], res["s_max"]) == (0, 1, 0.0, 2, 0, s.max())
    assert pc.bits_equal(q, q0) and pc.bits_equal(t, t0) and res["lm_iterations"] == r0["lm_iterations"] and res["final_cost"] == r0["final_cost"]
    # an empty R
    q, t, res = pg.optimize_robust(case["q"], case["t"], plain, **OPTIONS)
    assert (res["status"], res["outer_iterations"], res["mu"], res["robust_edges"]) == (0, 1, 0.0, 0) and pc.bits_equal(q, q0) and pc.bits_equal(t, t0)
    # a non-finite flagged edge
    _, bad = pc.failing_case()
    edges = bad["edges"].copy(); edges["flags"][-1] = pg.EDGE_ROBUST
    q, t, res = pg.optimize_robust(bad["q"], bad["t"], edges, **OPTIONS)
    assert (res["status"], res["termination"], res["outer_iterations"]) == (2, 5, 0) and pc.bits_equal(q, bad["q"]) and pc.bits_equal(t, bad["t"]) and (res["weights"] == 1).all()
    # no nodes to solve
    assert pg.optimize_robust(case["q"][:1], case["t"][:1], plain[:0])[2]["status"] == 1
    # the cap
    a = rc.case_a()
    m = rc.model(a, max_outer_iterations=2)
    w = m["res"]["weights"][a["edges"]["flags"] != 0]
    assert m["res"]["outer_iterations"] == 2 and ((w > 0) & (w < 1)).any() and m["res"]["inliers"] + m["res"]["outliers"] < m["res"]["robust_edges"]


@pytest.mark.parametrize("mu", [1e-3, 0.05, 1.0, 40.0])
def test_the_weight_formula_is_continuous_at_lo_and_hi(mu):
    c2 = rc.C2
    lo, hi = pg.gnc_thresholds(mu, c2)
    assert lo < c2 < hi and abs(lo * hi - c2 * c2) <= 1e-12 * c2 * c2
    for s, w in ((lo, 1.0), (hi, 0.0)):
        inside = pg.gnc_weights(np.array([s * (1 - 1e-9), s, s * (1 + 1e-9)]), mu, c2)
        mid = np.sqrt(c2 * mu * (mu + 1.0) / s) - mu                        # the middle branch evaluated at the threshold itself
        assert abs(mid - w) <= 1e-12 * (1 + mu) and np.abs(inside - w).max() <= 1e-8 * (1 + mu)
    w = pg.gnc_weights(np.linspace(lo, hi, 101), mu, c2)
    assert (np.diff(w) <= 0).all() and w[0] == 1.0 and w[-1] == 0.0 and (w[1:-1] > 0).all() and (w[1:-1] < 1).all()
    assert pg.gnc_weights(np.array([0.0, np.inf]), mu, c2).tolist() == [1.0, 0.0]
