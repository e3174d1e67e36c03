"""posegraph.propose_links, posegraph.frame_from_link, loopreg.link_request and loopreg.link_from_result (no GPU): the numpy definitions the
device is held against in tests/test_gpu_graph_links.py.  The new proposal is tied to the old one: over the nodes a loop proposal may take,
it selects the same nodes with the same bits."""
import importlib

import numpy as np
import pytest

import graph_joint_cases as jc
import graph_propose_cases as gc

pg = importlib.import_module("a-loam_amd.posegraph")
lr = importlib.import_module("a-loam_amd.loopreg")


@pytest.mark.parametrize("case", [c for c in gc.CASES if c["params"]["growth_m_per_node"] == 0.0], ids=lambda c: c["name"])
def test_with_no_frame_it_is_the_loop_proposal_over_the_eligible_nodes(case):
    """frame = None and seq_i's nodes = nodes 0 .. j - min_gap of the one chain: the same (i, d2) as propose_loops with no growth term, bit for
    bit in dist2 and in the guess.  (The windows differ by design: a link's is clamped at the top.)"""
    p = case["params"]
    q, t = gc.poses(gc.GRAPHS[case["graph"]], case["pose"])
    j, eligible = case["j"], max(0, case["j"] - p["min_gap"] + 1)
    old, n_old, d_old = pg.propose_loops(q, t, j, seq=0, pose=case["pose"], **p)
    new, n_new, d_new = pg.propose_links(q[:eligible], t[:eligible], q, t, j, None, p["radius_m"], p["half_window"], p["separation"], p["K"], pose=case["pose"])
    assert n_new == n_old and d_new.tobytes() == d_old.tobytes()
    for f in ("i", "j", "first", "pose", "q", "t"):
        assert new[f].tobytes() == old[f].tobytes(), f
    assert (new["count"][:n_new] == np.minimum(old["i"][:n_old] + p["half_window"], eligible - 1) - old["first"][:n_old] + 1).all()
    assert (new["seq_i"][:n_new] == 0).all() and (new["seq_j"][:n_new] == 1).all() and not new[n_new:].tobytes().strip(b"\0")
    if case["expect"] is not None:
        assert new["i"][:n_new].tolist() == case["expect"]


def test_moving_the_session_and_passing_the_frame_selects_the_same_nodes():
    g = gc.GRAPHS["laps1"]
    A = (pg.stored_q(jc.FRAME[0]), np.array(jc.FRAME[1]))
    qa, ta = pg.compose(*pg.inverse(*A), g["q"], g["t"])
    assert np.abs(ta - g["t"]).max() > 50.0
    for j in gc.LAPS_QUERIES:
        home = pg.propose_links(g["q"], g["t"], g["q"], g["t"], j, None, 3.0, 3, 6, 4)
        away = pg.propose_links(g["q"], g["t"], qa, ta, j, A, 3.0, 3, 6, 4)
        flat = pg.propose_links(g["q"], g["t"], qa, ta, j, np.concatenate(A), 3.0, 3, 6, 4)
        assert home[1] == away[1] >= 2 and home[0]["i"].tolist() == away[0]["i"].tolist() and home[0]["count"].tolist() == away[0]["count"].tolist()
        assert np.abs(home[0]["q"] - away[0]["q"]).max() < 1e-12 and np.abs(home[0]["t"] - away[0]["t"]).max() < 1e-9 and np.abs(home[2] - away[2]).max() < 1e-9
        assert away[0].tobytes() == flat[0].tobytes()
        assert pg.propose_links(g["q"], g["t"], qa, ta, j, None, 3.0, 3, 6, 4)[1] == 0     # without the frame the session is 100 m away


def test_the_window_is_clamped_at_both_ends():
    t = np.zeros((21, 3))
    t[:, 0] = 10.0 * np.arange(21)
    q = np.tile([0.0, 0.0, 0.0, 1.0], (21, 1))
    tj = np.array([[200.0, 1.0, 0.0], [0.0, 1.0, 0.0], [100.0, 1.0, 0.0]])
    qj = q[:3]
    for j, (i, first, count) in enumerate(((20, 16, 5), (0, 0, 5), (10, 6, 9))):
        req, n, d2 = pg.propose_links(q, t, qj, tj, j, None, 2.0, 4, 0, 2, seq_i=3, seq_j=5, pose=pg.POSE_ENTERED)
        r = req[0]
        assert n == 1 and (int(r["seq_i"]), int(r["i"]), int(r["first"]), int(r["count"]), int(r["seq_j"]), int(r["j"]), int(r["pose"])) == (3, i, first, count, 5, j, 0)
        assert d2[0] == 1.0 and r["t"].tolist() == [0.0, 1.0, 0.0] and int(r["pad"]) == 0 and r["reserved"] == 0.0
    one = pg.propose_links(q[:1], t[:1], qj, tj, 1, None, 2.0, 100, 0, 1)[0][0]
    assert (int(one["first"]), int(one["count"])) == (0, 1)


def test_frame_from_link_is_the_alignment_of_a_joined_member():
    g = pg.drifted_laps(4, 30, 0)
    d = pg.cut_drive(g, 12, jc.FRAME)
    (n0, e0), (n1, e1) = d["members"]
    link = d["links"][0]
    i, j = int(link["i"]), int(link["j"])
    A = pg.frame_from_link(n0["q_opt"][i], n0["t_opt"][i], link, n1["q_opt"][j], n1["t_opt"][j])
    _, _, (qa, ta) = pg.align_member(n1, e1, n0["q_opt"][i], n0["t_opt"][i], link, j, False)
    assert A[0].tobytes() == qa.tobytes() and A[1].tobytes() == ta.tobytes()
    assert n1["q_opt"].tobytes() == d["members"][1][0]["q_opt"].tobytes()             # no side effects
    # A undoes the frame F the second session was cut into.  The link is the cut odometry edge, and drifted_laps builds its chain as
    # X[k] = X[k - 1] o Z_k, so X_i o Z is X[c] but for rounding and A o F is the identity but for rounding: four quaternion products (a few
    # eps = 2.2e-16 each) and about ten rounded vector operations on coordinates of up to |t_F| + radius = 110 m (half an ulp, 7e-15 m, per
    # term, three terms per sum; each product's error turned by a 110 m lever into 1e-13 m) add up to below 1e-12 m.  Bounds: ten times that.
    back = pg.compose(*A, *jc.FRAME)
    assert (i, j) == (11, 0) and np.abs(back[1]).max() < 1e-11 and np.abs(back[0][:3]).max() < 1e-14 and abs(abs(back[0][3]) - 1.0) < 1e-14


def test_link_request_and_link_from_result_round_trip(binding):
    q, t = pg.qexp(np.array([0.1, -0.2, 0.3])), np.array([1.0, 2.0, 3.0])
    r = lr.link_request(2, 7, 4, 6, 0, 31, q, t, pose=pg.POSE_ENTERED)
    assert r.dtype == binding.GRAPH_LINK_REQUEST_DTYPE and r.shape == (1,)
    assert (int(r["seq_i"][0]), int(r["i"][0]), int(r["first"][0]), int(r["count"][0]), int(r["seq_j"][0]), int(r["j"][0]), int(r["pose"][0])) == (2, 7, 4, 6, 0, 31, 0)
    assert r["q"][0].tolist() == q.tolist() and r["t"][0].tolist() == t.tolist() and int(r["pad"][0]) == 0 and r["reserved"][0] == 0.0
    assert lr.link_request(0, 1, 0, 2, 1, 0, q, t)["pose"][0] == pg.POSE_OPTIMIZED
    assert binding.Aloam.graph_link_requests([(2, 7, 4, 6, 0, 31, 0, q, t)]).tobytes() == r.tobytes()
    res = np.zeros(1, binding.GRAPH_LOOP_RESULT_DTYPE)[0]
    res["status"], res["q"], res["t"] = lr.LOOP_OK, q * (1 + 1e-9), t
    res["info"], res["info_left"] = np.arange(21) + 1.0, np.arange(21) + 100.0
    link = lr.link_from_result(res, 2, 7, 0, 31)
    assert link.dtype == pg.LINK_DTYPE and link.shape == (1,)
    l = link[0]
    assert (int(l["seq_i"]), int(l["i"]), int(l["seq_j"]), int(l["j"]), int(l["flags"])) == (2, 7, 0, 31, pg.EDGE_ROBUST)
    assert l["info"].tolist() == res["info"].tolist() and l["t"].tolist() == t.tolist()      # the right-tangent information, not info_left
    assert abs(np.linalg.norm(l["q"]) - 1.0) < 1e-15 and np.abs(l["q"] - q).max() < 1e-8
    assert int(lr.link_from_result(res, 2, 7, 0, 31, robust=False)["flags"][0]) == 0
    for status in (lr.LOOP_NO_CLOUDS, lr.LOOP_TARGET_TOO_SMALL, lr.LOOP_TOO_LARGE, lr.LOOP_SOLVE_FAILED):
        res["status"] = status
        assert lr.link_from_result(res, 2, 7, 0, 31) is None
