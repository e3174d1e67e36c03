"""posegraph.propose_loops / posegraph.unclosed, the numpy definition of aloam_graph_propose_loops (no GPU): against a restatement written
here (sort every hit by (d2, i), then filter greedily), on every constructed case of graph_propose_cases.py; the records against what
aloam_graph_register_loops asks of a request; the guess against posegraph.relative_pose, bit for bit."""
import numpy as np
import pytest

import graph_propose_cases as gc
from graph_propose_cases import pg

IDS = [c["name"] for c in gc.CASES]


def restated(t, j, radius_m, growth_m_per_node, min_gap, half_window, separation, K):
    """[(i, d2), ...] of the nodes taken: all hits sorted by (d2, i), then one pass that keeps a hit when no kept one lies within `separation`."""
    hits = []
    for i in range(0, j - min_gap + 1):
        dx, dy, dz = (np.float64(a) - np.float64(b) for a, b in zip(t[i], t[j]))
        d2 = (dx * dx + dy * dy) + dz * dz
        r = np.float64(j - i) * np.float64(growth_m_per_node) + np.float64(radius_m)
        if d2 <= r * r:
            hits.append((float(d2), i))
    kept = []
    for d2, i in sorted(hits):
        if len(kept) < K and all(abs(i - k) > separation for k, _ in kept):
            kept.append((i, d2))
    return kept


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_the_model_against_the_restatement(c):
    nodes = gc.GRAPHS[c["graph"]]
    q, t = gc.poses(nodes, c["pose"])
    req, count, dist2 = gc.model(c, seq=3)
    want = restated(t, c["j"], **c["params"])
    K, hw = c["params"]["K"], c["params"]["half_window"]
    assert count == len(want) and req.dtype == pg.LOOP_REQUEST_DTYPE and req.shape == (K,) and dist2.shape == (K,)
    assert req["i"][:count].tolist() == [i for i, _ in want] and dist2[:count].tobytes() == np.array([d for _, d in want], np.float64).tobytes()
    if c["expect"] is not None:
        assert req["i"][:count].tolist() == c["expect"]
    assert req[count:].tobytes() == bytes(req.itemsize * (K - count)) and dist2[count:].tobytes() == bytes(8 * (K - count))
    for r in req[:count]:
        i, j = int(r["i"]), int(r["j"])
        assert (int(r["seq"]), j, int(r["pose"])) == (3, c["j"], c["pose"]) and not r["pad"].any() and r["reserved"] == 0.0
        # what aloam_graph_register_loops asks of a request
        assert r["first"] == max(0, i - hw) and r["first"] <= i < r["first"] + r["count"] and r["first"] + r["count"] - 1 == i + hw
        assert not (r["first"] <= j < r["first"] + r["count"]) and r["first"] >= 0 and r["first"] + r["count"] <= len(nodes)
        assert abs(np.linalg.norm(r["q"]) - 1.0) <= 1e-6 and np.isfinite(r["t"]).all()
        qd, td = pg.relative_pose(q[i], t[i], q[j], t[j])
        assert r["q"].tobytes() == qd.tobytes() and r["t"].tobytes() == td.tobytes()


def test_the_two_poses_give_different_answers():
    a, b = (gc.model(c) for c in gc.CASES if c["graph"] == "estimates")
    assert a[1] == b[1] == 2 and a[0]["i"][:2].tolist() != b[0]["i"][:2].tolist()
    assert a[0]["q"][1].tobytes() != b[0]["q"][0].tobytes()                       # node 4 under the entered poses and under the estimates


def test_the_laps_take_one_node_per_earlier_pass():
    """A lap has 40 nodes: the nodes taken lie whole laps behind j (to the few nodes the drift shifts them by), each in a lap of its own."""
    for c in gc.CASES:
        if c["graph"].startswith("laps"):
            req, count, _ = gc.model(c)
            back = (c["j"] - req["i"][:count]) / 40.0
            assert count >= 1 and np.abs(back - np.round(back)).max() <= 0.1 and len(set(np.round(back).tolist())) == count, (c["name"], req["i"][:count])


def test_unclosed_drops_what_lies_next_to_an_edge():
    req = np.zeros(4, pg.LOOP_REQUEST_DTYPE)
    req["i"], req["j"] = [10, 50, 90, 10], [200, 200, 200, 300]
    edges = pg.make_edges(0, np.array([12, 88, 10]), np.array([203, 204, 250]), np.tile([0.0, 0, 0, 1], (3, 1)), np.zeros((3, 3)), np.eye(6))
    assert pg.unclosed(req, edges, 3)["i"].tolist() == [50, 90, 10] and pg.unclosed(req, edges, 3)["j"].tolist() == [200, 200, 300]
    assert pg.unclosed(req, edges, 4)["i"].tolist() == [50, 10]
    assert pg.unclosed(req, edges, 50)["i"].tolist() == []
    assert pg.unclosed(req, edges[:0], 3).tobytes() == req.tobytes() and pg.unclosed(req, [(10, 300)], 0)["j"].tolist() == [200, 200, 200]
