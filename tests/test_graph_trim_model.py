"""posegraph.trim / graph_records.trim_keyframes, the numpy definition of aloam_graph_trim (no GPU): the classification of every (i, j)
against a restatement written here, the stable order, bit copies where the definition says copy, the residual of an anchored edge against
the original's on the full graph, trim(trim(g, a), b) == trim(g, a + b), and the request checks of the proposal on a trimmed graph."""
import numpy as np
import pytest

import graph_trim_cases as tc
from graph_trim_cases import gr, pg

EPS = np.finfo(np.float64).eps


def restated(i, j, f):
    """The header's five rules, read one after the other."""
    if j > f and (i >= f or i == -1):
        return pg.TRIM_KEPT
    if j > f and 0 <= i < f:
        return pg.TRIM_ANCHORED
    if i > f and j == f:
        return pg.TRIM_KEPT_ON_FIRST
    if i > f and 0 <= j < f:
        return pg.TRIM_REVERSE
    return pg.TRIM_FIXED


@pytest.mark.parametrize("n,f", [(12, 1), (12, 5), (12, 10), (3, 1)])
def test_every_pair_of_endpoints_is_classified_as_the_header_says(n, f):
    ends = sorted({-1, 0, f - 1, f, f + 1, n - 1} & set(range(-1, n)))
    pairs = [(i, j) for i in ends for j in ends if j >= 0 and i != j]
    i, j = np.array(pairs).T
    code = pg.trim_classes(i, j, f)
    assert code.tolist() == [restated(a, b, f) for a, b in pairs]
    nodes = tc.random_nodes(1, n)
    edges = tc.random_edges(2, i, j)
    n2, e2, stats = pg.trim(nodes, edges, f)
    keep = code <= pg.TRIM_KEPT_ON_FIRST
    assert stats.tolist() == [n - f, int(keep.sum()), int((code == pg.TRIM_ANCHORED).sum()), int((code == pg.TRIM_FIXED).sum()), int((code == pg.TRIM_REVERSE).sum())]
    assert len(e2) == keep.sum() and (e2["j"] >= 0).all() and (e2["j"] < n - f).all() and (e2["i"] >= -1).all() and (e2["i"] < n - f).all() and (e2["i"] != e2["j"]).all()
    assert (e2["j"] == j[keep] - f).all()
    assert (e2["i"] == np.where((code[keep] == pg.TRIM_ANCHORED) | (i[keep] < 0), -1, i[keep] - f)).all()


@pytest.mark.parametrize("pattern", tc.PATTERNS)
def test_the_patterns_are_valid_edges_of_the_classes_they_name(pattern):
    n, f = tc.N_EDGE_GRAPH, tc.F_EDGE_GRAPH
    for count in tc.EDGE_COUNTS:
        i, j = tc.pattern_pairs(pattern, count, n, f)
        assert len(i) == count and ((i >= -1) & (i < n) & (j >= 0) & (j < n) & (i != j)).all(), (pattern, count)
    code = set(pg.trim_classes(*tc.pattern_pairs(pattern, 600, n, f), f).tolist())
    want = {"kept": {0, 2}, "removed": {4}, "alternating": {0, 1, 4}, "robust": {0, 1, 4}, "reverse": {0, 2, 3}, "anchors": {0, 4}, "endpoints": {0, 1, 2, 3, 4}}[pattern]
    assert code == want, (pattern, code)


@pytest.mark.parametrize("pattern", tc.PATTERNS)
def test_stable_order_and_bit_copies(pattern):
    nodes, edges, f = tc.edge_case(pattern, 257)
    edges["info"][:, 0] = np.arange(len(edges))                       # a serial number that the trim must carry along
    n2, e2, stats = pg.trim(nodes, edges, f)
    assert n2.tobytes() == nodes[f:].tobytes() and n2 is not nodes
    serial = e2["info"][:, 0].astype(int)
    assert (np.diff(serial) > 0).all()                                 # the stored order
    src = edges[serial]
    code = pg.trim_classes(src["i"], src["j"], f)
    assert set(code.tolist()) <= {pg.TRIM_KEPT, pg.TRIM_ANCHORED, pg.TRIM_KEPT_ON_FIRST} and len(e2) == (pg.trim_classes(edges["i"], edges["j"], f) <= 2).sum()
    for field in ("seq", "flags", "info"):
        assert e2[field].tobytes() == src[field].tobytes(), field
    plain = code != pg.TRIM_ANCHORED
    assert e2["q"][plain].tobytes() == src["q"][plain].tobytes() and e2["t"][plain].tobytes() == src["t"][plain].tobytes()
    a = ~plain
    if a.any():
        q, t = pg.compose(nodes["q_opt"][src["i"][a]], nodes["t_opt"][src["i"][a]], src["q"][a], src["t"][a])
        assert e2["q"][a].tobytes() == q.tobytes() and e2["t"][a].tobytes() == t.tobytes()        # as computed, not renormalised
    if pattern == "robust":
        assert 0 < (e2["flags"] == pg.EDGE_ROBUST).sum() < len(e2)


def test_first_zero_changes_nothing():
    nodes, edges, _ = tc.edge_case("endpoints", 60)
    n2, e2, stats = pg.trim(nodes, edges, 0)
    assert n2.tobytes() == nodes.tobytes() and e2.tobytes() == edges.tobytes() and stats.tolist() == [len(nodes), 60, 0, 0, 0]
    with pytest.raises(AssertionError):
        pg.trim(nodes, edges, len(nodes))
    with pytest.raises(AssertionError):
        pg.trim(nodes, edges, -1)


@pytest.fixture(scope="module")
def solved():
    g = pg.drifted_laps(5, 48, 9)
    edges = np.concatenate([g["odom"], g["loop"], pg.false_loops(g, 2, 3)])
    q, t, res = pg.optimize(g["q"], g["t"], edges)
    assert res["status"] == 0
    nodes = np.zeros(len(q), pg.NODE_DTYPE)
    nodes["q"], nodes["t"], nodes["q_opt"], nodes["t_opt"] = g["q"], g["t"], q, t
    return nodes, edges


@pytest.mark.parametrize("f", [1, 7, 17, 30, 46])
def test_an_anchored_edge_keeps_its_residual(solved, f):
    """The kept nodes are perturbed; the dropped ones stay at their estimates.  E = Z'^-1 o X_j with Z' = X_i o Z against
    Z^-1 o X_i^-1 o X_j: the same pose composed in another order, a handful of roundings on components of size max(1, |t|)."""
    nodes, edges = solved
    rng = np.random.default_rng(f)
    moved = nodes.copy()
    dq, dt = pg.qexp(0.05 * rng.standard_normal((len(nodes) - f, 3))), 0.3 * rng.standard_normal((len(nodes) - f, 3))
    moved["q_opt"][f:], moved["t_opt"][f:] = pg.qmul(dq, nodes["q_opt"][f:]), nodes["t_opt"][f:] + dt
    n2, e2, stats = pg.trim(moved, edges, f)
    code = pg.trim_classes(edges["i"], edges["j"], f)
    anchored_new = (e2["i"] == -1)
    anchored_old = code == pg.TRIM_ANCHORED
    assert stats[2] == anchored_old.sum() == anchored_new.sum() > 0
    r_old = pg.residual(moved["q_opt"], moved["t_opt"], edges[anchored_old])
    r_new = pg.residual(n2["q_opt"], n2["t_opt"], e2[anchored_new])
    bound = 64 * EPS * max(1.0, np.abs(moved["t_opt"]).max())
    worst = np.abs(r_new - r_old).max()
    print("f", f, "anchored", int(anchored_old.sum()), "worst", worst, "bound", bound)
    assert worst <= bound
    kept_old = (code == pg.TRIM_KEPT) | (code == pg.TRIM_KEPT_ON_FIRST)
    assert pg.residual(n2["q_opt"], n2["t_opt"], e2[~anchored_new]).tobytes() == pg.residual(moved["q_opt"], moved["t_opt"], edges[kept_old]).tobytes()
    s_old = np.einsum("ea,eab,eb->e", r_old, pg.info_full(edges["info"][anchored_old]), r_old)
    s_new = np.einsum("ea,eab,eb->e", r_new, pg.info_full(e2["info"][anchored_new]), r_new)
    assert np.allclose(s_new, s_old, rtol=1e-9, atol=1e-18)


@pytest.mark.parametrize("a,b", [(0, 5), (5, 0), (1, 1), (7, 9), (16, 1), (3, 30)])
def test_two_trims_are_one(solved, a, b):
    nodes, edges = solved
    edges = np.concatenate([edges, tc.random_edges(9, *tc.pattern_pairs("endpoints", 25, len(nodes), a + b if a + b > 1 else 5))])
    n1, e1, _ = pg.trim(nodes, edges, a)
    n2, e2, s2 = pg.trim(n1, e1, b)
    n3, e3, s3 = pg.trim(nodes, edges, a + b)
    assert n2.tobytes() == n3.tobytes() and e2.tobytes() == e3.tobytes() and s2[:2].tolist() == s3[:2].tolist()


def test_the_proposal_runs_on_a_trimmed_graph(solved):
    """propose_loops and unclosed take a trimmed graph as any other: the requests are those of the full graph with the indices shifted,
    when no hit lies among the dropped nodes."""
    nodes, edges = solved
    f = 10
    n2, e2, _ = pg.trim(nodes, edges, f)
    p = dict(radius_m=4.0, growth_m_per_node=0.0, min_gap=8, half_window=0, separation=0, K=16)
    found = 0
    for j in range(len(nodes) - 1, f + p["min_gap"], -1):
        full, nfull, _ = pg.propose_loops(nodes["q_opt"], nodes["t_opt"], j, **p)
        cut, ncut, _ = pg.propose_loops(n2["q_opt"], n2["t_opt"], j - f, **p)
        assert nfull < p["K"]
        want = full[:nfull][full["i"][:nfull] >= f].copy()
        want["i"] -= f; want["j"] -= f; want["first"] -= f
        assert cut[:ncut].tobytes() == want.tobytes(), j
        open_ = pg.unclosed(cut[:ncut], e2[e2["i"] >= 0], 2)
        assert len(open_) <= ncut
        found += ncut
    assert found > 0


def test_the_keyframe_store_follows():
    counts = np.array([[3, 1], [0, 2], [4, 0], [0, 0], [2, 5]])
    kf = tc.clouds(counts)
    desc = gr.descriptors(kf)
    assert desc["first"].tolist() == [[0, 0], [3, 1], [3, 3], [7, 3], [7, 3]] and desc["count"].tolist() == counts.tolist()
    for f in range(5):
        d2, corner, surf, freed = gr.trim_keyframes(desc, kf[0][0], kf[1][0], f)
        assert freed.tolist() == desc["first"][f].tolist()
        assert d2["count"].tolist() == counts[f:].tolist() and d2["first"].tolist() == (desc["first"][f:] - desc["first"][f]).tolist()
        assert corner.tobytes() == kf[0][0][freed[0]:].tobytes() and surf.tobytes() == kf[1][0][freed[1]:].tobytes()
        assert len(corner) == counts[f:, 0].sum() and len(surf) == counts[f:, 1].sum()
    n2, e2, kf2, out = tc.model(tc.random_nodes(0, 5), np.zeros(0, pg.EDGE_DTYPE), kf, 2)
    assert out.tolist() == [3, 0, 0, 0, 0, 3, 3, 0] and kf2[0][1].tolist() == [0, 4, 4, 6] and kf2[1][1].tolist() == [0, 0, 0, 5]
    rec = gr.pack(n2, e2, kf2, (0.4, 0.8))
    assert gr.check(rec, kf_capacity=(16, 16), resolutions=(0.4, 0.8)) is None          # what aloam_graph_load asks of a record
