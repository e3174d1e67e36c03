"""aloam_graph_trim on the MI355X against posegraph.trim and graph_records.trim_keyframes, byte for byte: exported nodes,
edges, keyframe clouds, aloam_graph_info and the eight integers of the call.

One context holds every graph of graph_trim_cases.py, built in numpy and entered in one aloam_graph_load of records made with
graph_records.pack; the model is fed what the device exports before the trim.  All calls are made once (the fixture) and the tests look at
what they left.  The points carry their own index in their bits.  A second, small context enters a chain through mapping steps and
aloam_graph_add_nodes (the keyframe store keeps a node's stacks, so a node needs a step), trims it and adds the next node."""
import numpy as np
import pytest

import graph_trim_cases as tc
from graph_trim_cases import gr, pg
from test_gpu_graph_map import LEAF, Q_ID, cloud, context
from test_gpu_graph_records import feed
from test_gpu_posegraph import OPTIONS, against_model

pytestmark = pytest.mark.gpu

EDGE_SLOTS = {(p, e): k for k, (p, e) in enumerate((p, e) for p in tc.PATTERNS for e in tc.EDGE_COUNTS)}
NODE_SLOTS = {c: len(EDGE_SLOTS) + k for k, c in enumerate(tc.NODE_CASES)}
CLOUD_SLOTS = {k: len(EDGE_SLOTS) + len(NODE_SLOTS) + k for k in range(len(tc.CLOUD_CASES))}
_next = len(EDGE_SLOTS) + len(NODE_SLOTS) + len(CLOUD_SLOTS)
LIST_GRAPHS = (("edges", "endpoints", 257), ("edges", "robust", 600), ("cloud", 5, None))
LIST_SLOTS = {(which, g): _next + 3 * which + g for which in range(3) for g in range(3)}          # forward, backward, alone
UNLISTED, REFUSED, EMPTY, TRIMMED, WHOLE = (_next + 9 + k for k in range(5))
BATCH = _next + 14
MAX_NODES, MAX_EDGES = 600, 640
DRIVE_NODES, DRIVE_FIRST = 60, 20
PROPOSE = dict(radius_m=4.0, growth_m_per_node=0.0, min_gap=8, half_window=0, separation=0, K=16)


def record_of(nodes, edges, counts_or_kf, slot):
    kf = counts_or_kf if isinstance(counts_or_kf, tuple) else tc.clouds(counts_or_kf)
    return gr.pack(nodes, edges, kf, LEAF, seq=slot)


def list_graph(g):
    kind, a, b = LIST_GRAPHS[g]
    if kind == "edges":
        nodes, edges, f = tc.edge_case(a, b, seed=50 + g)
        return nodes, edges, tc.small_counts(len(nodes)), f
    nodes, counts, f = tc.cloud_case(a)
    return nodes, tc.random_edges(77, *tc.pattern_pairs("endpoints", 30, 4, 2)), counts, f


def drive():
    """A drifted chain with loop edges and an anchor, solved (one solves before trimming), the nodes above DRIVE_FIRST then moved by a few
    centimetres and milliradians so that the solve behind the trim has work to do; real-valued clouds of a few dozen points per node."""
    g = pg.drifted_laps(8, DRIVE_NODES, 8)
    edges = np.concatenate([g["odom"], g["loop"], pg.anchor_from_localization(45, g["q_true"][45], g["t_true"][45] + 0.01, 4 * g["info"])])
    q, t, res = pg.optimize(g["q"], g["t"], edges, **OPTIONS)
    assert res["status"] == 0
    rng = np.random.default_rng(4)
    above = DRIVE_NODES - DRIVE_FIRST - 1
    q[DRIVE_FIRST + 1:] = pg.qmul(pg.qexp(2e-3 * rng.standard_normal((above, 3))), q[DRIVE_FIRST + 1:])
    t[DRIVE_FIRST + 1:] += 0.02 * rng.standard_normal((above, 3))
    nodes = np.zeros(DRIVE_NODES, pg.NODE_DTYPE)
    nodes["q"], nodes["t"], nodes["q_opt"], nodes["t_opt"], nodes["frame"] = g["q"], g["t"], q, t, np.arange(DRIVE_NODES)
    per = [(cloud(rng, 20, (10, 10, 3)), cloud(rng, 40, (12, 12, 3))) for _ in range(DRIVE_NODES)]
    kf = tuple((np.concatenate([p[cls] for p in per]), np.concatenate([[0], np.cumsum([len(p[cls]) for p in per])])) for cls in (0, 1))
    return nodes, edges, kf


def state(gpu, b):
    """What the C ABI tells about slot b: counts, nodes, edges (seq checked and taken out), keyframes per class, the cursors."""
    info = gpu.graph_info(b)
    e = gpu.graph_export(b, edges=True)
    assert (e["seq"] == b).all()
    e["seq"] = 0
    kf = tuple(gpu.graph_export_keyframes(b, feature_class=cls) for cls in (0, 1))
    return dict(counts=(info["nodes"], info["edges"]), nodes=gpu.graph_export(b), edges=e, kf=kf, points=gpu.graph_keyframe_info(b)["points"])


def same(a, b):
    return (a["counts"] == b["counts"] and a["nodes"].tobytes() == b["nodes"].tobytes() and a["edges"].tobytes() == b["edges"].tobytes() and
            a["points"] == b["points"] and all(x[0].tobytes() == y[0].tobytes() and x[1].tolist() == y[1].tolist() for x, y in zip(a["kf"], b["kf"])))


def expected(before, first):
    """The model on a slot's exported state: the state the trim must leave, and the eight integers."""
    n2, e2, kf2, out = tc.model(before["nodes"], before["edges"], before["kf"], first)
    return dict(counts=(len(n2), len(e2)), nodes=n2, edges=e2, kf=kf2, points=[len(kf2[0][0]), len(kf2[1][0])]), out


def differences(world, slots):
    bad = []
    for b in slots:
        want, out = expected(world["before"][b], world["first"][b])
        got = world["after"][b]
        print("slot", b, "first", world["first"][b], "before", world["before"][b]["counts"], world["before"][b]["points"], "out", world["out"][b].tolist())
        if not same(got, want) or world["out"][b].tolist() != out.tolist():
            bad.append((b, world["out"][b].tolist(), out.tolist()))
    return bad


@pytest.fixture(scope="module")
def world(binding):
    gpu = context(binding, batch=BATCH, nodes=MAX_NODES, edges=MAX_EDGES, keyframes=(tc.KF_CAPACITY, tc.KF_CAPACITY))
    recs, first = {}, {}
    for (p, e), b in EDGE_SLOTS.items():
        nodes, edges, f = tc.edge_case(p, e, seed=b)
        recs[b], first[b] = record_of(nodes, edges, tc.small_counts(len(nodes)), b), f
    for (n, f), b in NODE_SLOTS.items():
        edges = tc.random_edges(b, *tc.pattern_pairs("endpoints", 90, n, max(2, min(f, n - 3)))) if n > 5 else tc.random_edges(b, [0, 1, 2, 3, -1], [1, 2, 3, 4, 2])
        recs[b], first[b] = record_of(tc.random_nodes(b, n), edges, tc.small_counts(n), b), f
    for k, b in CLOUD_SLOTS.items():
        nodes, counts, f = tc.cloud_case(k)
        recs[b], first[b] = record_of(nodes, tc.random_edges(b, [0, 1, 2, 1], [1, 2, 3, 3]), counts, b), f
    for (which, g), b in LIST_SLOTS.items():
        nodes, edges, counts, f = list_graph(g)
        recs[b], first[b] = record_of(nodes, edges, counts, b), f
    nodes, edges, _ = tc.edge_case("endpoints", 60, seed=5)
    for b in (UNLISTED, REFUSED):
        recs[b], first[b] = record_of(nodes, edges, tc.small_counts(len(nodes)), b), 3
    dn, de, dkf = drive()
    for b in (TRIMMED, WHOLE):
        recs[b], first[b] = record_of(dn, de, dkf, b), DRIVE_FIRST
    slots = sorted(recs)
    assert EMPTY not in recs and len(slots) == BATCH - 1
    gpu.graph_load(slots, np.concatenate([recs[b] for b in slots]), np.concatenate([[0], np.cumsum([len(recs[b]) for b in slots])]))
    gpu.synchronize()
    w = dict(gpu=gpu, B=binding, first=first, before={b: state(gpu, b) for b in slots}, out={}, after={})

    def trim(listed):
        out = gpu.graph_trim(listed, [first[b] for b in listed])
        for k, b in enumerate(listed):
            w["out"][b] = out[k]
    trim(list(EDGE_SLOTS.values()))                                   # every edge case in one call, and so on
    trim(list(NODE_SLOTS.values()))
    trim(list(CLOUD_SLOTS.values()))
    trim([LIST_SLOTS[0, g] for g in (0, 1, 2)])
    trim([LIST_SLOTS[1, g] for g in (2, 1, 0)])
    for g in (0, 1, 2):
        trim([LIST_SLOTS[2, g]])
    trim([TRIMMED])
    for b in slots:
        if b in w["out"]:
            w["after"][b] = state(gpu, b)
    # ---- downstream of the trim, on the trimmed slot and its untrimmed twin
    N, f = DRIVE_NODES, DRIVE_FIRST
    w["map"] = [gpu.graph_export_map([(TRIMMED, 0, N - f, pose)]) for pose in (0, 1)], [gpu.graph_export_map([(WHOLE, f, N - f, pose)]) for pose in (0, 1)]
    js = list(range(f + PROPOSE["min_gap"] + 1, N))
    w["propose"] = js, gpu.graph_propose_loops([(TRIMMED, j - f) for j in js], **PROPOSE), gpu.graph_propose_loops([(WHOLE, j) for j in js], **PROPOSE)
    blob, off = gpu.graph_save([TRIMMED])
    w["saved"] = np.array(blob[off[0]:off[1]])
    w["solve"] = gpu.graph_optimize([TRIMMED], **OPTIONS)[0]
    yield w
    gpu.close()


@pytest.mark.parametrize("pattern", tc.PATTERNS)
def test_edges_against_the_model(world, pattern):
    """E = 0, 1, 255, 256, 257, 600: no tile, one record, one short of a tile, a tile, one more, three tiles with a remainder."""
    slots = [EDGE_SLOTS[pattern, e] for e in tc.EDGE_COUNTS]
    assert not differences(world, slots)
    big = world["out"][EDGE_SLOTS[pattern, 600]]
    want = dict(kept=(600, 0, 0, 0), removed=(0, 0, 600, 0), alternating=(400, 200, 200, 0), robust=(400, 200, 200, 0), reverse=(300, 0, 0, 300))
    if pattern in want:
        assert tuple(big[[1, 2, 3, 4]]) == want[pattern], big
    if pattern == "endpoints":
        assert all(big[k] > 0 for k in (1, 2, 3, 4)), big
    if pattern == "robust":
        flags = world["after"][EDGE_SLOTS[pattern, 600]]["edges"]["flags"]
        assert 0 < (flags == pg.EDGE_ROBUST).sum() < len(flags)


def test_nodes_against_the_model(world):
    """first = 0, 1 and N - 1 of five nodes; 255, 256 and 257 of 600: the kept part ends inside, at and behind a step of the row's shift."""
    assert not differences(world, NODE_SLOTS.values())
    zero = NODE_SLOTS[5, 0]
    assert same(world["after"][zero], dict(world["before"][zero])) and world["out"][zero].tolist() == [5, 5, 0, 0, 0, 0, 0, 0]      # first = 0 changes nothing
    assert world["out"][NODE_SLOTS[5, 4]][0] == 1 and world["out"][NODE_SLOTS[600, 257]][0] == 343


def test_clouds_against_the_model(world):
    """Per class (d, m): m = 0, m < d, m = d, m = d + 1 (one point for the tail), d = 1 with three chunks and five points, and d one short of,
    at and one past the chunk with two chunks and three points; the surf class of every slot takes another case than the corner class."""
    assert not differences(world, CLOUD_SLOTS.values())
    for k, b in CLOUD_SLOTS.items():
        cases = tc.CLOUD_CASES[k], tc.CLOUD_CASES[(k + 3) % len(tc.CLOUD_CASES)]
        assert cases[0] != cases[1]
        assert world["out"][b][[5, 6]].tolist() == [c[0] for c in cases] and world["after"][b]["points"] == [c[1] for c in cases], (k, cases)
        for cls in (0, 1):                                            # the points name the place they came from
            p = world["after"][b]["kf"][cls][0].view(np.uint32)
            assert (p[:, 0] == cases[cls][0] + np.arange(cases[cls][1])).all() and (p[:, 1] == cls).all() and (p[:, 2] >= 2).all()


def test_a_sequence_does_not_depend_on_its_list(world):
    for g in (0, 1, 2):
        slots = [LIST_SLOTS[which, g] for which in range(3)]
        assert not differences(world, slots)
        a, b, c = (world["after"][s] for s in slots)
        assert same(a, b) and same(a, c), g
        assert world["out"][slots[0]].tolist() == world["out"][slots[1]].tolist() == world["out"][slots[2]].tolist()
        assert world["out"][slots[0]][2] > 0


def test_refusals_and_unlisted_slots(world):
    gpu, B = world["gpu"], world["B"]
    L = B.lib()
    nodes = world["before"][REFUSED]["counts"][0]
    for seqs, first in (([REFUSED], [-1]), ([REFUSED], [nodes]), ([REFUSED, REFUSED], [1, 1]), ([UNLISTED, REFUSED], [1, nodes]), ([EMPTY], [0]),
                        ([REFUSED, EMPTY], [1, 0]), ([BATCH], [0]), ([-1], [0])):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_trim(seqs, first)
        assert e.value.code == B.E_ARG, (seqs, first)
    ids, f = np.array([REFUSED], np.int32), np.array([1], np.int32)
    assert L.aloam_graph_trim(gpu.h, None, f.ctypes.data, 1, None) == B.E_ARG and L.aloam_graph_trim(gpu.h, ids.ctypes.data, None, 1, None) == B.E_ARG
    assert L.aloam_graph_trim(gpu.h, ids.ctypes.data, f.ctypes.data, -1, None) == B.E_ARG
    assert L.aloam_graph_trim(gpu.h, None, None, 0, None) == 0                      # n = 0 is ALOAM_OK
    gpu.synchronize()
    for b in (REFUSED, UNLISTED):
        assert same(state(gpu, b), world["before"][b]), b                           # rows and counts as they were, after every other trim too
    assert gpu.graph_info(EMPTY)["nodes"] == 0 and gpu.graph_info(EMPTY)["edges"] == 0
    assert same(state(gpu, WHOLE), world["before"][WHOLE])


def test_state_error_before_graph_enable(binding):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=4096)
    try:
        with pytest.raises(binding.AloamError) as e:
            gpu.graph_trim([0], [0])
        assert e.value.code == binding.E_STATE
    finally:
        gpu.close()


def test_the_map_of_the_kept_nodes_is_the_same(world):
    trimmed, whole = world["map"]
    for pose in (0, 1):
        (tt, tp, to, ts), (wt, wp, wo, ws) = trimmed[pose], whole[pose]
        assert len(tt) > 0 and len(tp) > 0
        assert tt.tobytes() == wt.tobytes() and tp.tobytes() == wp.tobytes() and to.tolist() == wo.tolist() and ts.tobytes() == ws.tobytes(), pose


def test_the_proposal_shifts_by_first(world):
    js, (treq, tcnt, td2), (wreq, wcnt, wd2) = world["propose"]
    f, found = DRIVE_FIRST, 0
    for k, j in enumerate(js):
        assert wcnt[k] < PROPOSE["K"]
        keep = wreq[k]["i"][:wcnt[k]] >= f
        want = wreq[k][:wcnt[k]][keep].copy()
        want["seq"] = TRIMMED; want["i"] -= f; want["j"] -= f; want["first"] -= f
        assert treq[k][:tcnt[k]].tobytes() == want.tobytes() and td2[k][:tcnt[k]].tobytes() == wd2[k][:wcnt[k]][keep].tobytes(), j
        found += int(tcnt[k])
    assert found > 0


def test_the_saved_record_is_the_models(world):
    want, _ = expected(world["before"][TRIMMED], DRIVE_FIRST)
    edges = want["edges"].copy()
    edges["seq"] = TRIMMED
    rec = gr.pack(want["nodes"], edges, want["kf"], LEAF, seq=TRIMMED)
    assert len(world["saved"]) == len(rec) and np.array_equal(world["saved"], rec)
    assert gr.check(rec, kf_capacity=(tc.KF_CAPACITY, tc.KF_CAPACITY), resolutions=LEAF, max_nodes=MAX_NODES, max_edges=MAX_EDGES) is None


def test_the_solve_of_the_trimmed_graph(world):
    """aloam_graph_optimize on the trimmed slot against posegraph.optimize on the model's output, compared as test_gpu_posegraph.py compares:
    status, counts, initial cost to 1e-12 relative, poses and final cost to 8 eps_ref, the entered poses untouched (measured: poses 3.6e-12,
    cost 1.1e-14).  The preconditioner's bound is held per LM iteration here, not in total: with function_tolerance = 0 a solve runs until
    its cost stops changing in the last bit, and how many iterations that takes is rounding (25 on the device, 21 for the dense model, 7 for
    chain_pcg, each with one PCG iteration per LM iteration: a chain with anchors is exactly the preconditioner's block-tridiagonal form)."""
    want, out = expected(world["before"][TRIMMED], DRIVE_FIRST)
    assert out[2] > 0 and (want["edges"]["i"] == -1).sum() == out[2] + 1          # the anchored loop edges, and the anchor the drive had
    res = world["solve"]
    against_model(world["gpu"], TRIMMED, res, want["nodes"], want["edges"], "trimmed drive %d / %d" % (DRIVE_NODES, DRIVE_FIRST), chain=False)
    _, _, mc = pg.chain_pcg(want["nodes"]["q_opt"], want["nodes"]["t_opt"], want["edges"], **OPTIONS)
    print("PCG per LM iteration: device %d / %d, chain_pcg %d / %d" % (res["pcg_iterations"], res["lm_iterations"], mc["pcg_iterations"], mc["lm_iterations"]))
    assert res["accepted_steps"] > 0 and res["pcg_iterations"] * mc["lm_iterations"] <= 2 * mc["pcg_iterations"] * res["lm_iterations"]


def test_the_next_node_follows_the_trim(binding):
    """Two slots are fed the same clouds and poses.  Slot 0 is trimmed at 3 of 6 nodes; the next aloam_graph_add_nodes puts its node at index
    nodes' with its odometry edge at edges', both the twin's bytes with the indices shifted, and its clouds at the rewound cursors."""
    gpu = context(binding, batch=2, nodes=16, edges=32)
    try:
        rng = np.random.default_rng(12)

        def step(k):
            one = (cloud(rng, 40, (5, 5, 2)), cloud(rng, 200, (8, 8, 2)), Q_ID, (0.5 * k, 0.1 * k, 0.0))
            feed(gpu, [one, one], [0, 1])
        for k in range(6):
            step(k)
        for b in (0, 1):
            n = gpu.graph_export(b)
            q, t = pg.relative_pose(n["q"][1], n["t"][1], n["q"][5], n["t"][5])
            gpu.graph_add_edges(pg.make_edges(b, 1, 5, q, t + 0.01, np.eye(6) * 50.0))
        before = state(gpu, 0)
        out = gpu.graph_trim([0], [3])[0]
        want, model_out = expected(before, 3)
        after = state(gpu, 0)
        assert same(after, want) and out.tolist() == model_out.tolist() and out[[0, 1, 2]].tolist() == [3, 3, 1]
        step(6)
        a, b = state(gpu, 0), state(gpu, 1)
        assert a["counts"] == (4, 4) and b["counts"] == (7, 7)
        assert a["nodes"][:3].tobytes() == want["nodes"].tobytes() and a["edges"][:3].tobytes() == want["edges"].tobytes()
        assert a["nodes"][3].tobytes() == b["nodes"][6].tobytes()
        ea, eb = a["edges"][3], b["edges"][6]
        assert (ea["i"], ea["j"], eb["i"], eb["j"]) == (2, 3, 5, 6)
        assert all(ea[k].tobytes() == eb[k].tobytes() for k in ("q", "t", "info", "flags"))
        for cls in (0, 1):
            (pa, oa), (pb, ob) = a["kf"][cls], b["kf"][cls]
            assert oa[3] == want["points"][cls] and oa.tolist() == (ob[3:] - ob[3]).tolist()          # the new clouds start at the rewound cursor
            assert pa.tobytes() == pb[ob[3]:].tobytes() and oa[4] > oa[3]
        assert a["points"] == [int(a["kf"][0][1][-1]), int(a["kf"][1][1][-1])]
    finally:
        gpu.close()
