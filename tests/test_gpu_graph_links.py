"""Links measured on the MI355X (aloam_graph_register_links / aloam_graph_search_links / aloam_graph_propose_links).

Registration.  The strongest check is the twin identity: sequences 0 and 1 are fed the same keyframes, so a link request with its target in
one and its source in the other must give, byte for byte, what the loop request inside one sequence gives - result, search record, score
table and filtered target - for seq_i < seq_j and for seq_i > seq_j.  Sequence 2 holds the same clouds at entered poses moved by 2 rad and
100 m: no pose of seq_j is read, so a link into it gives the same bytes again, and is held against the numpy model with the bounds of
tests/test_gpu_loop_register.py.  The keyframes are hand-made as there (aloam_set_last + aloam_mapping_step with the solver off).

Proposal.  Byte for byte against posegraph.propose_links fed the exported nodes; the graphs are entered without clouds through
aloam_graph_load, as tests/test_gpu_graph_propose.py enters its own.  Coordinates of the constructed cases are small integers or halves, so
every d2 is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import graph_joint_cases as jc
import graph_propose_cases as gc
import loopreg_model as M
from posegraph_cases import OPTIONS, eps_ref
from test_gpu_loop_register import CAP_CORNER, CAP_SURF, INFO, Z_BOUND, check_against_model, context, drive, feed, guess_of, model_target, raw, unit

pytestmark = pytest.mark.gpu
pg = importlib.import_module("a-loam_amd.posegraph")
lr = importlib.import_module("a-loam_amd.loopreg")
gr = importlib.import_module("a-loam_amd.graph_records")
SLOTS = 8
SEARCH = dict(radius_m=0.5, step_m=0.5, yaw_deg=2.5, yaw_step_deg=2.5)            # 27 nodes
EXTRA_SURF = (255, 256, 257, None, 1023, 1024, 1025, 2047, 2048, 2049)            # nodes 10 .. 19 of sequences 0 and 1; None: an empty corner cloud
SENTINEL, TAIL = 0xA5, 64


def lattice(n):
    """n points, one per 0.4 m voxel (at the voxels' centres): the surf filter keeps every one."""
    k = np.arange(n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = (k % 32 - 16 + 0.5) * 0.4, ((k // 32) % 32 - 16 + 0.5) * 0.4, (k // 1024 - 2 + 0.5) * 0.4
    return p


def link_of(loop):
    """(seq, i, j, first, count, pose, q, t) of a loop request -> the link tuple with everything but seq_i / seq_j filled in."""
    seq, i, j, first, count, pose, q, t = loop
    return lambda seq_i, seq_j: (seq_i, i, first, count, seq_j, j, pose, q, t)


@pytest.fixture(scope="module")
def world(binding):
    """Sequences 0 and 1: the noise-free room of loopreg_model.fixture(seed=7) and ten more nodes each (EXTRA_SURF); sequence 1 gets one node
    more than sequence 0.  Sequence 2: the same ten keyframes, entered at poses moved by graph_joint_cases.FRAME (2 rad, 100 m)."""
    fx = M.fixture(seed=7)
    q2, t2 = pg.compose(*jc.FRAME, np.array(fx["q"]), np.array(fx["t"]))
    moved = dict(fx, q=list(q2), t=list(t2))
    gpu = context(binding, 3, loops=(SLOTS, CAP_CORNER, CAP_SURF))
    gpu.profile_enable(True)
    stacks = drive(gpu, binding, [fx, fx, moved])
    src_c, src_s = stacks[0][9]
    keep = (moved["raw"][9][0], moved["raw"][9][1], moved["q"][9], moved["t"][9])
    for n in EXTRA_SURF:
        c = src_c if n else np.zeros((0, 4), np.float32)
        s = src_s if n is None else src_s[:n] if n <= len(src_s) else lattice(n)
        one = (c, s, fx["q"][9], fx["t"][9])
        got = feed(gpu, binding, [one, one, keep], [0, 1])
        for b in (0, 1):
            stacks[b].append(got[b])
    stacks[1].append(feed(gpu, binding, [(src_c, src_s, fx["q"][9], fx["t"][9])] * 2 + [keep], [1])[1])
    sizes = [len(s[1]) for s in stacks[0][10:]]
    print("surf points of nodes 10 .. 19:", sizes, "corner:", [len(s[0]) for s in stacks[0][10:]])
    assert sizes == [n if n else len(src_s) for n in EXTRA_SURF] and len(stacks[0][13][0]) == 0
    nodes = [gpu.graph_export(b) for b in range(3)]
    assert [len(n) for n in nodes] == [20, 21, 10] and raw(nodes[0]) == raw(nodes[1][:20])
    assert all(raw(stacks[0][k][cls]) == raw(stacks[1][k][cls]) for k in range(20) for cls in (0, 1))
    assert all(raw(stacks[0][k][cls]) == raw(stacks[2][k][cls]) for k in range(10) for cls in (0, 1))
    assert np.abs(nodes[2]["t"] - nodes[0]["t"][:10]).max() > 50.0
    yield {"gpu": gpu, "fx": [fx, fx, moved], "stacks": stacks, "nodes": nodes, "B": binding}
    gpu.close()


def loop_requests(w):
    nd = w["nodes"][0]
    reqs = [(0, 4, 9, 0, 9, 0) + guess_of(pg, nd, 4, 9), (0, 4, 9, 4, 1, 0) + guess_of(pg, nd, 4, 9), (0, 2, 9, 1, 5, 1) + guess_of(pg, nd, 2, 9, opt=True)]
    reqs += [(0, 4, j, 0, 9, 0) + guess_of(pg, nd, 4, j) for j in range(10, 20)]
    return reqs


def test_twin_identity_of_the_registration(world):
    """register_links(seq_i, seq_j) == register_loops(seq_i) byte for byte in dst and in every slot's filtered target, with the rows of the
    source before and behind the rows of the target; in rounds (13 requests over 8 slots)."""
    gpu = world["gpu"]
    loops = loop_requests(world)
    for seq_i, seq_j in ((0, 1), (1, 0), (0, 2)):
        mine = [l for l in loops if seq_j != 2 or l[2] < 10]
        inside = [(seq_i,) + l[1:] for l in mine]
        want = gpu.graph_register_loops(inside)
        want_targets = [[gpu.graph_loop_target(s, cls) for cls in (0, 1)] for s in range(min(len(mine), SLOTS))]
        got = gpu.graph_register_links([link_of(l)(seq_i, seq_j) for l in mine])
        got_targets = [[gpu.graph_loop_target(s, cls) for cls in (0, 1)] for s in range(min(len(mine), SLOTS))]
        print(f"seq_i {seq_i} seq_j {seq_j}: statuses {[int(r['status']) for r in got]}, sources {[r['source_points'].tolist() for r in got]}")
        assert [raw(r) for r in got] == [raw(r) for r in want], (seq_i, seq_j)
        assert all(raw(a[cls]) == raw(b[cls]) and len(a[cls]) for a, b in zip(got_targets, want_targets) for cls in (0, 1))
        assert int(got[0]["status"]) == lr.LOOP_OK and got[0]["n_plane"] > 500
    sizes = [r["source_points"].tolist() for r in gpu.graph_register_links([link_of(l)(0, 1) for l in loops])]
    assert [s[1] for s in sizes[3:]] == [n if n else len(world["stacks"][0][9][1]) for n in EXTRA_SURF] and sizes[6][0] == 0


def test_twin_identity_of_the_search(world):
    gpu = world["gpu"]
    loops = loop_requests(world)[:3]
    for seq_i, seq_j in ((0, 1), (1, 0)):
        want = gpu.graph_search_loops([(seq_i,) + l[1:] for l in loops], search=SEARCH, scores=True)
        want_target = [gpu.graph_loop_target(1, cls) for cls in (0, 1)]
        got = gpu.graph_search_links([link_of(l)(seq_i, seq_j) for l in loops], search=SEARCH, scores=True)
        got_target = [gpu.graph_loop_target(1, cls) for cls in (0, 1)]
        assert want[2].shape == (3, 27) and all(raw(a) == raw(b) for a, b in zip(got, want)), (seq_i, seq_j)
        assert all(raw(a) == raw(b) for a, b in zip(got_target, want_target))
        assert int(got[0][0]["status"]) == lr.LOOP_OK


def test_against_the_model(world):
    """Target: nodes 0 .. 8 of sequence 0; source: node 9 of sequence 2, whose poses live 100 m and 2 rad away.  The target bit for bit, counts,
    iterations and termination equal, Z, info and cost within the bounds tests/test_gpu_loop_register.py holds a loop to."""
    gpu = world["gpu"]
    qg, tg = guess_of(pg, world["nodes"][0], 4, 9)
    res = gpu.graph_register_links([(0, 4, 0, 9, 2, 9, 0, qg, tg)])[0]
    want = model_target(lr, world, 0, 4, 0, 9)
    for cls in (0, 1):
        got = gpu.graph_loop_target(0, cls)
        assert got.shape == want[cls].shape and np.array_equal(got.view(np.uint32), want[cls].view(np.uint32)), cls
    check_against_model(world["B"], lr, world, 0, 9, res, label="link 0 <- 2")
    fx = world["fx"][0]
    qt, tt = pg.relative_pose(fx["q_true"][4], fx["t_true"][4], fx["q_true"][9], fx["t_true"][9])
    r0, d0 = M.pose_error(qg, tg, qt, tt)
    print(f"the guess is off by {d0:.4f} m and {r0:.4f} rad")
    assert 0.39 < d0 < 0.41 and 0.07 < r0 < 0.071


def test_source_shapes_against_the_model(world):
    """Sources of 255, 256 and 257 surf points and one with an empty corner cloud, held in sequence 1, against targets of sequence 0."""
    gpu = world["gpu"]
    nd = world["nodes"][0]
    res = gpu.graph_register_links([(0, 4, 0, 9, 1, j, 0) + guess_of(pg, nd, 4, j) for j in (10, 11, 12, 13)])
    for r, j in enumerate((10, 11, 12, 13)):
        check_against_model(world["B"], lr, world, 0, j, res[r], label=f"source node {j} of sequence 1 ({res[r]['source_points'].tolist()} points)")


def test_the_two_node_counts_are_held_apart(world):
    """Sequence 1 holds 21 nodes, sequence 0 holds 20: j = 20 of seq_j = 1 is past seq_i's nodes and succeeds; a window that reaches node 20
    is inside seq_j's nodes but not inside seq_i's and is refused; j = 20 of seq_j = 0 is refused."""
    gpu, B = world["gpu"], world["B"]
    qg, tg = guess_of(pg, world["nodes"][1], 4, 20)
    res = gpu.graph_register_links([(0, 4, 0, 9, 1, 20, 0, qg, tg)])[0]
    same = gpu.graph_register_links([(0, 4, 0, 9, 1, 9, 0, qg, tg)])[0]
    assert int(res["status"]) == lr.LOOP_OK and raw(res) == raw(same)                # node 20 holds the clouds of node 9
    for bad in ((0, 19, 12, 9, 1, 9, 0, qg, tg), (1, 4, 0, 9, 0, 20, 0, qg, tg)):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_links([bad])
        assert e.value.code == B.E_ARG
    assert int(gpu.graph_register_links([(1, 19, 12, 9, 0, 9, 0, qg, tg)])[0]["status"]) in (lr.LOOP_OK, lr.LOOP_SOLVE_FAILED)   # the same window inside seq_i = 1


def test_a_result_does_not_depend_on_the_other_requests_or_the_round(world):
    gpu = world["gpu"]
    links = [link_of(l)(0, 1) for l in loop_requests(world)[:7]] + [link_of(loop_requests(world)[0])(1, 0), link_of(loop_requests(world)[0])(0, 2)]
    lone = [raw(gpu.graph_register_links([l])[0]) for l in links]
    assert len(set(lone)) >= 7
    together = gpu.graph_register_links(links)
    assert [raw(r) for r in together] == lone
    back = gpu.graph_register_links(links[::-1])
    assert [raw(r) for r in back][::-1] == lone
    n = 4 * SLOTS + 3                                                               # five rounds: the fifth takes the first's slot of both rings
    many = gpu.graph_register_links([links[k % len(links)] for k in range(n)], pinned=False)
    assert [raw(many[k]) for k in range(n)] == [lone[k % len(links)] for k in range(n)]
    found = gpu.graph_search_links([links[k % len(links)] for k in range(2 * SLOTS + 1)], search=SEARCH)
    alone = gpu.graph_search_links([links[2]], search=SEARCH)
    assert raw(found[0][2]) == raw(alone[0][0]) == raw(found[0][2 + len(links)]) and raw(found[1][2]) == raw(alone[1][0])


def test_twin_identity_with_the_odd_sized_clouds_in_the_target(world):
    """The target window covers nodes 10 .. 19, whose surf clouds hold 255 / 256 / 257, 1023 / 1024 / 1025 and 2047 / 2048 / 2049 points
    (the transform loop of the gather takes a node 1024 points at a time) and one of which has no corner cloud: the link's bytes and its
    filtered target are the loop's, both ways round, and the target is loopreg.target_cloud bit for bit."""
    gpu = world["gpu"]
    qg, tg = guess_of(pg, world["nodes"][0], 15, 9)
    for seq_i, seq_j in ((0, 1), (1, 0)):
        want = gpu.graph_register_loops([(seq_i, 15, 9, 10, 10, 0, qg, tg), (seq_i, 19, 9, 12, 8, 0, qg, tg)])
        want_targets = [[gpu.graph_loop_target(s, cls) for cls in (0, 1)] for s in (0, 1)]
        got = gpu.graph_register_links([(seq_i, 15, 10, 10, seq_j, 9, 0, qg, tg), (seq_i, 19, 12, 8, seq_j, 9, 0, qg, tg)])
        got_targets = [[gpu.graph_loop_target(s, cls) for cls in (0, 1)] for s in (0, 1)]
        print(f"seq_i {seq_i}: raw targets {[r['target_raw'].tolist() for r in got]}, filtered {[r['target_points'].tolist() for r in got]}, statuses {[int(r['status']) for r in got]}")
        assert [raw(r) for r in got] == [raw(r) for r in want], (seq_i, seq_j)
        assert all(raw(a[cls]) == raw(b[cls]) and len(a[cls]) for a, b in zip(got_targets, want_targets) for cls in (0, 1))
        assert got[0]["target_raw"].tolist() == [sum(len(world["stacks"][0][k][cls]) for k in range(10, 20)) for cls in (0, 1)]
        model = model_target(lr, world, 0, 15, 10, 10)
        for cls in (0, 1):
            assert got_targets[0][cls].shape == model[cls].shape and np.array_equal(got_targets[0][cls].view(np.uint32), model[cls].view(np.uint32)), cls


def live_state(gpu, B, b):
    """Every getter of one sequence, as bytes: the four fields of the map pose, the map's figures, the cubes of both classes, both stacks, the
    graph's nodes and edges, the keyframe store."""
    p = gpu.map_pose(b)
    return (raw(p["q_w"]), raw(p["t_w"]), raw(p["q_wmap_wodom"]), raw(p["t_wmap_wodom"]), gpu.map_info(b),
            [[(i, raw(c)) for i, c in sorted(gpu.map_cubes(cls, b).items())] for cls in (0, 1)],
            raw(gpu.map_cloud(B.MAP_CORNER_STACK, b)), raw(gpu.map_cloud(B.MAP_SURF_STACK, b)), raw(gpu.graph_export(b)), raw(gpu.graph_export(b, edges=True)),
            gpu.graph_keyframe_info(b), gpu.graph_info(b))


def test_opt_in_a_twin_that_never_calls_a_link_function(binding):
    """Two contexts fed the same drive of two sequences.  One calls register_links, search_links and propose_links, the other never calls a
    link function.  Every getter of both sequences is equal behind the link calls, and again after a further fed keyframe in both; the loop
    calls then return the same bytes in both; the twin's loop_register slot counts no launch and no other slot differs but pose_graph, by
    the one proposal."""
    fx = M.fixture(seed=7)
    twins = []
    try:
        for _ in range(2):
            gpu = context(binding, 2, loops=(SLOTS, CAP_CORNER, CAP_SURF))
            twins.append(gpu)
            gpu.profile_enable(True)
            drive(gpu, binding, [fx, fx])
        a, b = twins
        nd = a.graph_export(0)
        assert raw(nd) == raw(b.graph_export(0))
        assert all(live_state(a, binding, s) == live_state(b, binding, s) for s in (0, 1))
        qg, tg = guess_of(pg, nd, 4, 9)
        links = [(0, 4, 0, 9, 1, 9, 0, qg, tg), (1, 2, 1, 5, 0, 9, 0) + guess_of(pg, nd, 2, 9), (0, 4, 4, 1, 1, 3, 0) + guess_of(pg, nd, 4, 3)]
        res = a.graph_register_links(links * 4)                                     # two rounds over the eight slots
        found = a.graph_search_links(links, search=SEARCH)
        prop = a.graph_propose_links([(1, 9, 0), (0, 3, 1)], radius_m=2.0, half_window=2, separation=1, K=4)
        assert int(res[0]["status"]) == lr.LOOP_OK and int(found[0][0]["status"]) == lr.LOOP_OK and int(prop[1][0]) >= 1
        assert all(live_state(a, binding, s) == live_state(b, binding, s) for s in (0, 1))
        step = (fx["raw"][3][0], fx["raw"][3][1], fx["q"][3], fx["t"][3])
        for g in twins:                                                             # a further keyframe in both
            feed(g, binding, [step, step], [0, 1])
        assert all(live_state(a, binding, s) == live_state(b, binding, s) for s in (0, 1)) and a.graph_info(0)["nodes"] == 11
        pa, pb = a.profile(), b.profile()
        assert pa["loop_register"]["launches"] >= 2 and pb["loop_register"]["launches"] == 0
        assert pa["pose_graph"]["launches"] == pb["pose_graph"]["launches"] + 1
        for name in pb:
            if name not in ("loop_register", "pose_graph"):
                assert pa[name]["launches"] == pb[name]["launches"], name
        live_nodes = a.graph_export(1)
        assert raw(live_nodes) == raw(b.graph_export(1))
        loops = [(0, 4, 9, 0, 9, 0, qg, tg), (1, 4, 10, 2, 7, 0) + guess_of(pg, live_nodes, 4, 10)]
        P = dict(radius_m=2.0, growth_m_per_node=0.0, min_gap=3, half_window=2, separation=1, K=4)
        for call in (lambda g: [raw(r) for r in g.graph_register_loops(loops)], lambda g: [raw(x) for x in g.graph_search_loops(loops, search=SEARCH, scores=True)],
                     lambda g: [raw(np.ascontiguousarray(x)) for x in g.graph_propose_loops([(0, 10), (1, 9)], **P)]):
            assert call(a) == call(b)
        assert all(live_state(a, binding, s) == live_state(b, binding, s) for s in (0, 1))
    finally:
        for g in twins:
            g.close()


def test_the_loop_calls_are_what_they_were(world):
    """Before and after link calls: register_loops, search_loops and propose_loops return the same bytes; the live sequences are untouched; a
    link call is timed under loop_register like a loop call, and the proposal under pose_graph."""
    gpu, B = world["gpu"], world["B"]
    loops = loop_requests(world)[:3]
    P = dict(radius_m=3.0, growth_m_per_node=0.0, min_gap=3, half_window=2, separation=1, K=4)

    def calls():
        return ([raw(r) for r in gpu.graph_register_loops(loops)], [raw(a) for a in gpu.graph_search_loops(loops, search=SEARCH, scores=True)],
                [raw(np.ascontiguousarray(a)) for a in gpu.graph_propose_loops([(0, 9), (1, 20)], **P)])

    def live():
        return [(raw(gpu.map_pose(b)["q_w"]), raw(gpu.map_pose(b)["t_w"]), gpu.map_info(b), raw(gpu.graph_export(b)), gpu.graph_keyframe_info(b), gpu.graph_info(b),
                 raw(gpu.map_cloud(B.MAP_SURF_STACK, b))) for b in range(3)]
    before, state = calls(), live()
    p0 = gpu.profile()
    gpu.graph_register_loops(loops)
    p1 = gpu.profile()
    gpu.graph_register_links([link_of(l)(0, 1) for l in loops])
    p2 = gpu.profile()
    gpu.graph_search_links([link_of(l)(1, 0) for l in loops], search=SEARCH)
    gpu.graph_propose_links([(1, 20, 0), (2, 9, 0)], radius_m=200.0, half_window=2, K=4)
    p3 = gpu.profile()
    assert calls() == before and live() == state
    d = lambda a, b, k: b[k]["launches"] - a[k]["launches"]
    assert d(p0, p1, "loop_register") == d(p1, p2, "loop_register") >= 1 and d(p2, p3, "loop_register") >= 1 and d(p2, p3, "pose_graph") >= 1
    assert all(d(p0, p3, k) == 0 for k in p0 if k not in ("loop_register", "pose_graph")), {k: d(p0, p3, k) for k in p0}


def test_refusals_change_nothing(world):
    import torch
    gpu, B = world["gpu"], world["B"]
    qg, tg = guess_of(pg, world["nodes"][0], 4, 9)
    good = (0, 4, 0, 9, 1, 9, 0, qg, tg)
    before = [(raw(gpu.graph_export(b)), raw(gpu.graph_export(b, edges=True)), gpu.graph_keyframe_info(b), gpu.graph_info(b)) for b in range(3)]
    dst = torch.full((2 * 448,), 0xAB, dtype=torch.uint8, pin_memory=True)
    found = torch.full((2 * 160,), 0xAB, dtype=torch.uint8, pin_memory=True)
    bad = [(3, 4, 0, 9, 1, 9, 0, qg, tg), (-1, 4, 0, 9, 1, 9, 0, qg, tg), (0, 4, 0, 9, 3, 9, 0, qg, tg), (0, 4, 0, 9, -1, 9, 0, qg, tg), (0, 4, 0, 9, 0, 9, 0, qg, tg),
           (1, 4, 0, 9, 1, 15, 0, qg, tg), (0, 4, 0, 0, 1, 9, 0, qg, tg), (0, 4, -1, 9, 1, 9, 0, qg, tg), (0, 4, 0, 21, 1, 9, 0, qg, tg), (0, 9, 0, 9, 1, 9, 0, qg, tg),
           (0, 4, 5, 3, 1, 9, 0, qg, tg), (0, 4, 0, 9, 1, 21, 0, qg, tg), (0, 4, 0, 9, 1, -1, 0, qg, tg), (0, 4, 0, 9, 2, 10, 0, qg, tg), (0, 4, 0, 9, 1, 9, 2, qg, tg),
           (0, 4, 0, 9, 1, 9, 0, qg * 1.001, tg), (0, 4, 0, 9, 1, 9, 0, qg * np.array([1, 1, 1, np.nan]), tg), (0, 4, 0, 9, 1, 9, 0, qg, tg * np.array([1, np.inf, 1]))]
    for b in bad:
        for call in (lambda: gpu.graph_register_links_into([good, b], dst.data_ptr()), lambda: gpu.graph_search_links_into([good, b], dst.data_ptr(), found.data_ptr())):
            with pytest.raises(B.AloamError) as e:
                call()
            assert e.value.code == B.E_ARG, b
    for kw in ({"outer_iterations": 0}, {"lm_max_iterations": -1}):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_links_into([good], dst.data_ptr(), gpu.graph_loop_options(**kw))
        assert e.value.code == B.E_ARG
    with pytest.raises(B.AloamError) as e:
        gpu.graph_search_links_into([good], dst.data_ptr(), found.data_ptr(), search=gpu.graph_loop_search(yaw_deg=90.0, yaw_step_deg=1.0))
    assert e.value.code == B.E_ARG
    pageable = np.zeros(448, np.uint8)
    for ptr in (pageable.ctypes.data, 0, dst.data_ptr() + 4):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_links_into([good], ptr)
        assert e.value.code == B.E_ARG
    with pytest.raises(B.AloamError) as e:
        gpu.graph_search_links_into([good], dst.data_ptr(), 0)
    assert e.value.code == B.E_ARG
    L = B.lib()
    one = gpu.graph_link_requests([good])
    assert L.aloam_graph_register_links(gpu.h, None, 1, None, C.c_void_p(dst.data_ptr())) == B.E_ARG
    assert L.aloam_graph_register_links(gpu.h, one.ctypes.data, -1, None, C.c_void_p(dst.data_ptr())) == B.E_ARG
    assert L.aloam_graph_register_links(gpu.h, None, 0, None, None) == 0 and L.aloam_graph_search_links(gpu.h, None, 0, None, None, None, None, None) == 0
    gpu.synchronize()
    assert bool((dst == 0xAB).all()) and bool((found == 0xAB).all()) and not pageable.any()
    assert before == [(raw(gpu.graph_export(b)), raw(gpu.graph_export(b, edges=True)), gpu.graph_keyframe_info(b), gpu.graph_info(b)) for b in range(3)]
    gpu.graph_register_links_into([good], dst.data_ptr())                           # and the call they vary is accepted
    gpu.synchronize()
    assert int(dst.numpy()[:448].view(B.GRAPH_LOOP_RESULT_DTYPE)[0]["status"]) == lr.LOOP_OK
    bare = context(B, 2, loops=None)
    try:
        for call in (lambda: bare.graph_register_links_into([good], dst.data_ptr()), lambda: bare.graph_search_links_into([good], dst.data_ptr(), found.data_ptr()),
                     lambda: bare.graph_register_links_into([], 0)):
            with pytest.raises(B.AloamError) as e:
                call()
            assert e.value.code == B.E_STATE
    finally:
        bare.close()


def test_target_node_counts_around_the_gathers_workgroups(binding):
    """1, 15, 16 and 17 target nodes against the 16 workgroups per (slot, class): the link's bytes are the loop's, the 17-node target is
    loopreg.target_cloud bit for bit."""
    fx = M.fixture(seed=13, n_target=17)
    gpu = context(binding, 2, loops=(4, 1 << 13, 1 << 15), keyframes=(1 << 13, 1 << 15))
    try:
        stacks = drive(gpu, binding, [fx, fx])
        nd = gpu.graph_export(0)
        i, j = fx["i"], fx["j"]
        qg, tg = guess_of(pg, nd, i, j)
        windows = [(i, 1), (1, 15), (1, 16), (0, 17)]
        want = gpu.graph_register_loops([(1, i, j, first, count, 0, qg, tg) for first, count in windows])
        got = gpu.graph_register_links([(1, i, first, count, 0, j, 0, qg, tg) for first, count in windows])
        target = [gpu.graph_loop_target(3, cls) for cls in (0, 1)]
    finally:
        gpu.close()
    print("raw targets", [r["target_raw"].tolist() for r in got], "statuses", [int(r["status"]) for r in got])
    assert [raw(r) for r in got] == [raw(r) for r in want] and int(got[3]["status"]) == lr.LOOP_OK
    model = lr.target_cloud(nd["q"], nd["t"], stacks[1], i, 0, 17, M.LEAF, M.voxel_filter)
    for cls in (0, 1):
        assert target[cls].shape == model[cls].shape and np.array_equal(target[cls].view(np.uint32), model[cls].view(np.uint32)), cls


def test_statuses_known_before_any_point_is_touched(binding):
    """The surf rows take nine keyframes, not ten: node 9 of both sequences is kept without clouds (NO_CLOUDS as a source).  The enabled surf
    capacity is below nine nodes' raw points (TOO_LARGE); its neighbour in the batch is what it is alone."""
    fx = M.fixture(seed=7)
    gpu = context(binding, 2, keyframes=(1 << 13, 9 * 1100), loops=(4, CAP_CORNER, 4000))
    try:
        for k in range(10):
            for b in (0, 1):
                gpu.set_last(fx["raw"][k][0], fx["raw"][k][1], b); gpu.set_full_cloud(fx["raw"][k][1][:4], b)
                gpu.set_state([0, 0, 0, 1], [0, 0, 0], fx["q"][k], fx["t"][k], b)
            gpu.mapping_step()
            gpu.graph_add_nodes([0, 1], INFO)
        with pytest.raises(binding.AloamError) as e:
            gpu.synchronize()
        assert e.value.code == binding.E_CAPACITY
        assert gpu.graph_keyframe_info(1)["dropped_nodes"] == 1
        nd = gpu.graph_export(0)
        g9, g8 = guess_of(pg, nd, 4, 9), guess_of(pg, nd, 4, 8)
        ok = (0, 4, 3, 3, 1, 8, 0) + g8
        alone = gpu.graph_register_links([ok])[0]
        res = gpu.graph_register_links([(0, 4, 0, 8, 1, 8, 0) + g8, ok, (0, 4, 3, 3, 1, 9, 0) + g9, (1, 9, 9, 1, 0, 4, 0) + guess_of(pg, nd, 9, 4)])
    finally:
        gpu.close()
    assert [int(r["status"]) for r in res] == [lr.LOOP_TOO_LARGE, lr.LOOP_OK, lr.LOOP_NO_CLOUDS, lr.LOOP_NO_CLOUDS]
    assert res[0]["target_raw"][1] > 4000 and np.array_equal(res[0]["q"], unit(g8[0])) and not res[0]["info"].any()
    assert raw(res[1]) == raw(alone) and res[2]["source_points"].tolist() == [0, 0] and np.array_equal(res[2]["t"], g9[1])


def test_the_measured_link_joins_the_sessions(world):
    """The link 0 <- 2 through loopreg.link_from_result into aloam_graph_optimize_joint with align, against posegraph.optimize_joint fed the
    same link and the exported rows, within the tolerance of tests/test_gpu_graph_joint.py.  Node 9 of the second session lands within the
    5 cm of the truth that tests/test_gpu_loop_register.py asks of the loop closed inside one sequence."""
    gpu, fx = world["gpu"], world["fx"][0]
    qg, tg = guess_of(pg, world["nodes"][0], 4, 9)
    res = gpu.graph_register_links([(0, 4, 0, 9, 2, 9, 0, qg, tg)])[0]
    link = lr.link_from_result(res, 0, 4, 2, 9)
    assert link is not None and int(link["flags"][0]) == pg.EDGE_ROBUST and raw(link["info"][0]) == raw(res["info"])
    before = [(gpu.graph_export(b), gpu.graph_export(b, edges=True)) for b in (0, 2)]
    out = gpu.graph_optimize_joint([([0, 2], link, [0, 1])], **OPTIONS)[0]
    after = [gpu.graph_export(b) for b in (0, 2)]
    want, m, _ = pg.optimize_joint(before, link, seqs=[0, 2], align=[0, 1], **OPTIONS)
    q, t = np.concatenate([a["q_opt"] for a in after]), np.concatenate([a["t_opt"] for a in after])
    qm, tm = np.concatenate([w[0]["q_opt"] for w in want]), np.concatenate([w[0]["t_opt"] for w in want])
    diff = pg.pose_difference(q, t, qm, tm)
    d9 = np.linalg.norm(after[1]["t_opt"][9] - fx["t_true"][9])
    print(f"joint solve: status {out['status']}, device against the model {diff:.3e} (tolerance {8 * eps_ref():.2e}); node 9 of the second session {d9:.4f} m from the truth, "
          f"entered {np.linalg.norm(world['nodes'][0]['t'][9] - fx['t_true'][9]):.4f} m")
    assert int(out["status"]) == 0 == m["status"] and diff <= 8 * eps_ref() and d9 < 0.05
    A = pg.frame_from_link(before[0][0]["q_opt"][4], before[0][0]["t_opt"][4], link[0], before[1][0]["q_opt"][9], before[1][0]["t_opt"][9])
    placed = pg.compose(*A, before[1][0]["q_opt"], before[1][0]["t_opt"])
    assert np.abs(placed[1] - after[1]["t_opt"]).max() < 1e-6                       # one link: the solve leaves the aligned session where A put it


# ---- the proposal ------------------------------------------------------------------------------------------------------------------------
LINE_COUNTS = (255, 256, 257, 1023, 1024, 1025)
HITS = gc.HITS


def line(n):
    t = np.zeros((n, 3))
    t[:, 0] = 4.0 * np.arange(n)
    return gc.make_nodes(t)


def query_nodes():
    """The query session: node 0 at the origin, node 1 beside node 0 of a line, nodes 2 .. 7 beside the last node of every line, node 8 at
    (1, 2, 3) for `estimates`, node 9 far from everything, node 10 on the z axis for the window's top; rotations and estimates of their own."""
    rng = np.random.default_rng(5)
    t = np.zeros((11, 3))
    t[1] = (-1.0, 1.0, 0.0)
    for k, n in enumerate(LINE_COUNTS):
        t[2 + k] = (4.0 * (n - 1) + 1.0, 1.0, 0.0)
    t[8], t[9], t[10] = (1.0, 2.0, 3.0), (0.0, 5.0e5, 0.0), (0.0, 0.0, 0.5)
    q = pg.qexp(rng.uniform(-1.0, 1.0, (11, 3)))
    return gc.make_nodes(t, q)


P_GRAPHS = {"query": query_nodes(), "crowd": gc.GRAPHS["crowd"], "rim": gc.GRAPHS["rim"], "ties": gc.GRAPHS["ties"], "passes": gc.GRAPHS["passes"],
            "estimates": gc.GRAPHS["estimates"], "laps": gc.GRAPHS["laps1"]}
P_GRAPHS.update({"line%d" % n: line(n) for n in LINE_COUNTS})
A_FRAME = (pg.stored_q(jc.FRAME[0]), np.array(jc.FRAME[1]))
_lq, _lt = pg.compose(*pg.inverse(*A_FRAME), gc.GRAPHS["laps1"]["q"], gc.GRAPHS["laps1"]["t"])
P_GRAPHS["laps away"] = gc.make_nodes(_lt, _lq)                                    # the laps session in a frame of its own: A carries it back
P_NAMES = list(P_GRAPHS)
P_SEQ = {name: s for s, name in enumerate(P_NAMES)}


def pcase(name, graph_i, graph_j, j, frame=None, expect=None, pose=pg.POSE_OPTIMIZED, **p):
    return dict(name=name, i=graph_i, jg=graph_j, j=j, frame=frame, expect=expect, pose=pose, p=dict(dict(radius_m=4.0, half_window=0, separation=0, K=3), **p))


def proposal_cases():
    n = 3 * HITS
    cases = []
    for k, c in enumerate(LINE_COUNTS):
        cases.append(pcase("line %d, first" % c, "line%d" % c, "query", 1, expect=[0], half_window=3))
        cases.append(pcase("line %d, last" % c, "line%d" % c, "query", 2 + k, expect=[c - 1, c - 2], radius_m=6.0, half_window=3))
    for h in (HITS - 2, HITS - 1, HITS, 3 * HITS):                                  # h + 1 hits: node n itself lies at the origin
        cases.append(pcase("crowd, %d hits" % (h + 1), "crowd", "query", 0, expect=[n, n - 1, n - 2, n - 3], radius_m=0.5 * h, K=4))
        cases.append(pcase("crowd, %d hits, wide separation" % (h + 1), "crowd", "query", 0, radius_m=0.5 * h, separation=HITS + 76, K=16))
    cases.append(pcase("rim, on it", "rim", "query", 0, expect=[40, 7], radius_m=5.0, K=4))
    cases.append(pcase("rim, just inside it", "rim", "query", 0, expect=[40], radius_m=float(np.nextafter(5.0, 0.0)), K=4))
    cases.append(pcase("ties, three", "ties", "query", 0, expect=[500, 5, 3, 200, 450], radius_m=5.0, K=16))
    cases.append(pcase("ties, K = 1", "ties", "query", 0, expect=[500], radius_m=5.0, K=1))
    cases.append(pcase("ties, the lowest shadowed", "ties", "query", 0, expect=[500, 5, 200, 450], radius_m=5.0, separation=2, K=4))
    for sep in (0, 2, 6, 50):
        cases.append(pcase("passes, separation %d" % sep, "passes", "query", 0, radius_m=4.0, half_window=5, separation=sep, K=16))
    cases.append(pcase("window clamped at 0", "line255", "query", 1, expect=[0], half_window=4))
    cases.append(pcase("window clamped at the top", "crowd", "query", 10, expect=[n - 1, n - 2, n], radius_m=1.0, half_window=4))
    cases.append(pcase("no hit", "line1024", "query", 9, expect=[], K=16))
    cases.append(pcase("estimates, entered", "estimates", "query", 8, expect=[30, 4, 9], radius_m=3.0, half_window=2, K=4, pose=pg.POSE_ENTERED))
    cases.append(pcase("estimates, optimised", "estimates", "query", 8, expect=[30, 12, 4], radius_m=3.0, half_window=2, K=4, pose=pg.POSE_OPTIMIZED))
    for j in gc.LAPS_QUERIES:
        cases.append(pcase("laps, a real frame, j %d" % j, "laps", "laps away", j, frame=A_FRAME, radius_m=3.0, half_window=3, separation=6, K=4))
        cases.append(pcase("laps, no frame, j %d" % j, "laps", "laps away", j, radius_m=150.0, half_window=3, separation=6, K=4))
    return cases


def frames_arg(frame):
    return None if frame is None else np.concatenate([frame[0], frame[1]])[None]


def p_expected(w, c):
    ni, nj = w["nodes"][P_SEQ[c["i"]]], w["nodes"][P_SEQ[c["jg"]]]
    req, count, d2 = pg.propose_links(*gc.poses(ni, c["pose"]), *gc.poses(nj, c["pose"]), c["j"], c["frame"], seq_i=P_SEQ[c["i"]], seq_j=P_SEQ[c["jg"]], pose=c["pose"], **c["p"])
    return req.tobytes(), count, d2.tobytes()


def p_got(out, k):
    req, counts, d2 = out
    return req[k].tobytes(), int(counts[k]), d2[k].tobytes()


@pytest.fixture(scope="module")
def pworld(binding):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=len(P_NAMES), max_points=4096)
    gpu.graph_enable(max(len(g) for g in P_GRAPHS.values()), 16)
    recs = [gr.pack(P_GRAPHS[name], np.zeros(0, pg.EDGE_DTYPE), seq=P_SEQ[name]) for name in P_NAMES]
    gpu.graph_load(list(range(len(P_NAMES))), np.concatenate(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]))
    gpu.synchronize()
    w = dict(gpu=gpu, B=binding, nodes={s: gpu.graph_export(s) for s in range(len(P_NAMES))}, cases=proposal_cases())
    w["out"] = [gpu.graph_propose_links([(P_SEQ[c["jg"]], c["j"], P_SEQ[c["i"]])], frames=frames_arg(c["frame"]), pose=c["pose"], **c["p"]) for c in w["cases"]]
    yield w
    gpu.close()


def test_every_proposal_case_against_the_model(pworld):
    bad = []
    for c, out in zip(pworld["cases"], pworld["out"]):
        want, have = p_expected(pworld, c), p_got(out, 0)
        taken = out[0][0]["i"][:have[1]].tolist()
        print(c["name"], "count", have[1], "taken", taken, "windows", [(int(r["first"]), int(r["count"])) for r in out[0][0][:have[1]]])
        if have != want or (c["expect"] is not None and taken != c["expect"]):
            bad.append((c["name"], taken))
    assert not bad, bad


def test_the_list_and_the_rescan_agree_and_empty_rows_are_zero(pworld):
    outs = {c["name"]: out for c, out in zip(pworld["cases"], pworld["out"])}
    a, b, c, d = (outs["crowd, %d hits" % (h + 1)] for h in (HITS - 2, HITS - 1, HITS, 3 * HITS))       # 1023, 1024: the list; 1025, 3073: the rescan
    assert p_got(a, 0) == p_got(b, 0) == p_got(c, 0) == p_got(d, 0) and p_got(a, 0)[1] == 4
    wide = outs["crowd, %d hits, wide separation" % (3 * HITS + 1)]
    assert int(wide[1][0]) == 3 and not wide[0][0][3:].tobytes().strip(b"\0") and not wide[2][0][3:].any()
    none = outs["no hit"]
    assert int(none[1][0]) == 0 and not none[0].tobytes().strip(b"\0") and not none[2].any()
    top = outs["window clamped at the top"][0][0]
    n = 3 * HITS
    assert [(int(r["first"]), int(r["count"])) for r in top[:3]] == [(n - 5, 6), (n - 6, 7), (n - 4, 5)]
    low = outs["window clamped at 0"][0][0]
    assert (int(low[0]["first"]), int(low[0]["count"])) == (0, 5)


def test_no_frame_against_the_identity_frame(pworld):
    """The selection and the indices are equal; the guess's bits are not claimed (the identity costs roundings)."""
    gpu = pworld["gpu"]
    ident = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    for name, j in (("ties", 0), ("estimates", 8), ("line257", 4)):
        q = [(P_SEQ["query"], j, P_SEQ[name])]
        kw = dict(radius_m=6.0, half_window=2, separation=1, K=8)
        a, b = gpu.graph_propose_links(q, **kw), gpu.graph_propose_links(q, frames=ident, **kw)
        assert int(a[1][0]) == int(b[1][0]) >= 1 and a[2].tobytes() == b[2].tobytes()
        for f in ("seq_i", "i", "first", "count", "seq_j", "j", "pose"):
            assert a[0][f].tolist() == b[0][f].tolist(), f
        assert np.abs(a[0]["q"] - b[0]["q"]).max() < 1e-12 and np.abs(a[0]["t"] - b[0]["t"]).max() < 1e-9


def test_a_real_frame_brings_the_session_home(pworld):
    """The laps session moved by A^-1 and queried with A takes the nodes the unmoved session takes from itself."""
    gpu = pworld["gpu"]
    for j in gc.LAPS_QUERIES:
        home = pg.propose_links(P_GRAPHS["laps"]["q"], P_GRAPHS["laps"]["t"], P_GRAPHS["laps"]["q"], P_GRAPHS["laps"]["t"], j, None, 3.0, 3, 6, 4)
        out = gpu.graph_propose_links([(P_SEQ["laps away"], j, P_SEQ["laps"])], frames=frames_arg(A_FRAME), radius_m=3.0, half_window=3, separation=6, K=4)
        assert int(out[1][0]) == home[1] >= 1 and out[0][0]["i"].tolist() == home[0]["i"].tolist(), j
        assert np.abs(out[0][0]["t"] - home[0]["t"]).max() < 1e-9


def test_a_query_does_not_depend_on_its_batch_and_nothing_else_is_written(pworld):
    import torch
    gpu = pworld["gpu"]
    kw = dict(radius_m=5.0, half_window=3, separation=2, K=4)
    qs = [(P_SEQ["query"], 0, P_SEQ[n]) for n in ("ties", "rim", "crowd", "passes", "line1025")] + [(P_SEQ["query"], 9, P_SEQ["ties"]), (P_SEQ["laps"], 45, P_SEQ["ties"]),
                                                                                                      (P_SEQ["query"], 1, P_SEQ["line256"])]
    frames = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (len(qs), 1))
    frames[1] = np.concatenate(A_FRAME)
    lone = [p_got(gpu.graph_propose_links([q], frames=frames[k:k + 1], **kw), 0) for k, q in enumerate(qs)]
    assert sum(l[1] > 0 for l in lone) >= 5
    fwd = gpu.graph_propose_links(qs, frames=frames, **kw)
    back = gpu.graph_propose_links(qs[::-1], frames=frames[::-1], pinned=False, **kw)
    n = len(qs)
    assert [p_got(fwd, k) for k in range(n)] == lone and [p_got(back, n - 1 - k) for k in range(n)] == lone
    rounds = gc.constant("kProposeStageItems") + 5
    idx = [k % n for k in range(rounds)]
    long = gpu.graph_propose_links([qs[k] for k in idx], frames=frames[idx], **kw)
    assert all(p_got(long, k) == lone[idx[k]] for k in range(rounds))
    K = kw["K"]
    sizes = dict(dst=n * K * 96, counts=n * 4, dist2=n * K * 8)
    for with_dist2 in (True, False):
        buf = {k: torch.full((v + TAIL,), SENTINEL, dtype=torch.uint8, pin_memory=True) for k, v in sizes.items()}
        gpu.graph_propose_links_into(qs, buf["dst"].data_ptr(), buf["counts"].data_ptr(), buf["dist2"].data_ptr() if with_dist2 else 0, frames=frames, **kw)
        gpu.synchronize()
        whole = dict(dst=fwd[0].tobytes(), counts=fwd[1].astype(np.int32).tobytes(), dist2=fwd[2].tobytes())
        for k, size in sizes.items():
            b = buf[k].numpy()
            assert (b[size:] == SENTINEL).all(), k
            if with_dist2 or k != "dist2":
                assert b[:size].tobytes() == whole[k], k
            else:
                assert (b == SENTINEL).all()
    assert all(gpu.graph_export(s).tobytes() == pworld["nodes"][s].tobytes() for s in pworld["nodes"])     # the graphs are only read


def test_proposal_refusals_leave_the_destinations_alone(pworld):
    import torch
    gpu, B = pworld["gpu"], pworld["B"]
    K = 4
    buf = {k: torch.full((v,), SENTINEL, dtype=torch.uint8, pin_memory=True) for k, v in dict(dst=2 * K * 96 + 16, counts=2 * 4 + 16, dist2=2 * K * 8 + 16).items()}
    ptr = {k: v.data_ptr() for k, v in buf.items()}
    Q, T, R = P_SEQ["query"], P_SEQ["ties"], P_SEQ["rim"]
    ident = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (2, 1))
    good = dict(queries=[(Q, 0, T), (Q, 0, R)], dst=ptr["dst"], counts=ptr["counts"], dist2=ptr["dist2"], frames=ident, pose=1, radius_m=5.0, half_window=3, separation=2, K=K)
    pageable = np.zeros(4096, np.uint8)

    def frame(**at):
        f = ident.copy()
        for k, v in at.items():
            f[1, int(k[1:])] = v
        return f
    refused = [dict(queries=[(-1, 0, T)]), dict(queries=[(len(P_NAMES), 0, T)]), dict(queries=[(Q, 0, -1)]), dict(queries=[(Q, 0, len(P_NAMES))]), dict(queries=[(Q, 0, Q)]),
               dict(queries=[(Q, -1, T)]), dict(queries=[(Q, 11, T)]), dict(queries=[(Q, 0, T), (R, 41, T)]), dict(pose=2), dict(pose=-1), dict(radius_m=float("nan")),
               dict(radius_m=float("inf")), dict(radius_m=-1.0), dict(half_window=-1), dict(separation=-1), dict(K=0), dict(K=17),
               dict(frames=frame(f3=1.001)), dict(frames=frame(f0=float("nan"))), dict(frames=frame(f5=float("inf"))),
               dict(dst=pageable.ctypes.data), dict(counts=pageable.ctypes.data), dict(dist2=pageable.ctypes.data), dict(dst=0), dict(counts=0),
               dict(dst=ptr["dst"] + 4), dict(counts=ptr["counts"] + 2), dict(dist2=ptr["dist2"] + 4)]
    for change in refused:
        a = dict(good, **change)
        if len(a["queries"]) != 2:
            a["frames"] = a["frames"][:len(a["queries"])]
        with pytest.raises(B.AloamError) as e:
            gpu.graph_propose_links_into(a.pop("queries"), a.pop("dst"), a.pop("counts"), a.pop("dist2"), **a)
        assert e.value.code == B.E_ARG, change
    L = B.lib()
    qs = np.array(good["queries"], np.int32)
    tail = (1, 5.0, 3, 2, K, ptr["dst"], ptr["counts"], ptr["dist2"])
    assert L.aloam_graph_propose_links(gpu.h, qs.ctypes.data, None, -1, *tail) == B.E_ARG and L.aloam_graph_propose_links(gpu.h, None, None, 2, *tail) == B.E_ARG
    assert L.aloam_graph_propose_links(gpu.h, None, None, 0, *tail) == 0            # n = 0 is ALOAM_OK
    gpu.synchronize()
    assert all((v.numpy() == SENTINEL).all() for v in buf.values())
    assert all(gpu.graph_info(s)["nodes"] == len(P_GRAPHS[n]) for n, s in P_SEQ.items())
    a = dict(good)
    gpu.graph_propose_links_into(a.pop("queries"), a.pop("dst"), a.pop("counts"), a.pop("dist2"), **a)      # and the call they vary is accepted
    gpu.synchronize()
    assert buf["counts"].numpy()[:8].view(np.int32).tolist() == [4, 2]
    bare = B.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=4096)
    try:
        with pytest.raises(B.AloamError) as e:
            bare.graph_propose_links_into([(0, 0, 1)], ptr["dst"], ptr["counts"], 0, radius_m=3.0)
        assert e.value.code == B.E_STATE
    finally:
        bare.close()
