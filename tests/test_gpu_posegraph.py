"""Pose graphs on the MI355X (aloam_graph_*): the store against aloam_export_poses and the numpy model, the batched solve against the
model's dense Levenberg-Marquardt (a-loam_amd/posegraph.py), its independence of the list, and every refusal.

Graphs are entered through aloam_set_state (the odometry pose each node reads) and aloam_graph_add_nodes; the model is fed what the device
exports (entered poses, odometry edges), so both sides solve the same problem bit for bit.  Tolerance for poses and cost: 8 eps_ref
(posegraph_cases.eps_ref(), what two CPU solvers differ by on the 300-node graph, measured in the run): the device's LM takes another path - inexact PCG steps - to the same minimum.
Every comparison prints the device's deviation."""
import ctypes as C

import numpy as np
import pytest

import posegraph_cases as pc
from posegraph_cases import OPTIONS, eps_ref, pg

pytestmark = pytest.mark.gpu


def tol():
    return 8 * eps_ref()


def ctx(binding, B, max_nodes=320, max_edges=420, graph=True, **kw):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=B, max_points=4096, **kw)
    if graph:
        gpu.graph_enable(max_nodes, max_edges)
    return gpu


def state(gpu, seq):
    n, e = gpu.graph_export(seq), gpu.graph_export(seq, edges=True)
    return n, e


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def solve_model(nodes, edges, robust_delta=1.0, chain=False):
    o = dict(OPTIONS, huber_delta=robust_delta)
    return (pg.chain_pcg if chain else pg.optimize)(nodes["q_opt"], nodes["t_opt"], edges, **o)


def against_model(gpu, seq, res, nodes0, edges, what, chain=True):
    """The device's result for `seq` against the model started from the same estimates: cost, poses, gradient, PCG count."""
    q, t, m = solve_model(nodes0, edges)
    out = gpu.graph_export(seq)
    dev = pg.pose_difference(out["q_opt"], out["t_opt"], q, t)
    dcost = abs(res["final_cost"] - m["final_cost"])
    g = float(np.abs(pg.gradient(out["q_opt"], out["t_opt"], edges, OPTIONS["huber_delta"])).max())
    print(f"{what}: device vs model pose {dev:.3e} cost {dcost:.3e} (tolerance {tol():.2e}); termination {res['termination']} LM {res['lm_iterations']} "
          f"accepted {res['accepted_steps']} PCG {res['pcg_iterations']}; model LM {m['lm_iterations']}; model gradient at device poses {g:.3e}")
    assert res["status"] == 0 and res["nodes"] == len(nodes0) and res["edges"] == len(edges)
    assert np.isclose(res["initial_cost"], m["initial_cost"], rtol=1e-12, atol=0)
    assert dev <= tol() and dcost <= tol()
    if res["termination"] == 3:
        assert g <= 2 * OPTIONS["gradient_tolerance"]
    assert all(out[f].tobytes() == nodes0[f].tobytes() for f in ("q", "t", "frame"))                    # the entered poses never change
    if chain:
        _, _, mc = solve_model(nodes0, edges, chain=True)
        print(f"{what}: PCG iterations device {res['pcg_iterations']}, model chain_pcg {mc['pcg_iterations']}")
        assert res["pcg_iterations"] <= 2 * mc["pcg_iterations"]
    return out, (q, t)


@pytest.fixture(scope="module")
def laps():
    return pg.drifted_laps(1, 300, 2)


def test_nodes_are_the_exported_poses_and_edges_the_relative_poses(binding):
    import torch
    gpu = ctx(binding, 3)
    d = pg.drifted_laps(5, 9, 0)
    info = d["info"]
    rec = torch.zeros(3 * C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)
    want = {0: [], 2: []}
    for k in range(9):
        listed = [0, 2] if k % 2 == 0 else [0]                     # sequence 2 takes every other pose; sequence 1 never
        for b in listed:
            gpu.set_state(pc.IDENT_Q, pc.ZERO_T, d["q"][k], d["t"][k], seq=b)
        gpu.export_poses(rec.data_ptr())
        assert gpu.graph_add_nodes(listed, info) == [len(want[b]) for b in listed]
        gpu.synchronize()
        recs = (binding.AloamPoseRecord * 3).from_buffer_copy(rec.numpy().tobytes())
        for b in listed:
            want[b].append((np.array(recs[b].q_w), np.array(recs[b].t_w)))
    assert gpu.graph_info(1) == {"nodes": 0, "edges": 0, "max_nodes": 320, "max_edges": 420}
    worst = 0.0
    for b in (0, 2):
        n, e = state(gpu, b)
        assert len(n) == len(want[b]) and len(e) == len(n) - 1 and (n["frame"] == -1).all()
        q, t = np.array([w[0] for w in want[b]]), np.array([w[1] for w in want[b]])
        assert bits(n["q"]).tobytes() == bits(q).tobytes() and bits(n["t"]).tobytes() == bits(t).tobytes()
        qz, tz = pg.relative_pose(q[:-1], t[:-1], q[1:], t[1:])
        worst = max(worst, np.abs(e["q"] - qz).max(), np.abs(e["t"] - tz).max())
        assert (e["i"] == np.arange(len(e))).all() and (e["j"] == np.arange(1, len(n))).all() and (e["seq"] == b).all() and (e["flags"] == 0).all()
        assert np.array_equal(e["info"], np.tile(pg.info_upper(info), (len(e), 1)))
        # the estimate: node 0 as entered, then X_opt[k - 1] o Z
        assert bits(n["q_opt"][0]).tobytes() == bits(n["q"][0]).tobytes() and bits(n["t_opt"][0]).tobytes() == bits(n["t"][0]).tobytes()
        qo, to = pg.compose(n["q_opt"][:-1], n["t_opt"][:-1], e["q"], e["t"])
        worst = max(worst, np.abs(n["q_opt"][1:] - qo).max(), np.abs(n["t_opt"][1:] - to).max())
    print(f"odometry edges and estimates against relative_pose / compose: {worst:.3e} (bound 1e-14)")
    assert worst <= 1e-14
    gpu.close()


def test_six_adds_in_a_row_wrap_the_staging_ring(binding):
    """Six aloam_graph_add_nodes calls with nothing synchronising between them: the pinned ring of four slots wraps, so calls five and six
    fill the slots of calls one and two.  Every call lists other sequences with another information, so a slot filled too early shows as a
    node in the wrong row or an edge with the wrong information.  Nodes and edges equal those of a context that synchronised after every
    call, byte for byte."""
    d = pg.drifted_laps(5, 4, 0)
    lists = [[0, 1, 2, 3], [3, 1], [2], [0, 3, 2], [1, 0], [3, 2, 1, 0]]
    out = []
    for wait in (False, True):
        gpu = ctx(binding, 4, max_nodes=8, max_edges=8)
        for b in range(4):
            gpu.set_state(pc.IDENT_Q, pc.ZERO_T, d["q"][b], d["t"][b], seq=b)
        for k, listed in enumerate(lists):
            gpu.graph_add_nodes(listed, np.stack([np.eye(6) * (10.0 * k + b + 1) for b in listed]))
            if wait:
                gpu.synchronize()
        out.append([state(gpu, b) for b in range(4)])
        gpu.close()
    for b in range(4):
        (n0, e0), (n1, e1) = out[0][b], out[1][b]
        calls = [k for k, listed in enumerate(lists) if b in listed]
        assert len(n0) == len(calls) == len(n1) and len(e0) == len(calls) - 1 == len(e1)
        assert n0.tobytes() == n1.tobytes() and e0.tobytes() == e1.tobytes()
        assert np.array_equal(e0["info"], np.stack([pg.info_upper(np.eye(6) * (10.0 * k + b + 1)) for k in calls[1:]]))


def test_with_mapping_the_node_is_the_map_pose(binding):
    import torch
    gpu = ctx(binding, 2, graph=False)
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 16)
    gpu.graph_enable(4, 4)
    gpu.set_map_frame([10, 10, 5], [0.0, 0.0, np.sin(0.1), np.cos(0.1)], [1.0, 2.0, 3.0], 7, seq=1)
    rec = torch.zeros(2 * C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)
    gpu.export_poses(rec.data_ptr())
    gpu.graph_add_nodes([1], np.eye(6))
    n = gpu.graph_export(1)
    r = (binding.AloamPoseRecord * 2).from_buffer_copy(rec.numpy().tobytes())[1]
    assert bits(n["q"][0]).tobytes() == bits(np.array(r.map_q_w)).tobytes() and bits(n["t"][0]).tobytes() == bits(np.array(r.map_t_w)).tobytes()
    assert n["frame"][0] == r.map_frames
    gpu.close()


def test_a_pure_chain_is_already_optimal(binding, laps):
    gpu = ctx(binding, 1)
    pc.enter(gpu, {0: (laps["q"][:70], laps["t"][:70])}, laps["info"])
    before, edges = state(gpu, 0)
    res = gpu.graph_optimize([0], **OPTIONS)[0]
    after = gpu.graph_export(0)
    # cost 0 up to the roundings of re-evaluating Z^-1 o X[k-1]^-1 o X[k] with the estimates: |r| <= 1e-13 (a handful of roundings on
    # translations of ten metres and on quaternions composed 70 times), s <= |r|^2 |Omega| with |Omega| = 4e4
    bound = 0.5 * len(edges) * 6 * (1e-13) ** 2 * 4e4
    print(f"pure chain: cost {res['final_cost']:.3e} (bound {bound:.1e}), gradient {res['gradient_max']:.3e}, termination {res['termination']}")
    assert res["status"] == 0 and res["accepted_steps"] == 0 and res["final_cost"] == res["initial_cost"] <= bound
    assert bits(after).tobytes() == bits(before).tobytes()
    gpu.close()


def test_drifted_laps_reach_the_models_minimum(binding, laps):
    gpu = ctx(binding, 2)
    pc.enter(gpu, {1: (laps["q"], laps["t"])}, laps["info"])
    gpu.graph_add_edges(pc.with_seq(laps["loop"], 1))
    nodes0, edges = state(gpu, 1)
    assert len(nodes0) == 300 and len(edges) == 301
    res = gpu.graph_optimize([1], **OPTIONS)[0]
    out, _ = against_model(gpu, 1, res, nodes0, edges, "drifted laps 300 / 2")
    before, after = pg.ate(nodes0["t_opt"], laps["t_true"]), pg.ate(out["t_opt"], laps["t_true"])
    print(f"ATE before {before:.4f} m, after {after:.4f} m")
    assert after < before
    gpu.close()


def test_a_hub_with_seventy_loops_and_three_anchors(binding):
    d = pg.drifted_laps(3, 90, 0)
    gpu = ctx(binding, 1, max_nodes=96, max_edges=200)
    pc.enter(gpu, {0: (d["q"], d["t"])}, d["info"])
    rng = np.random.default_rng(11)
    others = np.array([k for k in range(1, 90) if k != 40][:70])
    qz, tz = pg.relative_pose(d["q_true"][40], d["t_true"][40], d["q_true"][others], d["t_true"][others])
    qz = pg.qmul(qz, pg.qexp(5e-3 * rng.standard_normal((70, 3))))
    loops = pg.make_edges(0, np.full(70, 40), others, qz, tz + 5e-2 * rng.standard_normal((70, 3)), d["info"])
    loops[::2] = pg.make_edges(0, others[::2], np.full(35, 40), *pg.inverse(qz[::2], loops["t"][::2]), d["info"])   # both orientations
    anchors = np.concatenate([pg.anchor_from_localization(j, d["q_true"][j], d["t_true"][j] + 0.01, 4 * d["info"]) for j in (17, 55, 88)])
    gpu.graph_add_edges(np.concatenate([loops, anchors]))
    nodes0, edges = state(gpu, 0)
    assert len(edges) == 89 + 73 and (edges["i"] == -1).sum() == 3
    res = gpu.graph_optimize([0], **OPTIONS)[0]
    against_model(gpu, 0, res, nodes0, edges, "hub 70 + 3 anchors")
    gpu.close()


def test_a_robust_edge_discounts_an_outlier(binding):
    d = pg.drifted_laps(7, 60, 3)
    bad = d["loop"][1:2].copy()
    bad["t"] += [4.0, -3.0, 1.0]
    gpu = ctx(binding, 3, max_nodes=64, max_edges=80)
    pc.enter(gpu, {b: (d["q"], d["t"]) for b in range(3)}, d["info"])
    clean = np.concatenate([d["loop"][:1], d["loop"][2:]])
    flagged = bad.copy()
    flagged["flags"] = binding.GRAPH_EDGE_ROBUST
    gpu.graph_add_edges(np.concatenate([pc.with_seq(clean, 0), pc.with_seq(clean, 1), pc.with_seq(bad, 1), pc.with_seq(clean, 2), pc.with_seq(flagged, 2)]))
    start = {b: state(gpu, b) for b in range(3)}
    res = gpu.graph_optimize([0, 1, 2], **OPTIONS)
    out = {}
    for b, what in ((0, "no outlier"), (1, "outlier, plain"), (2, "outlier, robust")):
        out[b], _ = against_model(gpu, b, res[b], *start[b], what, chain=False)
    to_clean = lambda b: pg.pose_difference(out[b]["q_opt"], out[b]["t_opt"], out[0]["q_opt"], out[0]["t_opt"])
    print(f"distance to the outlier-free optimum: robust {to_clean(2):.4f}, plain {to_clean(1):.4f}")
    assert to_clean(2) < to_clean(1)
    gpu.close()


def test_results_do_not_depend_on_the_list(binding, laps):
    sizes = {0: 1, 1: 2, 2: 65, 3: 257, 4: 300, 5: 40}

    def loop(pairs):                                                # exact measurements between nodes of the ground truth
        i, j = np.array(pairs).T
        return pg.make_edges(0, i, j, *pg.relative_pose(laps["q_true"][i], laps["t_true"][i], laps["q_true"][j], laps["t_true"][j]), laps["info"])

    loops = {2: loop([(3, 60)]), 3: loop([(5, 250), (40, 200)]), 4: laps["loop"], 5: loop([(2, 35)])}

    def run(order):
        gpu = ctx(binding, 7)
        pc.enter(gpu, {b: (laps["q"][:n], laps["t"][:n]) for b, n in sizes.items()}, laps["info"])
        gpu.graph_add_edges(np.concatenate([pc.with_seq(e, b) for b, e in loops.items()]))
        untouched = gpu.graph_export(5)
        res = {}
        for group in order:
            r = gpu.graph_optimize(group, **OPTIONS)
            res.update({b: r[i].tobytes() for i, b in enumerate(group)})
        nodes = {b: gpu.graph_export(b).tobytes() for b in range(5)}
        assert gpu.graph_export(5).tobytes() == untouched.tobytes() and gpu.graph_info(6)["nodes"] == 0       # unlisted: as they were
        gpu.close()
        return res, nodes

    together = run([[0, 1, 2, 3, 4]])
    alone = run([[b] for b in range(5)])
    backwards = run([[4, 3, 2, 1, 0]])
    assert together == alone == backwards
    r = {b: np.frombuffer(v, binding.GRAPH_RESULT_DTYPE)[0] for b, v in together[0].items()}
    assert r[0]["status"] == binding.GRAPH_NO_EDGES and (r[0]["nodes"], r[0]["edges"]) == (1, 0)
    assert r[1]["status"] == 0 and all(r[b]["status"] == 0 and r[b]["accepted_steps"] > 0 for b in (2, 3, 4))
    print({b: (int(r[b]["lm_iterations"]), int(r[b]["pcg_iterations"]), int(r[b]["termination"])) for b in r})
    # nodes without a single edge (after a clear, one node again): NO_EDGES as well
    gpu = ctx(binding, 1)
    pc.enter(gpu, {0: (laps["q"][:3], laps["t"][:3])}, laps["info"])
    gpu.graph_clear([0])
    pc.enter(gpu, {0: (laps["q"][:1], laps["t"][:1])}, laps["info"])
    assert gpu.graph_optimize([0])[0]["status"] == binding.GRAPH_NO_EDGES
    gpu.close()


def test_warm_start(binding):
    d = pg.drifted_laps(2, 80, 2)
    gpu = ctx(binding, 1)
    pc.enter(gpu, {0: (d["q"][:70], d["t"][:70])}, d["info"])
    gpu.graph_add_edges(d["loop"][:1])
    # The default function tolerance, as a caller would run it: where the first solve stopped, a step changes the cost by less than its
    # rounding (a sum of 70 terms of magnitude 0.1, each good to 1e-13), and with a tolerance of 0 such a step is accepted or not by chance.
    options = dict(OPTIONS, function_tolerance=1e-10)
    first = gpu.graph_optimize([0], **options)[0]
    solved = gpu.graph_export(0)
    second = gpu.graph_optimize([0], **options)[0]
    print(f"first: termination {first['termination']} accepted {first['accepted_steps']}; second: termination {second['termination']} "
          f"LM {second['lm_iterations']} accepted {second['accepted_steps']}")
    assert first["accepted_steps"] > 0 and second["accepted_steps"] == 0 and second["status"] == 0
    assert gpu.graph_export(0).tobytes() == solved.tobytes()
    # a node added afterwards continues from the optimised estimate
    gpu.set_state(pc.IDENT_Q, pc.ZERO_T, d["q"][70], d["t"][70])
    gpu.graph_add_nodes([0], d["info"])
    n, e = state(gpu, 0)
    qo, to = pg.compose(n["q_opt"][69], n["t_opt"][69], e["q"][-1], e["t"][-1])
    assert e["i"][-1] == 69 and e["j"][-1] == 70
    assert np.abs(n["q_opt"][70] - qo).max() <= 1e-14 and np.abs(n["t_opt"][70] - to).max() <= 1e-14
    assert np.abs(n["t_opt"][70] - n["t"][70]).max() > 1e-3                     # not the drifted pose
    gpu.close()


def test_states_and_errors_queue_nothing(binding, laps):
    import torch
    L = binding.lib()
    info = laps["info"]
    off = ctx(binding, 2, graph=False)
    ids = np.zeros(1, np.int32)
    for rc in (L.aloam_graph_add_nodes(off.h, binding._p(ids), 1, binding._p(np.zeros(21))), L.aloam_graph_clear(off.h, binding._p(ids), 1),
               L.aloam_graph_info(off.h, 0, binding._p(np.zeros(4, np.int32))), L.aloam_graph_optimize(off.h, binding._p(ids), 1, None, None)):
        assert rc == binding.E_STATE                                               # not enabled
    off.close()
    gpu = ctx(binding, 2, max_nodes=4, max_edges=4)
    with pytest.raises(binding.AloamError) as err:
        gpu.graph_enable(4, 4)
    assert err.value.code == binding.E_STATE
    pc.enter(gpu, {0: (laps["q"][:4], laps["t"][:4]), 1: (laps["q"][:2], laps["t"][:2])}, info)
    before = [state(gpu, b) for b in range(2)]

    def refused(code, call):
        with pytest.raises(binding.AloamError) as err:
            call()
        assert err.value.code == code, err.value
        assert [gpu.graph_info(b) for b in range(2)] == [dict(nodes=4, edges=3, max_nodes=4, max_edges=4), dict(nodes=2, edges=1, max_nodes=4, max_edges=4)]

    ok = pg.make_edges(1, 0, 1, pc.IDENT_Q, pc.ZERO_T, info)
    refused(binding.E_CAPACITY, lambda: gpu.graph_add_nodes([1, 0], info))                                   # a full node row, after a good one
    refused(binding.E_CAPACITY, lambda: gpu.graph_add_edges(np.concatenate([pc.with_seq(ok, 0)] * 2)))       # one fits, two do not
    for field, value in (("seq", 2), ("i", -2), ("i", 2), ("j", -1), ("j", 2), ("i", 1), ("flags", 2)):
        e = ok.copy(); e[field] = value
        refused(binding.E_ARG, lambda: gpu.graph_add_edges(np.concatenate([ok, e])))                         # bad indices, after a good edge
    for what in ("nan", "indefinite", "semidefinite", "q_norm", "q_nan", "t_inf"):
        e = ok.copy()
        if what == "nan": e["info"][0, 3] = np.nan
        if what == "indefinite": e["info"][0] = pg.info_upper(np.diag([1, 1, 1, 1, 1, -1.0]))
        if what == "semidefinite": e["info"][0] = pg.info_upper(np.ones((6, 6)))
        if what == "q_norm": e["q"][0] = [0, 0, 0, 1.00001]
        if what == "q_nan": e["q"][0] = [np.nan, 0, 0, 1]
        if what == "t_inf": e["t"][0] = [np.inf, 0, 0]
        refused(binding.E_ARG, lambda: gpu.graph_add_edges(e))
    refused(binding.E_ARG, lambda: gpu.graph_add_nodes([1], np.diag([1, 1, 1, 1, 1, 0.0])))
    refused(binding.E_ARG, lambda: gpu.graph_add_nodes([1, 1], info))
    pageable = np.zeros(4 * 240, np.uint8)
    refused(binding.E_ARG, lambda: gpu.graph_export_into(0, 0, 2, pageable.ctypes.data))                     # refused destinations
    refused(binding.E_ARG, lambda: gpu.graph_export_into(0, 0, 2, pageable.ctypes.data, edges=True))
    refused(binding.E_ARG, lambda: gpu.graph_export_into(0, 0, 2, 0))
    refused(binding.E_ARG, lambda: gpu.graph_export_into(0, 3, 2, torch.zeros(512, dtype=torch.uint8, pin_memory=True).data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_optimize_into([0], pageable.ctypes.data))
    refused(binding.E_ARG, lambda: gpu.graph_optimize_into([0, 0], torch.zeros(128, dtype=torch.uint8, pin_memory=True).data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_optimize([0], huber_delta=0.0))
    on_device = torch.zeros(240, dtype=torch.uint8, device="cuda")                                          # edges are read on the host
    refused(binding.E_ARG, lambda: gpu._check(L.aloam_graph_add_edges(gpu.h, C.c_void_p(on_device.data_ptr()), 1)))
    assert [(n.tobytes(), e.tobytes()) for n, e in (state(gpu, b) for b in range(2))] == [(n.tobytes(), e.tobytes()) for n, e in before]
    # a unit quaternion within 1e-6 is stored normalised
    e = ok.copy(); e["q"][0] = [0, 0, 0, 1 + 5e-7]
    gpu.graph_add_edges(e)
    assert np.abs(gpu.graph_export(1, edges=True)["q"][-1] - [0, 0, 0, 1]).max() <= 2.3e-16
    # reset leaves the graph alone; clear empties it and the row starts again
    gpu.reset_sequences([0, 1])
    assert [(n.tobytes(), e.tobytes()) for n, e in (state(gpu, b) for b in range(1))] == [(before[0][0].tobytes(), before[0][1].tobytes())]
    gpu.graph_clear([0])
    assert gpu.graph_info(0)["nodes"] == 0 and gpu.graph_info(1)["nodes"] == 2
    pc.enter(gpu, {0: (laps["q"][5:7], laps["t"][5:7])}, info)
    n = gpu.graph_export(0)
    assert len(n) == 2 and np.array_equal(n["t"], laps["t"][5:7]) and gpu.graph_info(0)["edges"] == 1
    gpu.close()


def test_a_context_without_graphs_is_unchanged(binding, sequence):
    import torch
    scans, _, _, model = sequence("VLP-16", 3, seed=3)
    out = []
    for graph in (False, True):
        gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=1, max_points=40000)
        gpu.profile_enable(True)
        if graph:
            gpu.graph_enable(8, 8)
        for s in scans:
            gpu.scan_register(s)
            gpu.odometry_step()
            if graph:
                gpu.graph_add_nodes([0], np.eye(6) * 100.0)
        if graph:
            r = gpu.graph_optimize([0])[0]
            assert r["status"] == 0 and (r["nodes"], r["edges"]) == (3, 2)
        rec = torch.zeros(C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)
        gpu.export_poses(rec.data_ptr())
        gpu.synchronize()
        got = {k: v.tobytes() for k, v in gpu.pose().items()}
        got.update(record=rec.numpy().tobytes(), stats=str(gpu.odom_stats()), features={k: v.tobytes() for k, v in gpu.features().items()},
                   corr=[a.tobytes() for a in gpu.correspondences()])
        prof = gpu.profile()
        assert prof["pose_graph"]["launches"] == (1 if graph else 0)
        got["launches"] = {k: v["launches"] for k, v in prof.items() if k != "pose_graph"}
        out.append(got)
        gpu.close()
    assert out[0] == out[1]
