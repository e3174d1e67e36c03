"""A solved pose graph carried into the live pose and the window map on the MI355X (aloam_graph_apply): the correction and the live poses
against posegraph.apply_correction fed the node bits exported before the call; the rebuilt window, bit for bit and in order, against
atlas.window_from_keyframes fed the device's stacks, the read-back estimates and the oracle's input-order voxel filter; a twin context
prepared with aloam_set_map / aloam_set_map_frame that continues with the same bits; pools, list independence, stream order, the host
state, the refusals and the opt-in.

Hand-made clouds with the solver off (lm_max_iterations = 0), as in test_gpu_graph_map.py, except for the twin continuation, which drives
rendered VLP-16 sweeps of 250 columns through the whole pipeline with the solver on."""
import importlib

import numpy as np
import pytest

from test_gpu_graph_map import INFO, LEAF, Q_ID, Q_X, Q_Z, boundary_points, cloud, context, step

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
# sequence 1 of the map tests: seven rotated keyframes over cubes -3 .. 3, the last one well inside its cube (-2, 1, -1)
POSES_A = [(Q_Z, (-130.0, -60.0, -120.0)), (Q_ID, (-60.0, 110.0, 0.0)), (Q_ID, (0.0, 0.0, 0.0)), (Q_X, (60.0, -110.0, 120.0)),
           (Q_Z, (130.0, 60.0, 0.0)), (Q_ID, (10.0, 10.0, -60.0)), (Q_X, (-85.0, 35.0, -35.0))]
POSES_0 = [(Q_ID, (1.0, 2.0, 0.5)), (Q_Z, (4.0, 2.0, 0.5)), (Q_ID, (8.0, 3.0, 0.6))]
POSES_2 = [(Q_ID, (5.0, 0.0, 0.0)), (Q_ID, (600.0, 0.0, 0.0)), (Q_Z, (9.0, 1.0, 0.0))]      # the second one 600 m away
POSE, MAP = 1, 3


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


@pytest.fixture(scope="module")
def pg():
    return importlib.import_module("a-loam_amd.posegraph")


def anchor(binding, pg, seq, j, node, dt, rot=(0.0, 0.0, 0.0), weight=400.0):
    """An anchor of node j: its entered pose turned by `rot` (a rotation vector) and moved by `dt`."""
    e = np.zeros(1, binding.GRAPH_EDGE_DTYPE)
    e["seq"], e["i"], e["j"], e["flags"] = seq, -1, j, 0
    q = pg.qmul(pg.qexp(np.array(rot, np.float64)), node["q"])
    e["q"], e["t"] = q / np.linalg.norm(q), node["t"] + np.array(dt)
    e["info"] = (np.eye(6) * weight)[np.triu_indices(6)]
    return e


def getters(gpu, binding, b, store=True):
    """Everything the C ABI tells about sequence b, as bytes."""
    out = [gpu.graph_export(b).tobytes(), gpu.graph_export(b, edges=True).tobytes()]
    out.append(gpu.map_cloud(binding.MAP_CORNER_STACK, b).tobytes() + gpu.map_cloud(binding.MAP_SURF_STACK, b).tobytes())
    out.append(gpu.map_cloud(binding.MAP_REGISTERED, b).tobytes())
    out.append(repr(sorted(gpu.map_info(b).items())))
    out.append(b"".join(v.tobytes() for _, v in sorted(gpu.map_pose(b).items())))
    out.append(b"".join(np.asarray(v).tobytes() for _, v in sorted(gpu.pose(b).items())))
    for cls in (0, 1):
        cubes = gpu.map_cubes(cls, b)
        out.append(repr(sorted(cubes)) + repr([len(cubes[k]) for k in sorted(cubes)]))
        out.append(b"".join(cubes[k].tobytes() for k in sorted(cubes)))
    if store:
        out.append(repr(gpu.graph_keyframe_info(b)))
    return out


def make_world(binding, pg, batch=3, solve=True):
    """Three sequences with 3, 7 and 3 keyframes (POSES_0, POSES_A with the boundary coordinates in keyframe 2, POSES_2), every sequence
    stepped seven times (0 and 2 drive on behind their last keyframe), anchors that disagree with the entered poses by decimetres and a
    few degrees, and a solve.  Returns the context and the stacks of every node."""
    rng = np.random.default_rng(41)
    gpu = context(binding, batch=batch)
    stacks = [[], [], []]
    for k in range(7):
        q0, t0 = POSES_0[k] if k < 3 else (Q_ID, (8.0 + k, 3.0, 0.6))
        q2, t2 = POSES_2[k] if k < 3 else (Q_Z, (9.0 + 0.5 * k, 1.0, 0.0))
        c1, f1 = cloud(rng, 300, (30, 30, 10)), cloud(rng, 1500, (40, 40, 20))
        if k == 2:
            c1, f1 = np.concatenate([boundary_points(), c1]), np.concatenate([boundary_points(), f1])
        inputs = [(cloud(rng, 80, (10, 10, 2)), cloud(rng, 500, (15, 15, 3)), q0, t0), (c1, f1, *POSES_A[k]),
                  (cloud(rng, 100, (10, 10, 2)), cloud(rng, 400, (15, 15, 3)), q2, t2)][:batch]
        add = [b for b in ([1] + ([0, 2] if k < 3 else [])) if b < batch]
        got = step(gpu, binding, inputs, add)
        for b in add:
            stacks[b].append(got[b])
    nodes = [gpu.graph_export(b) for b in range(batch)]
    edges = [anchor(binding, pg, 0, 2, nodes[0][2], (0.3, -0.2, 0.1), (0.0, 0.0, 0.03))]
    if batch > 1:
        edges += [anchor(binding, pg, 1, 3, nodes[1][3], (0.4, -0.3, 0.2)), anchor(binding, pg, 1, 6, nodes[1][6], (-0.5, 0.6, -0.1), (0.02, -0.01, 0.05))]
    if batch > 2:
        edges += [anchor(binding, pg, 2, 2, nodes[2][2], (-0.2, 0.4, 0.0), (0.0, 0.0, -0.04))]
    gpu.graph_add_edges(np.concatenate(edges))
    if solve:
        res = gpu.graph_optimize(list(range(batch)))
        assert (res["status"] == binding.GRAPH_OK).all()
    return gpu, stacks


ALL = [(0, 0, 3, MAP), (1, 0, 7, MAP), (2, 0, 3, MAP)]


@pytest.fixture(scope="module")
def applied(binding, pg):
    """The world above with all three sequences applied in one call; what the getters said before, the results, and the context as the call
    left it.  The tests that share it only read."""
    gpu, stacks = make_world(binding, pg)
    nodes = [gpu.graph_export(b) for b in range(3)]
    poses = [gpu.map_pose(b) for b in range(3)]
    res = gpu.graph_apply(ALL)
    yield {"gpu": gpu, "stacks": stacks, "nodes": nodes, "poses": poses, "res": res}
    gpu.close()


def window_model(atlas, O, nodes, stacks, first, count, cen):
    st = {}
    nd = nodes[first:first + count]
    cut = atlas.window_from_keyframes(nd["q_opt"], nd["t_opt"], stacks[first:first + count], LEAF, lambda p, leaf: O.voxel_filter(p, leaf, canonical=True), cen, st)
    return cut, st


def same_window(gpu, cut, seq):
    for cls in (0, 1):
        got = gpu.map_cubes(cls, seq)
        if sorted(got) != sorted(cut[cls]):
            return False
        for k in got:
            if got[k].shape != cut[cls][k].shape or not np.array_equal(got[k].view(np.uint32), np.asarray(cut[cls][k], np.float32).view(np.uint32)):
                return False
    return True


def pose_deviation(got_q, got_t, want_q, want_t):
    """max |difference| in units of the bound 64 eps max(1, |t|)."""
    return max(np.abs(got_q - want_q).max() / (64 * EPS), np.abs(got_t - want_t).max() / (64 * EPS * max(1.0, np.abs(want_t).max())))


# ---- 1. pose and rebase ------------------------------------------------------------------------------------------------------------------
def test_pose_and_rebase_against_the_model(binding, pg):
    """ALOAM_GRAPH_APPLY_POSE alone, no keyframe store: graphs of 1, 5 and 9 nodes, the last at 30 km, anchors that move the last node by
    about 2 m and 10 degrees; sequences 0 and 2 are applied, sequence 1 is not."""
    gpu = context(binding, keyframes=None)
    rng = np.random.default_rng(5)
    far = np.array([30000.0, -20000.0, 100.0])
    count = (1, 5, 9)

    def pose(b, k):
        k = min(k, count[b] - 1)
        if b == 0:
            return Q_Z, (3.0, 4.0, 0.5)
        if b == 1:
            return (Q_Z if k % 2 else Q_ID), (2.0 * k, 0.3 * k, 0.0)
        return pg.qexp(np.array([0.0, 0.0, 0.1 * k])), tuple(far + np.array([1.5 * k, 0.2 * k, 0.0]))
    small = lambda: (cloud(rng, 40, (5, 5, 1)), cloud(rng, 200, (8, 8, 2)))
    for k in range(9):
        step(gpu, binding, [(*small(), *pose(b, k)) for b in range(3)], [b for b in range(3) if k < count[b]])
    assert [gpu.graph_info(b)["nodes"] for b in range(3)] == [1, 5, 9]
    n = [gpu.graph_export(b) for b in range(3)]
    gpu.graph_add_edges(np.concatenate([anchor(binding, pg, b, count[b] - 1, n[b][-1], (1.5, -1.2, 0.4), (0.0, 0.0, 0.17), 1e4) for b in (1, 2)]))
    res = gpu.graph_optimize([0, 1, 2])
    assert res["status"].tolist() == [binding.GRAPH_NO_EDGES, binding.GRAPH_OK, binding.GRAPH_OK]
    n = [gpu.graph_export(b) for b in range(3)]
    e = [gpu.graph_export(b, edges=True) for b in range(3)]
    moved = np.linalg.norm(n[2]["t_opt"][-1] - n[2]["t"][-1])
    assert 1.0 < moved < 3.0 and np.abs(n[2]["t"][-1]).max() > 29000.0, moved
    mp = [gpu.map_pose(b) for b in range(3)]
    info = [gpu.map_info(b) for b in range(3)]
    other = getters(gpu, binding, 1, store=False)
    out = gpu.graph_apply([(0, 0, 0, POSE), (2, 3, 2, POSE)])
    assert out["status"].tolist() == [binding.GRAPH_APPLIED] * 2 and out["nodes"].tolist() == [1, 9]
    worst = 0.0
    for r, b in zip(out, (0, 2)):
        (qd, td), live, (qr, tr) = pg.apply_correction(n[b]["q"], n[b]["t"], n[b]["q_opt"], n[b]["t_opt"],
                                                       [(mp[b]["q_wmap_wodom"], mp[b]["t_wmap_wodom"]), (mp[b]["q_w"], mp[b]["t_w"])])
        now = gpu.map_pose(b)
        worst = max(worst, pose_deviation(r["q_corr"], r["t_corr"], qd, td), pose_deviation(now["q_wmap_wodom"], now["t_wmap_wodom"], *live[0]),
                    pose_deviation(now["q_w"], now["t_w"], *live[1]))
        after = gpu.graph_export(b)
        assert after["q"].tobytes() == n[b]["q_opt"].tobytes() == qr.tobytes() and after["t"].tobytes() == n[b]["t_opt"].tobytes() == tr.tobytes()
        assert after["q_opt"].tobytes() == n[b]["q_opt"].tobytes() and after["t_opt"].tobytes() == n[b]["t_opt"].tobytes()
        assert after["frame"].tobytes() == n[b]["frame"].tobytes() and gpu.graph_export(b, edges=True).tobytes() == e[b].tobytes()
        assert gpu.map_info(b) == info[b] and r["cen"].tolist() == [info[b]["cenW"], info[b]["cenH"], info[b]["cenD"]]      # the window stays
        assert r["cubes"].tolist() == [0, 0] and r["points"].tolist() == [0, 0] and r["outside_window"] == 0
    print(f"correction and live poses against apply_correction: {worst:.3f} of the bound 64 eps max(1, |t|)")
    assert worst <= 1.0
    assert np.abs(out[1]["t_corr"]).max() > 100.0                            # a rotation about an origin 36 km away: D's translation is large
    assert getters(gpu, binding, 1, store=False) == other
    # a node entered afterwards: its odometry edge starts at the optimised last node
    step(gpu, binding, [(*small(), pg.qexp(np.array([0.0, 0.0, 0.1 * (b + 1)])), tuple(np.array(pose(b, 99)[1]) + np.array([1.0, 0.5, 0.0]))) for b in range(3)], [0, 2])
    worst = 0.0
    for b in (0, 2):
        K = count[b]
        nn, ee = gpu.graph_export(b), gpu.graph_export(b, edges=True)
        now = gpu.map_pose(b)
        assert len(nn) == K + 1 and ee["i"][-1] == K - 1 and ee["j"][-1] == K
        assert nn["q"][K].tobytes() == now["q_w"].tobytes() and nn["t"][K].tobytes() == now["t_w"].tobytes()
        qz, tz = pg.relative_pose(n[b]["q_opt"][K - 1], n[b]["t_opt"][K - 1], nn["q"][K], nn["t"][K])
        worst = max(worst, np.abs(ee["q"][-1] - qz).max(), np.abs(ee["t"][-1] - tz).max())
        assert np.abs(nn["t"][K] - n[b]["t_opt"][K - 1]).max() < 2.0          # entered in the corrected frame, a metre from the optimised last node
    print(f"the first odometry edge behind an apply against relative_pose(X_opt[K-1], new): {worst:.3e} (bound 1e-14)")
    assert worst <= 1e-14
    gpu.graph_add_edges(anchor(binding, pg, 0, 1, gpu.graph_export(0)[1], (0.3, 0.4, -0.2), (0.0, 0.02, 0.0)))
    nn = [gpu.graph_export(b) for b in (0, 2)]
    ee = [gpu.graph_export(b, edges=True) for b in (0, 2)]
    want = [pg.cost(a["q_opt"], a["t_opt"], d) for a, d in zip(nn, ee)]
    again = gpu.graph_optimize([0, 2])
    print(f"initial cost of the second solve: {again['initial_cost'].tolist()} against the model's {want}")
    assert min(want) > 1e-3 and np.allclose(again["initial_cost"], want, rtol=1e-12, atol=0.0)
    gpu.close()


# ---- 2. the map ----------------------------------------------------------------------------------------------------------------------------
def test_the_window_equals_the_model(O, binding, atlas, pg, applied):
    gpu, res = applied["gpu"], applied["res"]
    assert res["status"].tolist() == [binding.GRAPH_APPLIED] * 3 and res["nodes"].tolist() == [3, 7, 3]
    b = 1
    now, info = gpu.map_pose(b), gpu.map_info(b)
    cen = atlas.window_centre(now["t_w"])
    assert cen == (12, 9, 6)                                                  # the sensor's cube (-2, 1, -1), reached well inside it
    assert np.abs((now["t_w"] + 25.0) / 50.0 - np.round((now["t_w"] + 25.0) / 50.0)).min() > 0.1
    assert (info["cenW"], info["cenH"], info["cenD"]) == cen == tuple(res[b]["cen"].tolist())
    nodes = gpu.graph_export(b)
    assert nodes["q_opt"].tobytes() == applied["nodes"][b]["q_opt"].tobytes() and nodes["q"].tobytes() == nodes["q_opt"].tobytes()
    assert not np.array_equal(applied["nodes"][b]["t"], nodes["t"])            # the solve had moved them
    cut, st = window_model(atlas, O, nodes, applied["stacks"][b], 0, 7, cen)
    keys = np.array([atlas.ijk_of(k) for k in cut[1]]) - np.array(cen)
    assert (keys.min(0) <= -3).all() and (keys.max(0) >= 3).all()             # cubes -3 .. 3 on every axis, so the window order is a permutation of the tile order
    assert same_window(gpu, cut, b)
    assert res[b]["cubes"].tolist() == st["cubes"] and res[b]["points"].tolist() == st["window_points"]
    assert res[b]["raw_points"].tolist() == st["raw_points"] and res[b]["outside_window"] == st["outside_window"] == 0
    # the live poses moved by the correction the record reports
    (qd, td), live, _ = pg.apply_correction(applied["nodes"][b]["q"], applied["nodes"][b]["t"], nodes["q_opt"], nodes["t_opt"],
                                            [(applied["poses"][b]["q_wmap_wodom"], applied["poses"][b]["t_wmap_wodom"]), (applied["poses"][b]["q_w"], applied["poses"][b]["t_w"])])
    dev = max(pose_deviation(res[b]["q_corr"], res[b]["t_corr"], qd, td), pose_deviation(now["q_wmap_wodom"], now["t_wmap_wodom"], *live[0]),
              pose_deviation(now["q_w"], now["t_w"], *live[1]))
    print(f"sequence 1 with the map: {dev:.3f} of the bound")
    assert dev <= 1.0
    # sequence 0 drove on behind its last keyframe: the window is centred on where the sensor is now, not on the last node
    cut0, st0 = window_model(atlas, O, gpu.graph_export(0), applied["stacks"][0], 0, 3, atlas.window_centre(gpu.map_pose(0)["t_w"]))
    assert same_window(gpu, cut0, 0) and res[0]["points"].tolist() == st0["window_points"] and sum(st0["window_points"]) > 0


# ---- 3. outside the window ---------------------------------------------------------------------------------------------------------------
def test_a_keyframe_outside_the_window_is_left_out_and_counted(O, binding, atlas, applied):
    gpu, res, b = applied["gpu"], applied["res"], 2
    cen = atlas.window_centre(gpu.map_pose(b)["t_w"])
    nodes = gpu.graph_export(b)
    cut, st = window_model(atlas, O, nodes, applied["stacks"][b], 0, 3, cen)
    far = atlas.tiles_from_keyframes(nodes["q_opt"][1:2], nodes["t_opt"][1:2], applied["stacks"][b][1:2], LEAF, lambda p, leaf: O.voxel_filter(p, leaf, canonical=True))
    assert len(far[1]) > 0 and (far[0]["cube"][:, 0] >= 11).all()
    assert res[b]["outside_window"] == st["outside_window"] == len(far[1])
    assert same_window(gpu, cut, b) and res[b]["points"].tolist() == st["window_points"] and res[b]["cubes"].tolist() == st["cubes"]
    # the other cubes are what the two near keyframes make alone
    near = [applied["stacks"][b][0], (np.zeros((0, 4), np.float32),) * 2, applied["stacks"][b][2]]
    alone, _ = window_model(atlas, O, nodes, near, 0, 3, cen)
    assert same_window(gpu, alone, b)
    assert res[b]["raw_points"].tolist() == [sum(len(s[c]) for s in applied["stacks"][b]) for c in (0, 1)]


# ---- 4. twin continuation ----------------------------------------------------------------------------------------------------------------
def test_a_twin_prepared_with_set_map_continues_with_the_same_bits(binding, atlas, pg, sequence):
    """Six rendered sweeps through register, odometry and mapping with the solver on, a node per sweep, an anchor and a solve, in two
    contexts.  One applies; the other is given the exported map of the same nodes cut at the read-back centre (aloam_set_map) and the
    read-back correction (aloam_set_map_frame).  Three further full steps give the same map pose, stacks, registered cloud and cubes."""
    scans = sequence("VLP-16", 9, seed=5, columns=250)[0]
    pair = []
    for _ in range(2):
        gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=3, max_points=4096)
        gpu.mapping_enable(0.4, 0.8, pool_points=1 << 16)
        gpu.graph_enable(16, 32)
        gpu.graph_keyframes_enable(1 << 14, 1 << 16)
        for k in range(6):
            gpu.scan_register([scans[k]] * 3)
            gpu.odometry_step()
            gpu.mapping_step()
            gpu.graph_add_nodes([0, 1, 2], INFO)
        n = gpu.graph_export(1)
        gpu.graph_add_edges(anchor(binding, pg, 1, 5, n[5], (0.3, -0.25, 0.05), (0.0, 0.0, 0.02)))
        assert gpu.graph_optimize([1])[0]["status"] == binding.GRAPH_OK
        pair.append(gpu)
    a, b = pair
    assert getters(a, binding, 1) == getters(b, binding, 1)
    before = a.map_pool_info()
    res = a.graph_apply([(1, 0, 6, MAP)])[0]
    assert res["status"] == binding.GRAPH_APPLIED and sum(res["points"]) > 500 and a.map_pool_info()["growths"] == before["growths"]
    now, info = a.map_pose(1), a.map_info(1)
    cen = (info["cenW"], info["cenH"], info["cenD"])
    tiles, points, _, _ = b.graph_export_map([(1, 0, 6, binding.GRAPH_POSE_OPTIMIZED)])
    cut = atlas.Atlas(tiles, points).cut(cen)
    for cls in (0, 1):
        b.set_map(cut[cls], cls, 1)
    b.set_map_frame(cen, now["q_wmap_wodom"], now["t_wmap_wodom"], info["frame_count"], 1)
    assert same_window(a, cut, 1)

    def view(g):
        out = [b"".join(v.tobytes() for _, v in sorted(g.map_pose(1).items())), repr(sorted(g.map_info(1).items()))]
        out += [g.map_cloud(w, 1).tobytes() for w in (binding.MAP_CORNER_STACK, binding.MAP_SURF_STACK, binding.MAP_REGISTERED)]
        for cls in (0, 1):
            cubes = g.map_cubes(cls, 1)
            out.append(repr([(k, len(cubes[k])) for k in sorted(cubes)]))
            out.append(b"".join(cubes[k].tobytes() for k in sorted(cubes)))
        return out
    for k in range(6, 9):
        for g in pair:
            g.scan_register([scans[k]] * 3)
            g.odometry_step()
            g.mapping_step()
        va, vb = view(a), view(b)
        assert va == vb, k
        assert a.map_info(1)["from_map_surf"] > 50                            # the solve ran against the rebuilt map
    assert a.map_pose(1)["t_w"].tobytes() != a.map_pose(0)["t_w"].tobytes()   # the same sweeps without the apply: the correction stayed in the drive
    for g in pair:
        g.close()


# ---- 5. pools ----------------------------------------------------------------------------------------------------------------------------
def small_pool_world(binding, pool_limit=None):
    """Ten keyframes of 600 surf points over a 80 x 80 x 40 m box, the live map emptied behind every step: the steps never grow a pool of
    4096 points, and the map of the ten keyframes holds about 6000 surf points."""
    rng = np.random.default_rng(12)
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=3, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(0.4, 0.8, pool_points=4096, pool_limit=pool_limit)
    gpu.graph_enable(16, 32)
    gpu.graph_keyframes_enable(1 << 12, 1 << 14)
    stacks = []
    for k in range(10):
        got = step(gpu, binding, [(cloud(rng, 60, (30, 30, 10)), cloud(rng, 600, (40, 40, 20)), Q_ID, (0.5 * k, 0.2 * k, 0.0))] * 3, [0, 1, 2])
        stacks.append(got[1])
        for b in range(3):
            for cls in (0, 1):
                gpu.set_map({}, cls, b)
    return gpu, stacks


def test_a_window_larger_than_the_pool_row_grows_the_pools(O, binding, atlas):
    gpu, stacks = small_pool_world(binding)
    before = gpu.map_pool_info()
    assert before["pool_points"] == 4096 and before["growths"] == 0
    res = gpu.graph_apply([(1, 0, 10, MAP)])[0]
    after = gpu.map_pool_info()
    assert res["status"] == binding.GRAPH_APPLIED and res["points"][1] > 4096
    assert after["pool_points"] == 8192 and after["growths"] == 1 and after["live_max"] >= res["points"][1]
    cut, st = window_model(atlas, O, gpu.graph_export(1), stacks, 0, 10, atlas.window_centre(gpu.map_pose(1)["t_w"]))
    assert same_window(gpu, cut, 1) and res["points"].tolist() == st["window_points"]
    # the next step sizes the pools from the new totals and keeps the map
    step(gpu, binding, [(stacks[0][0], stacks[0][1], Q_ID, (5.0, 2.0, 0.0))] * 3, [])
    assert sum(len(v) for v in gpu.map_cubes(1, 1).values()) >= res["points"][1]
    gpu.close()


def test_at_the_pool_limit_the_call_is_refused_with_nothing_changed(binding):
    gpu, _ = small_pool_world(binding, pool_limit=4096)
    assert gpu.map_pool_info()["limit"] == 4096
    before = [getters(gpu, binding, b) for b in range(3)]
    with pytest.raises(binding.AloamError) as e:
        gpu.graph_apply([(0, 0, 2, MAP), (1, 0, 10, MAP)])
    assert e.value.code == binding.E_CAPACITY and "pool limit" in str(e.value)
    assert [getters(gpu, binding, b) for b in range(3)] == before and gpu.map_pool_info()["pool_points"] == 4096
    gpu.close()


# ---- 6. list independence ------------------------------------------------------------------------------------------------------------------
def test_a_sequences_bits_do_not_depend_on_the_list(binding, pg, applied):
    together = [getters(applied["gpu"], binding, b) for b in range(3)]
    gpu, _ = make_world(binding, pg)
    alone = np.concatenate([gpu.graph_apply([r]) for r in ALL])
    assert [getters(gpu, binding, b) for b in range(3)] == together and alone.tobytes() == applied["res"].tobytes()
    gpu.close()
    gpu, _ = make_world(binding, pg)
    backwards = gpu.graph_apply(ALL[::-1], pinned=False)                      # results into device memory
    assert [getters(gpu, binding, b) for b in range(3)] == together and backwards[::-1].tobytes() == applied["res"].tobytes()
    gpu.close()


# ---- 7. stream order -----------------------------------------------------------------------------------------------------------------------
def test_optimize_apply_step_need_no_synchronise_in_between(binding, pg):
    import torch
    views = []
    for wait in (False, True):
        gpu, _ = make_world(binding, pg, solve=False)
        rng = np.random.default_rng(8)
        for b in range(3):                                                    # the inputs of the step, staged before the three calls
            c, f = cloud(rng, 80, (10, 10, 2)), cloud(rng, 500, (15, 15, 3))
            gpu.set_last(c, f, b)
            gpu.set_full_cloud(f[:4], b)
            gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(Q_Z, np.float64), np.array([3.0 + b, -2.0, 0.3]), b)
        gpu.synchronize()
        r0 = torch.zeros(3 * 64, dtype=torch.uint8).pin_memory()
        r1 = torch.zeros(3 * 104, dtype=torch.uint8).pin_memory()
        gpu.graph_optimize_into([0, 1, 2], r0.data_ptr(), gpu.graph_options())
        if wait:
            gpu.synchronize()
        gpu.graph_apply_into([(0, 0, 3, MAP), (1, 0, 7, POSE), (2, 1, 2, MAP)], r1.data_ptr())
        if wait:
            gpu.synchronize()
        gpu.mapping_step()
        gpu.synchronize()
        res = r1.numpy().view(binding.GRAPH_APPLY_RESULT_DTYPE)
        assert res["status"].tolist() == [0, 0, 0] and (r0.numpy().view(binding.GRAPH_RESULT_DTYPE)["status"] == binding.GRAPH_OK).all()
        views.append(([getters(gpu, binding, b) for b in range(3)], r0.numpy().tobytes(), r1.numpy().tobytes()))
        gpu.close()
    assert views[0] == views[1]


# ---- 8. host state -------------------------------------------------------------------------------------------------------------------------
def test_the_host_state_follows_an_apply(binding, pg):
    rng = np.random.default_rng(3)
    gpu = context(binding, batch=2, nodes=8, edges=8, keyframes=(4096, 8192))
    gpu.map_spill_enable(64, 1 << 14)
    inputs = lambda k: [(cloud(rng, 80, (10, 10, 2)), cloud(rng, 600, (15, 15, 3)), Q_ID, (2.0 * k, 0.5 * b, 0.0)) for b in range(2)]
    for k in range(3):
        step(gpu, binding, inputs(k), [0, 1])
    gpu.set_map_frozen([1, 1])
    step(gpu, binding, inputs(3), [])                                         # a frozen step: something to score against
    gpu.set_map_frozen(None)
    cand = binding.map_corrections([Q_ID], [(0.0, 0.0, 0.0)])
    gpu.score_map_corrections([0, 1], cand)
    assert (gpu.export_pose_information(binding.INFO_MAPPING, [0, 1])["status"] != binding.INFO_NONE).all()
    gpu.graph_add_edges(anchor(binding, pg, 0, 2, gpu.graph_export(0)[2], (0.2, 0.1, 0.0)))
    gpu.graph_optimize([0])
    spill = [gpu.map_spill_info(b) for b in range(2)]
    graph = [gpu.graph_info(b) for b in range(2)]
    assert gpu.graph_apply([(0, 0, 3, MAP)])[0]["status"] == binding.GRAPH_APPLIED
    with pytest.raises(binding.AloamError) as e:
        gpu.score_map_corrections([0], cand)
    assert e.value.code == binding.E_STATE
    gpu.score_map_corrections([1], cand)                                      # the sequence that was not listed keeps its state
    st = gpu.export_pose_information(binding.INFO_MAPPING, [0, 1])["status"]
    assert st[0] == binding.INFO_NONE and st[1] != binding.INFO_NONE
    assert [gpu.map_spill_info(b) for b in range(2)] == spill and [gpu.graph_info(b) for b in range(2)] == graph
    gpu.graph_add_nodes([0], INFO)                                            # has_stacks is kept: the stacks are in the sensor frame
    assert gpu.graph_info(0)["nodes"] == 4
    gpu.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_everything_as_it_was(binding, pg, atlas):
    import torch
    gpu, _ = make_world(binding, pg)
    dst = torch.full((3 * 104,), 0x5A, dtype=torch.uint8).pin_memory()
    pageable = np.zeros(3 * 104, np.uint8)

    def refused(code, f):
        with pytest.raises(binding.AloamError) as e:
            f()
        assert e.value.code == code, str(e.value)
    before = [getters(gpu, binding, b) for b in range(3)]
    for bad in ((3, 0, 0, POSE), (-1, 0, 0, POSE), (0, 0, 1, POSE), (1, -1, 2, MAP), (1, 0, -1, MAP), (1, 5, 3, MAP), (1, 0, 8, POSE), (1, 0, 7, 0), (1, 0, 7, 2),
                (1, 0, 7, 4), (1, 0, 7, 7), (1, 0, 7, -1)):
        refused(binding.E_ARG, lambda: gpu.graph_apply_into([(0, 0, 3, MAP), bad], dst.data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_apply_into([(1, 0, 7, MAP)], pageable.ctypes.data))
    refused(binding.E_ARG, lambda: gpu.graph_apply_into([(1, 0, 7, MAP)], 0))
    refused(binding.E_ARG, lambda: gpu.graph_apply_into([(1, 0, 7, MAP)], dst.data_ptr() + 4))
    gpu.set_map_frozen([0, 1, 0])
    refused(binding.E_STATE, lambda: gpu.graph_apply_into([(0, 0, 3, POSE), (1, 0, 7, POSE)], dst.data_ptr()))
    gpu.set_map_frozen(None)
    tile = np.zeros(1, binding.MAP_TILE_DTYPE)
    tile["count"], tile["feature_class"] = 4, 1
    gpu.atlas_load(tile, np.ones((4, 4), np.float32))
    gpu.atlas_attach([0, 0, 1])
    refused(binding.E_STATE, lambda: gpu.graph_apply_into([(2, 0, 3, MAP)], dst.data_ptr()))
    gpu.atlas_attach(None)
    gpu.graph_apply_into([], dst.data_ptr())                                  # n = 0 is fine and does nothing
    gpu.synchronize()
    assert (dst.numpy() == 0x5A).all()
    assert [getters(gpu, binding, b) for b in range(3)] == before
    # an empty graph: ALOAM_GRAPH_APPLY_NO_NODES, nothing changed, beside a sequence that is applied
    gpu.graph_clear([2])
    before = [getters(gpu, binding, b) for b in range(3)]
    res = gpu.graph_apply([(2, 0, 0, MAP), (0, 0, 3, POSE)])
    assert res["status"].tolist() == [binding.GRAPH_APPLY_NO_NODES, binding.GRAPH_APPLIED] and res[0]["nodes"] == 0 and res[0]["q_corr"].tolist() == [0, 0, 0, 1]
    after = [getters(gpu, binding, b) for b in range(3)]
    assert after[2] == before[2] and after[1] == before[1] and after[0] != before[0]
    gpu.close()
    # the order of the enables
    g = binding.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=4096, lm_max_iterations=0)
    refused2 = lambda code, req: refused(code, lambda: g.graph_apply_into(req, dst.data_ptr()))
    refused2(binding.E_STATE, [(0, 0, 0, POSE)])                             # before aloam_graph_enable
    g.graph_enable(8, 8)
    refused2(binding.E_STATE, [(0, 0, 0, POSE)])                             # before aloam_mapping_enable
    g.mapping_enable(0.4, 0.8, pool_points=1 << 12)
    refused2(binding.E_STATE, [(0, 0, 0, MAP)])                              # the map before aloam_graph_keyframes_enable
    assert g.graph_apply([(0, 0, 0, POSE)])[0]["status"] == binding.GRAPH_APPLY_NO_NODES
    g.close()


# ---- 10. opt-in ------------------------------------------------------------------------------------------------------------------------------
def test_a_context_that_never_applies_is_what_it_was(binding, pg):
    """Twins through the calls of test_gpu_graph_map.test_opt_in_changes_nothing_else (store enabled); one of them also applies sequence 1
    at the end.  Sequence 0 gives the same bits from every getter in both, the twin that never applies launches what that test pins
    (graph_map: the four captures), and the other differs in the graph_map slot alone."""
    runs = []
    for apply in (False, True):
        rng = np.random.default_rng(77)
        gpu = context(binding, batch=2, nodes=8, edges=8, keyframes=(4096, 8192))
        gpu.profile_enable(True)
        for k in range(3):
            inputs = [(cloud(rng, 80, (10, 10, 2)), cloud(rng, 600, (15, 15, 3)), Q_Z if k == 1 else Q_ID, (3.0 * k, 0.5 * b, 0.0)) for b in range(2)]
            step(gpu, binding, inputs, [0, 1] if k != 1 else [1])
        gpu.graph_optimize([0, 1])
        gpu.graph_clear([1])
        step(gpu, binding, inputs, [1])
        if apply:
            assert gpu.graph_apply([(1, 0, 1, MAP)])[0]["status"] == binding.GRAPH_APPLIED
        runs.append((getters(gpu, binding, 0), getters(gpu, binding, 1), gpu.profile()))
        gpu.close()
    (s0, s1, p0), (a0, a1, p1) = runs
    assert s0 == a0 and s1 != a1
    assert p0["graph_map"]["launches"] == 4
    for name in p0:
        assert p0[name]["launches"] == p1[name]["launches"] or name == "graph_map", name
    assert p1["graph_map"]["launches"] > 4
