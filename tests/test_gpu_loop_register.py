"""Loop edges measured on the MI355X (aloam_graph_loops_enable / aloam_graph_register_loops): the filtered target bit for bit against
loopreg.target_cloud, the registration against the numpy model of tests/loopreg_model.py, the shapes at which the new kernels can go
wrong, independence of the other requests, the statuses, the tangent of the edge's information in a corridor, a loop closed with the
measured edge, and the refusals.

The keyframes are hand-made as in test_gpu_graph_map.py: aloam_set_last + aloam_mapping_step with the context's solver off
(lm_max_iterations = 0), so a node's pose is the pose handed in and its clouds are the voxel filter of the cloud handed in.  The scene and
the drive are those of loopreg_model.fixture: nine target nodes along 8 m, one source node entered about 0.4 m and 4 degrees off."""
import importlib
import math

import numpy as np
import pytest

import loopreg_model as M

pytestmark = pytest.mark.gpu
INFO = np.eye(6) * 100.0
KF_CORNER, KF_SURF = 1 << 13, 1 << 15
SLOTS, CAP_CORNER, CAP_SURF = 8, 4096, 16384
Z_BOUND = 1e-8                       # what tests/test_gpu_mapping.py allows the map pose against the oracle


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("a-loam_amd.loopreg")


@pytest.fixture(scope="module")
def P():
    return importlib.import_module("a-loam_amd.posegraph")


def context(binding, batch, loops=(SLOTS, CAP_CORNER, CAP_SURF), keyframes=(KF_CORNER, KF_SURF), nodes=32):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(*M.LEAF, pool_points=1 << 16)
    gpu.graph_enable(nodes, 64)
    if keyframes:
        gpu.graph_keyframes_enable(*keyframes)
    if loops:
        gpu.graph_loops_enable(*loops)
    return gpu


def feed(gpu, binding, inputs, add):
    """One mapping step of every sequence - inputs[b] = (corner, surf, q, t) - then a node for the sequences in `add`; returns their stacks."""
    for b, (corner, surf, q, t) in enumerate(inputs):
        gpu.set_last(corner, surf, b)
        gpu.set_full_cloud(surf[:4], b)
        gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(q, np.float64), np.array(t, np.float64), b)
    gpu.mapping_step()
    if add:
        gpu.graph_add_nodes(add, INFO)
    gpu.synchronize()
    return {b: (gpu.map_cloud(binding.MAP_CORNER_STACK, b), gpu.map_cloud(binding.MAP_SURF_STACK, b)) for b in add}


def drive(gpu, binding, fixtures, negate=()):
    """The ten keyframes of every fixture, sequence b = fixtures[b]; the entered quaternion of every third node is negated for the
    sequences in `negate`.  Returns stacks[b][k] = (corner, surf)."""
    stacks = [[] for _ in fixtures]
    for k in range(len(fixtures[0]["raw"])):
        inputs = [(fx["raw"][k][0], fx["raw"][k][1], -fx["q"][k] if (b in negate and k % 3 == 2) else fx["q"][k], fx["t"][k]) for b, fx in enumerate(fixtures)]
        got = feed(gpu, binding, inputs, list(range(len(fixtures))))
        for b in got:
            stacks[b].append(got[b])
    return stacks


def guess_of(P, nodes, i, j, opt=False):
    q, t = (nodes["q_opt"], nodes["t_opt"]) if opt else (nodes["q"], nodes["t"])
    return P.relative_pose(q[i], t[i], q[j], t[j])


def unit(q):
    """The guess as aloam_graph_register_loops stores it: divided by its norm, the squares summed in index order."""
    q = [float(v) for v in q]
    nn = 0.0
    for v in q:
        nn += v * v
    nn = math.sqrt(nn)
    return np.array([v / nn for v in q])


def raw(rec):
    return np.ascontiguousarray(rec).view(np.uint8).tobytes()


@pytest.fixture(scope="module")
def world(binding, P):
    """Shared by the tests below.  Sequence 0: the noise-free room, then nodes 10 .. 12 whose surf clouds hold 255, 256 and 257 points and
    node 13 with an empty corner cloud.  Sequence 1: the room with 1 cm noise, every third entered quaternion negated; a solve with a made-up
    loop edge has moved its estimates.  Sequence 2: a floor-only world."""
    fxs = [M.fixture(seed=7), M.fixture(seed=8, noise=0.01), M.fixture(seed=9, kind="floor")]
    gpu = context(binding, 3)
    stacks = drive(gpu, binding, fxs, negate=(1,))
    fx = fxs[0]
    src_c, src_s = stacks[0][9]
    for n in (255, 256, 257, None):                       # filtered points are alone in their voxels: filtering them again keeps every one
        c = src_c if n else np.zeros((0, 4), np.float32)
        s = src_s[:n] if n else src_s
        keep = [(fxs[b]["raw"][9][0], fxs[b]["raw"][9][1], fxs[b]["q"][9], fxs[b]["t"][9]) for b in (1, 2)]
        got = feed(gpu, binding, [(c, s, fx["q"][9], fx["t"][9])] + keep, [0])
        stacks[0].append(got[0])
    assert [len(s[1]) for s in stacks[0][10:13]] == [255, 256, 257] and len(stacks[0][13][0]) == 0
    # sequence 1: a loop edge that is off by 0.2 m, so that the solve moves the estimates away from the entered poses
    n1 = gpu.graph_export(1)
    qz, tz = guess_of(P, n1, 4, 9)
    gpu.graph_add_edges(P.make_edges(1, 4, 9, unit(qz)[None], (tz + np.array([0.2, 0.1, 0.0]))[None], INFO * 10, robust=True))
    gpu.graph_optimize([1])
    nodes = [gpu.graph_export(b) for b in range(3)]
    assert np.abs(nodes[1]["t_opt"] - nodes[1]["t"]).max() > 0.01
    yield {"gpu": gpu, "fx": fxs, "stacks": stacks, "nodes": nodes}
    gpu.close()


def model_target(L, w, seq, i, first, count, opt=False):
    nd = w["nodes"][seq]
    return L.target_cloud(nd["q_opt"] if opt else nd["q"], nd["t_opt"] if opt else nd["t"], w["stacks"][seq], i, first, count, M.LEAF, M.voxel_filter)


def test_target_bit_for_bit(binding, world, L, P):
    """graph_loop_target against loopreg.target_cloud fed the stacks read back with aloam_get_map_cloud and the poses read back with
    aloam_graph_export: entered and optimised poses, negated quaternions, nine nodes (a surf target above 8192 raw points: the 1024-thread
    filter) and one node."""
    gpu = world["gpu"]
    cases = [(0, 4, 9, 0, 9, 0), (1, 4, 9, 0, 9, 0), (1, 4, 9, 0, 9, 1), (0, 4, 9, 4, 1, 0), (1, 2, 9, 1, 5, 1)]
    assert (world["nodes"][1]["q"][2] == -world["fx"][1]["q"][2]).all()
    reqs = [c + guess_of(P, world["nodes"][c[0]], c[1], c[2]) for c in cases]
    res = gpu.graph_register_loops(reqs)
    for r, (seq, i, j, first, count, pose) in enumerate(cases):
        want = model_target(L, world, seq, i, first, count, bool(pose))
        raw_n = [sum(len(world["stacks"][seq][k][cls]) for k in range(first, first + count)) for cls in (0, 1)]
        print(f"request {r}: raw target {raw_n}, filtered {[len(w) for w in want]}")
        assert res[r]["target_raw"].tolist() == raw_n and res[r]["target_points"].tolist() == [len(w) for w in want]
        assert res[r]["source_points"].tolist() == [len(world["stacks"][seq][j][cls]) for cls in (0, 1)]
        for cls in (0, 1):
            got = gpu.graph_loop_target(r, cls)
            assert got.shape == want[cls].shape and np.array_equal(got.view(np.uint32), want[cls].view(np.uint32)), (r, cls)
    assert max(sum(len(world["stacks"][0][k][1]) for k in range(9)), 0) > 8192


def check_against_model(binding, L, w, seq, j, res, noisy=False, label="", outer=2):
    information = importlib.import_module("a-loam_amd.information")
    P = importlib.import_module("a-loam_amd.posegraph")
    tc, ts = model_target(L, w, seq, 4, 0, 9)
    qg, tg = guess_of(P, w["nodes"][seq], 4, j)
    src = w["stacks"][seq][j]
    m = M.register(tc, ts, src[0], src[1], unit(qg), tg, outer_iterations=outer)
    dq, dt = np.abs(res["q"] - m["q"]).max(), np.abs(res["t"] - m["t"]).max()
    print(f"{label}: device factors {res['n_line']} + {res['n_plane']} (model {m['n_line']} + {m['n_plane']}), LM {res['lm_iterations']} / {m['lm_iterations']}, "
          f"termination {res['lm_termination']} / {m['lm_termination']}, |dq| {dq:.2e} |dt| {dt:.2e}")
    assert int(res["status"]) == m["status"] == L.LOOP_OK
    if noisy:
        lo, hi = M.factor_bounds(src[0], src[1], tc, ts, m["par_last"])
        print(f"{label}: model bounds of the factor count {lo} .. {hi}")
        assert lo <= int(res["n_line"]) + int(res["n_plane"]) <= hi
    else:
        assert (int(res["n_line"]), int(res["n_plane"]), int(res["lm_iterations"]), int(res["lm_termination"])) == (m["n_line"], m["n_plane"], m["lm_iterations"], m["lm_termination"])
    assert dq < Z_BOUND and dt < Z_BOUND
    if not noisy:
        # the yardsticks of tests/test_gpu_pose_information.py, the model evaluated on the same records at the device's Z
        want = information.information_from_factors(m["factors"][0], m["factors"][1], res["q"], res["t"])
        H, Hm = P.info_full(res["info_left"]), want["info"]
        dia = np.sqrt(np.diag(Hm))
        dH = (np.abs(H - Hm) / np.outer(dia, dia)).max()
        dc = abs(res["cost"] - want["cost"]) / want["cost"]
        E, Em = P.info_full(res["info"]), L.edge_information(Hm, res["q"])
        de = (np.abs(E - Em) / np.outer(np.sqrt(np.diag(Em)), np.sqrt(np.diag(Em)))).max()
        print(f"{label}: max |d info_left| / sqrt(HiiHjj) {dH:.3g}, max |d info| / sqrt(EiiEjj) {de:.3g}, cost rel {dc:.3g}")
        assert dH <= 1e-10 and de <= 1e-10 and dc <= 1e-12
    return m


def test_registration_against_the_model(binding, world, L, P):
    gpu = world["gpu"]
    reqs = [(b, 4, 9, 0, 9, 0) + guess_of(P, world["nodes"][b], 4, 9) for b in (0, 1)]
    res = gpu.graph_register_loops(reqs)
    m = check_against_model(binding, L, world, 0, 9, res[0], label="noise-free")
    check_against_model(binding, L, world, 1, 9, res[1], noisy=True, label="1 cm noise")
    for outer in (1, 3):                                 # round r writes factor_num[r & 1]: the result reads the LAST round's, whatever its parity
        one = gpu.graph_register_loops(reqs[:1], outer_iterations=outer)[0]
        mo = check_against_model(binding, L, world, 0, 9, one, label=f"outer_iterations = {outer}", outer=outer)
        assert (raw(one["q"]) != raw(res[0]["q"])) and (mo["n_line"], mo["n_plane"]) != (0, 0)
    fx = world["fx"][0]
    (qt, tt) = P.relative_pose(fx["q_true"][4], fx["t_true"][4], fx["q_true"][9], fx["t_true"][9])
    r0, d0 = M.pose_error(reqs[0][6], reqs[0][7], qt, tt)
    r1, d1 = M.pose_error(res[0]["q"], res[0]["t"], qt, tt)
    print(f"device registration: rotation {r0:.4f} -> {r1:.2e} rad, translation {d0:.4f} -> {d1:.2e} m")
    assert r1 <= 0.1 * r0 and d1 <= 0.1 * d0 and m["n_line"] > 50 and m["n_plane"] > 500


def test_shapes_at_which_the_kernels_can_go_wrong(binding, world, L, P):
    """Source surf clouds of 255, 256 and 257 points (the tile boundary of the fit), a source with an empty corner cloud, a target of one
    node, guesses with w < 0 - each against the model; the guess with w < 0 gives the pose of its twin."""
    gpu = world["gpu"]
    nd = world["nodes"][0]
    reqs = [(0, 4, j, 0, 9, 0) + guess_of(P, nd, 4, j) for j in (10, 11, 12, 13)]
    qg, tg = guess_of(P, nd, 4, 9)
    reqs += [(0, 4, 9, 4, 1, 0, qg, tg), (0, 4, 9, 0, 9, 0, -qg, tg), (0, 4, 9, 0, 9, 0, qg, tg)]
    res = gpu.graph_register_loops(reqs)
    for r, j in enumerate((10, 11, 12, 13)):
        assert res[r]["source_points"].tolist() == [len(world["stacks"][0][j][0]), len(world["stacks"][0][j][1])]
        check_against_model(binding, L, world, 0, j, res[r], label=f"source node {j} ({res[r]['source_points'].tolist()} points)")
    # one node: the model on the one-node target
    tc, ts = model_target(L, world, 0, 4, 4, 1)
    src = world["stacks"][0][9]
    m = M.register(tc, ts, src[0], src[1], unit(qg), tg)
    print(f"one-node target {len(tc)} + {len(ts)}: device {res[4]['n_line']} + {res[4]['n_plane']}, model {m['n_line']} + {m['n_plane']}, status {res[4]['status']}")
    assert int(res[4]["status"]) == m["status"] and (int(res[4]["n_line"]), int(res[4]["n_plane"])) == (m["n_line"], m["n_plane"])
    assert np.abs(res[4]["q"] - m["q"]).max() < Z_BOUND and np.abs(res[4]["t"] - m["t"]).max() < Z_BOUND
    # w < 0: the same rotation; the solve keeps the sign it was given
    assert qg[3] > 0 and res[5]["q"][3] < 0 and int(res[5]["status"]) == L.LOOP_OK
    assert np.abs(res[5]["q"] + res[6]["q"]).max() < Z_BOUND and np.abs(res[5]["t"] - res[6]["t"]).max() < Z_BOUND
    assert (int(res[5]["n_line"]), int(res[5]["n_plane"])) == (int(res[6]["n_line"]), int(res[6]["n_plane"]))
    assert np.abs(res[5]["info"] - res[6]["info"]).max() <= 1e-9 * np.abs(res[6]["info"]).max()


@pytest.fixture(scope="module")
def twins(binding):
    """Two fresh contexts fed the noise-free drive alone: one enables the feature, the other never does."""
    fx = M.fixture(seed=7)
    out = []
    for loops in ((SLOTS, CAP_CORNER, CAP_SURF), None):
        gpu = context(binding, 1, loops=loops)
        gpu.profile_enable(True)
        stacks = drive(gpu, binding, [fx])
        out.append({"gpu": gpu, "stacks": stacks, "nodes": gpu.graph_export(0)})
    yield fx, out
    for o in out:
        o["gpu"].close()


def test_a_result_does_not_depend_on_the_other_requests(binding, world, twins, P):
    gpu = world["gpu"]
    nd = world["nodes"]
    a = (0, 4, 9, 0, 9, 0) + guess_of(P, nd[0], 4, 9)
    others = [(1, 4, 9, 0, 9, 0) + guess_of(P, nd[1], 4, 9), (1, 2, 9, 1, 5, 1) + guess_of(P, nd[1], 2, 9), (0, 4, 10, 0, 9, 0) + guess_of(P, nd[0], 4, 10),
              (2, 4, 9, 0, 9, 0) + guess_of(P, nd[2], 4, 9), (0, 0, 9, 0, 3, 0) + guess_of(P, nd[0], 0, 9), (0, 4, 13, 2, 5, 0) + guess_of(P, nd[0], 4, 13),
              (1, 8, 0, 5, 4, 0) + guess_of(P, nd[1], 8, 0)]
    alone = raw(gpu.graph_register_loops([a])[0])
    among = gpu.graph_register_loops(others[:3] + [a] + others[3:])
    assert raw(among[3]) == alone
    lone = [raw(gpu.graph_register_loops([o])[0]) for o in others]
    assert [raw(among[k]) for k in (0, 1, 2, 4, 5, 6, 7)] == lone
    rev = gpu.graph_register_loops((others[:3] + [a] + others[3:])[::-1])
    assert raw(rev[4]) == alone and [raw(rev[k]) for k in (7, 6, 5, 3, 2, 1, 0)] == lone
    twice = gpu.graph_register_loops([a, others[0], a])
    assert raw(twice[0]) == alone == raw(twice[2])
    many = gpu.graph_register_loops(([a] + others) * 2 + [a], pinned=False)       # n = 2 * max_requests + 1: three rounds, into device memory
    assert len(many) == 2 * SLOTS + 1 and all(raw(many[k]) == alone for k in (0, SLOTS, 2 * SLOTS))
    assert [raw(many[SLOTS + 1 + k]) for k in range(7)] == lone
    # another context: the batch-1 twin (fed the same drive alone, already used by other tests) against the batch-3 world context
    fx, (on, off) = twins
    b = (0, 4, 9, 0, 9, 0) + guess_of(P, on["nodes"], 4, 9)
    assert raw(on["nodes"]) == raw(nd[0][:10]) and raw(on["gpu"].graph_register_loops([b])[0]) == alone


def test_a_call_of_six_rounds_wraps_the_request_ring(binding, twins, P):
    """5 * max_requests + 1 requests in one plain call: six rounds through the pinned ring of four slots, so rounds five and six fill the
    slots of rounds one and two.  Five different requests in turn (a round holds eight: every round differs from the one whose slot it
    takes); every result is byte-identical to the same request run alone."""
    fx, (on, off) = twins
    gpu, nd = on["gpu"], on["nodes"]
    kinds = [(0, 4, 9, 0, 9, 0) + guess_of(P, nd, 4, 9), (0, 0, 9, 0, 3, 0) + guess_of(P, nd, 0, 9), (0, 2, 9, 1, 5, 0) + guess_of(P, nd, 2, 9),
             (0, 8, 0, 5, 4, 0) + guess_of(P, nd, 8, 0), (0, 6, 1, 3, 6, 0) + guess_of(P, nd, 6, 1)]
    lone = [raw(gpu.graph_register_loops([k])[0]) for k in kinds]
    assert len(set(lone)) == len(kinds)
    n = 5 * SLOTS + 1
    many = gpu.graph_register_loops([kinds[k % 5] for k in range(n)])
    assert len(many) == n and [raw(many[k]) for k in range(n)] == [lone[k % 5] for k in range(n)]


def test_statuses(binding, world, L, P):
    gpu = world["gpu"]
    nd = world["nodes"]
    qg, tg = guess_of(P, nd[2], 4, 9)
    far_q, far_t = guess_of(P, nd[0], 4, 9)
    far_t = far_t + np.array([30.0, 0.0, 0.0])
    res = gpu.graph_register_loops([(2, 4, 9, 0, 9, 0, qg * (1 + 5e-7), tg), (0, 4, 9, 0, 9, 0, far_q, far_t)])
    # a floor-only world: no corner target at all
    assert int(res[0]["status"]) == L.LOOP_TARGET_TOO_SMALL and res[0]["target_points"][0] == 0 and res[0]["target_points"][1] > 50
    assert np.array_equal(res[0]["q"], unit(qg * (1 + 5e-7))) and np.array_equal(res[0]["t"], tg) and not res[0]["info"].any() and not res[0]["info_left"].any()
    # a guess 30 m off finds no neighbour: the model has no factor and calls that SOLVE_FAILED
    tc, ts = model_target(L, world, 0, 4, 0, 9)
    src = world["stacks"][0][9]
    m = M.register(tc, ts, src[0], src[1], unit(far_q), far_t)
    assert m["status"] == L.LOOP_SOLVE_FAILED and (m["n_line"], m["n_plane"]) == (0, 0)
    assert int(res[1]["status"]) == L.LOOP_SOLVE_FAILED and (int(res[1]["n_line"]), int(res[1]["n_plane"])) == (0, 0)
    assert np.array_equal(res[1]["q"], unit(far_q)) and np.array_equal(res[1]["t"], far_t) and not res[1]["info"].any()


def test_a_target_above_the_capacity_is_too_large_and_leaves_its_neighbour_alone(binding, twins, L, P):
    fx, (on, off) = twins
    small = context(binding, 1, loops=(4, CAP_CORNER, 4000))
    try:
        drive(small, binding, [fx])
        nd = small.graph_export(0)
        big = (0, 4, 9, 0, 9, 0) + guess_of(P, nd, 4, 9)
        ok = (0, 4, 9, 3, 3, 0) + guess_of(P, nd, 4, 9)
        alone = small.graph_register_loops([ok])[0]
        res = small.graph_register_loops([big, ok])
        assert int(res[0]["status"]) == L.LOOP_TOO_LARGE and res[0]["target_raw"][1] > 4000 and np.array_equal(res[0]["q"], unit(big[6])) and not res[0]["info"].any()
        assert int(alone["status"]) == L.LOOP_OK and raw(res[1]) == raw(alone)
        assert raw(alone) == raw(on["gpu"].graph_register_loops([ok])[0])           # the capacity is no part of the result
    finally:
        small.close()


def test_a_node_kept_without_clouds_gives_no_clouds(binding, L, P):
    fx = M.fixture(seed=7)
    gpu = context(binding, 1, keyframes=(1 << 13, 9 * 1100), loops=(2, CAP_CORNER, CAP_SURF))   # the surf row takes nine keyframes, not ten
    try:
        for k in range(10):
            gpu.set_last(fx["raw"][k][0], fx["raw"][k][1], 0); gpu.set_full_cloud(fx["raw"][k][1][:4], 0)
            gpu.set_state([0, 0, 0, 1], [0, 0, 0], fx["q"][k], fx["t"][k], 0)
            gpu.mapping_step()
            gpu.graph_add_nodes([0], INFO)
        with pytest.raises(binding.AloamError) as e:
            gpu.synchronize()
        assert e.value.code == binding.E_CAPACITY and "keyframe store full" in str(e.value)
        assert gpu.graph_keyframe_info(0)["dropped_nodes"] == 1
        nd = gpu.graph_export(0)
        res = gpu.graph_register_loops([(0, 4, 9, 0, 9, 0) + guess_of(P, nd, 4, 9), (0, 9, 4, 9, 1, 0) + guess_of(P, nd, 9, 4), (0, 4, 8, 0, 8, 0) + guess_of(P, nd, 4, 8)])
        assert [int(r["status"]) for r in res] == [L.LOOP_NO_CLOUDS, L.LOOP_NO_CLOUDS, L.LOOP_OK]      # node j, every target node, neither
        assert np.array_equal(res[0]["q"], unit(guess_of(P, nd, 4, 9)[0])) and res[0]["source_points"].tolist() == [0, 0]
    finally:
        gpu.close()


def test_a_target_above_65536_raw_points_takes_the_general_filter(binding, L, P):
    """Sixty-four target nodes along the same 8 m: the surf target holds more raw points than the single-workgroup filters take (65 536
    points, 24 576 runs), so the feature's own scratch of the general tile-sort path is used.  Target bit for bit, registration against the model."""
    fx = M.fixture(seed=13, n_target=64)
    gpu = context(binding, 1, loops=(2, 1 << 14, 1 << 17), keyframes=(1 << 14, 1 << 17), nodes=80)
    try:
        stacks = drive(gpu, binding, [fx])
        nd = gpu.graph_export(0)
        i, j = fx["i"], fx["j"]
        qg, tg = guess_of(P, nd, i, j)
        res = gpu.graph_register_loops([(0, i, j, 0, 64, 0, qg, tg)])[0]
        got = [gpu.graph_loop_target(0, cls) for cls in (0, 1)]
    finally:
        gpu.close()
    want = L.target_cloud(nd["q"], nd["t"], stacks[0], i, 0, 64, M.LEAF, M.voxel_filter)
    print(f"raw target {res['target_raw'].tolist()}, filtered {res['target_points'].tolist()}")
    assert res["target_raw"][1] > 65536 and res["target_raw"].tolist() == [sum(len(s[cls]) for s in stacks[0][:64]) for cls in (0, 1)]
    for cls in (0, 1):
        assert got[cls].shape == want[cls].shape and np.array_equal(got[cls].view(np.uint32), want[cls].view(np.uint32)), cls
    m = M.register(want[0], want[1], stacks[0][j][0], stacks[0][j][1], unit(qg), tg)
    assert int(res["status"]) == m["status"] == L.LOOP_OK and (int(res["n_line"]), int(res["n_plane"])) == (m["n_line"], m["n_plane"])
    assert np.abs(res["q"] - m["q"]).max() < Z_BOUND and np.abs(res["t"] - m["t"]).max() < Z_BOUND


def test_a_target_a_million_metres_out_keeps_the_near_result(binding, L, P):
    """The keyframes are fed near the origin; anchor edges and a solve then move the ESTIMATES of nodes 1 .. 8 out by 1e6 m (node 0 is fixed
    and pulls node 1 back by 1e-4 m, so the target is nodes 2 .. 8, node i = 4 among them).  With pose = OPTIMIZED the target is built from
    t_k - t_i of numbers near 1e6: bit for bit loopreg.target_cloud at the exported estimates.  The model's band between the far and the
    near request is measured here and is zero: the differences t_k - t_i lose at most the ulp of 1e6 (1.2e-10 m), which the f32 points of
    the target do not see, so both filtered targets hold the same points and both solves the same bits.  The device's far Z is therefore
    held to its near Z within twice the Z bound (measured: 0), and to the far model within the bound (3.5e-18 / 2.8e-16 in q / t)."""
    fx = M.fixture(seed=7)
    shift = np.array([1.0e6, 0.0, 0.0])
    gpu = context(binding, 1, loops=(2, CAP_CORNER, CAP_SURF))
    try:
        stacks = drive(gpu, binding, [fx])
        nd = gpu.graph_export(0)
        qg, tg = guess_of(P, nd, 4, 9)
        near = gpu.graph_register_loops([(0, 4, 9, 2, 7, 0, qg, tg)])[0]
        gpu.graph_add_edges(np.concatenate([P.anchor_from_localization(k, nd["q"][k], nd["t"][k] + shift, np.eye(6) * 1e12) for k in range(1, 9)]))
        solve = gpu.graph_optimize([0])[0]
        out = gpu.graph_export(0)
        far = gpu.graph_register_loops([(0, 4, 9, 2, 7, 1, qg, tg)])[0]
        got = [gpu.graph_loop_target(0, cls) for cls in (0, 1)]
    finally:
        gpu.close()
    moved = np.abs(out["t_opt"][2:9] - nd["t"][2:9] - shift).max()
    print(f"solve status {solve['status']}, LM {solve['lm_iterations']}; nodes 2 .. 8 off their shifted places by {moved:.2e} m, |t_opt[4]| {np.linalg.norm(out['t_opt'][4]):.1f}")
    assert int(solve["status"]) == binding.GRAPH_OK and moved < 1e-6 and np.linalg.norm(out["t_opt"][4]) > 9.9e5
    want = L.target_cloud(out["q_opt"], out["t_opt"], stacks[0], 4, 2, 7, M.LEAF, M.voxel_filter)
    for cls in (0, 1):
        assert got[cls].shape == want[cls].shape and np.array_equal(got[cls].view(np.uint32), want[cls].view(np.uint32)), cls
    assert np.abs(got[1][:, :3]).max() < 30.0                                     # the frame of node i: tens of metres
    src = stacks[0][9]
    m_far = M.register(want[0], want[1], src[0], src[1], unit(qg), tg)
    m_near = M.register(*L.target_cloud(nd["q"], nd["t"], stacks[0], 4, 2, 7, M.LEAF, M.voxel_filter), src[0], src[1], unit(qg), tg)
    band = max(np.abs(m_far["q"] - m_near["q"]).max(), np.abs(m_far["t"] - m_near["t"]).max())
    dev = max(np.abs(far["q"] - near["q"]).max(), np.abs(far["t"] - near["t"]).max())
    print(f"far against near: device {dev:.3e}, model {band:.3e}; far device against far model |dq| {np.abs(far['q'] - m_far['q']).max():.2e} |dt| {np.abs(far['t'] - m_far['t']).max():.2e}")
    assert int(far["status"]) == int(near["status"]) == m_far["status"] == L.LOOP_OK
    assert (int(far["n_line"]), int(far["n_plane"])) == (m_far["n_line"], m_far["n_plane"]) and (int(near["n_line"]), int(near["n_plane"])) == (m_near["n_line"], m_near["n_plane"])
    assert np.abs(far["q"] - m_far["q"]).max() < Z_BOUND and np.abs(far["t"] - m_far["t"]).max() < Z_BOUND
    assert band == 0.0 and dev <= 2 * Z_BOUND


def test_the_information_of_a_corridor_is_in_the_edges_tangent(binding, L, P):
    """A corridor whose axis lies 50 degrees off node i's x axis (the scene and the path are turned, the sensors' headings are not), Z turned
    by another 0.3 rad: the weakest direction of the translation marginal of `info` is the axis in node j's frame, that of `info_left` the
    axis in node i's frame, as the model's are.  Dropping or transposing T = blockdiag(R_Z, R_Z) swaps or misplaces them."""
    yaw = math.radians(50.0)
    fx = M.fixture(seed=11, kind="corridor", axis_yaw=yaw)
    gpu = context(binding, 1, loops=(2, CAP_CORNER, CAP_SURF))
    try:
        stacks = drive(gpu, binding, [fx])
        nd = gpu.graph_export(0)
        qg, tg = guess_of(P, nd, 4, 9)
        res = gpu.graph_register_loops([(0, 4, 9, 0, 9, 0, qg, tg)])[0]
        tc, ts = L.target_cloud(nd["q"], nd["t"], stacks[0], 4, 0, 9, M.LEAF, M.voxel_filter)
        m = M.register(tc, ts, stacks[0][9][0], stacks[0][9][1], unit(qg), tg)
    finally:
        gpu.close()
    assert int(res["status"]) == m["status"] == L.LOOP_OK

    def weakest(H):
        Mt = H[3:, 3:] - H[:3, 3:].T @ np.linalg.solve(H[:3, :3], H[:3, 3:])
        w, v = np.linalg.eigh(Mt)
        return w, v[:, 0]
    axis = np.array([math.cos(yaw), math.sin(yaw), 0.0])
    a_i, a_j = P.qrot(P.qconj(fx["q_true"][4]), axis), P.qrot(P.qconj(fx["q_true"][9]), axis)
    print(f"the corridor axis in node i's frame {a_i}, in node j's {a_j}")
    assert abs(math.degrees(math.atan2(a_i[1], a_i[0])) - 50.0) < 1.0 and abs(a_j[0]) < 0.9        # the weak direction is no sensor's x axis
    for name, a_own, a_other in (("info", a_j, a_i), ("info_left", a_i, a_j)):
        w, v = weakest(P.info_full(res[name]))
        wm, vm = weakest(m[name])
        print(f"{name}: translation marginal {w}, weakest . own axis {abs(v @ a_own):.6f}, . the other frame's {abs(v @ a_other):.6f}; model {abs(vm @ a_own):.6f}")
        assert w[0] > 0 and w[0] < 0.2 * w[1]
        assert abs(v @ a_own) > 0.999 and abs(v @ a_other) < 0.97 and abs(vm @ a_own) > 0.999 and abs(abs(v @ vm) - 1) < 1e-6


def test_the_measured_edge_closes_the_loop(binding, world, L, P):
    """The ten-node graph of sequence 0 gets the robust edge of its result; aloam_graph_optimize follows aloam_graph_add_edges without a
    synchronise.  Node j ends where the numpy solve of the same graph puts it, and the trajectory error falls."""
    gpu, fx = world["gpu"], world["fx"][0]
    nd = world["nodes"][0][:10]
    qg, tg = guess_of(P, nd, 4, 9)
    res = gpu.graph_register_loops([(0, 4, 9, 0, 9, 0, qg, tg)])[0]
    edge = L.edge_from_result(res, 0, 4, 9)
    assert edge is not None and int(edge["flags"][0]) == P.EDGE_ROBUST
    buf = __import__("torch").zeros(64, dtype=__import__("torch").uint8, pin_memory=True)
    gpu.graph_add_edges(edge)
    gpu.graph_optimize_into([0], buf.data_ptr(), gpu.graph_options())              # no synchronise between the two calls
    gpu.synchronize()
    out = buf.numpy().view(binding.GRAPH_RESULT_DTYPE)[0]
    assert int(out["status"]) == binding.GRAPH_OK
    after = gpu.graph_export(0)[:10]
    edges = gpu.graph_export(0, edges=True)
    odometry = edges[(edges["j"] < 10) & (edges["i"] == edges["j"] - 1)]
    assert len(odometry) == 9 and raw(edges[-1]) == raw(edge[0])
    qm, tm, _ = P.optimize(nd["q"], nd["t"], np.concatenate([odometry, edge]))     # (nodes 10 .. 13 hang off node 9 by odometry edges alone)
    d_dev, d_mod = np.linalg.norm(after["t_opt"][9] - fx["t_true"][9]), np.linalg.norm(tm[9] - fx["t_true"][9])
    ate0, ate1 = P.ate(nd["t"], fx["t_true"]), P.ate(after["t_opt"], fx["t_true"])
    print(f"node j from the truth: entered {np.linalg.norm(nd['t'][9] - fx['t_true'][9]):.4f} m, device {d_dev:.4f} m, numpy solve {d_mod:.4f} m; ATE {ate0:.4f} -> {ate1:.4f} m")
    assert d_dev <= d_mod + 1e-5 and d_dev < 0.05 and ate1 < ate0
    gpu.graph_loop_target(0, 0)                                                     # (the scratch is still there)


def test_refusals_change_nothing(binding, world, P):
    gpu = world["gpu"]
    B = binding
    nd = world["nodes"][0]
    qg, tg = guess_of(P, nd, 4, 9)
    good = (0, 4, 9, 0, 9, 0, qg, tg)
    before = (raw(gpu.graph_export(0)), raw(gpu.graph_export(0, edges=True)), gpu.graph_keyframe_info(0), raw(gpu.map_pose(0)["q_w"]), gpu.map_info(0))
    torch = __import__("torch")
    dst = torch.full((2 * 448,), 0xAB, dtype=torch.uint8, pin_memory=True)
    nodes0 = gpu.graph_info(0)["nodes"]
    bad = [(3, 4, 9, 0, 9, 0, qg, tg), (-1, 4, 9, 0, 9, 0, qg, tg), (0, 4, 9, 0, 0, 0, qg, tg), (0, 4, 9, -1, 9, 0, qg, tg), (0, 4, 9, 0, nodes0 + 1, 0, qg, tg),
           (0, 9, 4, 0, 9, 0, qg, tg), (0, 4, 5, 0, 9, 0, qg, tg), (0, 4, nodes0, 0, 9, 0, qg, tg), (0, 4, -1, 0, 9, 0, qg, tg), (0, 4, 9, 0, 9, 2, qg, tg),
           (0, 4, 9, 0, 9, 0, qg * 1.001, tg), (0, 4, 9, 0, 9, 0, qg * np.array([1, 1, 1, np.nan]), tg), (0, 4, 9, 0, 9, 0, qg, tg * np.array([1, np.inf, 1]))]
    for b in bad:
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_loops_into([good, b], dst.data_ptr())
        assert e.value.code == B.E_ARG, b
    for kw in ({"outer_iterations": 0}, {"lm_max_iterations": -1}):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_loops_into([good], dst.data_ptr(), gpu.graph_loop_options(**kw))
        assert e.value.code == B.E_ARG
    pageable = np.zeros(448, np.uint8)
    for ptr in (pageable.ctypes.data, 0):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_register_loops_into([good], ptr)
        assert e.value.code == B.E_ARG
    gpu.graph_register_loops_into([], 0)                                            # n = 0 is ALOAM_OK
    for args in ((-1, 0), (SLOTS, 0), (0, 2)):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_loop_target(*args)
        assert e.value.code == B.E_ARG
    with pytest.raises(B.AloamError) as e:
        gpu.graph_loops_enable(4, 100, 100)                                         # once per context
    assert e.value.code == B.E_STATE
    gpu.synchronize()
    assert bool((dst == 0xAB).all()) and not pageable.any()
    after = (raw(gpu.graph_export(0)), raw(gpu.graph_export(0, edges=True)), gpu.graph_keyframe_info(0), raw(gpu.map_pose(0)["q_w"]), gpu.map_info(0))
    assert before == after
    # before aloam_graph_keyframes_enable / aloam_graph_loops_enable, and sizes out of range
    bare = context(binding, 1, loops=None, keyframes=None)
    try:
        with pytest.raises(B.AloamError) as e:
            bare.graph_loops_enable(4, 100, 100)
        assert e.value.code == B.E_STATE
        bare.graph_keyframes_enable(1 << 10, 1 << 12)
        for call in (lambda: bare.graph_register_loops_into([good], dst.data_ptr()), lambda: bare.graph_loop_target(0, 0)):
            with pytest.raises(B.AloamError) as e:
                call()
            assert e.value.code == B.E_STATE
        for sizes in ((0, 100, 100), ((1 << 15) + 1, 100, 100), (4, 0, 100), (4, 100, (1 << 24) + 1)):
            with pytest.raises(B.AloamError) as e:
                bare.graph_loops_enable(*sizes)
            assert e.value.code == B.E_ARG
        bare.graph_loops_enable(1, 100, 100)                                        # a refusal left nothing behind that blocks the call
    finally:
        bare.close()


def test_opt_in_changes_nothing_else(binding, twins, P):
    """The twin that never enables the feature returns the same bits from every getter through the drive, its profiling slot counts no
    launch; after a call the enabled context's live sequence, and a following mapping step, are those of the twin."""
    fx, (on, off) = twins
    a, b = on["gpu"], off["gpu"]
    for k in range(10):
        for cls in (0, 1):
            assert np.array_equal(on["stacks"][0][k][cls].view(np.uint32), off["stacks"][0][k][cls].view(np.uint32))
    assert raw(on["nodes"]) == raw(off["nodes"])
    qg, tg = guess_of(P, on["nodes"], 4, 9)
    res = a.graph_register_loops([(0, 4, 9, 0, 9, 0, qg, tg)] * 3)
    assert int(res[0]["status"]) == 0

    def live(g):
        p = g.map_pose(0)
        return (raw(p["q_w"]), raw(p["t_w"]), raw(p["q_wmap_wodom"]), raw(p["t_wmap_wodom"]), g.map_info(0), [[(i, raw(c)) for i, c in sorted(g.map_cubes(cls, 0).items())] for cls in (0, 1)],
                raw(g.map_cloud(binding.MAP_CORNER_STACK, 0)), raw(g.map_cloud(binding.MAP_SURF_STACK, 0)), raw(g.graph_export(0)), g.graph_keyframe_info(0))
    assert live(a) == live(b)
    for g in (a, b):                                                              # a following step
        feed(g, binding, [(fx["raw"][3][0], fx["raw"][3][1], fx["q"][3], fx["t"][3])], [0])
    assert live(a) == live(b)
    pa, pb = a.profile(), b.profile()
    assert pa["loop_register"]["launches"] >= 1 and pb["loop_register"]["launches"] == 0
    for name in pb:
        if name != "loop_register":
            assert pa[name]["launches"] == pb[name]["launches"], name
