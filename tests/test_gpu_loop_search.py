"""A pose grid searched around a loop guess on the MI355X (aloam_graph_search_loops): every node's score against the numpy model of
tests/loopsearch_model.py and against a registration's first round on the device, two far guesses recovered, the grid of one node against
the plain call, the shapes at which the new kernels can go wrong, independence of the other requests, the skipped slots, the refusals,
and that the plain call is left alone.

Context, feed and drive are those of test_gpu_loop_register.py: hand-made keyframes with the context's solver off; the scene of
loopreg_model.fixture, nine target nodes along 8 m and one source node."""
import importlib

import numpy as np
import pytest

import loopreg_model as M
import loopsearch_model as S
from test_gpu_loop_register import CAP_CORNER, CAP_SURF, SLOTS, Z_BOUND, L, P, context, drive, guess_of, model_target, raw, twins, unit, world  # noqa: F401

pytestmark = pytest.mark.gpu
INFO = np.eye(6) * 100.0
SMALL = dict(radius_m=1.0, step_m=0.5, yaw_deg=5.0, yaw_step_deg=2.5)              # 125 nodes
ONE = dict(radius_m=0.0, step_m=0.5, yaw_deg=0.0, yaw_step_deg=2.5)
COUNTS = ("corner_factors", "surf_factors", "corner_found", "surf_found")


def grid_of(L, q, t, g):
    return L.search_grid(unit(q), t, g["radius_m"], g["step_m"], g["yaw_deg"], g["yaw_step_deg"])


@pytest.fixture(scope="module")
def near(world, L, P):
    """Shared by the first two tests: the near guess of sequence 0 searched over the 125-node grid, with its score table."""
    gpu = world["gpu"]
    qg, tg = guess_of(P, world["nodes"][0], 4, 9)
    req = (0, 4, 9, 0, 9, 0, qg, tg)
    res, sres, sc = gpu.graph_search_loops([req], search=SMALL, scores=True)
    q, t, nodes = grid_of(L, qg, tg, SMALL)
    return {"req": req, "res": res[0], "search": sres[0], "scores": sc[0], "q": q, "t": t, "nodes": nodes}


def test_scores_equal_the_model(world, near, L):
    tc, ts = model_target(L, world, 0, 4, 0, 9)
    src = world["stacks"][0][9]
    q, t, nodes, sc, sr = near["q"], near["t"], near["nodes"], near["scores"], near["search"]
    K, centre = len(q), len(q) // 2
    assert K == 125 and sc.shape == (K,) and int(sr["nodes"]) == K and int(sr["status"]) == L.LOOP_OK
    want = S.score_nodes(src[0], src[1], tc, ts, q, t)
    bounds = S.node_bounds(src[0], src[1], tc, ts, q, t)
    skipped = [c for c in range(K) if bounds[c][0] != bounds[c][1]]
    worst = 0.0
    for c in range(K):
        if c in skipped:
            continue
        assert tuple(int(sc[c][k]) for k in COUNTS) == tuple(want[c][k] for k in COUNTS), (c, nodes[c], sc[c], want[c])
        worst = max(worst, abs(float(sc[c]["cost"]) - want[c]["cost"]) / max(want[c]["cost"], 1e-300))
    total = sc["corner_factors"] + sc["surf_factors"]
    print(f"{K} nodes, {len(skipped)} within the model's margin of a threshold; cost against the model: max relative {worst:.3e}; factors {total.min()} .. {total.max()}, "
          f"guess {total[centre]}; best node {int(sr['best'])} {nodes[int(sr['best'])].tolist()}")
    assert len(skipped) <= K // 20 and worst <= 1e-9
    assert total.max() > total.min() and not sc["pad"].any()
    # the record against the table, the table's winner against the ranking
    best = int(sr["best"])
    assert best == L.search_best(sc, centre) and (int(sr["ix"]), int(sr["iy"]), int(sr["iyaw"])) == tuple(nodes[best])
    assert raw(sr["best_score"]) == raw(sc[best]) and raw(sr["guess_score"]) == raw(sc[centre])
    assert np.array_equal(sr["q"], q[best]) and np.array_equal(sr["t"], t[best]) and sr["reserved"] == 0 and not sr["pad"].any()
    order = sorted(range(K), key=lambda c: -(want[c]["corner_factors"] + want[c]["surf_factors"]))
    if not skipped and want[order[0]]["corner_factors"] + want[order[0]]["surf_factors"] > want[order[1]]["corner_factors"] + want[order[1]]["surf_factors"]:
        assert best == order[0] == L.search_best(want, centre)


def test_counts_equal_a_registrations_first_round(world, near, L):
    """Device against device: a plain registration started from a node's pose, one round and no solver iteration, evaluates that round's
    records at the same pose.  (The plain call divides its guess by its norm, which can move the last bit of a turned node's quaternion:
    the counts are compared as integers all the same, and a node at which they differed would sit on a threshold.)"""
    gpu = world["gpu"]
    q, t, sc = near["q"], near["t"], near["scores"]
    K = len(q)
    picks = sorted({K // 2, 0, int(near["search"]["best"]), 37, K - 1})
    assert len(picks) == 5
    res = gpu.graph_register_loops([(0, 4, 9, 0, 9, 0, q[c], t[c]) for c in picks], outer_iterations=1, lm_max_iterations=0)
    ok = 0
    for c, r in zip(picks, res):
        print(f"node {c}: plain status {r['status']}, factors {r['n_line']} + {r['n_plane']} (searched {sc[c]['corner_factors']} + {sc[c]['surf_factors']}), "
              f"cost {r['cost']:.12g} / {sc[c]['cost']:.12g}")
        if int(r["status"]) != L.LOOP_OK:
            continue
        ok += 1
        assert (int(r["n_line"]), int(r["n_plane"])) == (int(sc[c]["corner_factors"]), int(sc[c]["surf_factors"]))
        assert abs(float(r["cost"]) - float(sc[c]["cost"])) <= 1e-9 * float(sc[c]["cost"])
    assert ok >= 3


@pytest.mark.parametrize("k", [0, 1])
def test_the_far_guesses_are_recovered(world, L, P, k):
    gpu, fx = world["gpu"], world["fx"][0]
    tc, ts = model_target(L, world, 0, 4, 0, 9)
    src = world["stacks"][0][9]
    (_, _), (qt, tt) = M.request_of(fx)
    qf, tf = S.far_guess(fx, *S.FAR_GUESSES[k])
    req = (0, 4, 9, 0, 9, 0, qf, tf)
    res, sres = gpu.graph_search_loops([req])
    res, sres = res[0], sres[0]
    plain = gpu.graph_register_loops([req])[0]
    q, t, nodes = L.search_grid(unit(qf), tf, *S.DEFAULT_GRID)
    best, score, fitted = S.best_node(src[0], src[1], tc, ts, q, t, len(q) // 2)
    dp = M.pose_error(plain["q"], plain["t"], qt, tt)
    ds = M.pose_error(res["q"], res["t"], qt, tt)
    print(f"far guess {k}: plain call ends {dp[1]:.3f} m / {dp[0]:.3f} rad off (status {plain['status']}); best node device {int(sres['best'])} model {best} "
          f"{nodes[best].tolist()} ({fitted} fitted exactly), factors {sres['best_score']['corner_factors']} + {sres['best_score']['surf_factors']} against the guess's "
          f"{sres['guess_score']['corner_factors']} + {sres['guess_score']['surf_factors']}; searched call ends {ds[1]:.2e} m / {ds[0]:.2e} rad off")
    assert dp[1] > 0.5                                                               # the condition on the inputs (test_loopsearch_model.py)
    assert int(sres["nodes"]) == 1859 and int(sres["best"]) == best
    assert tuple(int(sres["best_score"][c]) for c in COUNTS) == tuple(score[c] for c in COUNTS)
    assert np.array_equal(sres["q"], q[best]) and np.array_equal(sres["t"], t[best])
    m = M.register(tc, ts, src[0], src[1], q[best], t[best])
    assert int(res["status"]) == m["status"] == L.LOOP_OK
    assert (int(res["n_line"]), int(res["n_plane"]), int(res["lm_iterations"]), int(res["lm_termination"])) == (m["n_line"], m["n_plane"], m["lm_iterations"], m["lm_termination"])
    assert np.abs(res["q"] - m["q"]).max() < Z_BOUND and np.abs(res["t"] - m["t"]).max() < Z_BOUND
    assert ds[1] < 1e-2 and ds[0] < 1e-3


def requests(world, P):
    """Nine requests over the three sequences: both rooms, the sources of 255 / 256 / 257 surf points and the one without corners, optimised
    poses, a target of one node, the floor-only sequence."""
    nd = world["nodes"]
    g = lambda b, i, j: guess_of(P, nd[b], i, j)
    return [(0, 4, 9, 0, 9, 0) + g(0, 4, 9), (1, 4, 9, 0, 9, 0) + g(1, 4, 9), (0, 4, 10, 0, 9, 0) + g(0, 4, 10), (0, 4, 11, 0, 9, 0) + g(0, 4, 11),
            (0, 4, 12, 0, 9, 0) + g(0, 4, 12), (0, 4, 13, 0, 9, 0) + g(0, 4, 13), (1, 2, 9, 1, 5, 1) + g(1, 2, 9), (0, 4, 9, 4, 1, 0) + g(0, 4, 9),
            (2, 4, 9, 0, 9, 0) + g(2, 4, 9)]


def test_a_grid_of_one_node_is_the_plain_call(world, L, P):
    gpu = world["gpu"]
    reqs = requests(world, P)
    plain = gpu.graph_register_loops(reqs)
    res, sres, sc = gpu.graph_search_loops(reqs, search=ONE, scores=True)
    assert raw(res) == raw(plain) and sc.shape == (len(reqs), 1)
    for r, rq in enumerate(reqs[:-1]):
        assert int(sres[r]["best"]) == 0 and int(sres[r]["nodes"]) == 1 and (int(sres[r]["ix"]), int(sres[r]["iy"]), int(sres[r]["iyaw"])) == (0, 0, 0)
        assert np.array_equal(sres[r]["q"], unit(rq[6])) and np.array_equal(sres[r]["t"], rq[7])
        assert raw(sres[r]["best_score"]) == raw(sres[r]["guess_score"]) == raw(sc[r][0])
    assert [int(s) for s in sres["status"]] == [L.LOOP_OK] * 8 + [L.LOOP_TARGET_TOO_SMALL] and int(sres[8]["best"]) == -1
    assert int(sc[0][0]["surf_factors"]) > 500 and int(sc[5][0]["corner_found"]) == 0 and int(plain[5]["source_points"][0]) == 0


@pytest.mark.parametrize("grid", [ONE, dict(radius_m=0.0, step_m=0.5, yaw_deg=2.5, yaw_step_deg=2.5), dict(radius_m=0.5, step_m=0.5, yaw_deg=0.0, yaw_step_deg=0.0),
                                  dict(radius_m=0.5, step_m=0.5, yaw_deg=2.5, yaw_step_deg=2.5)], ids=["K1", "K3", "K9", "K27"])
def test_shapes_at_which_the_kernels_can_go_wrong(world, L, P, grid):
    """K of 1, 3 (yaw only), 9 (x, y only) and 27; 1, 3 and 9 requests (fewer and more than 8 slots in flight, and 9 > max_requests = 8: two
    rounds); sources of 255 / 256 / 257 surf points and an empty corner cloud.  Every result against the same request run alone."""
    gpu = world["gpu"]
    reqs = requests(world, P)
    K = len(grid_of(L, reqs[0][6], reqs[0][7], grid)[0])
    alone = [gpu.graph_search_loops([rq], search=grid, scores=True) for rq in reqs]
    assert all(a[2].shape == (1, K) and int(a[1][0]["nodes"]) == K for a in alone)
    for n in (1, 3, 9):
        res, sres, sc = gpu.graph_search_loops(reqs[:n], search=grid, scores=True)
        for r in range(n):
            assert (raw(res[r]), raw(sres[r]), raw(sc[r])) == (raw(alone[r][0][0]), raw(alone[r][1][0]), raw(alone[r][2][0])), (n, r)
    # the small sources are searched like the others: their scores are no copy of a neighbour's
    assert len({raw(a[2][0]) for a in alone}) == len(alone) and all(int(a[1][0]["best"]) >= 0 for a in alone[:8])
    assert all(int(a[2][0]["surf_found"].max()) > 100 for a in alone[2:5]) and int(alone[5][2][0]["corner_found"].max()) == 0


def test_rounds_bounded_by_the_pairs_of_a_round(binding, L, P):
    """20 slots and a grid of 14175 nodes: 2^18 / K = 18 requests make a round, fewer than the slots.  Requests of the first and of the second
    round against the same request run alone."""
    fx = M.fixture(seed=7)
    gpu = context(binding, 1, loops=(20, CAP_CORNER, CAP_SURF))
    grid = dict(radius_m=3.5, step_m=0.5, yaw_deg=31.0, yaw_step_deg=1.0)
    try:
        drive(gpu, binding, [fx])
        nd = gpu.graph_export(0)
        qg, tg = guess_of(P, nd, 4, 9)
        K = len(grid_of(L, qg, tg, grid)[0])
        assert K == 14175 and (1 << 18) // K == 18
        a = (0, 4, 9, 0, 9, 0, qg, tg)
        b = (0, 4, 9, 2, 5, 0, qg, tg + np.array([0.2, 0.0, 0.0]))
        alone = [gpu.graph_search_loops([rq], search=grid) for rq in (a, b)]
        res, sres = gpu.graph_search_loops([a] * 17 + [b, a, b], search=grid)
    finally:
        gpu.close()
    assert int(alone[0][1][0]["best"]) != int(alone[1][1][0]["best"]) or raw(alone[0][0][0]) != raw(alone[1][0][0])
    for r, w in ((0, 0), (16, 0), (17, 1), (18, 0), (19, 1)):
        assert (raw(res[r]), raw(sres[r])) == (raw(alone[w][0][0]), raw(alone[w][1][0])), r


def test_a_result_does_not_depend_on_the_other_requests(world, L, P):
    gpu = world["gpu"]
    reqs = requests(world, P)
    a = reqs[0]
    alone = tuple(raw(v[0]) for v in gpu.graph_search_loops([a], search=SMALL, scores=True))
    one = gpu.graph_search_loops(reqs[1:4] + [a] + reqs[4:], search=SMALL, scores=True)
    two = gpu.graph_search_loops([reqs[8], a, reqs[6]], search=SMALL, scores=True)
    assert tuple(raw(v[3]) for v in one) == alone and tuple(raw(v[1]) for v in two) == alone
    rev = gpu.graph_search_loops((reqs[1:4] + [a] + reqs[4:])[::-1], search=SMALL, scores=True, pinned=False)
    assert tuple(raw(v[5]) for v in rev) == alone
    assert [raw(one[0][k]) for k in (0, 1, 2, 4)] == [raw(rev[0][8 - k]) for k in (0, 1, 2, 4)]


def skipped_is_the_plain_call(L, rq, res, sres, sc, plain, status):
    assert int(sres["status"]) == status and int(sres["best"]) == -1 and (int(sres["ix"]), int(sres["iy"]), int(sres["iyaw"])) == (0, 0, 0)
    assert not np.ascontiguousarray(sc).view(np.uint8).any() and not np.ascontiguousarray(sres["best_score"]).view(np.uint8).any()
    assert not np.ascontiguousarray(sres["guess_score"]).view(np.uint8).any()
    assert np.array_equal(sres["q"], unit(rq[6])) and np.array_equal(sres["t"], rq[7]) and raw(res) == raw(plain) and int(res["status"]) == status


def test_skipped_slots(binding, world, twins, L, P):
    gpu = world["gpu"]
    reqs = requests(world, P)
    floor, ok = reqs[8], reqs[0]
    alone = gpu.graph_search_loops([ok], search=SMALL, scores=True)
    plain = gpu.graph_register_loops([floor])
    res, sres, sc = gpu.graph_search_loops([floor, ok], search=SMALL, scores=True)
    skipped_is_the_plain_call(L, floor, res[0], sres[0], sc[0], plain[0], L.LOOP_TARGET_TOO_SMALL)
    assert (raw(res[1]), raw(sres[1]), raw(sc[1])) == tuple(raw(v[0]) for v in alone)                         # the neighbour is untouched
    # a grid 50 m from everything: no node has a factor, the centre node - the guess - is taken
    far = ok[:7] + (ok[7] + np.array([50.0, 0.0, 0.0]),)
    res, sres, sc = gpu.graph_search_loops([far], search=SMALL, scores=True)
    assert not (sc[0]["corner_factors"] + sc[0]["surf_factors"]).any() and int(sres[0]["best"]) == 62 and int(sres[0]["status"]) == L.LOOP_OK
    assert np.array_equal(sres[0]["q"], unit(far[6])) and np.array_equal(sres[0]["t"], far[7])
    assert raw(res[0]) == raw(gpu.graph_register_loops([far])[0]) and int(res[0]["status"]) == L.LOOP_SOLVE_FAILED
    # a target above the capacity
    fx, _ = twins
    small = context(binding, 1, loops=(4, CAP_CORNER, 4000))
    try:
        drive(small, binding, [fx])
        nd = small.graph_export(0)
        big = (0, 4, 9, 0, 9, 0) + guess_of(P, nd, 4, 9)
        fits = (0, 4, 9, 3, 3, 0) + guess_of(P, nd, 4, 9)
        alone = small.graph_search_loops([fits], search=SMALL, scores=True)
        plain = small.graph_register_loops([big])
        res, sres, sc = small.graph_search_loops([big, fits], search=SMALL, scores=True)
        skipped_is_the_plain_call(L, big, res[0], sres[0], sc[0], plain[0], L.LOOP_TOO_LARGE)
        assert (raw(res[1]), raw(sres[1]), raw(sc[1])) == tuple(raw(v[0]) for v in alone) and int(res[1]["status"]) == L.LOOP_OK
    finally:
        small.close()
    # a node kept without clouds
    gpu = context(binding, 1, keyframes=(1 << 13, 9 * 1100), loops=(2, CAP_CORNER, CAP_SURF))             # the surf row takes nine keyframes, not ten
    try:
        for k in range(10):
            gpu.set_last(fx["raw"][k][0], fx["raw"][k][1], 0); gpu.set_full_cloud(fx["raw"][k][1][:4], 0)
            gpu.set_state([0, 0, 0, 1], [0, 0, 0], fx["q"][k], fx["t"][k], 0)
            gpu.mapping_step()
            gpu.graph_add_nodes([0], INFO)
        with pytest.raises(binding.AloamError) as e:
            gpu.synchronize()
        assert e.value.code == binding.E_CAPACITY
        nd = gpu.graph_export(0)
        none = (0, 4, 9, 0, 9, 0) + guess_of(P, nd, 4, 9)
        fits = (0, 4, 8, 0, 8, 0) + guess_of(P, nd, 4, 8)
        alone = gpu.graph_search_loops([fits], search=SMALL, scores=True)
        plain = gpu.graph_register_loops([none])
        res, sres, sc = gpu.graph_search_loops([none, fits], search=SMALL, scores=True)
        skipped_is_the_plain_call(L, none, res[0], sres[0], sc[0], plain[0], L.LOOP_NO_CLOUDS)
        assert (raw(res[1]), raw(sres[1]), raw(sc[1])) == tuple(raw(v[0]) for v in alone) and int(res[1]["status"]) == L.LOOP_OK
    finally:
        gpu.close()


def test_refusals_change_nothing(binding, world, P):
    gpu, B = world["gpu"], binding
    torch = importlib.import_module("torch")
    qg, tg = guess_of(P, world["nodes"][0], 4, 9)
    good = (0, 4, 9, 0, 9, 0, qg, tg)
    before = tuple(raw(v) for v in gpu.graph_search_loops([good], search=SMALL, scores=True))
    dst = torch.full((2 * 448,), 0xAB, dtype=torch.uint8, pin_memory=True)
    sdst = torch.full((2 * 160,), 0xAB, dtype=torch.uint8, pin_memory=True)
    sc = torch.full((2 * 125 * 32,), 0xAB, dtype=torch.uint8, pin_memory=True)
    grid = gpu.graph_loop_search(**SMALL)
    nodes0 = gpu.graph_info(0)["nodes"]

    def refused(code, reqs, d=None, s=None, c=None, search=grid, options=None):
        with pytest.raises(B.AloamError) as e:
            gpu.graph_search_loops_into(reqs, dst.data_ptr() if d is None else d, sdst.data_ptr() if s is None else s, sc.data_ptr() if c is None else c, search, options)
        assert e.value.code == code, (reqs, search, options)

    # the request checks of the plain call
    for b in ((3, 4, 9, 0, 9, 0, qg, tg), (-1, 4, 9, 0, 9, 0, qg, tg), (0, 4, 9, 0, 0, 0, qg, tg), (0, 4, 9, -1, 9, 0, qg, tg), (0, 4, 9, 0, nodes0 + 1, 0, qg, tg),
              (0, 9, 4, 0, 9, 0, qg, tg), (0, 4, 5, 0, 9, 0, qg, tg), (0, 4, nodes0, 0, 9, 0, qg, tg), (0, 4, -1, 0, 9, 0, qg, tg), (0, 4, 9, 0, 9, 2, qg, tg),
              (0, 4, 9, 0, 9, 0, qg * 1.001, tg), (0, 4, 9, 0, 9, 0, qg * np.array([1, 1, 1, np.nan]), tg), (0, 4, 9, 0, 9, 0, qg, tg * np.array([1, np.inf, 1]))):
        refused(B.E_ARG, [good, b])
    for kw in ({"outer_iterations": 0}, {"lm_max_iterations": -1}):
        refused(B.E_ARG, [good], options=gpu.graph_loop_options(**kw))
    # the grid: negative or non-finite values, more than 31 yaw steps to either side, more than 2^14 nodes
    for kw in ({"radius_m": -1.0}, {"step_m": -0.5}, {"yaw_deg": -1.0}, {"yaw_step_deg": -2.5}, {"radius_m": float("nan")}, {"step_m": float("inf")}, {"yaw_deg": float("inf")},
               {"yaw_deg": 80.0}, {"radius_m": 32.0}, {"radius_m": 1e300, "step_m": 1e-300}, {"radius_m": 4.0, "yaw_deg": 31.0, "yaw_step_deg": 1.0}):
        refused(B.E_ARG, [good], search=gpu.graph_loop_search(**kw))
    # pageable or missing destinations
    pageable = np.zeros(125 * 32, np.uint8)
    refused(B.E_ARG, [good], d=pageable.ctypes.data)
    refused(B.E_ARG, [good], s=pageable.ctypes.data)
    refused(B.E_ARG, [good], c=pageable.ctypes.data)
    with pytest.raises(B.AloamError) as e:
        gpu.graph_search_loops_into([good], dst.data_ptr(), 0, 0, grid)
    assert e.value.code == B.E_ARG
    with pytest.raises(B.AloamError) as e:
        gpu.graph_search_loops_into([good], 0, sdst.data_ptr(), 0, grid)
    assert e.value.code == B.E_ARG
    gpu.graph_search_loops_into([], 0, 0, 0, grid)                                  # n = 0 is ALOAM_OK
    with pytest.raises(B.AloamError) as e:
        gpu.graph_search_loops_into([], 0, 0, 0, gpu.graph_loop_search(yaw_deg=80.0))   # ... behind the checks of the grid
    assert e.value.code == B.E_ARG
    gpu.synchronize()
    assert bool((dst == 0xAB).all()) and bool((sdst == 0xAB).all()) and bool((sc == 0xAB).all()) and not pageable.any()
    assert tuple(raw(v) for v in gpu.graph_search_loops([good], search=SMALL, scores=True)) == before
    bare = context(binding, 1, loops=None)
    try:
        with pytest.raises(B.AloamError) as e:
            bare.graph_search_loops_into([good], dst.data_ptr(), sdst.data_ptr(), 0, grid)
        assert e.value.code == B.E_STATE
    finally:
        bare.close()


def test_opt_in_changes_nothing_else(twins, P):
    """Until this test the enabled twin has never called the new entry point: its plain call's bits and its loop_register launches per
    plain call are taken first, then it searches once, then the plain call gives the same bits and counts the same launches.  The twin
    without the feature has the same profiling names and no launch in the slot."""
    fx, (on, off) = twins
    a = on["gpu"]
    qg, tg = guess_of(P, on["nodes"], 4, 9)
    req = (0, 4, 9, 0, 9, 0, qg, tg)
    before = raw(a.graph_register_loops([req])[0])
    p0 = a.profile()["loop_register"]["launches"]
    a.graph_register_loops([req])
    per_call = a.profile()["loop_register"]["launches"] - p0
    res, sres = a.graph_search_loops([req], search=SMALL)
    assert int(sres[0]["best"]) >= 0
    p1 = a.profile()["loop_register"]["launches"]
    assert raw(a.graph_register_loops([req])[0]) == before
    assert a.profile()["loop_register"]["launches"] - p1 == per_call
    names = set(a.profile())
    assert names == set(off["gpu"].profile()) and off["gpu"].profile()["loop_register"]["launches"] == 0
