"""The numpy model of aloam_graph_search_loops (a-loam_amd/loopreg.py search_grid / search_best, tests/loopsearch_model.py), no GPU: the grid,
the ranking, and the condition on the inputs of the GPU tests - from two far guesses the plain registration ends metres off with status OK,
and the registration started from the grid's best node ends where the near guess ends."""
import importlib
import math

import numpy as np
import pytest

import loopreg_model as M
import loopsearch_model as S


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("a-loam_amd.loopreg")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_grid_is_ordered_yaw_then_y_then_x_around_the_guess(L):
    R = importlib.import_module("a-loam_amd.relocalize")
    assert L.grid_axes is R.grid_axes
    qg = M.quat_z(0.4, 0.03)
    tg = np.array([1.25, -3.5, 0.75])
    q, t, nodes = L.search_grid(qg, tg, 1.0, 0.5, 5.0, 2.5)
    lin, yaw = R.grid_axes(1.0, 0.5, 5.0, 2.5)
    assert len(lin) == 5 and len(yaw) == 5 and q.shape == (125, 4) and t.shape == (125, 3) and nodes.shape == (125, 3) and nodes.dtype.kind == "i"
    want = [(ix, iy, iyaw) for iyaw in range(-2, 3) for iy in range(-2, 3) for ix in range(-2, 3)]
    assert nodes.tolist() == [list(w) for w in want]
    c = 62
    assert nodes[c].tolist() == [0, 0, 0] and np.array_equal(bits(q[c]), bits(qg)) and np.array_equal(bits(t[c]), bits(tg))
    # a node: the guess turned about the z axis of node i's frame through t_g, then shifted; z, roll and pitch untouched
    P = importlib.import_module("a-loam_amd.posegraph")
    for c in (0, 37, 124):
        ix, iy, iyaw = nodes[c]
        assert np.allclose(t[c], tg + np.array([ix * 0.5, iy * 0.5, 0.0]), atol=0, rtol=1e-15) and t[c][2] == tg[2]
        dq = M.quat_z(math.radians(iyaw * 2.5))
        assert np.abs(q[c] - P.qmul(dq, qg)).max() < 1e-15
        assert abs(np.linalg.norm(q[c]) - 1.0) < 1e-15
    # every pose of one yaw shares its quaternion's bits; the centre row of every yaw keeps t_g's bits
    assert all(np.array_equal(bits(q[k * 25]), bits(q[k * 25 + 24])) for k in range(5))
    assert all(np.array_equal(bits(t[k * 25 + 12]), bits(tg)) for k in range(5))
    # shapes of one axis, and the refusals of the call restated
    assert [len(L.search_grid(qg, tg, *g)[0]) for g in ((0, 0, 0, 0), (0, 0.5, 2.5, 2.5), (0.5, 0.5, 0, 0), (0.5, 0.5, 2.5, 2.5), S.DEFAULT_GRID)] == [1, 3, 9, 27, 1859]
    for g in ((1.0, 0.5, 80.0, 2.5), (64.0, 0.5, 0.0, 0.0)):
        with pytest.raises(ValueError):
            L.search_grid(qg, tg, *g)


def test_the_centre_node_keeps_negative_zeros(L):
    qg, tg = np.array([-0.0, 0.0, -0.0, 1.0]), np.array([-0.0, 2.0, -0.0])
    q, t, nodes = L.search_grid(qg, tg, 0.5, 0.5, 2.5, 2.5)
    c = len(q) // 2
    assert nodes[c].tolist() == [0, 0, 0] and np.array_equal(bits(q[c]), bits(qg)) and np.array_equal(bits(t[c]), bits(tg))
    assert np.signbit(t[c][0]) and np.signbit(t[c][2]) and np.signbit(q[c][0])
    assert all(np.signbit(t[k][2]) for k in range(len(t)))                           # z is never touched
    one = L.search_grid(qg, tg, 0.0, 0.0, 0.0, 0.0)
    assert len(one[0]) == 1 and np.array_equal(bits(one[0][0]), bits(qg)) and np.array_equal(bits(one[1][0]), bits(tg))


def test_the_ranking_and_the_zero_factor_rule(L):
    sc = lambda cf, sf, cost: {"corner_factors": cf, "surf_factors": sf, "corner_found": cf, "surf_found": sf, "cost": cost}
    assert L.search_best([sc(1, 2, 5.0), sc(2, 2, 9.0), sc(3, 1, 9.0), sc(0, 4, 8.0)], 1) == 3                # most factors, then the lower cost
    assert L.search_best([sc(1, 2, 5.0), sc(2, 2, 9.0), sc(3, 1, 9.0)], 0) == 1                               # ... then the lower index
    assert L.search_best([sc(2, 2, float("nan")), sc(3, 1, 1e300), sc(0, 0, 0.0)], 2) == 1                    # NaN ranks as +infinity
    assert L.search_best([sc(0, 0, 0.0)] * 27, 13) == 13                                                      # no factor anywhere: the guess, not index 0
    assert L.search_best([sc(0, 0, 0.0)] * 26 + [sc(0, 1, 3.0)], 13) == 26
    binding = importlib.import_module("a-loam_amd.binding")
    arr = np.zeros(5, binding.MAP_SCORE_DTYPE)
    assert L.search_best(arr, 2) == 2
    arr["surf_factors"][4] = 7
    assert L.search_best(arr, 2) == 4


@pytest.fixture(scope="module")
def scene(L):
    fx = M.fixture(seed=7)
    clouds = M.keyframe_clouds(fx)
    tc, ts = L.target_cloud(fx["q"], fx["t"], clouds, fx["i"], fx["first"], fx["count"], M.LEAF, M.voxel_filter)
    return fx, tc, ts, clouds[fx["j"]]


def test_the_near_guess_is_inside_the_basin(scene):
    fx, tc, ts, src = scene
    (qg, tg), (qt, tt) = M.request_of(fx)
    r0, d0 = M.pose_error(qg, tg, qt, tt)
    res = M.register(tc, ts, src[0], src[1], qg, tg)
    r1, d1 = M.pose_error(res["q"], res["t"], qt, tt)
    print(f"near guess {d0:.3f} m, {r0:.4f} rad -> {d1:.2e} m, {r1:.2e} rad; factors {res['n_line']} + {res['n_plane']}")
    assert res["status"] == 0 and abs(d0 - 0.399) < 1e-3 and abs(r0 - 0.0705) < 1e-4
    assert abs(d1 - 9.1e-3) < 1e-4 and abs(r1 - 3.9e-4) < 1e-5 and (res["n_line"], res["n_plane"]) == (169, 1078)


@pytest.mark.parametrize("k", [0, 1])
def test_a_far_guess_is_lost_without_the_search_and_recovered_with_it(L, scene, k):
    """The two far guesses of the GPU tests.  The plain model ends more than 0.5 m off with status OK; the model's best node of the default
    grid lies inside the basin, and the registration from it ends within 1e-2 m and 1e-3 rad of the truth (the near guess ends at 9.1e-3 m
    and 3.9e-4 rad: the target and the source hold their own samples of the scene, so that is where the truth of this fixture is)."""
    fx, tc, ts, src = scene
    (_, _), (qt, tt) = M.request_of(fx)
    shift, dyaw = S.FAR_GUESSES[k]
    qf, tf = S.far_guess(fx, shift, dyaw)
    plain = M.register(tc, ts, src[0], src[1], qf, tf)
    rp, dp = M.pose_error(plain["q"], plain["t"], qt, tt)
    print(f"far guess {k}: plain registration ends {dp:.3f} m, {rp:.3f} rad off, factors {plain['n_line']} + {plain['n_plane']}, status {plain['status']}")
    assert plain["status"] == L.LOOP_OK and dp > 0.5
    q, t, nodes = L.search_grid(qf, tf, *S.DEFAULT_GRID)
    assert len(q) == 1859
    centre = len(q) // 2
    best, score, fitted = S.best_node(src[0], src[1], tc, ts, q, t, centre)
    guess = S.score_nodes(src[0], src[1], tc, ts, q, t, only=[centre])[centre]
    rb, db = M.pose_error(q[best], t[best], qt, tt)
    print(f"far guess {k}: guess node {guess['corner_factors'] + guess['surf_factors']} factors, best node {best} {nodes[best].tolist()} "
          f"{score['corner_factors'] + score['surf_factors']} factors ({fitted} nodes fitted exactly), {db:.3f} m, {rb:.4f} rad off the truth")
    assert score["corner_factors"] + score["surf_factors"] > guess["corner_factors"] + guess["surf_factors"] and db < 0.5
    res = M.register(tc, ts, src[0], src[1], q[best], t[best])
    rs, ds = M.pose_error(res["q"], res["t"], qt, tt)
    print(f"far guess {k}: registration from the best node ends {ds:.2e} m, {rs:.2e} rad off, factors {res['n_line']} + {res['n_plane']}")
    assert res["status"] == L.LOOP_OK and ds < 1e-2 and rs < 1e-3
