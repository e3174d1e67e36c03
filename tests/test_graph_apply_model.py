"""The numpy definition of aloam_graph_apply: posegraph.apply_correction (the correction D of a solved graph, the live poses moved by it,
the rebase of the nodes) and atlas.window_from_keyframes (the window cut from the map of the keyframes at a centre that puts the sensor's
cube in the middle)."""
import importlib

import numpy as np
import pytest

from test_gpu_graph_map import BOUNDARY, boundary_points

EPS = np.finfo(np.float64).eps
LEAF = (0.4, 0.8)


@pytest.fixture(scope="module")
def pg():
    return importlib.import_module("a-loam_amd.posegraph")


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


@pytest.fixture(scope="module")
def solved(pg):
    """drifted_laps with one loop edge, solved by the dense reference: the nodes as entered and as estimated."""
    d = pg.drifted_laps(4, 40, 1, per_lap=30)
    edges = np.concatenate([d["odom"], d["loop"]])
    q_opt, t_opt, res = pg.optimize(d["q"], d["t"], edges)
    assert res["status"] == 0 and res["final_cost"] < res["initial_cost"] and np.abs(t_opt[-1] - d["t"][-1]).max() > 1e-2
    return dict(q=d["q"], t=d["t"], q_opt=q_opt, t_opt=t_opt, edges=edges)


def close(got, want, scale=8.0):
    (gq, gt), (wq, wt) = got, want
    return np.abs(gq - wq).max() <= scale * EPS and np.abs(gt - wt).max() <= scale * EPS * max(1.0, np.abs(wt).max())


def test_the_live_pose_of_the_last_node_becomes_its_estimate(pg, solved):
    s = solved
    (qd, td), live, (qr, tr) = pg.apply_correction(s["q"], s["t"], s["q_opt"], s["t_opt"], [(s["q"][-1], s["t"][-1])])
    assert abs(np.linalg.norm(qd) - 1.0) <= 2 * EPS
    assert close(live[0], (s["q_opt"][-1], s["t_opt"][-1]))
    assert qr.tobytes() == s["q_opt"].tobytes() and tr.tobytes() == s["t_opt"].tobytes()          # the rebase is a bit copy
    assert qr is not s["q_opt"]


def test_a_pose_entered_later_gives_the_edge_from_the_estimate(pg, solved):
    """P is entered in the corrected frame as D o P; the odometry edge from the rebased last node is X_opt[K-1]^-1 o D o P, which is what
    the drift-frame edge X[K-1]^-1 o P was - and not what the entered pose of the last node would give without the rebase."""
    s = solved
    P = pg.compose(s["q"][-1], s["t"][-1], pg.qexp(np.array([0.01, -0.02, 0.05])), np.array([1.2, 0.1, -0.05]))
    (qd, td), live, (qr, tr) = pg.apply_correction(s["q"], s["t"], s["q_opt"], s["t_opt"], [P])
    edge = pg.relative_pose(qr[-1], tr[-1], *live[0])
    qi, ti = pg.inverse(s["q_opt"][-1], s["t_opt"][-1])
    assert close(edge, pg.compose(qi, ti, *pg.compose(qd, td, *P)), 16.0)
    assert close(edge, pg.relative_pose(s["q"][-1], s["t"][-1], *P), 64.0)
    wrong = pg.relative_pose(s["q"][-1], s["t"][-1], *live[0])                                  # without the rebase the edge is off by D
    assert np.abs(wrong[1] - edge[1]).max() > 1e-3


def test_a_second_apply_is_the_identity(pg, solved):
    s = solved
    live0 = [(s["q"][-1], s["t"][-1]), pg.compose(s["q"][-1], s["t"][-1], pg.qexp(np.array([0.0, 0.0, 0.3])), np.array([5.0, 1.0, 0.0]))]
    _, live1, (qr, tr) = pg.apply_correction(s["q"], s["t"], s["q_opt"], s["t_opt"], live0)
    (qd, td), live2, (qr2, tr2) = pg.apply_correction(qr, tr, s["q_opt"], s["t_opt"], live1)
    bound = 8 * EPS * max(1.0, np.abs(s["t_opt"][-1]).max())
    assert np.abs(qd - np.array([0.0, 0.0, 0.0, 1.0])).max() <= 8 * EPS and np.abs(td).max() <= bound
    for a, b in zip(live1, live2):
        assert close(b, a)
    assert qr2.tobytes() == qr.tobytes() and tr2.tobytes() == tr.tobytes()


def test_the_cost_of_the_rebased_graph_is_the_cost_before(pg, solved):
    s = solved
    before = pg.cost(s["q_opt"], s["t_opt"], s["edges"])
    _, _, (qr, tr) = pg.apply_correction(s["q"], s["t"], s["q_opt"], s["t_opt"], [])
    assert pg.cost(qr, tr, s["edges"]) == before                                                # entered poses = estimates: bit for bit
    assert pg.cost(s["q"], s["t"], s["edges"]) != before


def test_the_window_centre_follows_cube_coord_at_the_boundaries(atlas):
    """(10, 10, 5) minus int((v + 25) / 50), minus one more when v + 25 < 0, of the f64 position: at -75, -25, 25, one f32 ulp either side
    (the table of the graph-map tests) and one f64 ulp either side (where v + 25 may round onto the boundary, as it does on the device)."""
    f32 = np.float32
    table = {(-75.0, -1): -2, (-75.0, 0): -2, (-75.0, 1): -1, (-25.0, -1): -1, (-25.0, 0): 0, (-25.0, 1): 0, (25.0, -1): 0, (25.0, 0): 1, (25.0, 1): 1}
    for v in (-75.0, -25.0, 25.0):
        near = [(float(np.nextafter(f32(v), f32(-1e9))), table[v, -1]), (v, table[v, 0]), (float(np.nextafter(f32(v), f32(1e9))), table[v, 1]),
                (float(np.nextafter(v, -1e9)), None), (float(np.nextafter(v, 1e9)), None)]
        for x, cube in near:
            s = x + 25.0
            plain = int(s / 50.0) - (1 if s < 0 else 0)
            assert cube is None or cube == plain, x
            for axis in range(3):
                t = np.array([3.0, 4.0, 5.0])
                t[axis] = x
                want = [10, 10, 5]
                want[axis] -= plain
                assert atlas.window_centre(t) == tuple(want), (x, axis)


def test_the_window_is_a_cut_of_the_tiles(O, atlas):
    """The boundary points of the graph-map tests in a keyframe at the identity, the window centred for a sensor at -75, -25, 25 and one
    ulp either side on every axis: the model equals Atlas.cut of tiles_from_keyframes, every boundary point sits in the cube cube_coord
    gives it, and the points the window leaves out are counted."""
    rng = np.random.default_rng(7)
    body = rng.uniform(-120.0, 120.0, (600, 4)).astype(np.float32)
    body[:, 3] = rng.integers(0, 16, 600)
    clouds = [(boundary_points(), np.concatenate([boundary_points(), body]))]
    q, t = np.array([[0.0, 0.0, 0.0, 1.0]]), np.zeros((1, 3))
    vf = lambda p, leaf: O.voxel_filter(p, leaf, canonical=True)
    tiles, points = atlas.tiles_from_keyframes(q, t, clouds, LEAF, vf)
    held = atlas.Atlas(tiles, points)
    seen = set()
    for axis in range(3):
        for v in BOUNDARY:
            for x in (np.nextafter(v, -1e9), v, np.nextafter(v, 1e9)):
                pos = np.zeros(3)
                pos[axis] = x
                cen = atlas.window_centre(pos)
                st = {}
                cut = atlas.window_from_keyframes(q, t, clouds, LEAF, vf, cen, st)
                want = held.cut(cen)
                for cls in (0, 1):
                    assert sorted(cut[cls]) == sorted(want[cls])
                    for k in cut[cls]:
                        assert np.array_equal(cut[cls][k].view(np.uint32), want[cls][k].view(np.uint32))
                        ijk = np.array(atlas.ijk_of(k)) - np.array(cen)
                        assert (atlas.cube_coord(cut[cls][k][:, :3]) == ijk).all()
                assert st["cubes"] == [len(c) for c in want] and st["window_points"] == [sum(len(p) for p in c.values()) for c in want]
                assert st["outside_window"] == len(points) - sum(st["window_points"])
                seen.add(cen)
    assert len(seen) >= 7                                                                       # the centre moved with the sensor's cube
    far = atlas.window_from_keyframes(q, t, clouds, LEAF, vf, (10 - 40, 10, 5), st := {})
    assert not far[0] and not far[1] and st["outside_window"] == len(points)
