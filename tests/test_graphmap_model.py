"""The model of the map assembled from keyframe clouds at a graph's poses (atlas.tiles_from_keyframes, what aloam_graph_export_map
computes): the cube arithmetic at its boundaries, the member order of a cube, the filter of every cube, and that the result is an atlas."""
import importlib

import numpy as np
import pytest

LEAF = (0.4, 0.8)
ID = (np.array([[0.0, 0.0, 0.0, 1.0]]), np.zeros((1, 3)))


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


def _cloud(rng, n, half):
    p = rng.uniform(-half, half, (n, 4)).astype(np.float32)
    p[:, 3] = rng.integers(0, 16, n)
    return p


def test_one_keyframe_at_the_identity_is_the_oracle_filter_of_each_cube(O, atlas):
    rng = np.random.default_rng(2)
    corner, surf = _cloud(rng, 400, 60.0), _cloud(rng, 3000, 90.0)
    st = {}
    tiles, points = atlas.tiles_from_keyframes(*ID, [(corner, surf)], LEAF, lambda p, leaf: O.voxel_filter(p, leaf, canonical=True), st)
    assert tiles["feature_class"].tolist() == sorted(tiles["feature_class"].tolist()) and set(tiles["feature_class"].tolist()) == {0, 1}
    assert tiles["first_point"].tolist() == np.concatenate([[0], np.cumsum(tiles["count"])[:-1]]).tolist() and int(tiles["count"].sum()) == len(points)
    assert not tiles["frame"].any()
    for cls, cl in enumerate((corner, surf)):
        cube = np.floor((cl[:, :3].astype(np.float64) + 25.0) / 50.0).astype(np.int64)       # the plain definition: floor, for every sign
        mine = tiles[tiles["feature_class"] == cls]
        keys = [tuple(int(v) for v in t["cube"]) for t in mine]
        assert keys == sorted(set(map(tuple, cube.tolist()))) and len(keys) > 8               # ascending in (cube[0], cube[1], cube[2]), each once
        for t, key in zip(mine, keys):
            want = O.voxel_filter(cl[np.all(cube == np.array(key), 1)], LEAF[cls], canonical=True)   # input order inside the cube
            got = points[int(t["first_point"]):int(t["first_point"]) + int(t["count"])]
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cls, key)
    assert st["raw_points"] == [len(corner), len(surf)] and st["outside"] == 0 and st["tiles"] == [int((tiles["feature_class"] == c).sum()) for c in (0, 1)]


def test_boundary_coordinates_land_in_the_cubes_of_cube_coord(atlas):
    f32 = np.float32
    below, above = (lambda v: np.nextafter(f32(v), f32(-1e9))), (lambda v: np.nextafter(f32(v), f32(1e9)))
    cases = [(below(-75), -2), (f32(-75), -2), (above(-75), -1), (below(-25), -1), (f32(-25), 0), (above(-25), 0),
             (below(25), 0), (f32(25), 1), (above(25), 1)]
    assert atlas.cube_coord(np.array([v for v, _ in cases], f32)).tolist() == [c for _, c in cases]
    for v, c in cases:                                     # int((v + 25) / 50), minus one when v + 25 < 0, in f64
        s = float(v) + 25.0
        assert int(s / 50.0) - (1 if s < 0 else 0) == c, v
    for axis in range(3):
        pts = np.zeros((len(cases), 4), f32)
        pts[:, axis] = [v for v, _ in cases]
        pts[:, (axis + 1) % 3] = 3.0 * np.arange(len(cases))                                 # apart: no two share a voxel
        tiles, points = atlas.tiles_from_keyframes(*ID, [(pts, pts[:0])], LEAF, lambda p, leaf: p)
        got = {int(t["cube"][axis]): points[int(t["first_point"]):int(t["first_point"]) + int(t["count"])][:, axis].tolist() for t in tiles}
        for c in (-2, -1, 0, 1):
            assert got[c] == [float(v) for v, cc in cases if cc == c], (axis, c)


def test_members_of_a_cube_are_concatenated_in_node_order_before_the_filter(O, atlas):
    # Three points of one 0.4 m cell whose f32 sum depends on the order (a sum of two does not: f32 addition commutes).  Keyframe 0 brings
    # two of them, keyframe 1 the third.
    rng = np.random.default_rng(0)
    for _ in range(1000):
        x = (10.0 + rng.uniform(0.01, 0.39, 3)).astype(np.float32)
        if np.float32(np.float32(x[0] + x[1]) + x[2]) != np.float32(np.float32(x[2] + x[0]) + x[1]):
            break
    else:
        pytest.fail("no order-dependent triple found")
    a = np.array([[x[0], 1.0, 1.0, 0.0], [x[1], 1.0, 1.0, 0.0]], np.float32)
    b = np.array([[x[2], 1.0, 1.0, 0.0]], np.float32)
    none = np.zeros((0, 4), np.float32)
    q, t = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)), np.zeros((2, 3))
    seen = []

    def vf(p, leaf):
        seen.append(np.array(p))
        return O.voxel_filter(p, leaf, canonical=True)
    t_ab, p_ab = atlas.tiles_from_keyframes(q, t, [(a, none), (b, none)], LEAF, vf)
    t_ba, p_ba = atlas.tiles_from_keyframes(q, t, [(b, none), (a, none)], LEAF, vf)
    assert np.array_equal(seen[0], np.concatenate([a, b])) and np.array_equal(seen[1], np.concatenate([b, a]))
    assert len(t_ab) == len(t_ba) == 1 and len(p_ab) == len(p_ba) == 1 and t_ab.tobytes() == t_ba.tobytes()
    assert p_ab[0, 0] != p_ba[0, 0]                         # the same three points, another sum


def test_poses_are_applied_in_the_device_operation_order(atlas):
    """associate_to_map restates quat_rotate + translation: against a rotation matrix within f32 rounding, and exactly for exact inputs."""
    rng = np.random.default_rng(5)
    p = _cloud(rng, 200, 40.0)
    q = np.array([0.6, 0.0, 0.0, 0.8])                      # 2 atan(0.75) about x
    w = atlas.associate_to_map(p, q, (1.5, -2.0, 0.25))
    R = np.array([[1, 0, 0], [0, 0.28, -0.96], [0, 0.96, 0.28]])
    assert np.allclose(w[:, :3], p[:, :3].astype(np.float64) @ R.T + np.array([1.5, -2.0, 0.25]), atol=1e-5) and np.array_equal(w[:, 3], p[:, 3])
    assert np.array_equal(atlas.associate_to_map(p, (0, 0, 0, 1), (0, 0, 0)), p)
    far = atlas.tiles_from_keyframes(np.array([[0, 0, 0, 1.0]]), np.array([[30000.0, 0, 0]]), [(p, p[:5])], LEAF, lambda x, leaf: x, st := {})
    assert len(far[0]) == 0 and st["outside"] == 205


def test_the_output_is_an_atlas_that_holds_every_key_once(O, atlas):
    rng = np.random.default_rng(8)
    q = np.array([[0, 0, 0, 1.0], [0, 0, 0.6, 0.8]])
    t = np.array([[0.0, 0, 0], [20.0, -30.0, 5.0]])
    clouds = [(_cloud(rng, 200, 50.0), _cloud(rng, 900, 70.0)) for _ in range(2)]
    tiles, points = atlas.tiles_from_keyframes(q, t, clouds, LEAF, lambda p, leaf: O.voxel_filter(p, leaf, canonical=True))
    held = atlas.Atlas(tiles, points)
    keys = [(tuple(int(v) for v in tl["cube"]), int(tl["feature_class"])) for tl in tiles]
    assert len(set(keys)) == len(keys) == sum(n for n, _ in held.counts())
    assert [n for _, n in held.counts()] == [int(tiles["count"][tiles["feature_class"] == c].sum()) for c in (0, 1)]
    for tl in tiles:                                        # unchanged by the atlas: one tile per key, nothing concatenated
        got = held.cubes[int(tl["feature_class"])][tuple(int(v) for v in tl["cube"])]
        assert np.array_equal(got, points[int(tl["first_point"]):int(tl["first_point"]) + int(tl["count"])])
