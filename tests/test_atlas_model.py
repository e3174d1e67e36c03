"""The window arithmetic behind the map spill, on the host (no GPU): (a) k_map_begin's literal shift loop - descriptors moved axis by axis,
shift by shift, the slab that falls off re-entering empty - replayed in numpy against the closed form the spill kernel uses, "a cube
survives iff every shifted index is in range"; (b) a-loam_amd/atlas.py: tiles of a window, cut again at another centre, are the same cubes."""
import importlib

import numpy as np
import pytest

atlas = importlib.import_module("a-loam_amd.atlas")
W, H, D = atlas.DIMS


def replay_shift_loop(table, center):
    """reference src/laserMapping.cpp:323-507 as k_map_begin runs it: table[i, j, k] = id of the cube held there (0 = empty).  Returns the
    table afterwards and the shift made."""
    T, c, s = table.copy(), list(center), [0, 0, 0]
    for axis, n in enumerate(atlas.DIMS):
        for _ in range(64):                                               # the guard of k_map_begin
            d = 1 if c[axis] < 3 else (-1 if c[axis] >= n - 3 else 0)
            if d == 0:
                break
            T = np.roll(T, d, axis=axis)                                  # every line moves by one ...
            edge = [slice(None)] * 3
            edge[axis] = 0 if d > 0 else n - 1
            T[tuple(edge)] = 0                                            # ... and the slab that fell off re-enters emptied
            c[axis] += d
            s[axis] += d
    return T, tuple(s)


def random_case(rng):
    table = np.zeros(atlas.DIMS, np.int64)
    n = int(rng.integers(0, 400))
    idx = rng.choice(atlas.N_CUBES, n, replace=False)
    table[np.unravel_index(idx, atlas.DIMS, order="F")] = idx + 1        # id = window index + 1 (index = i + 21 j + 441 k)
    center = tuple(int(rng.integers(-70, 91)) for _ in range(3))          # past the loop's guard of 64 shifts
    return table, center


def test_the_closed_form_equals_the_shift_loop():
    rng = np.random.default_rng(2024)
    beyond_guard = 0
    for _ in range(400):
        table, center = random_case(rng)
        after, s = replay_shift_loop(table, center)
        assert s == atlas.shift_of(center)
        beyond_guard += any(abs(d) == 64 for d in s)
        survivors = {int(v) - 1 for v in after.reshape(-1) if v}
        held = {int(v) - 1 for v in table.reshape(-1) if v}
        assert survivors == {i for i in held if atlas.survives(i, s)}
        for i in survivors:                                               # ... and each sits at its shifted index
            x, y, z = (a + d for a, d in zip(atlas.ijk_of(i), s))
            assert after[x, y, z] == i + 1
    assert beyond_guard > 0


def test_the_fallen_cubes_are_the_model_spill():
    rng = np.random.default_rng(7)
    for _ in range(100):
        table, center = random_case(rng)
        cen = tuple(int(v) for v in rng.integers(-5, 30, 3))
        after, s = replay_shift_loop(table, center)
        cubes = [{}, {}]
        for v in table.reshape(-1):
            if v:
                cubes[int(v) % 2][int(v) - 1] = np.full((int(v) % 17 + 1, 4), float(v), np.float32)
        tiles, points = atlas.spill_of(cubes, cen, s, frame=9)
        fell = sorted((int(v) % 2, int(v) - 1) for v in table.reshape(-1) if v and not (after == v).any())
        assert [(int(t["feature_class"]), atlas.index_of(*(int(a) + c for a, c in zip(t["cube"], cen)))) for t in tiles] == fell   # class rows, ascending index
        assert [int(t["count"]) for t in tiles] == [(i + 1) % 17 + 1 for _, i in fell] and all(int(t["frame"]) == 9 for t in tiles)
        assert tiles["first_point"].tolist() == np.concatenate([[0], np.cumsum(tiles["count"])[:-1]]).astype(np.int64).tolist()
        for t in tiles:
            p = points[int(t["first_point"]):int(t["first_point"]) + int(t["count"])]
            assert (p == float(atlas.index_of(*(int(a) + c for a, c in zip(t["cube"], cen))) + 1)).all()


def test_a_full_spill_drops_whole_tiles_and_keeps_later_ones():
    cubes = [{20: np.zeros((5, 4), np.float32), 41: np.zeros((300, 4), np.float32), 62: np.zeros((7, 4), np.float32)}, {}]
    dropped = []
    tiles, points = atlas.spill_of(cubes, (10, 10, 5), (1, 0, 0), room=[(16, 100), (16, 100)], dropped=dropped)
    assert tiles["count"].tolist() == [5, 7] and tiles["first_point"].tolist() == [0, 5] and dropped == [1, 300] and len(points) == 12
    tiles, _ = atlas.spill_of(cubes, (10, 10, 5), (1, 0, 0), room=[(1, 1000), (1, 1000)], dropped=dropped)
    assert tiles["count"].tolist() == [5] and dropped == [2, 307]


def random_map(rng, n_cubes, spread):
    keys = {tuple(int(v) for v in rng.integers(-spread, spread + 1, 3)) for _ in range(n_cubes)}
    return [{k: rng.normal(size=(int(rng.integers(1, 9)), 4)).astype(np.float32) for k in keys if rng.random() < 0.7} for _ in (0, 1)]


def as_tiles(world, order=None):
    tiles, pts, first = [], [], 0
    for cls in (0, 1):
        for key in (order or sorted)(world[cls]):
            t = np.zeros((), atlas.TILE_DTYPE)
            t["cube"], t["feature_class"], t["count"], t["first_point"] = key, cls, len(world[cls][key]), first
            tiles.append(t)
            pts.append(world[cls][key])
            first += len(world[cls][key])
    return np.array(tiles, atlas.TILE_DTYPE), np.concatenate(pts)


def test_window_tiles_cut_at_another_centre_are_the_same_cubes(tmp_path):
    rng = np.random.default_rng(3)
    world = random_map(rng, 300, 14)
    cen_a, cen_b = (10, 10, 5), (13, 4, 6)
    window = atlas.Atlas(*as_tiles(world)).cut(cen_a)                    # what a context would hold around cen_a
    tiles, points = atlas.tiles_of_window(window, cen_a, frame=3)
    atlas.save_atlas(tmp_path / "a.npz", tiles, points)
    tiles, points = atlas.load_atlas(tmp_path / "a.npz")
    again = atlas.Atlas(tiles, points).cut(cen_b)
    for cls in (0, 1):
        want = {}
        for key, p in world[cls].items():
            a = [k + c for k, c in zip(key, cen_a)]
            b = [k + c for k, c in zip(key, cen_b)]
            if all(0 <= x < n for x, n in zip(a, atlas.DIMS)) and all(0 <= x < n for x, n in zip(b, atlas.DIMS)):
                want[atlas.index_of(*b)] = p
        assert len(want) > 0 and set(again[cls]) == set(want)
        assert all(np.array_equal(again[cls][i].view(np.uint32), want[i].view(np.uint32)) for i in want)


def test_duplicate_tiles_concatenate_in_order():
    rng = np.random.default_rng(4)
    a, b, c = (rng.normal(size=(n, 4)).astype(np.float32) for n in (3, 5, 2))
    log = atlas.TileLog()
    for p, frame in ((a, 1), (b, 2)):
        log.add(*atlas.tiles_of_window([{100: p}, {}], (10, 10, 5), frame))
    log.add(np.zeros(0, atlas.TILE_DTYPE), np.zeros((0, 4), np.float32))     # an empty drain
    tiles, points = log.result(atlas.tiles_of_window([{100 + 21: c}, {100 + 21: c}], (10, 11, 5), 3))   # the same absolute cube seen from a shifted window
    assert tiles["first_point"].tolist() == [0, 3, 8, 10] and tiles["frame"].tolist() == [1, 2, 3, 3]
    at = atlas.Atlas(tiles, points)
    key = tuple(x - c for x, c in zip(atlas.ijk_of(100), (10, 10, 5)))
    assert np.array_equal(at.cubes[0][key], np.concatenate([a, b, c])) and np.array_equal(at.cubes[1][key], c)
    assert at.counts() == [(1, 10), (1, 2)]
    with pytest.raises(ValueError):
        atlas.Atlas(tiles, points[:-1])


def test_largest_window_equals_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(12):
        world = random_map(rng, int(rng.integers(1, 120)), int(rng.integers(1, 30)))
        at = atlas.Atlas(*as_tiles(world))
        for cls in (0, 1):
            keys = np.array(list(world[cls]), np.int64).reshape(-1, 3)
            n = np.array([len(world[cls][tuple(k)]) for k in keys], np.int64)
            best = 0
            if len(keys):
                lo, hi = keys.min(0), keys.max(0)
                for x in range(lo[0] - W + 1, hi[0] + 1):
                    for y in range(lo[1] - H + 1, hi[1] + 1):
                        inside_xy = (keys[:, 0] >= x) & (keys[:, 0] < x + W) & (keys[:, 1] >= y) & (keys[:, 1] < y + H)
                        if not inside_xy.any():
                            continue
                        for z in range(lo[2] - D + 1, hi[2] + 1):
                            best = max(best, int(n[inside_xy & (keys[:, 2] >= z) & (keys[:, 2] < z + D)].sum()))
            assert at.largest_window(cls) == best, (trial, cls)
