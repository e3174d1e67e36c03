"""What every cloud of tests/voxel_cases.py proves about itself, on the CPU: that it has the property it was built for (the kernels' own conditions
restated in numpy: runs, voxels, members, key_bits, cell_exact, the list vox_enlist picks, whether the instance keeps the segment), and that the
reference gives ONE answer on it - the oracle's filter in canonical order, the plain definition of the cases module and, where the cloud fits an LDS
instance, the lane-by-lane model of k_vox_lds agree bit for bit.  The GPU comparison (tests/test_gpu_voxel_edges.py) counts only as far as these hold."""
import numpy as np
import pytest

import voxel_cases as V
from conftest import bits_equal
from test_mapping_models import vox_lds_model

CASES = [(name, leaf) for name in V.ALL for leaf in V.LEAVES]


@pytest.mark.parametrize("name,leaf", CASES)
def test_case_has_its_property_and_the_reference_gives_one_answer(O, name, leaf):
    c = V.check(V.case(name, leaf))
    assert c.points.dtype == np.float32 and c.points.shape == (c.props["n"], 4)
    assert c.props["n"] < 3 or np.any(c.points[:, 3] != np.floor(c.points[:, 3])), "intensities carry a fraction"
    want = O.voxel_filter(c.points, leaf, canonical=True)
    assert len(want) == c.props["voxels"], (name, leaf, len(want), c.props["voxels"])
    assert bits_equal(V.plain_filter(c.points, leaf), want), (name, leaf)
    if c.props["kept"]:
        assert bits_equal(vox_lds_model(c.points, leaf, V.INSTANCES[c.props["cls"]][0]), want), (name, leaf)


@pytest.mark.parametrize("leaf", V.LEAVES)
def test_what_the_groups_of_cases_are_there_for(leaf):
    P = lambda name: V.case(name, leaf).props
    # 1. every list of vox_enlist at both of its ends, the general path one past the last; ring-like: short runs, voxels revisited
    assert [P(n)["cls"] for n in V.LIMITS] == ["tiny"] * 6 + ["small"] * 3 + ["big"] * 3 + ["general"]
    assert all(P(n)["kept"] for n in V.LIMITS[:-1]) and not P(V.LIMITS[-1])["kept"]
    assert all(P(n)["max_run"] <= 5 and P(n)["voxels"] < P(n)["runs"] for n in V.LIMITS[4:])
    assert any(P(n)["n"] % 64 for n in V.LIMITS)                                       # a partial last row of continuation bits
    # 2. run boundaries on, before and behind the first point of every wave but the first
    for cls in ("small", "big"):
        n, nw = V.INSTANCES[cls][2], V.INSTANCES[cls][0] // 64
        chunk = V.chunk_of(n, cls)
        assert chunk * nw == n
        for d in (0, -1, 1):
            p = P(f"runlen-{cls}@{d}")
            assert p["n"] == n and p["max_run"] == chunk + d and p["cls"] == cls
    assert P("interleave5000")["max_members"] == 5000 and P("interleave5000")["max_run"] == 1 and P("interleave5000")["voxels"] == 4
    assert all(P(f"onecell-{n}")["max_members"] == n > 8 * 64 for n in (2048, 8192, 65536))   # beyond the 8-wide batched load, beyond one wave
    # 3. the run capacity of the big instance, and one more
    assert P("capr-24576")["runs"] == V.INSTANCES["big"][1] and P("capr-24576")["kept"]
    assert P("capr-24577")["runs"] == V.INSTANCES["big"][1] + 1 and not P("capr-24577")["kept"] and P("capr-24577")["cls"] == "big"
    # 4. every number of radix passes (7 bits each), on both sides of each step, in every instance
    bits = {P(n)["key_bits"] for n in V.KEYBITS if P(n)["kept"]}
    assert {1, 7, 8, 14, 15, 21, 22, 28, 29} <= bits
    for cls in ("tiny", "small", "big"):
        assert {(P(n)["key_bits"] + 6) // 7 for n in V.KEYBITS + V.ARITH if P(n)["kept"] and P(n)["cls"] == cls} >= ({1, 2, 3, 4, 5} if cls == "tiny" else {3, 4})
    for n in V.KEYBITS[:-1]:
        assert P(n)["index_min"] == 0 and P(n)["index_max"] == P(n)["cells"] - 1
    assert {sum(d > 1 for d in P(n)["divb"]) for n in V.KEYBITS} == {1, 2, 3}
    # 5. div_b one more than PCL's dx; the guard at its edge; the index past 2^31
    assert P("minfrac09")["cells"] == 41 * 31 * 6 > P("minfrac09")["guard_cells"]
    assert P("guard-in")["guard_cells"] <= V.MAX_CELLS < P("guard-out")["guard_cells"] and not P("guard-in")["unfiltered"] and P("guard-out")["unfiltered"]
    for n in ("wrap-3d", "wrap-2d"):
        assert P(n)["guard_cells"] <= V.MAX_CELLS < P(n)["cells"] < 2 ** 32 and P(n)["index_max"] >= 2 ** 31 and not P(n)["unfiltered"]
    # 6. the general path: every merge depth up to three tiles and beyond, a last tile of one key, a voxel across one and across two tile edges
    far = [P(f"far-{n}") for n in V.FAR_SIZES]
    assert [p["tiles"] for p in far] == [1, 1, 1, 2, 2, 3, 3, 4] and [p["merge_levels"] for p in far] == [0, 0, 0, 1, 1, 2, 2, 2]
    assert [p["last_tile"] for p in far] == [1, 2047, 2048, 1, 2048, 1, 2048, 1]
    assert not any(p["cell_exact"] or p["kept"] or p["unfiltered"] for p in far)
    assert P("far-v2500")["voxel_tiles"] == 2 and P("far-v5000")["voxel_tiles"] == 3
    assert P("far-65537")["last_tile"] == 1 and P("far-65537")["index_max"] > 2 ** 23
    for n in V.GENERAL:
        assert not P(n)["kept"]
    for a in V.ARITH:                                                                   # the same box and the same cells as the cloud the LDS instance takes
        assert P(f"general-{a}")["divb"] == P(a)["divb"] and P(f"general-{a}")["unfiltered"] == P(a)["unfiltered"] and P(a)["kept"]


def _centre_cube(cubes):
    assert len(cubes) == 1, sorted(cubes)
    return next(iter(cubes.values()))


@pytest.mark.parametrize("total", V.CUBE_TOTALS)
def test_cube_segment_holds_the_stated_points_before_its_refilter(O, total):
    """The two frames of cube_frames(): after frame 1 the centre cube holds total // 2 points, frame 2's incoming filter passes the rest, every one a voxel
    of its own - so the cube's segment is `total` points when its in-place filter starts - and the cube afterwards is the plain definition of the two
    joined, half of frame 2 merged into occupied voxels."""
    for cls, leaf in enumerate(V.LEAVES):
        f1, f2 = V.cube_frames(total, leaf)
        orc = O.Oracle(16, 0.3, lm_max_iterations=0)
        orc.map_config(*V.LEAVES)
        clouds = lambda f: (f, f[:0]) if cls == 0 else (f[:0], f)
        orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], *clouds(f1), f1[:4])
        cube1 = _centre_cube(orc.map_cubes(cls))
        assert len(f1) == total // 2 and len(cube1) == len(f1)
        orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], *clouds(f2), f2[:4])
        stack2 = orc.map_cloud(O.MAP_SURF_STACK if cls else O.MAP_CORNER_STACK)
        assert len(stack2) == len(f2) == total - total // 2 and V.route(len(cube1) + len(stack2)) == V.route(total)
        cube2 = _centre_cube(orc.map_cubes(cls))
        assert len(cube2) == total - len(f2) // 2
        assert bits_equal(cube2, V.plain_filter(np.concatenate([cube1, stack2]), leaf)), (total, leaf)


@pytest.mark.parametrize("leaf", [V.LEAVES[1], 1e-5])
def test_sheet_frames_put_every_cube_on_the_small_list(O, leaf):
    """sheet_frames(): 25 cubes whose segments hold 2100 / 7000 points before the re-filter of frame 1 and 3100 / 8000 before that of frame 2 - all on
    the small list, long beside short - with merges in frame 2; at a leaf of 1e-5 m the 16 outer cubes hold cells beyond 2^23 (handed back) and
    the 9 inner ones do not (kept)."""
    f1, f2 = V.sheet_frames(leaf)
    orc = O.Oracle(16, 0.3, lm_max_iterations=0)
    orc.map_config(leaf, leaf)
    before = []
    for f in (f1, f2):
        held = {c: len(v) for c, v in orc.map_cubes(1).items()}
        orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], f[:0], f, f[:4])
        stack = orc.map_cloud(O.MAP_SURF_STACK)
        assert len(stack) == len(f)                                                     # the incoming filter merges nothing: what a cube gets is what the frame holds for it
        add = np.bincount(V.sheet_cube_of(stack), minlength=25)
        assert len(add) == 25 and (not held or set(add) == {1000})                      # frame 2 gives every cube the same number, so sizes add up cube by cube
        before.append(sorted(add) if not held else sorted(n + 1000 for n in held.values()))
    after = sorted(len(v) for v in orc.map_cubes(1).values())
    assert before[0] == [2100] * 13 + [7000] * 12 and before[1] == [3100] * 13 + [8000] * 12
    assert all(V.route(n) == "small" for n in before[0] + before[1])
    assert len(after) == 25 and all(a < b for a, b in zip(after, before[1]))            # every cube's second re-filter merges
    exact = [bool(np.all(np.abs(V.cells_of(f1[V.sheet_cube_of(f1) == c], leaf)) < V.EXACT_LIMIT)) for c in range(25)]
    assert exact.count(True) == (25 if leaf > 0.1 else 9)
    assert not V.properties(f1, leaf)["unfiltered"] or V.properties(f1, leaf)["guard_cells"] < 2 ** 63


def test_cube_beyond_the_guard_is_left_as_it_is(O):
    frames = V.unfiltered_cube_frames()
    assert all(V.properties(f, 0.03)["unfiltered"] for f in frames) and V.properties(np.concatenate(frames), 0.03)["unfiltered"]
    for canonical in (True, False):
        orc = O.Oracle(16, 0.3, lm_max_iterations=0, canonical_order=canonical)
        orc.map_config(0.03, 0.03)
        for k, f in enumerate(frames):
            orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], f, f, f[:4])
            for cls in (0, 1):
                assert bits_equal(_centre_cube(orc.map_cubes(cls)), np.concatenate(frames[: k + 1])), (canonical, k, cls)


def test_boxes_whose_cell_index_wraps_have_one_answer(O):
    """The suspect input of the cases module's docstring: three implementations, one result.  The oracle's filter against the plain definition is part
    of the per-case test above; here the mapping node compiled from the reference's own source (with the stand-in VoxelGrid it is built against) filters
    the same clouds, and its cubes equal the oracle's in the reference's order bit for bit.  The 3-D box is centred, so every voxel of it lands in the
    window and the cubes together hold exactly the incoming filter's centroids."""
    import ref_py
    if not ref_py.available():
        pytest.skip("oracle/_ref not built")
    corner, surf = V.case("wrap-3d", 0.4).points, V.case("wrap-2d", 0.4).points
    ref = ref_py.laser_mapping([dict(q_w=[0, 0, 0, 1.0], t_w=[0, 0, 0.0], corner_last=corner, surf_last=surf, cloud=surf[:4])], 0.4, 0.4)[0]
    orc = O.Oracle(16, 0.3, lm_max_iterations=0, canonical_order=False)
    orc.map_config(0.4, 0.4)
    orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], corner, surf, surf[:4])
    for cls, name in enumerate(("corner_map", "surf_map")):
        got = orc.map_cubes(cls)
        assert sorted(got) == sorted(ref[name]) and len(got) > 0
        for cube in got:
            assert bits_equal(got[cube], ref[name][cube]), (name, cube)
    stack = O.voxel_filter(corner, 0.4, canonical=False)
    held = np.concatenate(list(orc.map_cubes(0).values()))
    assert len(held) == len(stack) == V.case("wrap-3d", 0.4).props["voxels"]
    assert np.array_equal(np.sort(held.view(np.uint32).reshape(-1, 4), axis=0), np.sort(stack.view(np.uint32).reshape(-1, 4), axis=0))
