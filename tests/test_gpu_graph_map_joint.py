"""The map of joined sequences on the MI355X (aloam_graph_export_map_joint): tiles from the keyframes of several sequences, every
(cube, class) filtered once over all of its members.  The reference side is atlas.tiles_from_parts fed the stacks (read back with
aloam_get_map_cloud) and the nodes (read back with aloam_graph_export) plus the oracle's input-order voxel filter; every comparison of
tiles, points, offsets and stats is bit for bit.

The world is built as tests/test_gpu_graph_map.py builds its own: aloam_set_last + aloam_mapping_step on hand-made clouds, solver off."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_atlas import same_tiles
from test_gpu_graph_map import LEAF, POSES_1, Q_ID, Q_X, Q_Z, _getters, boundary_points, cloud, context, step

pytestmark = pytest.mark.gpu
A_FRAME = Q_Z + (40.0, -30.0, 10.0)                       # a non-trivial frame: q_A exactly unit
B_FRAME = Q_X + (-15.0, 70.0, 0.0)
GUARD = 0x5A


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


@pytest.fixture(scope="module")
def world(binding):
    """Three sequences, none of which a test below changes.  Sequence 0: one keyframe with an empty corner stack (its surf range is shorter
    than one piece of 4096 points).  Sequence 1: the seven rotated keyframes of POSES_1 over cubes -3 .. 3, with the boundary coordinates
    in keyframe 2.  Sequence 2: eighteen keyframes of about 4 k surf points in cube (0, 0, 0) and two neighbours - its surf range spans many
    pieces, with nodes straddling piece borders.  All three reach cube (0, 0, 0)."""
    rng = np.random.default_rng(41)
    gpu = context(binding)
    stacks = [[], [], []]
    for k in range(18):
        s0 = (np.zeros((0, 4), np.float32), cloud(rng, 300, (20, 20, 2)), Q_ID, (1.0, 2.0, 0.5))
        q1, t1 = POSES_1[min(k, 6)]
        c1, f1 = cloud(rng, 300, (30, 30, 10)), cloud(rng, 1500, (40, 40, 20))
        if k == 2:
            c1, f1 = np.concatenate([boundary_points(), c1]), np.concatenate([boundary_points(), f1])
        f2 = np.concatenate([cloud(rng, 3750, (24, 24, 24)), cloud(rng, 250, (20, 20, 20), (50, 0, 0)), cloud(rng, 50, (20, 20, 20), (0, 50, 0))])
        f2[:, 3] = np.sort(f2[:, 3])
        s2 = (cloud(rng, 1000, (24, 24, 24)), f2, Q_ID, (0.01 * k, -0.01 * k, 0.0))
        add = [2] + ([1] if k < 7 else []) + ([0] if k == 0 else [])
        got = step(gpu, binding, [s0, (c1, f1, q1, t1), s2], add)
        for b in add:
            stacks[b].append(got[b])
    nodes = [gpu.graph_export(b) for b in range(3)]
    assert [len(n) for n in nodes] == [1, 7, 18] and len(stacks[0][0][0]) == 0 and 0 < len(stacks[0][0][1]) < 4096
    edges = np.cumsum([len(s[1]) for s in stacks[2]])
    assert edges[-1] > 16 * 4096 and np.count_nonzero(edges[:-1] % 4096) >= 16   # many pieces; nodes straddle their borders
    yield {"gpu": gpu, "stacks": stacks, "nodes": nodes}
    gpu.close()


def parts_model(atlas, O, src, parts, frames=None, optimized=False, stats=None):
    """atlas.tiles_from_parts of parts = [(seq, first, count, frame), ...] read from src = {"nodes": ..., "stacks": ...}."""
    mp = []
    for seq, first, count, frame in parts:
        nd = src["nodes"][seq][first:first + count]
        mp.append((nd["q_opt"] if optimized else nd["q"], nd["t_opt"] if optimized else nd["t"], src["stacks"][seq][first:first + count], frame))
    return atlas.tiles_from_parts(mp, LEAF, lambda p, leaf: O.voxel_filter(p, leaf, canonical=True), frames, stats)


def piece(res, i):
    """Group (or request) i of a result, its first_point counted from its own first point."""
    tiles, points, off, _ = res
    t = tiles[off[0, i]:off[0, i + 1]].copy()
    t["first_point"] -= off[1, i]
    return t, points[off[1, i]:off[1, i + 1]]


def same_result(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def check_stats(s, st, outside=0, written=1):
    assert s["tiles"].tolist() == st["tiles"] and s["points"].tolist() == st["points"] and s["raw_points"].tolist() == st["raw_points"]
    assert s["outside"] == outside == st["outside"] and s["written"] == written


ALL = [(0, 0, 1, -1), (1, 0, 7, -1), (2, 0, 18, -1)]


def test_three_sequences_in_one_group_equal_the_model_and_are_not_three_maps(O, binding, atlas, world):
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    st = {}
    wt, wp = parts_model(atlas, O, world, ALL, stats=st)
    res = gpu.graph_export_map_joint([(ALL, E)])
    tiles, points, off, stats = res
    assert off.tolist() == [[0, len(wt)], [0, len(wp)]]
    assert same_tiles((tiles, points), (wt, wp)), (len(tiles), len(wt), len(points), len(wp))
    check_stats(stats[0], st)
    singles = [gpu.graph_export_map([(s, f, n, E)]) for s, f, n, _ in ALL]
    assert stats[0]["raw_points"].tolist() == np.sum([s[3][0]["raw_points"] for s in singles], 0).tolist()   # every member went in
    # cube (0, 0, 0), surf: members of all three sequences, filtered once - not the three per-sequence tiles laid end to end
    def centre(tl, pts):
        t = [x for x in tl if x["feature_class"] == 1 and tuple(x["cube"]) == (0, 0, 0)]
        assert len(t) == 1
        return pts[t[0]["first_point"]:t[0]["first_point"] + t[0]["count"]]
    joined, apart = centre(tiles, points), [centre(s[0], s[1]) for s in singles]
    assert all(len(a) > 0 for a in apart) and 0 < len(joined) < sum(len(a) for a in apart)
    assert joined.tobytes() != np.concatenate(apart).tobytes()
    assert len(tiles) < sum(len(s[0]) for s in singles)                                                        # one tile per key


def test_the_order_of_parts_is_honoured(O, binding, atlas, world):
    gpu = world["gpu"]
    st = {}
    want = parts_model(atlas, O, world, ALL[::-1], stats=st)
    tiles, points, off, stats = gpu.graph_export_map_joint([(ALL[::-1], binding.GRAPH_POSE_ENTERED)])
    assert same_tiles((tiles, points), want), (len(tiles), len(want[0]), len(points), len(want[1]))
    check_stats(stats[0], st)


def test_empty_pieces_in_all_three_forms(O, binding, atlas, world):
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    between = [(1, 0, 7, -1), (2, 5, 0, -1), (0, 0, 1, -1), (2, 3, 2, -1)]     # a count = 0 part between others; sequence 0 has no corner point
    alone = [(0, 0, 1, -1)]                                                     # the corner-less part as a group's only part
    res = gpu.graph_export_map_joint([(between, E), (alone, E), ([], E), ([(2, 0, 0, -1)], E)])
    for i, parts in enumerate((between, alone)):
        st = {}
        want = parts_model(atlas, O, world, parts, stats=st)
        assert same_tiles(piece(res, i), want), i
        check_stats(res[3][i], st)
    assert res[3][1]["tiles"][0] == 0 and res[3][1]["tiles"][1] > 0 and not (piece(res, 1)[0]["feature_class"] == 0).any()   # zero corner tiles
    for i in (2, 3):                                                            # no parts at all; one empty part
        s = res[3][i]
        assert len(piece(res, i)[0]) == 0 and not (s["tiles"].any() or s["points"].any() or s["raw_points"].any() or s["outside"]) and s["written"] == 1


def test_both_identities_hold_byte_for_byte(binding, world):
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    for seq, first, count in ((0, 0, 1), (1, 0, 7), (1, 2, 3), (2, 0, 18), (2, 4, 9), (2, 5, 0)):
        assert same_result(gpu.graph_export_map_joint([([(seq, first, count, -1)], E)]), gpu.graph_export_map([(seq, first, count, E)])), (seq, first, count)
    whole = gpu.graph_export_map_joint([([(2, 0, 18, -1)], E)])
    assert same_result(gpu.graph_export_map_joint([([(2, 0, 5, -1), (2, 5, 13, -1)], E)]), whole)
    assert same_result(gpu.graph_export_map_joint([([(2, 0, 1, -1), (2, 1, 16, -1), (2, 17, 1, -1)], E)]), whole)
    many = gpu.graph_export_map_joint([([(1, 0, 7, -1)], E), ([(0, 0, 1, -1)], E), ([(2, 4, 9, -1)], E)])       # a list of groups against a list of requests
    assert same_result(many, gpu.graph_export_map([(1, 0, 7, E), (0, 0, 1, E), (2, 4, 9, E)]))


def test_frames(O, binding, atlas, world):
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    frames = np.array([A_FRAME, B_FRAME], np.float64)
    cases = [[(1, 0, 7, 0), (2, 0, 18, -1)],                                   # a moved session beside one that stays
             [(1, 0, 3, 1), (0, 0, 1, -1), (1, 3, 4, 1)],                       # two parts share one frame index
             [(1, 0, 7, 0), (1, 0, 7, 1), (1, 0, 7, -1)]]                       # the same sequence under two frames, and as stored
    res = gpu.graph_export_map_joint([(p, E) for p in cases], frames=frames)
    for i, parts in enumerate(cases):
        st = {}
        want = parts_model(atlas, O, world, parts, frames, stats=st)
        assert same_tiles(piece(res, i), want), i
        check_stats(res[3][i], st)
    moved = piece(res, 0)
    assert not same_tiles(moved, parts_model(atlas, O, world, [(1, 0, 7, -1), (2, 0, 18, -1)]))
    # the identity frame is arithmetic all the same, and here it changes no bit: q = 1 q, t = t + 0
    ident = gpu.graph_export_map_joint([([(1, 0, 7, 0)], E)], frames=[(0, 0, 0, 1.0, 0, 0, 0)])
    assert same_tiles(ident[:2], parts_model(atlas, O, world, [(1, 0, 7, 0)], [(0, 0, 0, 1.0, 0, 0, 0)]))


def test_optimised_poses_after_a_real_join(O, binding, atlas):
    """Two sessions of four keyframes, the second entered in a frame of its own; one link, a joint solve with align.  The export at the
    optimised poses is the model fed the nodes read back after the solve, and differs from the export at the entered poses."""
    pg = importlib.import_module("a-loam_amd.posegraph")
    rng = np.random.default_rng(47)
    gpu = context(binding, batch=2, nodes=8, edges=16, keyframes=(4096, 16384))
    stacks = [[], []]
    for k in range(4):
        a = (cloud(rng, 200, (30, 30, 10)), cloud(rng, 1200, (40, 40, 20)), Q_ID, (12.0 * k, 0.5 * k, 0.0))
        b = (cloud(rng, 200, (30, 30, 10)), cloud(rng, 1200, (40, 40, 20)), Q_Z, (100.0 + 3.0 * k, -40.0 + 11.0 * k, 5.0))
        got = step(gpu, binding, [a, b], [0, 1])
        for s in (0, 1):
            stacks[s].append(got[s])
    before = [gpu.graph_export(b) for b in (0, 1)]
    link = np.zeros(1, binding.GRAPH_LINK_DTYPE)
    link["seq_i"], link["i"], link["seq_j"], link["j"] = 0, 1, 1, 2
    link["q"], link["t"] = Q_X, (4.0, -2.0, 0.5)
    link["info"] = (np.eye(6) * 100.0)[np.triu_indices(6)]
    res = gpu.graph_optimize_joint([([0, 1], link, [0, 1])])
    assert res[0]["status"] != binding.GRAPH_NO_EDGES                          # (the members' rows are written back whatever else the status is)
    after = [gpu.graph_export(b) for b in (0, 1)]
    assert np.array_equal(after[1]["t"], before[1]["t"]) and abs(after[1]["t_opt"] - before[1]["t_opt"]).max() > 10.0   # aligned into the group's frame
    src = {"nodes": after, "stacks": stacks}
    parts = [(0, 0, 4, -1), (1, 0, 4, -1)]
    st = {}
    want = parts_model(atlas, O, src, parts, optimized=True, stats=st)
    tiles, points, off, stats = gpu.graph_export_map_joint([(parts, binding.GRAPH_POSE_OPTIMIZED)])
    assert same_tiles((tiles, points), want), (len(tiles), len(want[0]))
    check_stats(stats[0], st)
    entered = gpu.graph_export_map_joint([(parts, binding.GRAPH_POSE_ENTERED)])
    assert same_tiles(entered[:2], parts_model(atlas, O, src, parts)) and not same_tiles(entered[:2], (tiles, points))
    # the unaligned session placed by a frame from the same link gives the map the alignment gives, up to what the solve moved: same cubes
    A = pg.frame_from_link(before[0]["q_opt"][1], before[0]["t_opt"][1], link[0], before[1]["q_opt"][2], before[1]["t_opt"][2])
    framed = gpu.graph_export_map_joint([([(0, 0, 4, -1), (1, 0, 4, 0)], binding.GRAPH_POSE_ENTERED)], frames=[np.concatenate(A)])
    assert same_tiles(framed[:2], parts_model(atlas, O, src, [(0, 0, 4, -1), (1, 0, 4, 0)], [np.concatenate(A)]))
    gpu.close()


def test_a_groups_bytes_do_not_depend_on_the_list(O, binding, atlas, world):
    """(The directory hint grown by an earlier call: test_a_directory_that_proves_too_small_doubles, in a context of its own.)"""
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    frames = [A_FRAME]
    G = [(2, 3, 6, -1), (1, 0, 7, 0), (0, 0, 1, -1)]
    others = [([(1, 0, 7, -1)], E), ([(2, 0, 18, -1), (0, 0, 1, 0)], E), ([(0, 0, 1, -1)], E)]
    st = {}
    want = parts_model(atlas, O, world, G, frames, stats=st)
    alone = gpu.graph_export_map_joint([(G, E)], frames=frames)
    assert same_tiles(piece(alone, 0), want)
    for at in (0, 1, 3):                                                        # first, middle and last of four
        groups = others[:at] + [(G, E)] + others[at:]
        res = gpu.graph_export_map_joint(groups, frames=frames)
        assert same_tiles(piece(res, at), want), at
        assert res[3][at].tobytes() == alone[3][0].tobytes(), at
        assert res[0]["first_point"].tolist() == np.concatenate([[0], np.cumsum(res[0]["count"])[:-1]]).tolist()
    twice = gpu.graph_export_map_joint([(G, E), others[0], (G, E)], frames=frames)
    assert same_tiles(piece(twice, 0), want) and same_tiles(piece(twice, 2), want) and twice[3][0].tobytes() == twice[3][2].tobytes()


def _into(gpu, binding, groups, cap_t, cap_p, room_t, room_p, frames=None):
    """The call into guarded device destinations: (tile bytes, points, offsets with four guard words, stats)."""
    import torch
    n = len(groups)
    tiles = torch.full(((room_t + 4) * 32,), GUARD, dtype=torch.uint8, device="cuda")
    pts = torch.full(((room_p + 64) * 4,), 12345.0, dtype=torch.float32, device="cuda")
    off = torch.full((2 * (n + 1) + 4,), -7, dtype=torch.int64).pin_memory()
    stats = torch.full(((n + 1) * 32,), GUARD, dtype=torch.uint8).pin_memory()
    gpu.graph_export_map_joint_into(groups, tiles.data_ptr(), cap_t, pts.data_ptr(), cap_p, off.data_ptr(), stats.data_ptr(), frames=frames)
    gpu.synchronize()
    assert off[2 * (n + 1):].tolist() == [-7] * 4 and (stats.numpy()[n * 32:] == GUARD).all()
    return tiles.cpu().numpy(), pts.cpu().numpy().reshape(-1, 4), off.numpy()[:2 * (n + 1)].reshape(2, n + 1).copy(), stats.numpy()[:n * 32].view(binding.GRAPH_MAP_STATS_DTYPE).copy()


def test_size_query_and_caps(O, binding, atlas, world):
    import torch
    gpu, E = world["gpu"], binding.GRAPH_POSE_ENTERED
    parts = [[(0, 0, 1, -1), (2, 1, 1, -1)], [(1, 0, 7, -1), (0, 0, 1, -1)], [(2, 2, 3, -1), (1, 4, 2, -1)]]
    groups = [(p, E) for p in parts]
    wants = [parts_model(atlas, O, world, p) for p in parts]
    nt, npts = [len(w[0]) for w in wants], [len(w[1]) for w in wants]
    to, po = np.concatenate([[0], np.cumsum(nt)]), np.concatenate([[0], np.cumsum(npts)])
    off = torch.full((2 * 4 + 4,), -7, dtype=torch.int64).pin_memory()
    gpu.graph_export_map_joint_into(groups, 0, 0, 0, 0, off.data_ptr())        # the size query writes offsets and nothing else
    gpu.synchronize()
    assert off[:4].tolist() == to.tolist() and off[4:8].tolist() == po.tolist() and off[8:].tolist() == [-7] * 4
    # caps of the first group alone; caps one point, then one tile, short of the whole list; caps of the whole list
    for cap_t, cap_p, written in ((nt[0], npts[0], [1, 0, 0]), (sum(nt), sum(npts) - 1, [1, 1, 0]), (sum(nt) - 1, sum(npts), [1, 1, 0]), (sum(nt), sum(npts), [1, 1, 1])):
        th, ph, o, st = _into(gpu, binding, groups, cap_t, cap_p, sum(nt), sum(npts))
        assert o.tolist() == [to.tolist(), po.tolist()] and st["written"].tolist() == written, (cap_t, cap_p)
        for i in range(3):
            t, p = th[to[i] * 32:to[i + 1] * 32], ph[po[i]:po[i + 1]]
            if written[i]:
                tt = t.view(binding.MAP_TILE_DTYPE).copy()
                tt["first_point"] -= po[i]
                assert same_tiles((tt, p), wants[i]), (cap_t, cap_p, i)
            else:
                assert (t == GUARD).all() and (p == 12345.0).all(), (cap_t, cap_p, i)
        assert (th[min(cap_t, sum(nt)) * 32:] == GUARD).all() and (ph[min(cap_p, sum(npts)):] == 12345.0).all()   # nothing lies past the caps
    # two small groups in front of a large one that does not fit
    parts = [[(0, 0, 1, -1)], [(2, 2, 1, -1), (0, 0, 1, -1)], [(1, 0, 7, -1), (2, 0, 18, -1)]]
    wants = [parts_model(atlas, O, world, p) for p in parts[:2]]
    nt, npts = [len(w[0]) for w in wants], [len(w[1]) for w in wants]
    th, ph, o, st = _into(gpu, binding, [(p, E) for p in parts], sum(nt) + 1, sum(npts) + 5, sum(nt) + 600, sum(npts) + 60000)
    assert st["written"].tolist() == [1, 1, 0] and o[0, :3].tolist() == [0, nt[0], sum(nt)] and o[0, 3] > sum(nt) + 1 and o[1, 3] > sum(npts) + 5
    assert (th[sum(nt) * 32:] == GUARD).all() and (ph[sum(npts):] == 12345.0).all()
    t1 = th[nt[0] * 32:sum(nt) * 32].view(binding.MAP_TILE_DTYPE).copy()
    t1["first_point"] -= npts[0]
    assert same_tiles((t1, ph[npts[0]:sum(npts)]), wants[1])


def test_points_outside_the_atlas_range_are_counted_per_group_and_left_out(O, binding, atlas):
    rng = np.random.default_rng(3)
    gpu = context(binding, batch=2, nodes=4, edges=4, keyframes=(4096, 8192))
    near = [(cloud(rng, 100, (10, 10, 2)), cloud(rng, 400, (15, 15, 3)), Q_ID, (5.0, 0.0, 0.0)), (cloud(rng, 90, (10, 10, 2)), cloud(rng, 300, (15, 15, 3)), Q_ID, (-5.0, 1.0, 0.0))]
    far = [(cloud(rng, 120, (10, 10, 2)), cloud(rng, 500, (15, 15, 3)), Q_ID, (30000.0, 0.0, 0.0)), near[1]]
    s0, s1 = step(gpu, binding, near, [0, 1]), step(gpu, binding, far, [0])
    src = {"nodes": [gpu.graph_export(b) for b in (0, 1)], "stacks": [[s0[0], s1[0]], [s0[1]]]}
    assert src["nodes"][0]["t"][1][0] == 30000.0
    groups = [[(1, 0, 1, -1), (0, 0, 2, -1)], [(1, 0, 1, -1), (0, 0, 1, -1)], [(0, 1, 1, -1)], [(1, 0, 1, 0)]]
    frames = [(0, 0, 0, 1.0, 0.0, -30000.0, 0.0)]                             # a frame can carry a part out of range too
    res = gpu.graph_export_map_joint([(p, 0) for p in groups], frames=frames)
    n_far = len(s1[0][0]) + len(s1[0][1])
    for i, (p, outside) in enumerate(zip(groups, (n_far, 0, n_far, len(s0[1][0]) + len(s0[1][1])))):
        st = {}
        want = parts_model(atlas, O, src, p, frames, stats=st)
        assert same_tiles(piece(res, i), want), i
        check_stats(res[3][i], st, outside=outside)
    assert same_tiles(piece(res, 0), piece(res, 1)) and len(piece(res, 2)[0]) == 0 and len(piece(res, 3)[0]) == 0
    gpu.close()


def test_a_directory_that_proves_too_small_doubles(O, binding, atlas):
    """Two sequences, one keyframe each of 4096 surf points with every point in a cube of its own (a 64 x 64 grid of cubes, the second
    shifted by half a grid): about 8200 (cube, piece) pairs, against a directory that starts at 4096 slots.  The transform runs again with
    the directory doubled, twice; the map is the model's, and the bytes are the same from the call that starts at the size it grew to."""
    gx, gy = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32))
    surf = np.zeros((4096, 4), np.float32)
    surf[:, 0], surf[:, 1], surf[:, 2] = 50.0 * gx.ravel() + 3.0, 50.0 * gy.ravel() - 4.0, 1.0
    surf[:, 3] = np.arange(4096) // 256
    rng = np.random.default_rng(6)
    gpu = context(binding, batch=2, nodes=4, edges=4, keyframes=(4096, 8192))
    gpu.profile_enable(True)
    got = step(gpu, binding, [(cloud(rng, 100, (10, 10, 2)), surf, Q_ID, (0.0, 0.0, 0.0)), (cloud(rng, 100, (10, 10, 2)), surf, Q_ID, (1600.0, 1.0, 0.0))], [0, 1])
    src = {"nodes": [gpu.graph_export(b) for b in (0, 1)], "stacks": [[got[0]], [got[1]]]}
    parts = [(1, 0, 1, -1), (0, 0, 1, -1)]
    st = {}
    wt, wp = parts_model(atlas, O, src, parts, stats=st)
    assert st["tiles"][1] == 4096 + 2048 and st["outside"] == 0               # the two grids overlap in half of their cubes
    base = gpu.profile()["graph_map"]["launches"]
    import torch
    off = torch.zeros(4, dtype=torch.int64).pin_memory()
    tl = torch.zeros(len(wt) * 32, dtype=torch.uint8).pin_memory()
    pt = torch.zeros((len(wp), 4), dtype=torch.float32).pin_memory()
    gpu.graph_export_map_joint_into([(parts, 0)], tl.data_ptr(), len(wt), pt.data_ptr(), len(wp), off.data_ptr())
    gpu.synchronize()
    assert off.tolist() == [0, len(wt), 0, len(wp)]
    assert same_tiles((tl.numpy().view(binding.MAP_TILE_DTYPE), pt.numpy()), (wt, wp))
    assert gpu.profile()["graph_map"]["launches"] == base + 3 + 1             # three transform passes and the rest
    first = (tl.numpy().copy(), pt.numpy().copy())
    gpu.graph_export_map_joint_into([(parts, 0)], tl.data_ptr(), len(wt), pt.data_ptr(), len(wp), off.data_ptr())   # the size is remembered
    gpu.synchronize()
    assert gpu.profile()["graph_map"]["launches"] == base + 3 + 1 + 2
    assert first[0].tobytes() == tl.numpy().tobytes() and first[1].tobytes() == pt.numpy().tobytes()                 # and the bytes do not depend on it
    gpu.close()


def test_joined_tiles_load_as_an_atlas_and_serve_a_window(O, binding, atlas):
    """The joined map of two sessions, exported into device memory, is loaded with aloam_atlas_load from there; a third, frozen sequence
    attached to it gets its window: the atlas cut at the window's centre, one cube per key."""
    import torch
    rng = np.random.default_rng(12)
    gpu = context(binding, batch=3, nodes=4, edges=4, keyframes=(4096, 8192))
    stacks = [[], []]
    for k in range(2):
        ins = [(cloud(rng, 150, (30, 30, 5)), cloud(rng, 900, (45, 45, 8)), Q_ID, (20.0 * k, 0.0, 0.0)), (cloud(rng, 150, (30, 30, 5)), cloud(rng, 900, (45, 45, 8)), Q_Z, (30.0, 25.0 * k, 0.0)),
               (cloud(rng, 50, (5, 5, 1)), cloud(rng, 200, (8, 8, 2)), Q_ID, (0.0, 0.0, 0.0))]
        got = step(gpu, binding, ins, [0, 1])
        stacks[0].append(got[0]); stacks[1].append(got[1])
    src = {"nodes": [gpu.graph_export(b) for b in (0, 1)], "stacks": stacks}
    parts = [(0, 0, 2, -1), (1, 0, 2, -1)]
    st = {}
    wt, wp = parts_model(atlas, O, src, parts, stats=st)
    tiles = torch.zeros(len(wt) * 32, dtype=torch.uint8, device="cuda")
    pts = torch.zeros((len(wp), 4), dtype=torch.float32, device="cuda")
    off = torch.zeros(4, dtype=torch.int64).pin_memory()
    gpu.graph_export_map_joint_into([(parts, binding.GRAPH_POSE_ENTERED)], tiles.data_ptr(), len(wt), pts.data_ptr(), len(wp), off.data_ptr())
    gpu.atlas_load(tiles, pts)                                                # synchronises; straight from device memory
    info = gpu.atlas_info()
    assert info["tiles"] == len(wt) and info["cubes"] == st["tiles"] and info["points"] == st["points"]
    held = atlas.Atlas(wt, wp)
    assert [c for c, _ in held.counts()] == st["tiles"]                       # one tile per key: nothing for the loader to merge
    gpu.reset_sequences([2])
    gpu.set_active([0, 0, 1])
    gpu.set_map_frozen([0, 0, 1])
    gpu.atlas_attach([0, 0, 1])
    step(gpu, binding, ins, [])
    m = gpu.map_info(2)
    want = held.cut((m["cenW"], m["cenH"], m["cenD"]))
    for cls in (0, 1):
        got = gpu.map_cubes(cls, 2)
        assert len(want[cls]) > 1 and set(got) == set(want[cls]), cls
        assert all(np.array_equal(got[i].view(np.uint32), want[cls][i].view(np.uint32)) for i in want[cls]), cls
    gpu.atlas_attach(None)
    gpu.close()


def test_refusals_leave_everything_as_it_was(binding, world):
    import torch
    gpu, E, L = world["gpu"], binding.GRAPH_POSE_ENTERED, binding.lib()
    good = [([(0, 0, 1, -1), (1, 0, 7, 0)], E), ([(2, 4, 9, -1)], E)]
    frames = np.array([A_FRAME], np.float64)
    before = gpu.graph_export_map_joint(good, frames=frames)
    held = [gpu.graph_keyframe_info(b) for b in range(3)]
    off = torch.full((16,), -7, dtype=torch.int64).pin_memory()
    tiles = torch.full((64 * 32,), GUARD, dtype=torch.uint8).pin_memory()
    pts = torch.full((4096, 4), 12345.0, dtype=torch.float32).pin_memory()
    stats = torch.full((8 * 32,), GUARD, dtype=torch.uint8).pin_memory()
    pageable = np.zeros(64, np.int64)

    def refused(code, word, f):
        with pytest.raises(binding.AloamError) as e:
            f()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))

    def call(groups, fr=frames, t=None, ct=64, p=None, cp=4096, o=None, s=None):
        gpu.graph_export_map_joint_into(groups, tiles.data_ptr() if t is None else t, ct, pts.data_ptr() if p is None else p, cp,
                                        off.data_ptr() if o is None else o, stats.data_ptr() if s is None else s, frames=fr)
    for word, bad in (("part 1: seq", (3, 0, 1, -1)), ("part 1: seq", (-1, 0, 1, -1)), ("part 1: [first", (1, -1, 2, -1)), ("part 1: [first", (1, 0, -1, -1)),
                      ("part 1: [first", (1, 5, 3, -1)), ("part 1: [first", (0, 0, 2, -1)), ("part 1: frame", (1, 0, 7, 1)), ("part 1: frame", (1, 0, 7, -2))):
        refused(binding.E_ARG, word, lambda: call([([(0, 0, 1, -1), bad], E)]))
    refused(binding.E_ARG, "part 0: frame", lambda: call([([(1, 0, 7, 0)], E)], fr=None))                                 # an index without frames
    for word, fr in (("frames[1]: q", [A_FRAME, (0, 0, 0, 1.001, 0, 0, 0)]), ("frames[0]: q", [(np.nan, 0, 0, 1.0, 0, 0, 0)]), ("frames[0]: t", [(0, 0, 0, 1.0, 0, np.inf, 0)])):
        refused(binding.E_ARG, word, lambda: call(good, fr=np.array(fr, np.float64)))
    for pose in (2, -1):
        refused(binding.E_ARG, "group 1: pose", lambda: call([good[0], (good[1][0], pose)]))
    pr, gr = binding.Aloam.graph_map_groups(good)
    for word, change in (("group 1: pad", (1, "pad", 1)), ("group 1: part_first", (1, "part_first", 1)), ("group 0: part_first", (0, "part_first", 1)),
                         ("group 1: part_count", (1, "part_count", -1)), ("group 1: part_first + part_count", (1, "part_count", 2)), ("n_parts", (1, "part_count", 0))):
        g2 = gr.copy()
        g2[change[1]][change[0]] = change[2]
        refused(binding.E_ARG, word, lambda: call((pr, g2)))
    big = np.zeros(32769, binding.GRAPH_MAP_GROUP_DTYPE)
    refused(binding.E_ARG, "n_groups", lambda: call((pr[:0], big)))
    # NULL lists and negative counts: the C call itself
    ptr = lambda a: a.ctypes.data
    dst = (tiles.data_ptr(), 64, pts.data_ptr(), 4096, off.data_ptr(), stats.data_ptr())
    for word, args in (("parts", (None, 3, ptr(frames), 1, ptr(gr), 2)), ("groups", (ptr(pr), 3, ptr(frames), 1, None, 2)), ("frames", (ptr(pr), 3, None, 1, ptr(gr), 2)),
                       ("n_parts", (ptr(pr), -1, ptr(frames), 1, ptr(gr), 2)), ("n_groups", (ptr(pr), 3, ptr(frames), 1, ptr(gr), -1)), ("n_frames", (ptr(pr), 3, ptr(frames), -1, ptr(gr), 2))):
        assert L.aloam_graph_export_map_joint(gpu.h, *args, *dst) == binding.E_ARG and word in L.aloam_last_error(gpu.h).decode(), word
    # the destinations, as for the exports
    refused(binding.E_ARG, "dst_offsets", lambda: call(good, o=0))
    refused(binding.E_ARG, "dst_offsets", lambda: call(good, o=pageable.ctypes.data))
    refused(binding.E_ARG, "tiles_dst", lambda: call(good, t=0))                                                          # NULL with a cap
    refused(binding.E_ARG, "cap", lambda: call(good, ct=-1))
    refused(binding.E_ARG, "cap", lambda: call(good, cp=-1))
    refused(binding.E_ARG, "points_dst", lambda: call(good, p=pts.data_ptr() + 4))
    refused(binding.E_ARG, "stats_dst", lambda: call(good, s=pageable.ctypes.data))
    # a (group, class) bounded by more pieces than the directory key numbers: refused before anything is queued, the group named
    refused(binding.E_CAPACITY, "group 1", lambda: call([good[0], ([(2, 0, 18, -1)] * 3700, E)]))
    gpu.synchronize()
    assert off.tolist() == [-7] * 16 and (tiles.numpy() == GUARD).all() and (pts.numpy() == 12345.0).all() and (stats.numpy() == GUARD).all()
    assert [gpu.graph_keyframe_info(b) for b in range(3)] == held
    assert same_result(gpu.graph_export_map_joint(good, frames=frames), before)
    off2 = torch.full((4,), -7, dtype=torch.int64).pin_memory()
    assert L.aloam_graph_export_map_joint(gpu.h, None, 0, None, 0, None, 0, None, 0, None, 0, C.c_void_p(off2.data_ptr()), None) == 0   # n_groups = 0 is ALOAM_OK
    gpu.synchronize()
    assert off2.tolist() == [0, 0, -7, -7]                                    # with the offsets written
    g = binding.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=4096, lm_max_iterations=0)
    g.mapping_enable(0.4, 0.8, pool_points=1 << 16)
    g.graph_enable(8, 8)
    with pytest.raises(binding.AloamError) as e:
        g.graph_export_map_joint_into([], 0, 0, 0, 0, off2.data_ptr())
    assert e.value.code == binding.E_STATE and "aloam_graph_keyframes_enable" in str(e.value)
    g.close()


def test_opt_in_changes_nothing_else(binding):
    """Twins through the same calls, one of which also makes the new call: the same bits from every getter; aloam_graph_export_map shows
    the same launch count in every profiling slot; the new call adds launches to graph_map only."""
    runs = []
    for joint in (False, True):
        rng = np.random.default_rng(77)
        gpu = context(binding, batch=2, nodes=8, edges=8, keyframes=(4096, 8192))
        gpu.profile_enable(True)
        for k in range(3):
            inputs = [(cloud(rng, 80, (10, 10, 2)), cloud(rng, 600, (15, 15, 3)), Q_Z if k == 1 else Q_ID, (3.0 * k, 0.5 * b, 0.0)) for b in range(2)]
            step(gpu, binding, inputs, [0, 1] if k != 1 else [1])
        gpu.graph_optimize([0, 1])
        p0 = gpu.profile()
        if joint:
            both = gpu.graph_export_map_joint([([(0, 0, 2, -1), (1, 0, 3, 0)], binding.GRAPH_POSE_OPTIMIZED)], frames=[A_FRAME])
            assert len(both[0]) > 0
        p1 = gpu.profile()
        per_request = gpu.graph_export_map([(0, 0, 2, 1), (1, 0, 3, 0)])
        p2 = gpu.profile()
        step(gpu, binding, inputs, [1])
        runs.append((_getters(gpu, binding, 2), [r.tobytes() for r in per_request], p0, p1, p2))
        gpu.close()
    (g0, m0, a0, a1, a2), (g1, m1, b0, b1, b2) = runs
    assert g0 == g1 and m0 == m1
    launches = lambda p: {k: v["launches"] for k, v in p.items()}
    assert launches(a0) == launches(a1) == launches(b0)
    added = {k: launches(b1)[k] - launches(b0)[k] for k in b0}
    assert added.pop("graph_map") == 2 * 2 and not any(added.values())          # (size query + export) x (the transform, the rest)
    assert {k: launches(a2)[k] - launches(a1)[k] for k in a1} == {k: launches(b2)[k] - launches(b1)[k] for k in b1}
