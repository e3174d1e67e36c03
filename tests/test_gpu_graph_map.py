"""Keyframe clouds of the pose graphs and the map rebuilt at the graph's poses on the MI355X (aloam_graph_keyframes_enable,
aloam_graph_export_keyframes, aloam_graph_export_map): the store holds each node's stacks bit for bit; the exported tiles are those of
atlas.tiles_from_keyframes fed the same stacks (read back with aloam_get_map_cloud), the same poses (read back with aloam_graph_export)
and the oracle's input-order voxel filter; every comparison of tiles and points is bit for bit.

The stacks are fed with aloam_set_last + aloam_mapping_step on hand-made clouds, solver off (lm_max_iterations = 0): the pose of a node is
the odometry pose handed in."""
import importlib

import numpy as np
import pytest

from test_gpu_atlas import same_tiles

pytestmark = pytest.mark.gpu
LEAF = (0.4, 0.8)
INFO = np.eye(6) * 100.0
KF_CORNER, KF_SURF = 1 << 15, 1 << 17
Q_ID, Q_Z, Q_X = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.6, 0.8), (0.6, 0.0, 0.0, 0.8)      # exactly unit quaternions
# sequence 1: seven keyframes over cubes -3 .. 3 on every axis
POSES_1 = [(Q_Z, (-130.0, -60.0, -120.0)), (Q_ID, (-60.0, 110.0, 0.0)), (Q_ID, (0.0, 0.0, 0.0)), (Q_X, (60.0, -110.0, 120.0)),
           (Q_Z, (130.0, 60.0, 0.0)), (Q_ID, (10.0, 10.0, -60.0)), (Q_X, (-75.0, 25.0, -25.0))]
BOUNDARY = (-75.0, -25.0, 25.0)


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


def context(binding, batch=3, nodes=32, edges=64, keyframes=(KF_CORNER, KF_SURF)):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 16)
    gpu.graph_enable(nodes, edges)
    if keyframes:
        gpu.graph_keyframes_enable(*keyframes)
    return gpu


def cloud(rng, n, half, centre=(0.0, 0.0, 0.0)):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = (np.asarray(centre) + rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half)).astype(np.float32)
    p[:, 3] = np.sort(rng.integers(0, 16, n))
    return p


def boundary_points():
    """World coordinates -75, -25, 25 and one ulp either side on each axis in turn, each point alone in its voxel."""
    out = []
    for axis in range(3):
        for i, v in enumerate(BOUNDARY):
            for j, x in enumerate((np.nextafter(np.float32(v), np.float32(-1e9)), np.float32(v), np.nextafter(np.float32(v), np.float32(1e9)))):
                p = np.full(4, 0.0, np.float32)
                p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = x, 3.0 + 4.0 * i, 5.0 + 4.0 * j
                out.append(p)
    return np.array(out, np.float32)


def step(gpu, binding, inputs, add):
    """One mapping step of every sequence - inputs[b] = (corner, surf, q, t) - then a node for the sequences in `add`.  Returns the stacks
    of every sequence as the device holds them."""
    for b, (corner, surf, q, t) in enumerate(inputs):
        gpu.set_last(corner, surf, b)
        gpu.set_full_cloud(surf[:4], b)
        gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(q, np.float64), np.array(t, np.float64), b)
    gpu.mapping_step()
    if add:
        gpu.graph_add_nodes(add, INFO)
    gpu.synchronize()
    return [(gpu.map_cloud(binding.MAP_CORNER_STACK, b), gpu.map_cloud(binding.MAP_SURF_STACK, b)) for b in range(len(inputs))]


@pytest.fixture(scope="module")
def world(binding):
    """Shared by the tests below, none of which changes it (no edge is added, nothing is solved or cleared).
    Sequence 0: one keyframe with an empty corner stack.  Sequence 1: the seven keyframes of POSES_1, rotated, over many cubes, with the
    boundary coordinates in keyframe 2.  Sequence 2: eighteen keyframes in the same few cubes, sized for every path of the voxel filter."""
    rng = np.random.default_rng(41)
    gpu = context(binding)
    stacks = [[], [], []]
    for k in range(18):
        s0 = (np.zeros((0, 4), np.float32), cloud(rng, 300, (20, 20, 2)), Q_ID, (1.0, 2.0, 0.5))
        q1, t1 = POSES_1[min(k, 6)]
        c1, f1 = cloud(rng, 300, (30, 30, 10)), cloud(rng, 1500, (40, 40, 20))
        if k == 2:
            c1, f1 = np.concatenate([boundary_points(), c1]), np.concatenate([boundary_points(), f1])
        # sequence 2: surf 3750 points in cube (0, 0, 0), 250 in (1, 0, 0), 50 in (0, 1, 0); corner 1000 in cube (0, 0, 0)
        f2 = np.concatenate([cloud(rng, 3750, (24, 24, 24)), cloud(rng, 250, (20, 20, 20), (50, 0, 0)), cloud(rng, 50, (20, 20, 20), (0, 50, 0))])
        f2[:, 3] = np.sort(f2[:, 3])
        s2 = (cloud(rng, 1000, (24, 24, 24)), f2, Q_ID, (0.01 * k, -0.01 * k, 0.0))
        add = [2] + ([1] if k < 7 else []) + ([0] if k == 0 else [])
        got = step(gpu, binding, [s0, (c1, f1, q1, t1), s2], add)
        for b in add:
            stacks[b].append(got[b])
    nodes = [gpu.graph_export(b) for b in range(3)]
    yield {"gpu": gpu, "stacks": stacks, "nodes": nodes}
    gpu.close()


def model(atlas, O, nodes, stacks, first=0, count=None, optimized=False, stats=None, sizes=None):
    count = len(nodes) - first if count is None else count
    nd = nodes[first:first + count]

    def vf(p, leaf):
        if sizes is not None:
            sizes.append(len(p))
        return O.voxel_filter(p, leaf, canonical=True)
    return atlas.tiles_from_keyframes(nd["q_opt"] if optimized else nd["q"], nd["t_opt"] if optimized else nd["t"], stacks[first:first + count], LEAF, vf, stats)


_MODEL = {}


def want(atlas, O, world, seq, first=0, count=None):
    """The model's map of nodes [first, first + count) of a sequence at the entered poses; computed once."""
    key = (seq, first, count)
    if key not in _MODEL:
        st, sizes = {}, []
        _MODEL[key] = (model(atlas, O, world["nodes"][seq], world["stacks"][seq], first, count, stats=st, sizes=sizes), st, sizes)
    return _MODEL[key]


def test_capture_keeps_each_nodes_stacks(binding, world):
    gpu = world["gpu"]
    assert [gpu.graph_info(b)["nodes"] for b in range(3)] == [1, 7, 18]        # a sequence listed in only some calls has only those nodes
    for b in range(3):
        for cls in (0, 1):
            pts, off = gpu.graph_export_keyframes(b, feature_class=cls)
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(s[cls]) for s in world["stacks"][b]])]).tolist(), (b, cls)
            assert np.array_equal(pts.view(np.uint32), np.concatenate([s[cls] for s in world["stacks"][b]]).view(np.uint32)), (b, cls)
    assert len(world["stacks"][0][0][0]) == 0 and len(world["stacks"][0][0][1]) > 0      # an empty corner stack is stored with count 0
    pts, off = gpu.graph_export_keyframes(1, first=2, count=3, feature_class=1, pinned=False)   # a partial range, into device memory
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(s[1]) for s in world["stacks"][1][2:5]])]).tolist()
    assert np.array_equal(pts.view(np.uint32), np.concatenate([s[1] for s in world["stacks"][1][2:5]]).view(np.uint32))
    pts, off = gpu.graph_export_keyframes(2, first=5, count=0)
    assert off.tolist() == [0] and len(pts) == 0
    info = gpu.graph_keyframe_info(2)
    assert info["points"] == [sum(len(s[c]) for s in world["stacks"][2]) for c in (0, 1)] and info["capacity"] == [KF_CORNER, KF_SURF]
    assert info["dropped_nodes"] == 0 and info["dropped_points"] == 0


def test_map_at_the_entered_poses_equals_the_model(O, binding, atlas, world):
    gpu = world["gpu"]
    (wt, wp), st, _ = want(atlas, O, world, 1)
    lo, hi = wt["cube"].min(0), wt["cube"].max(0)
    assert (lo <= -3).all() and (hi >= 3).all(), (lo, hi)                     # at least three cubes per axis sign
    kf = world["stacks"][1][2]
    for cls in (0, 1):                                                        # the boundary coordinates reached the stacks as they were
        for axis in range(3):
            for v in BOUNDARY:
                for x in (np.nextafter(np.float32(v), np.float32(-1e9)), np.float32(v), np.nextafter(np.float32(v), np.float32(1e9))):
                    assert np.any(kf[cls][:, axis] == x), (cls, axis, x)
    tiles, points, off, stats = gpu.graph_export_map([(1, 0, 7, binding.GRAPH_POSE_ENTERED)])
    assert off.tolist() == [[0, len(wt)], [0, len(wp)]]
    assert same_tiles((tiles, points), (wt, wp)), (len(tiles), len(wt), len(points), len(wp))
    s = stats[0]
    assert s["tiles"].tolist() == st["tiles"] and s["points"].tolist() == st["points"] and s["raw_points"].tolist() == st["raw_points"]
    assert s["outside"] == 0 and s["written"] == 1


def test_map_at_the_optimised_poses_equals_the_model_and_differs(O, binding, atlas):
    """A context of its own (the shared one is never solved): the seven poses of sequence 1 again, two anchor edges, a solve."""
    pg = importlib.import_module("a-loam_amd.posegraph")
    rng = np.random.default_rng(43)
    gpu = context(binding, batch=1, nodes=8, edges=16, keyframes=(4096, 16384))
    stacks = [step(gpu, binding, [(cloud(rng, 300, (30, 30, 10)), cloud(rng, 1500, (40, 40, 20)), q, t)], [0])[0] for q, t in POSES_1]
    n = gpu.graph_export(0)
    # two anchors that disagree with the entered poses by a few decimetres
    edges = np.zeros(2, binding.GRAPH_EDGE_DTYPE)
    for e, (j, dt) in zip(edges, ((3, (0.4, -0.3, 0.2)), (6, (-0.5, 0.6, -0.1)))):
        e["seq"], e["i"], e["j"], e["flags"] = 0, -1, j, 0
        e["q"], e["t"] = n["q"][j], n["t"][j] + np.array(dt)
        e["info"] = (np.eye(6) * 400.0)[np.triu_indices(6)]
    assert pg.EDGE_DTYPE == binding.GRAPH_EDGE_DTYPE
    gpu.graph_add_edges(edges)
    res = gpu.graph_optimize([0])
    assert res[0]["status"] == binding.GRAPH_OK and res[0]["final_cost"] < res[0]["initial_cost"]
    nodes = gpu.graph_export(0)
    assert np.array_equal(nodes["q"], n["q"]) and np.array_equal(nodes["t"], n["t"]) and not np.array_equal(nodes["t_opt"], n["t"])
    wt, wp = model(atlas, O, nodes, stacks, optimized=True)
    tiles, points, off, stats = gpu.graph_export_map([(0, 0, 7, binding.GRAPH_POSE_OPTIMIZED)])
    assert same_tiles((tiles, points), (wt, wp)), (len(tiles), len(wt), len(points), len(wp))
    entered = gpu.graph_export_map([(0, 0, 7, binding.GRAPH_POSE_ENTERED)])
    assert same_tiles(entered[:2], model(atlas, O, nodes, stacks)) and not same_tiles(entered[:2], (tiles, points))
    gpu.close()


def test_a_directory_that_proves_too_small_grows(O, binding, atlas):
    """Two keyframes of 4096 surf points, every point in a cube of its own (a 64 x 64 grid of cubes): about 8200 (cube, piece) pairs in four
    pieces, against a directory that starts at 4096 slots.  The transform is run again with the directory doubled, twice, and the map is the
    model's; the profiling slot counts the three transform passes and the rest (1 + 1 + 3 + 1: two captures, this export)."""
    gx, gy = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32))
    surf = np.zeros((4096, 4), np.float32)
    surf[:, 0], surf[:, 1], surf[:, 2] = 50.0 * gx.ravel() + 3.0, 50.0 * gy.ravel() - 4.0, 1.0
    surf[:, 3] = np.arange(4096) // 256
    rng = np.random.default_rng(6)
    gpu = context(binding, batch=1, nodes=4, edges=4, keyframes=(4096, 8192))
    gpu.profile_enable(True)
    stacks = [step(gpu, binding, [(cloud(rng, 100, (10, 10, 2)), surf, Q_ID, t)], [0])[0] for t in ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0))]
    assert [len(s[1]) for s in stacks] == [4096, 4096]
    st = {}
    wt, wp = model(atlas, O, gpu.graph_export(0), stacks, stats=st)
    assert st["tiles"][1] == 4096 and st["outside"] == 0
    import torch
    off = torch.zeros(4, dtype=torch.int64).pin_memory()
    tl = torch.zeros(len(wt) * 32, dtype=torch.uint8).pin_memory()
    pt = torch.zeros((len(wp), 4), dtype=torch.float32).pin_memory()
    gpu.graph_export_map_into([(0, 0, 2, 0)], tl.data_ptr(), len(wt), pt.data_ptr(), len(wp), off.data_ptr())
    gpu.synchronize()
    assert off.tolist() == [0, len(wt), 0, len(wp)]
    assert same_tiles((tl.numpy().view(binding.MAP_TILE_DTYPE), pt.numpy()), (wt, wp))
    assert gpu.profile()["graph_map"]["launches"] == 2 + 3 + 1
    gpu.graph_export_map_into([(0, 0, 2, 0)], tl.data_ptr(), len(wt), pt.data_ptr(), len(wp), off.data_ptr())   # the size is remembered
    gpu.synchronize()
    assert gpu.profile()["graph_map"]["launches"] == 2 + 3 + 1 + 2
    gpu.close()


def test_segments_take_every_path_of_the_voxel_filter(O, binding, atlas, world):
    gpu = world["gpu"]
    (wt, wp), st, sizes = want(atlas, O, world, 2)
    # corner: one cube of 18 keyframes x ~1000; surf: ~3700, ~250 and ~50 per keyframe in three cubes
    tiny, small, big, general = (sorted(s for s in sizes if lo < s <= hi) for lo, hi in ((0, 2048), (2048, 8192), (8192, 65536), (65536, 1 << 30)))
    assert len(tiny) >= 1 and len(small) >= 1 and len(big) >= 1 and len(general) >= 1, sizes
    assert general[-1] > 65536 + 256 and big[-1] < 65536 - 256 and small[-1] < 8192 - 256 and tiny[-1] < 2048 - 256, sizes   # on the side meant
    before = gpu.map_pool_info()
    tiles, points, off, stats = gpu.graph_export_map([(2, 0, 18, binding.GRAPH_POSE_ENTERED)])
    assert stats[0]["raw_points"].tolist() == st["raw_points"] == [sum(s for s, t in zip(sizes, wt) if t["feature_class"] == c) for c in (0, 1)]
    assert stats[0]["raw_points"][1] == sum(len(s[1]) for s in world["stacks"][2]) and stats[0]["outside"] == 0
    assert same_tiles((tiles, points), (wt, wp)), (len(tiles), len(wt), len(points), len(wp))
    after = gpu.map_pool_info()
    assert after["pool_points"] >= general[-1] and (before["pool_points"] >= general[-1] or after["growths"] == before["growths"] + 1)


def test_a_requests_bits_do_not_depend_on_the_list(O, binding, atlas, world):
    gpu = world["gpu"]
    E = binding.GRAPH_POSE_ENTERED
    reqs = [(0, 0, 1, E), (1, 0, 7, E), (2, 0, 18, E), (2, 4, 9, E)]
    wants = [want(atlas, O, world, 0)[0], want(atlas, O, world, 1)[0], want(atlas, O, world, 2)[0], want(atlas, O, world, 2, 4, 9)[0]]

    def part(res, i):
        tiles, points, off, _ = res
        t = tiles[off[0, i]:off[0, i + 1]].copy()
        t["first_point"] -= off[1, i]
        return t, points[off[1, i]:off[1, i + 1]]
    alone = [gpu.graph_export_map([r]) for r in reqs]
    together = gpu.graph_export_map(reqs)
    backwards = gpu.graph_export_map(reqs[::-1])
    for i in range(4):
        assert same_tiles(part(alone[i], 0), wants[i]), i
        assert same_tiles(part(together, i), wants[i]), i
        assert same_tiles(part(backwards, 3 - i), wants[i]), i
    assert together[0]["first_point"].tolist() == np.concatenate([[0], np.cumsum(together[0]["count"])[:-1]]).tolist()


def test_size_query_and_caps(O, binding, atlas, world):
    """Offsets and caps follow aloam_export_map_spill: the offsets are running sums over the list, always written, and a request is written
    when both of its ranges end inside the caps.  So a request behind one that does not fit is never written either (its ranges end further
    out still): which requests are left out is decided by where the list's running sums cross the caps."""
    import torch
    gpu = world["gpu"]
    E = binding.GRAPH_POSE_ENTERED
    reqs = [(0, 0, 1, E), (1, 0, 7, E), (2, 2, 3, E)]
    wants = [want(atlas, O, world, 0)[0], want(atlas, O, world, 1)[0], want(atlas, O, world, 2, 2, 3)[0]]
    nt, npts = [len(w[0]) for w in wants], [len(w[1]) for w in wants]
    GUARD = 0x5A
    off = torch.full((2 * 4 + 4,), -7, dtype=torch.int64).pin_memory()
    gpu.graph_export_map_into(reqs, 0, 0, 0, 0, off.data_ptr())               # the size query writes offsets and nothing else
    gpu.synchronize()
    assert off[:4].tolist() == np.concatenate([[0], np.cumsum(nt)]).tolist() and off[4:8].tolist() == np.concatenate([[0], np.cumsum(npts)]).tolist()
    assert off[8:].tolist() == [-7] * 4
    # caps of the first request alone; caps one point, then one tile, short of the whole list; caps of the whole list
    for cap_t, cap_p, written in ((nt[0], npts[0], [1, 0, 0]), (sum(nt), sum(npts) - 1, [1, 1, 0]), (sum(nt) - 1, sum(npts), [1, 1, 0]), (sum(nt), sum(npts), [1, 1, 1])):
        tiles = torch.full(((sum(nt) + 4) * 32,), GUARD, dtype=torch.uint8, device="cuda")
        pts = torch.full(((sum(npts) + 64) * 4,), 12345.0, dtype=torch.float32, device="cuda")
        stats = torch.zeros(3 * 32, dtype=torch.uint8).pin_memory()
        gpu.graph_export_map_into(reqs, tiles.data_ptr(), cap_t, pts.data_ptr(), cap_p, off.data_ptr(), stats.data_ptr())
        gpu.synchronize()
        st = stats.numpy().view(binding.GRAPH_MAP_STATS_DTYPE)
        assert st["written"].tolist() == written, (cap_t, cap_p)
        th, ph = tiles.cpu().numpy(), pts.cpu().numpy().reshape(-1, 4)
        to, po = np.concatenate([[0], np.cumsum(nt)]), np.concatenate([[0], np.cumsum(npts)])
        for i in range(3):
            t, p = th[to[i] * 32:to[i + 1] * 32], ph[po[i]:po[i + 1]]
            if written[i]:
                tt = t.view(binding.MAP_TILE_DTYPE).copy()
                tt["first_point"] -= po[i]
                assert same_tiles((tt, p), wants[i]), (cap_t, cap_p, i)
            else:
                assert (t == GUARD).all() and (p == 12345.0).all(), (cap_t, cap_p, i)
        assert (th[min(cap_t, sum(nt)) * 32:] == GUARD).all() and (ph[min(cap_p, sum(npts)):] == 12345.0).all()   # nothing lies past the caps
        assert off[8:].tolist() == [-7] * 4


def test_caps_that_fit_two_requests_but_not_the_large_one(O, binding, atlas, world):
    """Two small requests and a large one under caps sized for the two small ones: those two are written, the large one is not
    (written = 0) and nothing lies past the caps.  With running-sum offsets that is the list (small, small, large); listed (small, large,
    small) the last one's ranges end behind the large one's and it is left out too (the case above)."""
    import torch
    gpu = world["gpu"]
    E = binding.GRAPH_POSE_ENTERED
    reqs = [(0, 0, 1, E), (2, 2, 1, E), (1, 0, 7, E)]
    wants = [want(atlas, O, world, 0)[0], want(atlas, O, world, 2, 2, 1)[0], want(atlas, O, world, 1)[0]]
    nt, npts = [len(w[0]) for w in wants], [len(w[1]) for w in wants]
    cap_t, cap_p = nt[0] + nt[1] + 1, npts[0] + npts[1] + 5                   # room for the two small ones and a little more
    tiles = torch.full(((sum(nt) + 4) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    pts = torch.full(((sum(npts) + 64) * 4,), 12345.0, dtype=torch.float32, device="cuda")
    off = torch.zeros(8, dtype=torch.int64).pin_memory()
    stats = torch.zeros(3 * 32, dtype=torch.uint8).pin_memory()
    gpu.graph_export_map_into(reqs, tiles.data_ptr(), cap_t, pts.data_ptr(), cap_p, off.data_ptr(), stats.data_ptr())
    gpu.synchronize()
    assert stats.numpy().view(binding.GRAPH_MAP_STATS_DTYPE)["written"].tolist() == [1, 1, 0]
    th, ph = tiles.cpu().numpy(), pts.cpu().numpy().reshape(-1, 4)
    assert (th[(nt[0] + nt[1]) * 32:] == 0x5A).all() and (ph[npts[0] + npts[1]:] == 12345.0).all()
    t1 = th[nt[0] * 32:(nt[0] + nt[1]) * 32].view(binding.MAP_TILE_DTYPE).copy()
    t1["first_point"] -= npts[0]
    assert same_tiles((t1, ph[npts[0]:npts[0] + npts[1]]), wants[1])


def test_points_outside_the_atlas_range_are_counted_and_left_out(O, binding, atlas):
    rng = np.random.default_rng(3)
    gpu = context(binding, batch=1, nodes=4, edges=4, keyframes=(4096, 8192))
    inside = step(gpu, binding, [(cloud(rng, 100, (10, 10, 2)), cloud(rng, 400, (15, 15, 3)), Q_ID, (5.0, 0.0, 0.0))], [0])[0]
    far = step(gpu, binding, [(cloud(rng, 120, (10, 10, 2)), cloud(rng, 500, (15, 15, 3)), Q_ID, (30000.0, 0.0, 0.0))], [0])[0]
    nodes = gpu.graph_export(0)
    assert nodes["t"][1][0] == 30000.0
    st = {}
    wt, wp = model(atlas, O, nodes, [inside, far], stats=st)
    assert st["outside"] == len(far[0]) + len(far[1]) > 0
    tiles, points, off, stats = gpu.graph_export_map([(0, 0, 2, 0)])
    assert stats[0]["outside"] == st["outside"] and stats[0]["raw_points"].tolist() == [len(inside[0]), len(inside[1])]
    assert same_tiles((tiles, points), (wt, wp)) and (np.abs(tiles["cube"]) <= 1).all()
    only_far = gpu.graph_export_map([(0, 1, 1, 0)])
    assert len(only_far[0]) == 0 and len(only_far[1]) == 0 and only_far[3][0]["outside"] == st["outside"] and only_far[3][0]["written"] == 1
    gpu.close()


def test_a_full_store_keeps_nodes_without_clouds_and_says_so_once(binding):
    rng = np.random.default_rng(9)
    gpu = context(binding, batch=1, nodes=8, edges=8, keyframes=(250, 900))   # rows for two keyframes of ~100 corner / ~400 surf points

    def keyframe():
        for b, (corner, surf, q, t) in enumerate([(cloud(rng, 100, (10, 10, 2)), cloud(rng, 400, (15, 15, 3)), Q_ID, (0.0, 0.0, 0.0))]):
            gpu.set_last(corner, surf, b); gpu.set_full_cloud(surf[:4], b); gpu.set_state([0, 0, 0, 1], [0, 0, 0], q, t, b)
        gpu.mapping_step()
        gpu.graph_add_nodes([0], INFO)
    keyframe(); keyframe()
    gpu.synchronize()
    held = gpu.graph_keyframe_info(0)
    assert held["dropped_nodes"] == 0 and 150 < held["points"][0] <= 250 and 600 < held["points"][1] <= 900
    keyframe()
    with pytest.raises(binding.AloamError) as e:
        gpu.synchronize()
    assert e.value.code == binding.E_CAPACITY and "keyframe store full" in str(e.value)
    gpu.synchronize()                                                         # once
    info = gpu.graph_keyframe_info(0)
    assert gpu.graph_info(0)["nodes"] == 3 and info["dropped_nodes"] == 1 and info["points"] == held["points"]
    assert info["dropped_points"] == len(gpu.map_cloud(binding.MAP_CORNER_STACK)) + len(gpu.map_cloud(binding.MAP_SURF_STACK))
    for cls in (0, 1):
        pts, off = gpu.graph_export_keyframes(0, feature_class=cls)
        assert off[3] == off[2] == held["points"][cls] and len(pts) == held["points"][cls]      # the third node exists with counts of 0
    tiles, points, off, stats = gpu.graph_export_map([(0, 2, 1, 0)])
    assert len(tiles) == 0 and stats[0]["raw_points"].tolist() == [0, 0]
    gpu.graph_clear([0])
    keyframe(); keyframe()
    gpu.synchronize()                                                         # the rows take two keyframes again
    again = gpu.graph_keyframe_info(0)
    assert again["dropped_nodes"] == 1 and all(0 < p <= c for p, c in zip(again["points"], again["capacity"])) and gpu.graph_info(0)["nodes"] == 2
    assert gpu.graph_export_keyframes(0, feature_class=1)[1][2] == again["points"][1]
    gpu.close()


def test_exported_tiles_load_as_an_atlas_from_device_memory(O, binding, atlas, world):
    import torch
    gpu = world["gpu"]
    (wt, wp), st, _ = want(atlas, O, world, 1)
    tiles = torch.zeros(len(wt) * 32, dtype=torch.uint8, device="cuda")
    pts = torch.zeros((len(wp), 4), dtype=torch.float32, device="cuda")
    off = torch.zeros(4, dtype=torch.int64).pin_memory()
    gpu.graph_export_map_into([(1, 0, 7, binding.GRAPH_POSE_ENTERED)], tiles.data_ptr(), len(wt), pts.data_ptr(), len(wp), off.data_ptr())
    gpu.atlas_load(tiles, pts)                                                # synchronises; straight from device memory
    info = gpu.atlas_info()
    assert info["tiles"] == len(wt) and info["cubes"] == st["tiles"] and info["points"] == st["points"]
    held = atlas.Atlas(wt, wp)
    assert [c for c, _ in held.counts()] == st["tiles"]
    gpu.atlas_load(wt[:0], wp[:0])


def test_refusals_leave_everything_as_it_was(binding, world):
    import torch
    gpu = world["gpu"]
    E = binding.GRAPH_POSE_ENTERED

    def refused(code, f):
        with pytest.raises(binding.AloamError) as e:
            f()
        assert e.value.code == code, str(e.value)
    before = [gpu.graph_keyframe_info(b) for b in range(3)]
    off = torch.full((8,), -7, dtype=torch.int64).pin_memory()
    tiles = torch.full((64 * 32,), 0x5A, dtype=torch.uint8).pin_memory()
    pts = torch.full((4096, 4), 12345.0, dtype=torch.float32).pin_memory()
    pageable = np.zeros(64, np.int64)
    for bad in ((3, 0, 1, E), (-1, 0, 1, E), (1, -1, 2, E), (1, 0, -1, E), (1, 5, 3, E), (0, 0, 2, E), (1, 0, 7, 2), (1, 0, 7, -1)):
        refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E), bad], tiles.data_ptr(), 64, pts.data_ptr(), 4096, off.data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], tiles.data_ptr(), 64, pts.data_ptr(), 4096, 0))                      # no offsets
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], tiles.data_ptr(), 64, pts.data_ptr(), 4096, pageable.ctypes.data))   # pageable
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], 0, 64, pts.data_ptr(), 4096, off.data_ptr()))                         # NULL with a cap
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], tiles.data_ptr(), -1, pts.data_ptr(), 4096, off.data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], tiles.data_ptr(), 64, pts.data_ptr() + 4, 4096, off.data_ptr()))     # misaligned
    refused(binding.E_ARG, lambda: gpu.graph_export_map_into([(0, 0, 1, E)], tiles.data_ptr(), 64, pts.data_ptr(), 4096, off.data_ptr(), pageable.ctypes.data))
    for args in ((3, 0, 1, 0), (1, 0, 8, 0), (1, -1, 1, 0), (1, 0, 1, 2), (1, 0, 1, -1)):
        refused(binding.E_ARG, lambda: gpu.graph_export_keyframes_into(*args, pts.data_ptr(), 4096, off.data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_export_keyframes_into(1, 0, 1, 0, pts.data_ptr(), -1, off.data_ptr()))
    refused(binding.E_ARG, lambda: gpu.graph_export_keyframes_into(1, 0, 1, 0, pts.data_ptr(), 4096, pageable.ctypes.data))
    refused(binding.E_ARG, lambda: gpu.graph_keyframe_info(3))
    refused(binding.E_STATE, lambda: gpu.graph_keyframes_enable(1024, 1024))  # twice
    gpu.synchronize()
    assert off.tolist() == [-7] * 8 and (tiles.numpy() == 0x5A).all() and (pts.numpy() == 12345.0).all()
    assert [gpu.graph_keyframe_info(b) for b in range(3)] == before
    # the order of the enables, the sizes, and a sequence that holds no stacks
    g = binding.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=4096, lm_max_iterations=0)
    refused(binding.E_STATE, lambda: g.graph_keyframes_enable(1024, 1024))    # before aloam_graph_enable
    g.graph_enable(8, 8)
    refused(binding.E_STATE, lambda: g.graph_keyframes_enable(1024, 1024))    # before aloam_mapping_enable
    refused(binding.E_STATE, lambda: g.graph_export_map_into([], 0, 0, 0, 0, off.data_ptr()))
    refused(binding.E_STATE, lambda: g.graph_export_keyframes_into(0, 0, 0, 0, 0, 0, off.data_ptr()))
    refused(binding.E_STATE, lambda: g.graph_keyframe_info(0))
    g.mapping_enable(0.4, 0.8, pool_points=1 << 16)
    for sizes in ((0, 1024), (1024, 0), ((1 << 26) + 1, 1024), (1024, (1 << 26) + 1)):
        refused(binding.E_ARG, lambda: g.graph_keyframes_enable(*sizes))
    g.graph_add_nodes([0], INFO)
    refused(binding.E_STATE, lambda: g.graph_keyframes_enable(1024, 1024))    # a graph is not empty
    g.graph_clear([0])
    g.graph_keyframes_enable(1024, 1024)
    refused(binding.E_STATE, lambda: g.graph_add_nodes([0], INFO))            # no mapping step yet: no stacks
    assert g.graph_info(0)["nodes"] == 0
    rng = np.random.default_rng(1)
    g.set_active([1, 0])
    step_inputs = (cloud(rng, 50, (5, 5, 1)), cloud(rng, 200, (8, 8, 2)))
    g.set_last(*step_inputs, 0); g.set_full_cloud(step_inputs[1][:4], 0); g.set_state([0, 0, 0, 1], [0, 0, 0], [0, 0, 0, 1.0], [0, 0, 0.0], 0)
    g.mapping_step()
    g.set_active(None)
    refused(binding.E_STATE, lambda: g.graph_add_nodes([0, 1], INFO))         # sequence 1 sat the step out: nothing is queued for either
    assert g.graph_info(0)["nodes"] == 0 and g.graph_info(1)["nodes"] == 0
    g.graph_add_nodes([0], INFO)
    g.reset_sequences([0])
    refused(binding.E_STATE, lambda: g.graph_add_nodes([0], INFO))            # reset: the stacks are gone, the store is left alone
    g.synchronize()
    assert g.graph_info(0)["nodes"] == 1 and g.graph_keyframe_info(0)["points"][1] > 0
    g.close()


def _getters(gpu, binding, B):
    out = []
    for b in range(B):
        out.append(gpu.graph_export(b).tobytes())
        out.append(gpu.graph_export(b, edges=True).tobytes())
        out.append(gpu.map_cloud(binding.MAP_CORNER_STACK, b).tobytes() + gpu.map_cloud(binding.MAP_SURF_STACK, b).tobytes())
        out.append(repr(sorted(gpu.map_info(b).items())) + repr(gpu.map_pose(b)))
        out += [gpu.map_cubes(cls, b)[k].tobytes() for cls in (0, 1) for k in sorted(gpu.map_cubes(cls, b))]
    return out


def test_opt_in_changes_nothing_else(binding):
    """Twins, one with the store and one without, through the same calls: the same bits from every getter, the same launch counts per
    profiling slot except graph_map, which counts the capture launches and is 0 without the store."""
    runs = []
    for enabled in (False, True):
        rng = np.random.default_rng(77)
        gpu = context(binding, batch=2, nodes=8, edges=8, keyframes=(4096, 8192) if enabled else None)
        gpu.profile_enable(True)
        for k in range(3):
            inputs = [(cloud(rng, 80, (10, 10, 2)), cloud(rng, 600, (15, 15, 3)), Q_Z if k == 1 else Q_ID, (3.0 * k, 0.5 * b, 0.0)) for b in range(2)]
            step(gpu, binding, inputs, [0, 1] if k != 1 else [1])
        gpu.graph_optimize([0, 1])
        gpu.graph_clear([1])
        step(gpu, binding, inputs, [1])
        runs.append((_getters(gpu, binding, 2), gpu.profile()))
        gpu.close()
    (g0, p0), (g1, p1) = runs
    assert g0 == g1
    assert set(p0) == set(p1) and "graph_map" in p0
    for name in p0:
        if name != "graph_map":
            assert p0[name]["launches"] == p1[name]["launches"], name
    assert p0["graph_map"]["launches"] == 0 and p1["graph_map"]["launches"] == 4     # one capture launch per aloam_graph_add_nodes
