"""The map spill on the MI355X (aloam_map_spill_enable / aloam_export_map_spill): the cubes a window shift of the mapping step empties are
kept as tiles - the cubes the model says, every point, in the order of the contract - while the step computes what it computes without the
spill; the drain is stream-ordered; a full spill drops whole tiles and says so once; spill + window after a step hold every cube the map
held before it.  Every comparison is bit for bit.

Windows are put at the edge with aloam_set_map_frame as test_window_shift_of_a_frozen_map_is_a_pure_permutation does, and far cubes are
injected with aloam_set_map (a few hundred random cubes per class, 1 - 300 points each): no drive a test can afford travels the 850 m a
cube needs to fall off by itself."""
import importlib

import numpy as np
import pytest

from test_gpu_checkpoint import make
from test_gpu_localization import _mp, cubes, frame, world_cube
from test_gpu_sequence_lifecycle import _drives, diff, snap

pytestmark = pytest.mark.gpu
F = 4                                                    # frames mapped before the window is moved to the edge
MAX_TILES, MAX_POINTS = 1024, 1 << 16

# (cen, map <- odometry translation, the shift the step must make)
SHIFTS = {"x+": ((2, 10, 5), (0, 0, 0), (1, 0, 0)), "x-": ((18, 10, 5), (0, 0, 0), (-1, 0, 0)),
          "y+": ((10, 2, 5), (0, 0, 0), (0, 1, 0)), "y-": ((10, 18, 5), (0, 0, 0), (0, -1, 0)),
          "z+": ((10, 10, 2), (0, 0, 0), (0, 0, 1)), "z-": ((10, 10, 8), (0, 0, 0), (0, 0, -1)),
          "two-axes": ((2, 18, 5), (0, 0, 0), (1, -1, 0)),
          "multi": ((18, 2, 5), (130, -60, 0), (-4, 2, 0))}   # centre cube (3 + 18, -1 + 2, 5) = (21, 1, 5): four shifts down, two up


@pytest.fixture(scope="module")
def atlas():
    return importlib.import_module("a-loam_amd.atlas")


@pytest.fixture(scope="module")
def base(binding, sequence):
    """A record of one sequence after F mapped frames, the drive, and one context with the spill enabled (2 slots) for the tests to share."""
    drives, model = _drives(sequence, 1, F + 2)
    gpu = make(binding, model, 2, _mp(drives), True)
    gpu.map_spill_enable(MAX_TILES, MAX_POINTS)
    for k in range(F):
        frame(gpu, [drives[0][k], None])
    blob, off = gpu.save_sequences([0])
    yield {"drives": drives, "model": model, "gpu": gpu, "blob": np.array(blob), "off": off}
    gpu.close()


def far_cubes(atlas, have, cen, seed, n=300):
    """n random cubes of the window that `have` does not hold, 1 - 300 points each, inside their cubes for a window centred at cen."""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(atlas.N_CUBES), np.array(sorted(have), np.int64))
    out = {}
    for idx in rng.choice(free, n, replace=False):
        m = int(rng.integers(1, 301))
        centre = (np.array(atlas.ijk_of(int(idx))) - np.array(cen)) * 50.0
        p = np.concatenate([centre + rng.uniform(-24.0, 24.0, (m, 3)), rng.uniform(0, 1, (m, 1))], 1).astype(np.float32)
        out[int(idx)] = p
    return out


def arrange(atlas, base, gpu, slot, cen, t, seed=5, only_far=False, n_far=300):
    """Slot `slot` := the record, its map extended by far cubes, its window centred at `cen` with the correction translated by t.
    Returns the map as [{index: points}] * 2 and the frame count."""
    gpu.load_sequences([slot], base["blob"], base["off"])
    gpu.synchronize()
    before = []
    for cls in (0, 1):
        c = {} if only_far else gpu.map_cubes(cls, slot)
        c.update(far_cubes(atlas, c, cen, seed + cls, n_far))
        gpu.set_map(c, cls, seq=slot)
        before.append(c)
    p, fc = gpu.map_pose(slot), gpu.map_info(slot)["frame_count"]
    gpu.set_map_frame(cen, p["q_wmap_wodom"], np.array(p["t_wmap_wodom"]) + np.array(t, np.float64), fc, seq=slot)
    return before, fc


def same_tiles(got, want):
    (gt, gp), (wt, wp) = got, want
    return len(gt) == len(wt) and gt.tobytes() == wt.tobytes() and gp.shape == wp.shape and np.array_equal(gp.view(np.uint32), wp.view(np.uint32))


def keyed(atlas, tiles, points):
    """{(absolute cube, class): points}; every key once."""
    out = {}
    for t in tiles:
        key = (*(int(v) for v in t["cube"]), int(t["feature_class"]))
        assert key not in out, key
        out[key] = points[int(t["first_point"]):int(t["first_point"]) + int(t["count"])]
    return out


_RUNS = {}


def shifted_step(atlas, base, name, frozen):
    """One step of slot 0 across the shift `name`; cached: several tests look at the same step."""
    if (name, frozen) not in _RUNS:
        cen, t, s = SHIFTS[name]
        gpu = base["gpu"]
        gpu.export_map_spill([0, 1])                      # (whatever an earlier test left)
        before, fc = arrange(atlas, base, gpu, 0, cen, t)
        frame(gpu, [base["drives"][0][F], None], frozen=[frozen, False])
        spill = gpu.export_map_spill([0])
        info = gpu.map_info(0)
        _RUNS[(name, frozen)] = {"cen": cen, "s": s, "before": before, "frame": fc, "spill": spill, "after": cubes(gpu, 0), "info": info,
                                 "centre": tuple(a + c for a, c in zip(world_cube(gpu, 0), (info["cenW"], info["cenH"], info["cenD"]))),
                                 "window_tiles": atlas.window_tiles(gpu, 0), "spill_info": gpu.map_spill_info(0)}
    return _RUNS[(name, frozen)]


def valid_indices(centre):
    """The 5 x 5 x 3 cubes around the centre cube: what a growing step inserts into and re-filters (src/laserMapping.cpp:512-529, :737-801)."""
    return {i + 21 * j + 441 * k for i in range(centre[0] - 2, centre[0] + 3) for j in range(centre[1] - 2, centre[1] + 3)
            for k in range(centre[2] - 1, centre[2] + 2) if 0 <= i < 21 and 0 <= j < 21 and 0 <= k < 11}


@pytest.mark.parametrize("frozen", [False, True], ids=["growing", "frozen"])
@pytest.mark.parametrize("name", list(SHIFTS))
def test_spilled_tiles_are_the_cubes_the_shift_emptied(binding, atlas, base, name, frozen):
    r = shifted_step(atlas, base, name, frozen)
    cen, s = r["cen"], r["s"]
    assert (r["info"]["cenW"], r["info"]["cenH"], r["info"]["cenD"]) == tuple(c + d for c, d in zip(cen, s))
    want = atlas.spill_of(r["before"], cen, s, r["frame"])
    tiles, points, off = r["spill"]
    assert len(want[0]) > 0 and off.tolist() == [[0, len(want[0])], [0, len(want[1])]]
    assert same_tiles((tiles, points), want), (len(tiles), len(want[0]))   # absolute cube, class, count, frame, first_point, order, every point
    assert r["spill_info"]["tiles"] == [0, 0] and r["spill_info"]["dropped_tiles"] == 0      # drained with clear
    # the window afterwards is the permutation it is without the spill (a growing step has also inserted into its valid cubes)
    touched = set() if frozen else valid_indices(r["centre"])
    for cls in (0, 1):
        moved = {}
        for idx, pts in r["before"][cls].items():
            if atlas.survives(idx, s):
                i, j, k = (x + d for x, d in zip(atlas.ijk_of(idx), s))
                moved[atlas.index_of(i, j, k)] = pts
        assert set(moved) - touched == set(r["after"][cls]) - touched, cls
        for idx in set(moved) - touched:
            assert np.array_equal(moved[idx].view(np.uint32), r["after"][cls][idx].view(np.uint32)), (cls, idx)


@pytest.mark.parametrize("frozen", [False, True], ids=["growing", "frozen"])
@pytest.mark.parametrize("name", ["x+", "two-axes", "multi"])
def test_nothing_is_lost(binding, atlas, base, name, frozen):
    r = shifted_step(atlas, base, name, frozen)
    tiles, points = atlas.concatenate([r["spill"][:2], r["window_tiles"]])
    got = keyed(atlas, tiles, points)
    want = keyed(atlas, *atlas.tiles_of_window(r["before"], r["cen"]))
    cen_after = tuple(c + d for c, d in zip(r["cen"], r["s"]))
    touched = set() if frozen else {(*(x - c for x, c in zip(atlas.ijk_of(i), cen_after)), cls) for i in valid_indices(r["centre"]) for cls in (0, 1)}
    assert set(got) - touched == set(want) - touched                        # every cube once
    for key in set(want) - touched:
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key   # every bit
    at = atlas.Atlas(tiles, points)
    assert [n for n, _ in at.counts()] == [sum(1 for k in got if k[3] == cls) for cls in (0, 1)]


@pytest.mark.parametrize("frozen", [False, True], ids=["growing", "frozen"])
def test_the_spill_changes_nothing_else(binding, atlas, base, frozen):
    cen, t, s = SHIFTS["two-axes"]
    twins = []
    for spill in (True, False):
        gpu = make(binding, base["model"], 1, _mp(base["drives"]), True)
        if spill:
            gpu.map_spill_enable(MAX_TILES, MAX_POINTS)
        arrange(atlas, base, gpu, 0, cen, t)
        for k in (F, F + 1):                               # the shifting step and the one after it
            frame(gpu, [base["drives"][0][k]], frozen=[frozen])
        gpu.synchronize()
        twins.append(snap(binding, gpu, 0, True))
        if spill:
            assert sum(gpu.map_spill_info(0)["tiles"]) > 0
        gpu.close()
    assert not diff(*twins), diff(*twins)


def test_drains_are_stream_ordered(binding, atlas, base):
    import torch
    gpu, d = base["gpu"], base["drives"][0]
    gpu.export_map_spill([0, 1])
    (cen0, t0, s0), (cen1, t1, s1) = SHIFTS["x+"], SHIFTS["y-"]
    before0, fc0 = arrange(atlas, base, gpu, 0, cen0, t0, seed=11)
    before1, fc1 = arrange(atlas, base, gpu, 1, cen1, t1, seed=13)
    want0, want1 = atlas.spill_of(before0, cen0, s0, fc0), atlas.spill_of(before1, cen1, s1, fc1)
    gpu.synchronize()
    bufs = []
    for where in ({"pin_memory": True}, {"device": "cuda"}):
        bufs.append((torch.zeros(4096 * 32, dtype=torch.uint8, **where), torch.zeros((1 << 16, 4), dtype=torch.float32, **where),
                     torch.zeros(6, dtype=torch.int64, **where)))
    # step of slot 0 alone (slot 1 sits at its edge, idle), drain both; step of slot 1 alone, drain both; one synchronise
    for (tl, pt, of), scans in zip(bufs, ([d[F], None], [None, d[F]])):
        frame(gpu, scans, frozen=[True, True])
        gpu.export_map_spill_into([0, 1], tl.data_ptr(), 4096, pt.data_ptr(), 1 << 16, of.data_ptr(), clear=True)
    gpu.synchronize()
    got = [(tl.cpu().numpy().view(binding.MAP_TILE_DTYPE), pt.cpu().numpy(), of.cpu().numpy().reshape(2, 3)) for tl, pt, of in bufs]
    for (tl, pt, of), want, slot in zip(got, (want0, want1), (0, 1)):
        nt, npts = len(want[0]), len(want[1])
        assert nt > 0
        assert of.tolist() == ([[0, nt, nt], [0, npts, npts]] if slot == 0 else [[0, 0, nt], [0, 0, npts]])   # each drain holds its own step's tiles only
        assert same_tiles((tl[:nt], pt[:npts]), want), slot
    assert gpu.map_spill_info(0)["tiles"] == [0, 0] and gpu.map_spill_info(1)["tiles"] == [0, 0]


def test_clear_caps_destinations_and_resets(binding, atlas, base):
    import torch
    gpu, d = base["gpu"], base["drives"][0]
    gpu.export_map_spill([0, 1])
    cen, t, s = SHIFTS["z-"]
    before, fc = arrange(atlas, base, gpu, 0, cen, t, seed=17)
    want = atlas.spill_of(before, cen, s, fc)
    frame(gpu, [d[F], None])
    nt, npts = len(want[0]), len(want[1])
    held = [int((want[0]["feature_class"] == cls).sum()) for cls in (0, 1)]
    assert gpu.map_spill_info(0)["tiles"] == held and gpu.map_spill_info(1)["tiles"] == [0, 0]   # the idle slot spilled nothing
    a = gpu.export_map_spill([0], clear=False)
    assert same_tiles(a[:2], want) and gpu.map_spill_info(0)["tiles"] == held                   # clear = 0 leaves the spill
    # caps too small (either one): offsets only, nothing written, nothing cleared
    tl = torch.full((4096 * 32,), 0xAB, dtype=torch.uint8, pin_memory=True)
    pt = torch.full((1 << 16, 4), -7.0, dtype=torch.float32, pin_memory=True)
    of = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    for cap_t, cap_p in ((nt - 1, npts), (nt, npts - 1), (0, 0)):
        gpu.export_map_spill_into([0], tl.data_ptr(), cap_t, pt.data_ptr(), cap_p, of.data_ptr(), clear=True)
        gpu.synchronize()
        assert of.tolist() == [0, nt, 0, npts]
        assert bool((tl == 0xAB).all()) and bool((pt == -7.0).all())
        assert gpu.map_spill_info(0)["tiles"] == held
    # pageable destinations: refused, nothing queued
    pageable_t, pageable_p, pageable_o = np.zeros(4096 * 32, np.uint8), np.zeros((1 << 16, 4), np.float32), np.zeros(4, np.int64)
    for args in ((pageable_t.ctypes.data, nt, pt.data_ptr(), npts, of.data_ptr()), (tl.data_ptr(), nt, pageable_p.ctypes.data, npts, of.data_ptr()),
                 (tl.data_ptr(), nt, pt.data_ptr(), npts, pageable_o.ctypes.data), (0, nt, pt.data_ptr(), npts, of.data_ptr())):
        with pytest.raises(binding.AloamError) as e:
            gpu.export_map_spill_into([0], *args)
        assert e.value.code == binding.E_ARG
    with pytest.raises(binding.AloamError) as e:
        gpu.export_map_spill_into([0, 0], tl.data_ptr(), nt, pt.data_ptr(), npts, of.data_ptr())
    assert e.value.code == binding.E_ARG
    gpu.synchronize()
    assert gpu.map_spill_info(0)["tiles"] == held and not pageable_t.any() and not pageable_p.any()
    # a reset (and a load) leaves the slot's spill alone
    gpu.reset_sequences([0])
    gpu.synchronize()
    assert gpu.map_spill_info(0)["tiles"] == held
    gpu.load_sequences([0], base["blob"], base["off"])
    b = gpu.export_map_spill([0], clear=True, pinned=False)               # a device destination
    assert same_tiles(b[:2], want) and gpu.map_spill_info(0)["tiles"] == [0, 0]


def test_a_full_spill_drops_whole_tiles_and_says_so_once(binding, atlas, base):
    cen, t, s = SHIFTS["x+"]
    gpu = make(binding, base["model"], 1, _mp(base["drives"]), True)
    gpu.map_spill_enable(16, 400)
    before, fc = arrange(atlas, base, gpu, 0, cen, t, seed=23, only_far=True, n_far=600)
    everything = atlas.spill_of(before, cen, s, fc)
    dropped = []
    want = atlas.spill_of(before, cen, s, fc, room=[(16, 400), (16, 400)], dropped=dropped)
    assert 0 < len(want[0]) < len(everything[0]) and dropped[0] == len(everything[0]) - len(want[0])
    counts = want[0]["count"]
    assert int(everything[0]["count"].max()) > int(counts.max())            # a large tile is missing, smaller ones behind it are there
    frame(gpu, [base["drives"][0][F]], frozen=[True])
    with pytest.raises(binding.AloamError) as e:
        gpu.synchronize()
    assert e.value.code == binding.E_CAPACITY and "map spill full" in str(e.value)
    gpu.synchronize()                                                       # once
    info = gpu.map_spill_info(0)
    assert (info["dropped_tiles"], info["dropped_points"]) == tuple(dropped)
    assert same_tiles(gpu.export_map_spill([0])[:2], want)
    gpu.close()


def test_spill_states_and_arguments(binding, base):
    gpu = binding.Aloam(n_scans=base["model"].n_scans, min_range=base["model"].min_range, batch=1, max_points=_mp(base["drives"]))
    with pytest.raises(binding.AloamError) as e:
        gpu.map_spill_enable(16, 16)                                        # before aloam_mapping_enable
    assert e.value.code == binding.E_STATE
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 14)
    for call in (lambda: gpu.map_spill_info(0), lambda: gpu.export_map_spill([0])):
        with pytest.raises(binding.AloamError) as e:
            call()
        assert e.value.code == binding.E_STATE                              # not enabled
    for bad in ((0, 16), (16, 0), ((1 << 20) + 1, 16)):
        with pytest.raises(binding.AloamError) as e:
            gpu.map_spill_enable(*bad)
        assert e.value.code == binding.E_ARG
    gpu.map_spill_enable(16, 16)
    with pytest.raises(binding.AloamError) as e:
        gpu.map_spill_enable(16, 16)
    assert e.value.code == binding.E_STATE
    t, p, off = gpu.export_map_spill([0])
    assert len(t) == 0 and len(p) == 0 and off.tolist() == [[0, 0], [0, 0]]
    gpu.close()


def test_kitti_runner_writes_the_whole_map_as_tiles(atlas, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m, a = tmp_path / "map.npz", tmp_path / "atlas.npz"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "run_kitti.py"), "--selftest", "--mapping", "--out", str(tmp_path / "out"),
                        "--save-map", str(m), "--save-atlas", str(a)], capture_output=True, text=True)
    assert r.returncode == 0 and " atlas: " in r.stdout, r.stdout + r.stderr
    saved = np.load(m)
    got = keyed(atlas, *atlas.load_atlas(a))
    want = {}
    for cls in (0, 1):                                                      # the drive stays inside its first window: the atlas is that window
        off = np.concatenate([[0], np.cumsum(saved[f"counts{cls}"])])
        for j, idx in enumerate(saved[f"ids{cls}"]):
            want[(*(x - c for x, c in zip(atlas.ijk_of(int(idx)), saved["cen"])), cls)] = saved[f"points{cls}"][off[j]:off[j + 1]]
    assert len(want) > 0 and set(got) == set(want)
    assert all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) for k in want)


# ---- the atlas: an attached, frozen sequence's window is cut from a map of any extent ---------------------------------------------------
from test_gpu_localization import pose_part  # noqa: E402


def as_tiles(atlas, world):
    """world = [{absolute cube: points}] * 2 -> (tiles, points), one tile per cube."""
    tiles, pts, first = [], [], 0
    for cls in (0, 1):
        for key in sorted(world[cls]):
            t = np.zeros((), atlas.TILE_DTYPE)
            t["cube"], t["feature_class"], t["count"], t["first_point"] = key, cls, len(world[cls][key]), first
            tiles.append(t)
            pts.append(world[cls][key])
            first += len(world[cls][key])
    return np.array(tiles, atlas.TILE_DTYPE), np.concatenate(pts)


def long_world(seed=3):
    """A synthetic map 41 cubes long (2 km) and 3 wide, 1 - 300 points per cube, the points inside their cubes."""
    rng = np.random.default_rng(seed)
    world = [{}, {}]
    for cls in (0, 1):
        for x in range(-20, 21):
            for y in (-1, 0, 1):
                if rng.random() < 0.8:
                    m = int(rng.integers(1, 301))
                    world[cls][(x, y, 0)] = np.concatenate([np.array([x, y, 0]) * 50.0 + rng.uniform(-24.0, 24.0, (m, 3)), rng.uniform(0, 1, (m, 1))], 1).astype(np.float32)
    return world


def attached_context(binding, atlas, base, world, B=1, **kw):
    gpu = make(binding, base["model"], B, _mp(base["drives"]), True, **kw)
    gpu.atlas_load(*as_tiles(atlas, world))
    for b in range(B):
        gpu.load_sequences([b], base["blob"], base["off"])
    gpu.set_map_frozen([1] * B)
    gpu.atlas_attach([1] * B)
    return gpu


def window_is_the_cut(atlas, gpu, b, at):
    info = gpu.map_info(b)
    want = at.cut((info["cenW"], info["cenH"], info["cenD"]))
    got = cubes(gpu, b)
    for cls in (0, 1):
        assert set(got[cls]) == set(want[cls]), (b, cls)                     # nothing else is non-empty
        assert all(np.array_equal(got[cls][i].view(np.uint32), want[cls][i].view(np.uint32)) for i in want[cls]), (b, cls)
    return sum(len(p) for c in want for p in c.values())


@pytest.mark.parametrize("cen,t", [((10, 10, 5), (0, 0, 0)), ((4, 12, 6), (0, 0, 0)), ((10, 10, 5), (430, 20, 0)), ((2, 18, 5), (-300, 0, 0))])
def test_the_attached_window_is_the_atlas_cut_to_the_window(binding, atlas, base, cen, t):
    world = long_world()
    at = atlas.Atlas(*as_tiles(atlas, world))
    gpu = attached_context(binding, atlas, base, world)
    p, fc = gpu.map_pose(0), gpu.map_info(0)["frame_count"]
    gpu.set_map_frame(cen, p["q_wmap_wodom"], np.array(p["t_wmap_wodom"]) + np.array(t, np.float64), fc)
    d = base["drives"][0]
    frame(gpu, [d[F]], frozen=[True])
    gpu.synchronize()
    info = gpu.map_info(0)
    centre = [a + c for a, c in zip(world_cube(gpu, 0), (info["cenW"], info["cenH"], info["cenD"]))]
    assert all(3 <= c < n - 3 for c, n in zip(centre, atlas.DIMS))            # cut where the shifts lead: k_map_begin then shifts nothing
    total = window_is_the_cut(atlas, gpu, 0, at)
    assert total > 0 and len(gpu.map_cloud(binding.MAP_FULL, 0)) == total      # descriptors and pool rows agree
    # a jump of 8 cubes that does NOT mark the window stale (aloam_apply_map_corrections): the shift alone re-cuts it, and the cubes that
    # enter hold their atlas points
    before = (info["cenW"], info["cenH"], info["cenD"])
    p = gpu.map_pose(0)
    gpu.apply_map_corrections([0], binding.map_corrections([p["q_wmap_wodom"]], [np.array(p["t_wmap_wodom"]) + np.array([400.0, 0, 0])]), [0])
    frame(gpu, [d[F + 1]], frozen=[True])
    gpu.synchronize()
    info = gpu.map_info(0)
    s = atlas.shift_of((centre[0] + 8, centre[1], centre[2]))
    after = tuple(c + d for c, d in zip(before, s))
    assert (info["cenW"], info["cenH"], info["cenD"]) == after
    assert window_is_the_cut(atlas, gpu, 0, at) > 0
    if any(s):                                                                # cubes that ENTERED the window hold their atlas points (without the atlas: empty)
        inside = lambda key, cen: all(0 <= k + c < n for k, c, n in zip(key, cen, atlas.DIMS))
        assert any(inside(key, after) and not inside(key, before) for key in at.cubes[0])
    gpu.close()


def test_atlas_info_reports_what_was_loaded_and_nothing_is_lost_through_it(binding, atlas, base):
    r = shifted_step(atlas, base, "two-axes", True)
    tiles, points = atlas.concatenate([r["spill"][:2], r["window_tiles"]])
    want = keyed(atlas, *atlas.tiles_of_window(r["before"], r["cen"]))
    gpu = make(binding, base["model"], 1, _mp(base["drives"]), True)
    gpu.atlas_load(tiles, points)
    info = gpu.atlas_info()
    assert info["tiles"] == len(tiles)
    assert info["cubes"] == [sum(1 for k in want if k[3] == cls) for cls in (0, 1)]
    assert info["points"] == [sum(len(p) for k, p in want.items() if k[3] == cls) for cls in (0, 1)]
    at = atlas.Atlas(tiles, points)
    assert info["exact"] and info["largest_window"] == [at.largest_window(0), at.largest_window(1)]
    gpu.atlas_load(tiles[:0], points[:0])                                    # unload
    assert gpu.atlas_info()["tiles"] == 0
    gpu.close()


@pytest.mark.parametrize("recut", [False, True], ids=["record-cen", "recut-mid-run"])
def test_an_attached_run_is_a_loaded_frozen_run(binding, atlas, sequence, recut):
    F0, FN = 8, 34
    scans, R, t, model = sequence("HDL-64", FN, seed=41, columns=512, travel=True, step=2.0)
    mp = max(len(s) for s in scans) + 64
    gpu = make(binding, model, 2, mp, True)
    for k in range(F0):
        frame(gpu, [scans[k], None])
    blob, off = gpu.save_sequences([0])
    tiles, points = atlas.window_tiles(gpu, 0)
    gpu.atlas_load(tiles, points)
    gpu.load_sequences([0, 1], np.concatenate([np.array(blob)] * 2), np.array([0, off[1], 2 * off[1]], np.int64))
    gpu.set_map_frozen([1, 1])
    gpu.atlas_attach([0, 1])                                                 # twin A: the loaded record, frozen; twin B: attached
    info, p = gpu.map_info(1), gpu.map_pose(1)
    if recut:                                                                 # the sensor's cube at index 17 of the axis it travels along
        axis = int(np.argmax(np.abs(t[FN - 1] - t[0])))
        sign = 1 if (t[FN - 1] - t[0])[axis] > 0 else -1
        cen = [info["cenW"], info["cenH"], info["cenD"]]
        centre = world_cube(gpu, 1)[axis] + cen[axis]
        cen[axis] += (17 if sign > 0 else 3) - centre
        gpu.set_map_frame(cen, p["q_wmap_wodom"], p["t_wmap_wodom"], info["frame_count"], seq=1)
    cens = []
    for k in range(F0, FN):
        frame(gpu, [scans[k], scans[k]], frozen=[True, True])
        gpu.synchronize()
        a, b = pose_part(binding, gpu, 0), pose_part(binding, gpu, 1)
        ia, ib = gpu.map_info(0), gpu.map_info(1)
        cens.append((ib["cenW"], ib["cenH"], ib["cenD"]))
        if recut:                                                             # (ii): the pose does not depend on where the window sits; (i): cen too
            for i in (ia, ib):
                for key in ("cenW", "cenH", "cenD"):
                    i.pop(key)
            a["map_info"], b["map_info"] = repr(ia), repr(ib)                 # (with the compaction count, which pose_part leaves out: no frozen step compacts)
        else:
            assert ia == ib, (k, ia, ib)
        assert not diff(a, b), (k, diff(a, b))
    moved = [k for k in range(1, len(cens)) if cens[k] != cens[k - 1]]
    assert (len(moved) == 1 and sum(abs(x - y) for x, y in zip(cens[moved[0]], cens[moved[0] - 1])) == 1) if recut else not moved
    gpu.close()


@pytest.mark.parametrize("ref_order", [False, True], ids=["input-order", "reference-order-context"])
def test_tiles_of_one_cube_are_merged_by_one_voxel_filter(O, binding, atlas, base, ref_order):
    rng = np.random.default_rng(9)
    def tile(cube, cls, n, frame):
        p = np.concatenate([np.array(cube) * 50.0 + rng.uniform(-3.0, 3.0, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        return atlas.tiles_of_window([{atlas.index_of(*(c + z for c, z in zip(cube, (10, 10, 5)))): p} if cls == 0 else {}, {} if cls == 0 else {atlas.index_of(*(c + z for c, z in zip(cube, (10, 10, 5)))): p}], (10, 10, 5), frame)
    parts = [tile((0, 0, 0), 0, 500, 1), tile((1, 0, 0), 0, 300, 1), tile((0, 0, 0), 0, 700, 2), tile((0, 0, 0), 1, 400, 1), tile((2, 1, 0), 1, 90, 1),
             tile((0, 0, 0), 1, 300, 2), tile((0, 0, 0), 1, 9000, 3), tile((1, 0, 0), 1, 50, 3)]
    tiles, points = atlas.concatenate(parts)
    raw = atlas.Atlas(tiles, points)                                          # concatenation in array order
    gpu = make(binding, base["model"], 1, _mp(base["drives"]), True, ref_order=ref_order)
    gpu.atlas_load(tiles, points)
    gpu.set_map_frozen([1])
    gpu.atlas_attach([1])                                                     # a fresh sequence (cen = (10, 10, 5)): its first step cuts the window
    frame(gpu, [base["drives"][0][0]], frozen=[True])
    gpu.synchronize()
    got = cubes(gpu, 0)
    leaf = (0.4, 0.8)
    n_merged = 0
    for cls in (0, 1):
        assert set(got[cls]) == {atlas.index_of(*(c + z for c, z in zip(key, (10, 10, 5)))) for key in raw.cubes[cls]}
        for key, pts in raw.cubes[cls].items():
            several = sum(1 for t in tiles if tuple(t["cube"]) == key and t["feature_class"] == cls) > 1
            want = O.voxel_filter(pts, leaf[cls], canonical=True) if several else pts
            n_merged += several
            g = got[cls][atlas.index_of(*(c + z for c, z in zip(key, (10, 10, 5))))]
            assert g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32)), (cls, key, several)
    assert n_merged == 2 and gpu.atlas_info()["cubes"] == [2, 3]
    gpu.close()


def test_many_sequences_share_one_atlas(binding, atlas, base):
    world = long_world(seed=8)
    d = base["drives"][0]
    offsets = [150.0 * (b - 8) for b in range(16)]                            # centre cubes 10 + 3 (b - 8): eleven of the sixteen windows must move, each elsewhere
    def run(B, slots):
        gpu = attached_context(binding, atlas, base, world, B=B)
        for b, s in enumerate(slots):
            p, fc = gpu.map_pose(b), gpu.map_info(b)["frame_count"]
            gpu.set_map_frame((10, 10, 5), p["q_wmap_wodom"], np.array(p["t_wmap_wodom"]) + np.array([offsets[s], 0, 0]), fc, seq=b)
        frame(gpu, [d[F]] * B, frozen=[True] * B)
        frame(gpu, [d[F + 1]] * B, frozen=[True] * B)
        gpu.synchronize()
        out = [dict(pose_part(binding, gpu, b), cubes=[{c: _sha(p) for c, p in cl.items()} for cl in cubes(gpu, b)]) for b in range(B)]
        nbytes = gpu.atlas_info()["device_bytes"]
        gpu.close()
        return out, nbytes
    many, bytes16 = run(16, range(16))
    for s in range(16):
        single, bytes1 = run(1, [s])
        assert not diff(many[s], single[0]), (s, diff(many[s], single[0]))
        assert bytes1 == bytes16 > 0                                          # one atlas, whatever the batch
    assert len({repr(m["cubes"]) for m in many}) > 8                          # different windows of the same atlas


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_atlas_states_and_errors(binding, atlas, base):
    world = long_world(seed=2)
    tiles, points = as_tiles(atlas, world)
    gpu = make(binding, base["model"], 2, _mp(base["drives"]), True, pool=1 << 12, pool_limit=1 << 16)
    d = base["drives"][0]

    def refused(code, call):
        with pytest.raises(binding.AloamError) as e:
            call()
        assert e.value.code == code

    refused(binding.E_STATE, lambda: gpu.atlas_attach([1, 0]))               # no atlas
    gpu.atlas_attach(None)
    bad = tiles.copy()
    bad["first_point"][3] = len(points)
    refused(binding.E_ARG, lambda: gpu.atlas_load(bad, points))
    bad = tiles.copy()
    bad["feature_class"][0] = 2
    refused(binding.E_ARG, lambda: gpu.atlas_load(bad, points))
    assert gpu.atlas_info()["tiles"] == 0                                     # nothing changed
    gpu.atlas_load(tiles, points)
    need = max(gpu.atlas_info()["largest_window"])
    assert need > (1 << 12) and gpu.map_pool_info()["pool_points"] == 1 << 12
    gpu.atlas_attach([1, 0])
    assert gpu.map_pool_info()["pool_points"] >= need                          # attach grew the pools
    gpu.load_sequences([0, 1], np.concatenate([base["blob"]] * 2), np.array([0, base["off"][1], 2 * base["off"][1]], np.int64))
    refused(binding.E_STATE, lambda: gpu.atlas_load(tiles[:0], points[:0]))   # unload while attached
    refused(binding.E_STATE, lambda: gpu.atlas_load(tiles, points))          # replace while attached
    gpu.synchronize()
    fc = gpu.map_info(0)["frame_count"]
    gpu.set_active([1, 1])
    gpu.scan_register([d[F], d[F]], check=False)
    gpu.odometry_step()
    gpu.set_map_frozen([0, 0])
    refused(binding.E_STATE, gpu.mapping_step)                                # attached, active, not frozen: nothing queued
    gpu.synchronize()
    assert gpu.map_info(0)["frame_count"] == fc and gpu.map_info(1)["frame_count"] == fc
    gpu.set_map_frozen([1, 0])
    gpu.mapping_step()
    gpu.synchronize()
    at = atlas.Atlas(tiles, points)
    assert window_is_the_cut(atlas, gpu, 0, at) > 0
    # aloam_set_map_frame re-cuts at the new cen; aloam_apply_map_corrections does not touch the window
    p, fc = gpu.map_pose(0), gpu.map_info(0)["frame_count"]
    gpu.set_map_frame((6, 13, 5), p["q_wmap_wodom"], p["t_wmap_wodom"], fc)
    frame(gpu, [d[F + 1], None], frozen=[True, False])
    gpu.synchronize()
    assert gpu.map_info(0)["cenW"] == 6 and window_is_the_cut(atlas, gpu, 0, at) > 0
    gpu.close()
    # the largest window above the pool limit: ALOAM_E_CAPACITY, nothing changed
    gpu = make(binding, base["model"], 1, _mp(base["drives"]), True, pool=1 << 12, pool_limit=1 << 12)
    gpu.atlas_load(tiles, points)
    refused(binding.E_CAPACITY, lambda: gpu.atlas_attach([1]))
    assert gpu.map_pool_info()["pool_points"] == 1 << 12
    gpu.close()


def test_kitti_runner_localizes_in_its_own_atlas_like_in_its_own_map(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = [sys.executable, os.path.join(root, "tools", "run_kitti.py"), "--selftest"]
    m, a = tmp_path / "map.npz", tmp_path / "atlas.npz"
    r = subprocess.run(tool + ["--mapping", "--out", str(tmp_path / "out"), "--save-map", str(m), "--save-atlas", str(a)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    outs = {}
    for name, opt, f in (("map", "--prior-map", m), ("atlas", "--prior-atlas", a)):
        r = subprocess.run(tool + ["--out", str(tmp_path / name), opt, str(f)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = ([l for l in r.stdout.splitlines() if "localized" in l], np.loadtxt(tmp_path / name / "00_localized.txt"))
    assert outs["map"][0] == outs["atlas"][0] and len(outs["map"][0]) >= 2     # the per-sweep errors that are printed
    assert np.array_equal(outs["map"][1], outs["atlas"][1])                    # the same map, so the same poses


# ---- merges beyond the LDS filter, in several rounds, and larger than a pool row -----------------------------------------------------------
def test_large_and_many_merges_go_through_the_general_filter_in_rounds(O, binding, atlas, base):
    rng = np.random.default_rng(21)
    cen = (10, 10, 5)
    def tile(cube, cls, n, half, frame):
        p = np.concatenate([np.array(cube) * 50.0 + rng.uniform(-half, half, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        idx = atlas.index_of(*(c + z for c, z in zip(cube, cen)))
        return atlas.tiles_of_window([{idx: p}, {}] if cls == 0 else [{}, {idx: p}], cen, frame)
    # 160 cubes of two small tiles each: more merge jobs than one round takes at batch 1 (2 x 75 segments) ...
    small = [(x, y, 0) for x in range(-8, 8) for y in range(-5, 5)]
    parts = [tile(c, 0, 30, 2.0, f) for f in (1, 2) for c in small]
    # ... and one cube of two tiles of 40000 points: above the 65536 points the single-workgroup filters take, and above the pool row
    parts += [tile((0, 0, 1), 1, 40000, 10.0, 1), tile((0, 0, 1), 1, 40000, 10.0, 2)]
    tiles, points = atlas.concatenate(parts)
    raw = atlas.Atlas(tiles, points)
    small_pool = make(binding, base["model"], 1, _mp(base["drives"]), True, pool=1 << 14, pool_limit=1 << 14)
    with pytest.raises(binding.AloamError) as e:
        small_pool.atlas_load(tiles, points)                                   # the concatenation exceeds the pool limit: refused, no atlas
    assert e.value.code == binding.E_CAPACITY and small_pool.atlas_info()["tiles"] == 0
    small_pool.close()
    gpu = make(binding, base["model"], 1, _mp(base["drives"]), True, pool=1 << 14, pool_limit=1 << 18)
    gpu.atlas_load(tiles, points)
    assert gpu.map_pool_info()["pool_points"] >= 80000                         # grown for the concatenation
    gpu.set_map_frozen([1])
    gpu.atlas_attach([1])
    frame(gpu, [base["drives"][0][0]], frozen=[True])
    gpu.synchronize()                                                         # (would raise if a filter had run out of scratch)
    got = cubes(gpu, 0)
    leaf = (0.4, 0.8)
    for cls in (0, 1):
        assert len(got[cls]) == len(raw.cubes[cls]) == (160, 1)[cls]
        for key, pts in raw.cubes[cls].items():
            want = O.voxel_filter(pts, leaf[cls], canonical=True)
            g = got[cls][atlas.index_of(*(c + z for c, z in zip(key, cen)))]
            assert g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32)), (cls, key)
    info = gpu.atlas_info()
    assert info["cubes"] == [160, 1] and info["points"] == [sum(len(p) for p in c.values()) for c in got]
    gpu.close()


# ---- score -> apply -> next frame on an attached sequence: the window is not cut again and the grid is kept -----------------------------------
import ctypes as C  # noqa: E402

import test_gpu_relocalize as RL  # noqa: E402

rec, reloc = RL.rec, RL.reloc                                                # the fixtures of the unattached twin of this test


def test_applied_candidate_on_an_attached_sequence_continues_like_set_map_frame_and_keeps_the_grid(binding, atlas, rec, reloc):
    import torch
    q, t, _ = RL.spread(reloc, rec, 32, seed=11)
    cand = binding.map_corrections(q[1:], t[1:])
    guess = RL.displaced(reloc, rec, 1.5, -1.0, 4.0)
    out = {}
    for how in ("apply", "set_map_frame"):
        g = RL.loaded(binding, rec, 1)
        g.atlas_load(*atlas.window_tiles(g, 0))                               # the atlas: the record's own window
        g.set_map_frozen([True])
        g.atlas_attach([True])
        g.set_map_frame(rec["cen"], guess[0], guess[1], rec["frame_count"])
        g.mapping_step()                                                      # cuts the window (stale), builds the grid
        sc = torch.zeros(len(cand) * 32, dtype=torch.uint8).pin_memory()
        best = torch.zeros(1, dtype=torch.int32).pin_memory()
        g.score_map_corrections_into([0], cand.ctypes.data, len(cand), sc.data_ptr(), best.data_ptr())
        one = torch.zeros(32, dtype=torch.uint8).pin_memory()
        again = lambda: binding.lib().aloam_score_map_corrections(g.h, (C.c_int * 1)(0), 1, C.c_void_p(cand.ctypes.data), 1, C.c_void_p(one.data_ptr()), None)
        if how == "apply":                                                    # the host reads nothing back in between
            g.apply_map_corrections_from([0], cand.ctypes.data, len(cand), best.data_ptr())
            assert again() == 0                                               # not marked stale: still scorable
        else:
            g.synchronize()
            i = g.map_info(0)
            w = int(best[0])
            g.set_map_frame((i["cenW"], i["cenH"], i["cenD"]), cand[w]["q_wmap_wodom"], cand[w]["t_wmap_wodom"], i["frame_count"])
            assert again() == binding.E_STATE                                 # marked stale and invalidated: the next step cuts and builds anew
        g.scan_register([rec["scans"][RL.F + 1]], check=False)
        g.odometry_step()
        g.profile_enable(True)
        g.mapping_step()
        g.synchronize()
        prof = g.profile()
        out[how] = dict(part=pose_part(binding, g, 0), snap=snap(binding, g, 0, True), best=int(best[0]), grid_ms=prof["map_grid"]["total_ms"],
                        begin_ms=prof["map_begin"]["total_ms"], scores=sc.numpy().tobytes())
        g.profile_enable(False)
        g.close()
    a, b = out["apply"], out["set_map_frame"]
    assert a["best"] == b["best"] and a["scores"] == b["scores"]
    assert not diff(a["part"], b["part"]) and not diff(a["snap"], b["snap"]), (diff(a["part"], b["part"]), diff(a["snap"], b["snap"]))
    print(f"attached, step after: applied map_grid {a['grid_ms']:.4f} ms / map_begin {a['begin_ms']:.4f} ms; set_map_frame {b['grid_ms']:.4f} / {b['begin_ms']:.4f} ms")
    assert a["grid_ms"] < b["grid_ms"], (a["grid_ms"], b["grid_ms"])           # apply: MapGridSig left alone, the grid is reused; set_map_frame: re-cut and rebuilt
