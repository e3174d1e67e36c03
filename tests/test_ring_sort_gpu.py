"""The run-key sort of k_ring_features (bitonic_sort_blocked: every half-cleaner register-blocked, 32- and 64-bit keys) on rings built for it.

Ring ids come from the field (`ring_from_field=True`), so every ring's points are chosen freely:
  * "own run" rings: points 0.3 m apart along a slowly tightening spiral of radius ~100 m.  Consecutive points differ by more than
    0.2 m along x or y, so every member is a run of its own; the curvature stays below 0.1, so no point is taken as a corner and
    all n - 11 elements are members: the run count is chosen exactly (5, 8, 9, the powers of two 256 / 512 / 1024 and their
    neighbours, the full 2048; the ring of 5 runs has six elements, one of them on top of its predecessor);
  * a ring that re-enters voxels: blocks A A B A B B across a cell border, so a voxel has several runs and its members must
    still be summed in input order;
  * a ring whose box has more than 2^21 cells (64-bit keys), a ring on pcl::VoxelGrid's overflow path (box beyond
    2^31 cells: the members come back unfiltered), and one ring of 3011 points for the <4096> instance.
What each input really is (runs, voxels, cells of the box) is counted from the oracle's labels in `ring_facts`, without the GPU;
the GPU tests then compare all four feature clouds and the full cloud bit for bit with the oracle in canonical order.
"""
import numpy as np
import pytest
from conftest import bits_equal

FEATURES = ("cloud", "sharp", "less_sharp", "flat", "less_flat")
RINGS = 8
OWN_RUNS = [5, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048]


def spiral(n, ring, r0=100.0, d=0.3, z=0.0):
    """n points d apart, azimuth falling from pi, radius r0 shrinking by 27.5 m per turn"""
    th, out = np.pi, np.zeros((n, 4), np.float64)
    for i in range(n):
        r = r0 - 27.5 * (np.pi - th) / (2 * np.pi)
        out[i] = (r * np.cos(th), r * np.sin(th), z, ring)
        th -= d / r
    return out.astype(np.float32)


def five_runs(ring):
    """a ring needs six elements to be looked at: one of the six sits on its predecessor and shares its voxel"""
    p = spiral(17, ring)
    p[8, :3] = p[7, :3] + np.float32(0.001)
    return p


def reentering(ring, blocks=300, seed=3):
    """A A B A B B per pair of neighbouring 0.2 m cells along x at y = 30 m: both voxels of a block are left and entered again"""
    rng = np.random.default_rng(seed)
    pts = []
    for m in range(blocks):
        xa = -60.0 + 0.4 * m
        for cell in (0, 0, 1, 0, 1, 1):
            pts.append((xa + 0.2 * cell + rng.uniform(0.02, 0.18), 30.0 + rng.uniform(0.02, 0.18), rng.uniform(0.02, 0.18), ring))
    return np.array(pts, np.float32)


def big_box(ring, n=700):
    """helix of radius 30 m climbing 12 m: 300 x 300 x 60 cells > 2^21"""
    p = spiral(n, ring, r0=30.0)
    p[:, 2] = np.linspace(-6.0, 6.0, n, dtype=np.float32)
    return p


def overflowing(ring, n=1200):
    """200 points of the ring at 3e5 m: the box exceeds 2^31 cells, pcl::VoxelGrid returns its input"""
    rng = np.random.default_rng(0)
    ang = np.linspace(np.pi, -np.pi, n, endpoint=False)
    rad = 10 + 3 * np.sign(np.sin(6 * ang)) + rng.normal(size=n) * 0.02
    rad[300:500] = 3.0e5
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), np.tan(np.deg2rad(1.0)) * rad, np.full(n, ring)], 1).astype(np.float32)


def sweeps():
    """three sweeps of eight rings each: the thirteen own-run rings, then the special ones and three more lengths off the tile sizes"""
    kinds = [("five", 5)] + [("own", c) for c in OWN_RUNS[1:]] + [("reenter", 0), ("bigbox", 0), ("overflow", 0), ("own", 63), ("own", 65), ("own", 842), ("own", 2047),
                                              ("own", 129), ("own", 1500), ("own", 17), ("own", 16)]
    assert len(kinds) == 3 * RINGS
    out = []
    for s in range(3):
        rings = []
        for r in range(RINGS):
            kind, c = kinds[s * RINGS + r]
            rings.append(spiral(c + 11, r) if kind == "own" else five_runs(r) if kind == "five" else reentering(r) if kind == "reenter" else big_box(r) if kind == "bigbox" else overflowing(r))
        out.append((np.concatenate(rings), kinds[s * RINGS:(s + 1) * RINGS]))
    return out


def ring_facts(orc, fo):
    """per ring, from the oracle's cloud and labels alone: members, runs, occupied voxels and cells of the members' box"""
    starts, counts = orc.ring_ranges()
    _, lab, _ = orc.per_point()
    inv = np.float32(1.0) / np.float32(0.2)
    facts = []
    for s0, c0 in zip(starts, counts):
        L = c0 - 11
        if L < 6:
            facts.append(None); continue
        pts, member = fo["cloud"][s0 + 5:s0 + 5 + L, :3], lab[s0 + 5:s0 + 5 + L] <= 0
        cell = np.floor(pts * inv).astype(np.int64)
        differs = np.ones(L, bool)
        differs[1:] = (cell[1:] != cell[:-1]).any(1) | ~member[:-1]
        ext = cell[member].max(0) - cell[member].min(0) + 1
        facts.append({"members": int(member.sum()), "runs": int((member & differs).sum()), "voxels": len(np.unique(cell[member], axis=0)),
                      "box_cells": int(ext[0]) * int(ext[1]) * int(ext[2])})
    return facts


_REF = {}


def reference(O):
    """oracle features and ring facts of the three sweeps and of the long ring, computed once"""
    if not _REF:
        for name, (x, kinds) in list(zip("012", sweeps())) + [("long", (spiral(3011, 0), [("own", 3000)]))]:
            orc = O.Oracle(n_scans=RINGS, min_range=0.3, ring_from_field=True)
            fo = orc.scan_register(x)
            _REF[name] = (x, kinds, fo, ring_facts(orc, fo))
    return _REF


def test_inputs_are_what_they_claim(O):
    """CPU only: run counts, multi-run voxels and key widths of every ring, from the oracle's labels"""
    ref = reference(O)
    seen = []
    for name in "012":
        _, kinds, fo, facts = ref[name]
        per_ring = np.bincount(np.rint(fo["less_flat"][:, 3]).astype(np.int32), minlength=RINGS)
        for r, ((kind, c), f) in enumerate(zip(kinds, facts)):
            if kind == "five":
                assert f["runs"] == 5 and f["box_cells"] <= 1 << 21, (name, r, f)
                seen.append(5)
            elif kind == "own":
                assert f["members"] == c and f["runs"] == c and f["voxels"] == c and per_ring[r] == c, (name, r, c, f)
                assert f["box_cells"] <= 1 << 21, (name, r, f)                # 32-bit keys
                seen.append(c)
            elif kind == "reenter":
                assert f["runs"] > 1.3 * f["voxels"] and f["runs"] > 700 and f["box_cells"] <= 1 << 21 and per_ring[r] == f["voxels"], f
            elif kind == "bigbox":
                assert 1 << 21 < f["box_cells"] < 1 << 31 and f["runs"] > 400 and per_ring[r] == f["voxels"], f   # 64-bit keys
            else:
                assert f["box_cells"] > 1 << 31 and per_ring[r] == f["members"] > 1000, f                        # unfiltered
    assert set(OWN_RUNS) <= set(seen)
    _, _, fo, facts = ref["long"]
    assert facts[0]["runs"] == 3000 and facts[0]["voxels"] == 3000 and facts[0]["box_cells"] <= 1 << 20, facts[0]   # <4096>: 12 element bits, 32-bit keys up to 2^20 cells


def _assert_features_equal(fo, fg, ctx):
    for k in FEATURES:
        assert fo[k].shape == fg[k].shape, (ctx, k, fo[k].shape, fg[k].shape)
        assert bits_equal(fo[k], fg[k]), (ctx, k)


@pytest.mark.gpu
def test_ring_sort_run_counts_widths_and_paths(O, binding):
    """batch 3 x 8 rings through k_ring_features<2048>: every cloud of every sequence bit-equal to the oracle"""
    ref = reference(O)
    xs = [ref[name][0] for name in "012"]
    gpu = binding.Aloam(n_scans=RINGS, min_range=0.3, ring_from_field=True, batch=3, max_points=max(len(x) for x in xs) + 64,
                        max_ring_points=2059)                                # the default capacity, 4107, is the <4096> instance
    gpu.scan_register(xs)
    for b, name in enumerate("012"):
        _assert_features_equal(ref[name][2], gpu.features(b), ("sweep", name))
    gpu.close()


@pytest.mark.gpu
def test_long_ring_instance_with_3000_runs(O, binding):
    """k_ring_features<4096> (max_ring_points 4107): 3000 runs, 32-bit keys, two rounds of every register-blocked pass and the S = 512 level"""
    x, _, fo, _ = reference(O)["long"]
    gpu = binding.Aloam(n_scans=RINGS, min_range=0.3, ring_from_field=True, batch=2, max_points=4096, max_ring_points=4107)
    gpu.scan_register([x, x[:1511]])                                         # the second sequence: 1500 runs in the same instance
    _assert_features_equal(fo, gpu.features(0), "long ring")
    orc = O.Oracle(n_scans=RINGS, min_range=0.3, ring_from_field=True)
    _assert_features_equal(orc.scan_register(x[:1511]), gpu.features(1), "long ring, first half")
    gpu.close()
