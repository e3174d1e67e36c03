"""Place recognition, the numpy model alone (no GPU, no library): scan-context descriptors of a 300 m street drive find the stored place
and the yaw of queries rendered aside of it and turned; the sign convention of the shift; and the input checks the GPU tests rely on."""
import importlib
import math

import numpy as np
import pytest
import torch

import places_common as pc
from places_common import MATCH_DRIVE, MATCH_T, db_slots, kept, query_slots
from test_registration_models import exact_angle, ring_from_angle

pl = importlib.import_module("a-loam_amd.places")

QUERY_FRAMES = (21, 55, 97, 131, 171)
MOVES = ((0.0, 0.0), (1.5, 30.0), (-2.0, 180.0))         # metres sideways (the sensor's +y), degrees of extra yaw


def _rz(deg):
    a = math.radians(deg)
    return torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


@pytest.fixture(scope="module")
def street(syn):
    world = syn.make_street_world(7)
    R, t = syn.trajectory_travel(200, 1.6, seed=7)
    model = syn.sensor_model("HDL-64", columns=512)
    gen = torch.Generator().manual_seed(77 + 7)

    def render(Rk, tk):
        s = syn.render_scan(world, model, Rk, tk, 0.02, gen, max_range=syn.STREET_MAX_RANGE, cull=True).numpy()
        return pl.scan_context(kept(s, model.min_range))
    db = np.stack([render(R[k], t[k]) for k in range(0, 200, 2)])
    return R, t, db, render


def test_moved_and_turned_queries_find_their_place_and_yaw(street):
    R, t, db, render = street
    for k in QUERY_FRAMES:
        far = np.abs(2 * np.arange(len(db)) - k) > 8
        for side, yaw in MOVES:
            q = render(R[k] @ _rz(yaw), t[k] + R[k] @ torch.tensor([0.0, side, 0.0], dtype=torch.float64))
            ent, sh, di = pl.match(q, db, 1)
            d_far = pl.match(q, db[far], 1)[2][0]
            print(f"frame {k} side {side:+.1f} m yaw {yaw:5.1f} deg: entry {ent[0]} (frame {2 * ent[0]}) shift {sh[0]} d {di[0]:.3f}; best entry > 8 frames away {d_far:.3f}")
            assert abs(2 * int(ent[0]) - k) <= 2, (k, side, yaw, ent, di)
            want = round(yaw / pl.SECTOR_DEG) % pl.SECTORS
            assert min((int(sh[0]) - want) % pl.SECTORS, (want - int(sh[0])) % pl.SECTORS) <= 1, (k, side, yaw, sh)


def test_a_query_with_thirty_degrees_of_extra_yaw_matches_with_shift_five():
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((40000, 3)) * [25.0, 25.0, 1.5]).astype(np.float32)
    a = math.radians(30.0)                               # the sensor turned by +30 deg sees every point 30 deg further clockwise
    q = p.copy()
    q[:, 0] = (math.cos(a) * p[:, 0] + math.sin(a) * p[:, 1]).astype(np.float32)
    q[:, 1] = (-math.sin(a) * p[:, 0] + math.cos(a) * p[:, 1]).astype(np.float32)
    d, shift = pl.distance(pl.scan_context(q), pl.scan_context(p))
    assert shift == 5 and d < 0.02, (d, shift)
    # and the guess puts the sensor at the stored pose turned by +30 deg about its own z
    qc, tc = pl.guess_from_match([0, 0, 0, 1], [4.0, -2.0, 0.5], shift, [0, 0, 0, 1], [0, 0, 0])
    assert np.allclose(qc, [0, 0, math.sin(a / 2), math.cos(a / 2)]) and np.allclose(tc, [4.0, -2.0, 0.5])
    # an odometry pose that is not the identity is taken out again: map pose = correction * odometry pose
    oq, ot = np.array([0, 0, math.sin(0.2), math.cos(0.2)]), np.array([1.0, 2.0, 3.0])
    qc, tc = pl.guess_from_match([0, 0, 0, 1], [4.0, -2.0, 0.5], 0, oq, ot)
    from importlib import import_module
    rl = import_module("a-loam_amd.relocalize")
    assert np.allclose(rl._qmul(qc, oq), [0, 0, 0, 1]) and np.allclose(rl._qrot(qc, ot) + tc, [4.0, -2.0, 0.5])


def test_distance_rules():
    rng = np.random.default_rng(5)
    c = rng.random((pl.RINGS, pl.SECTORS)).astype(np.float32)
    c[:, 10:20] = 0
    assert pl.distance(c, c) == (pytest.approx(0.0, abs=1e-12), 0)
    d, s = pl.distance(np.roll(c, 7, axis=1), c)         # the stored place seen 7 sectors turned: Q[:, j] = C[:, j + 7] -> shift -7
    assert s == (pl.SECTORS - 7) and d == pytest.approx(0.0, abs=1e-12)
    assert pl.distance(np.zeros_like(c), c) == (math.inf, -1)
    ent, sh, di = pl.match(c, np.stack([c * 0, c, c]), 3)
    assert ent.tolist() == [1, 2, -1] and sh.tolist() == [0, 0, -1]      # ties rank by index; an entry without a valid shift is left out


def test_gpu_match_inputs_are_well_separated(sequence):
    """Input check of test_gpu_places.py: on every query it uses, consecutive entries among the model's T + 1 best differ by more than
    2e-4 in distance, twenty times the bound on the device's f32 error (1e-5): the device cannot rank them otherwise for a legitimate
    reason.  If this fails, change the seed of places_common.MATCH_DRIVE, not the tolerance."""
    kw = dict(MATCH_DRIVE)
    scans, R, t, model = sequence(kw.pop("name"), kw.pop("frames"), **kw)
    desc = np.stack([pl.scan_context(kept(s, model.min_range)) for s in scans])
    db = desc[db_slots()]
    for b in query_slots():
        d = np.sort(pl.shift_distances(desc[b], db).min(axis=1))[:MATCH_T + 1]
        assert np.all(np.diff(d) > 2e-4), (b, d)


def test_border_exception_is_rare_on_the_model_side(sequence):
    """At most 12 of a sweep's 1200 cells may depend on points within 4 ulp of a sector border (2 - 3 such points per 131 k-point sweep are
    expected): the cap the GPU descriptor test allows for, asserted on the sweeps it uses."""
    for name, cols, seed in (("HDL-64", 2048, 31), ("VLP-16", 600, 5)):
        scans, R, t, model = sequence(name, 2, seed=seed, columns=cols)
        for s in scans:
            lo, hi = pl.scan_context_bounds(kept(s, model.min_range))
            assert int((lo != hi).sum()) <= 12, (name, int((lo != hi).sum()))


# ---- input checks of test_gpu_places_edges.py -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_inputs(sequence, syn):
    """What the GPU test builds from the device's exported descriptors, built here from the model's."""
    kw = dict(MATCH_DRIVE)
    scans, R, t, model = sequence(kw.pop("name"), kw.pop("frames"), **kw)

    def desc(sweep):
        return pl.scan_context(kept(sweep, model.min_range))
    Qa, Qb = desc(scans[pc.DRIVE_FRAME_A]), desc(scans[pc.DRIVE_FRAME_B])
    P, S, F = desc(pc.periodic_sweep(model)), desc(pc.single_column_sweep(model)), desc(pc.few_column_sweep(model))
    main, kinds, dup = pc.edge_store(Qa, P, S)
    blocks = {"main": (main, kinds), "Z": pc.sparse_block(pc.Z_N, pc.Z_ROLLS, pc.Z_DUPS, Qa, dup), "W": pc.sparse_block(pc.W_N, pc.W_ROLLS, (), Qa, dup),
              "V": pc.separated_block(Qb)}
    return model, dict(Qa=Qa, Qb=Qb, P=P, S=S, F=F), blocks


def test_edge_store_puts_every_kind_in_every_wave_and_three_tiles(edge_inputs):
    model, Q, blocks = edge_inputs
    cells, kinds = blocks["main"]
    assert len(cells) == pc.EDGE_N == 3 * 128 + 37
    where = {}
    for i, (name, par) in enumerate(kinds):
        where.setdefault(name, []).append(i)
        where.setdefault((name, par), []).append(i)
    assert set(n for n in where if isinstance(n, str)) == {"roll", "noisy", "periodic", "fewcol", "single", "nomeet", "zero", "dup", "scaled", "random"}
    for name, idx in where.items():
        if isinstance(name, str) and name != "scaled":
            tw = [pc.tile_wave(i) for i in idx]
            assert {w for _, w in tw} == {0, 1, 2, 3} and len({t for t, _ in tw}) >= 3, (name, tw)
    for k in range(pl.SECTORS):                              # every roll at two indices that differ in wave and in tile
        a, b = where[("roll", k)]
        assert np.array_equal(cells[a], np.roll(Q["Qa"], k, axis=1)) and np.array_equal(cells[a], cells[b])
        assert pc.tile_wave(a)[0] != pc.tile_wave(b)[0] and pc.tile_wave(a)[1] != pc.tile_wave(b)[1], (k, a, b)
    dup = where["dup"]
    assert len(dup) == 12 and all(np.array_equal(cells[dup[0]], cells[i]) for i in dup)
    assert {par for name, par in kinds if name == "fewcol"} == {1, 2, 3}
    for i in where["fewcol"]:
        assert int(cells[i].any(axis=0).sum()) == kinds[i][1]
    for i in where["single"]:
        assert np.flatnonzero(cells[i].any(axis=0)).tolist() == [(pc.SINGLE_SECTOR + kinds[i][1]) % pl.SECTORS]
    for i in where["zero"]:
        assert not cells[i].any()
    # some entries never meet a column of the few-column query at some shifts, and do at others
    d = pl.shift_distances(Q["F"], cells[where["nomeet"]])
    assert np.all(np.isinf(d).any(axis=1) & np.isfinite(d).any(axis=1))
    # what a load accepts: finite, non-negative, positive cells inside [CELL_MIN, CELL_MAX]; the scaled records reach towards both ends
    for c, _ in blocks.values():
        assert np.all(np.isfinite(c)) and np.all(c >= 0) and np.all((c[c > 0] >= pc.CELL_MIN) & (c[c > 0] <= pc.CELL_MAX))
    lo, hi = (cells[where[("scaled", s * pc.SCALE_LOG2)][0]] for s in (-1, 1))
    assert 0 < lo[lo > 0].min() < 1e-16 and hi.max() > 1e15
    assert np.array_equal(lo * np.float32(2.0 ** pc.SCALE_LOG2), np.roll(Q["Qa"], pc.SCALED_ROLL, axis=1))
    # the sparse blocks: valid records in all four waves and at least three tiles of the ranges the GPU test takes
    z = sorted(list(pc.Z_ROLLS) + list(pc.Z_DUPS))
    assert {pc.tile_wave(p)[1] for p in z} == {0, 1, 2, 3} and {pc.tile_wave(p)[0] for p in z} == {0, 1, 2, 3}
    assert {pc.tile_wave(p - 128) for p in pc.Z_DUPS} == {(0, 0), (0, 1), (1, 2), (2, 1)}
    zc, zk = blocks["Z"]
    assert sorted(np.flatnonzero(zc.any(axis=(1, 2))).tolist()) == z and len(zc) == pc.Z_N
    wc, wk = blocks["W"]
    assert len(wc) == 303 and int(wc.any(axis=(1, 2)).sum()) == 3 and {pc.tile_wave(p) for p in pc.W_ROLLS} == {(0, 2), (1, 1), (2, 1)}
    assert max(pc.W_ROLLS) >= 256                            # the select loop's second pass
    assert pc.EDGE_TOTAL == 421 + 12 + 437 + 303 + 40


def test_periodic_sweep_ties_shift_k_with_k_plus_thirty(edge_inputs):
    model, Q, blocks = edge_inputs
    P = Q["P"]
    assert np.array_equal(P[:, :30].view(np.uint32), P[:, 30:].view(np.uint32))
    cols = P.any(axis=0)
    assert [s for s in range(30) if not cols[s]] == list(pc.EMPTY_COLUMNS) and not P[0].any() and P[1:].any(axis=1).all()
    assert len({P[:, s].tobytes() for s in range(30) if cols[s]}) == 28           # no shorter period
    lower = []
    for k in pc.TIE_KS:
        d = pl.shift_distances(P, np.roll(P, k, axis=1)[None])[0]
        s = k % 30
        assert d[s] == d[s + 30] and int(np.argmin(d)) == s and d[s] < 1e-12, (k, d[s], d[s + 30])
        assert np.sort(d)[2] > 1e-3, (k, np.sort(d)[:4])                              # every other shift is far off
        lower.append(s)
    crossing = [s for s in lower if s < 32 <= s + 30]
    assert {pc.h_of_shift(s) for s in crossing} == {0, 1}                             # the lower shift in either half of the lanes
    assert {(pc.h_of_shift(s), pc.h_of_shift(s + 30)) for s in crossing} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # the tie inside a lane and across lanes
    assert any(s + 30 < 32 for s in lower)                                            # and one tie inside the first accumulator


def test_crafted_queries_are_what_they_claim(edge_inputs, syn):
    model, Q, blocks = edge_inputs
    assert np.flatnonzero(Q["S"].any(axis=0)).tolist() == [pc.SINGLE_SECTOR] and int((Q["S"] > 0).sum()) >= 15
    assert np.flatnonzero(Q["F"].any(axis=0)).tolist() == list(pc.FEW_SECTORS)
    for sweep in (pc.low_sweep(model), pc.far_sweep(model)):
        p = kept(sweep, model.min_range)
        assert len(p) == len(sweep) and not pl.scan_context(p).any()
    assert np.all(pc.low_sweep(model)[:, 2] + np.float32(2.0) <= 0) and np.all(np.hypot(*pc.far_sweep(model)[:, :2].T) > 80.0)
    # single-column entries against the single-column query: cnt = 1 and exactly one valid shift, the one in the record's name
    cells, kinds = blocks["main"]
    for i, (name, s) in enumerate(kinds):
        if name == "single":
            d = pl.shift_distances(Q["S"], cells[i][None])[0]
            assert np.flatnonzero(np.isfinite(d)).tolist() == [s] and 1e-4 < d[s] < 0.2, (i, s, d[s])


def test_f32_restatement_stays_near_the_f64_model(edge_inputs):
    """eps_ref, the rounding error of a plain f32 evaluation of the documented arithmetic, over the whole adversarial store: the GPU tests
    allow the device 8 eps_ref, which must stay well inside the project's derived bound of 1e-4."""
    model, Q, blocks = edge_inputs
    store = np.concatenate([blocks[b][0] for b in ("main", "Z", "W", "V")])
    store = store[store.any(axis=(1, 2))]
    eps = pc.eps_ref([Q[n] for n in ("Qa", "Qb", "P", "S", "F")], store)
    print(f"eps_ref over {len(store)} non-zero entries x 5 queries x 60 shifts: {eps:.3e}; tol = 8 eps_ref = {8 * eps:.3e}")
    assert 0 < eps < 1e-4 / 8 / 4


def test_graded_block_and_rolled_entries_are_separated_where_equality_is_asserted(edge_inputs):
    model, Q, blocks = edge_inputs
    tol = 8 * pc.eps_ref([Q["Qa"], Q["Qb"]], np.concatenate([blocks["main"][0][:60], blocks["V"][0]]))
    d = pl.shift_distances(Q["Qb"], blocks["V"][0])
    best = np.sort(d.min(axis=1))
    assert np.all(np.diff(best) > 2 * tol) and np.all(np.diff(best)[:9] > 1e-5), np.diff(best)[:9]
    ranks = np.argsort(d.min(axis=1))
    assert ranks[:9].tolist() != sorted(ranks[:9].tolist())                          # the rank goes with the noise, not with the position
    two = np.sort(d, axis=1)[:, :2]
    assert np.all(two[:, 1] - two[:, 0] > 2 * tol)                                    # and the best shift of each is separated too
    # every roll of the drive descriptor: the best shift is k against the drive query, and no other shift comes within 2 tol
    cells, kinds = blocks["main"]
    for i, (name, k) in enumerate(kinds):
        if name in ("roll", "noisy", "scaled", "dup"):
            d = pl.shift_distances(Q["Qa"], cells[i][None])[0]
            k = pc.SCALED_ROLL if name == "scaled" else k
            assert int(np.argmin(d)) == k and np.sort(d)[1] - d[k] > 2 * tol, (i, name, k)


def front_end_rings(pts, R):
    """The ring the front end gives each point (-1: dropped), required to be the same 1e-3 degrees below and above the point's angle."""
    out = []
    for x, y, z in np.asarray(pts, np.float32):
        a = exact_angle(x, y, z)
        got = {ring_from_angle(a + d, R) for d in (np.float32(-1e-3), np.float32(0), np.float32(1e-3))}
        out.append(got.pop() if len(got) == 1 else -1)
    return np.array(out)


def test_scan_registration_keeps_every_crafted_point(syn):
    """A crafted sweep must reach the descriptor whole: every point passes the range filter and gets a ring, away from the decision's limits."""
    model = syn.sensor_model(MATCH_DRIVE["name"], columns=MATCH_DRIVE["columns"])
    for sweep in (pc.periodic_sweep(model), pc.single_column_sweep(model), pc.few_column_sweep(model), pc.low_sweep(model), pc.far_sweep(model)):
        assert len(kept(sweep, model.min_range)) == len(sweep) and np.all(front_end_rings(sweep, model.n_scans) >= 0)


@pytest.mark.parametrize("name,max_range,height,empty", [("HDL-64", 80.0, 2.0, 5), ("HDL-64", 50.0, 0.0, 3)])
def test_edge_sweep_meets_the_edges_it_names(syn, name, max_range, height, empty):
    model = syn.sensor_model(name, columns=512)
    pts, edges, expect = pc.edge_sweep(model, max_range, height, empty_ring=empty)
    p = kept(pts, model.min_range)
    assert len(p) == len(pts)                                                         # nothing falls to the range filter
    f = np.float32
    # each point's elevation is a ring's: the reference's ring decision accepts it, and ring `empty` gets no point
    el = pc.ring_elevations(model)
    ang = np.degrees(np.arctan(pts[:, 2].astype(np.float64) / np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))))
    ring = np.argmin(np.abs(ang[:, None] - el[None]), axis=1)
    near = np.abs(ang - el[ring])
    floor = [edges["z_at_floor"], edges["z_above_floor"]]
    assert np.all(np.delete(near, floor) < 1e-3) and np.all(near[floor] < 1e-3) and not np.any(ring == empty)
    assert np.array_equal(front_end_rings(pts, model.n_scans), ring) and np.any(np.abs(ring - empty) == 1)   # `empty` lies among the rings in use
    keep, r, s = pl._cell_indices(pts, max_range)
    x, y = pts[edges["rho_at_max"], :2]
    assert np.sqrt(x * x + y * y) == f(max_range) and r[edges["rho_at_max"]] == pl.RINGS and not keep[edges["rho_at_max"]]
    x, y = pts[edges["rho_below_max"], :2]
    assert np.sqrt(x * x + y * y) == np.nextafter(f(max_range), f(0)) and r[edges["rho_below_max"]] == pl.RINGS - 1
    assert np.signbit(pts[edges["minus_x_minus_zero"], 1]) and not np.signbit(pts[edges["minus_x_plus_zero"], 1]) and pts[edges["minus_x_plus_zero"], 1] == 0
    raw = (np.arctan2(pts[:, 1], pts[:, 0]).astype(f) + f(np.pi)) * f(60.0 / (2.0 * math.pi))
    assert int(raw[edges["minus_x_plus_zero"]]) == pl.SECTORS                         # sector 60 before the clamp
    assert pts[edges["z_at_floor"], 2] + f(height) == 0 and 0 < pts[edges["z_above_floor"], 2] + f(height) < 1e-6
    D = pl.scan_context(p, max_range, height)
    for n, (c, sec, v) in expect.items():
        i = edges[n]
        if v is None:
            assert not keep[i] or D[r[i], s[i]] == 0, n
        else:
            assert keep[i] and (int(r[i]), int(s[i])) == (c, sec) and D[c, sec] == f(v) and D[c, sec] > 0, (n, c, sec, v, r[i], s[i], D[c, sec])
    lo, hi = pl.scan_context_bounds(p, max_range, height)
    assert np.array_equal(lo, hi) and np.array_equal(lo, D)
    assert int((D > 0).sum()) > 60
