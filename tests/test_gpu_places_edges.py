"""Place recognition on the MI355X beyond one wave, one tile and small shifts: a loaded store of 1213 crafted records (places_common.py) puts
every kind of entry in all four waves and all four tiles of k_place_match, every shift 0 .. 59 at the top of a result, bit-for-bit ties
between shifts 30 apart, ranges that start anywhere, more than 256 entries under k_place_select, empty and single-column queries; and
crafted sweeps put k_place_descriptor at its edges with no border exception.

The reference is the float64 model (a-loam_amd/places.py) fed with the descriptors the device exported.  The tolerance is 8 eps_ref, where
eps_ref is the error of a plain float32 evaluation of the documented arithmetic over the same store and queries
(places_common.shift_distances_f32): the factor covers the undocumented grouping of the two K products of v_mfma_f32_32x32x2_f32.  Every
test prints eps_ref, the tolerance and the device's worst deviation so far."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import places_common as pc
from places_common import MATCH_DRIVE
from test_gpu_checkpoint import make

pytestmark = pytest.mark.gpu
pl = importlib.import_module("a-loam_amd.places")
T = 8


def _cells(rec):
    return np.swapaxes(rec["cells"], -1, -2)


def _records(binding, cells):
    rec = np.zeros(len(cells), binding.PLACE_DTYPE)
    rec["cells"] = np.swapaxes(cells, -1, -2)
    rec["q"][:, 3] = 1.0
    rec["slot"], rec["frame"] = -1, -1
    return rec


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _run(E, slots, ranges, check=True, pinned=True, T=T):
    """One aloam_places_match call: every row passes check_match, and every returned (entry, shift, distance bits) is the one the
    width-8 readback of the store gave for that (slot, entry).  check=False: the readback itself, as the fixture takes it."""
    res = E.gpu.places_match(slots, ranges, T, pinned=pinned)
    for i, (b, (lo, hi)) in enumerate(zip(slots, ranges)):
        if check:
            E.worst = max(E.worst, pc.check_match(res[i], E.desc[b], E.cells[lo:hi], lo, T, E.tol, d64=E.d64[b][lo:hi]))
            for r in res[i]:
                if r["entry"] >= 0:
                    e = int(r["entry"])
                    assert (int(_bits(r["distance"])), int(r["shift"])) == (int(E.bits[b][e]), int(E.shift[b][e])), (b, lo, hi, r, E.kinds[e])
    return res


def _readback(E, offset, check=True):
    """(distance bits [slot][entry], shift [slot][entry]; shift -1 = not returned) from ranges eight wide, every slot listed in every call."""
    N, B = len(E.cells), pc.EDGE_BATCH
    bits, shift = np.zeros((B, N), np.uint32), np.full((B, N), -1, np.int64)
    starts = ([0] if offset else []) + list(range(offset, N, T))
    for lo in starts:
        hi = offset if (offset and lo == 0) else min(lo + T, N)
        res = _run(E, list(range(B)), [(lo, hi)] * B, check=check)
        for b in range(B):
            for r in res[b]:
                if r["entry"] >= 0:
                    bits[b, r["entry"]], shift[b, r["entry"]] = _bits(r["distance"]), r["shift"]
    return bits, shift


def _report(E, what):
    print(f"{what}: eps_ref {E.eps:.3e}, tol = 8 eps_ref {E.tol:.3e}, worst |device - f64 model| so far {E.worst:.3e}")
    assert E.worst <= E.tol <= 1e-4


@pytest.fixture(scope="module")
def E(binding, sequence):
    kw = dict(MATCH_DRIVE)
    scans, R, t, model = sequence(kw.pop("name"), kw.pop("frames"), **kw)
    sweeps = [None] * pc.EDGE_BATCH
    for b in pc.SLOT_A:
        sweeps[b] = scans[pc.DRIVE_FRAME_A]
    sweeps[pc.SLOT_B] = scans[pc.DRIVE_FRAME_B]
    sweeps[pc.SLOT_PERIODIC], sweeps[pc.SLOT_SINGLE], sweeps[pc.SLOT_FEW] = pc.periodic_sweep(model), pc.single_column_sweep(model), pc.few_column_sweep(model)
    sweeps[pc.SLOT_LOW], sweeps[pc.SLOT_FAR] = pc.low_sweep(model), pc.far_sweep(model)
    edge_pts, edge_rows, edge_expect = pc.edge_sweep(model)
    sweeps[pc.SLOT_EDGES] = edge_pts
    sweeps = [np.ascontiguousarray(s[:, :3], dtype=np.float32) for s in sweeps]
    gpu = make(binding, model, pc.EDGE_BATCH, max(len(s) for s in sweeps) + 64, False)
    gpu.places_enable(pc.EDGE_TOTAL + 2)
    gpu.scan_register(sweeps, check=True)
    # the queries' descriptors first: the records are made of them
    assert gpu.places_add(range(pc.EDGE_BATCH)) == 0
    own = gpu.places_export()
    desc = [_cells(own[b]).copy() for b in range(pc.EDGE_BATCH)]
    gpu.places_clear()
    Qa, Qb = desc[pc.SLOT_A[0]], desc[pc.SLOT_B]
    main, kinds, dup = pc.edge_store(Qa, desc[pc.SLOT_PERIODIC], desc[pc.SLOT_SINGLE])
    blocks = [pc.sparse_block(pc.Z_N, pc.Z_ROLLS, pc.Z_DUPS, Qa, dup), pc.sparse_block(pc.W_N, pc.W_ROLLS, (), Qa, dup), pc.separated_block(Qb)]
    assert gpu.places_load(_records(binding, main)) == pc.MAIN0
    assert gpu.places_add(range(pc.EDGE_BATCH)) == pc.OWN0
    assert gpu.places_load(_records(binding, np.concatenate([c for c, _ in blocks]))) == pc.Z0
    assert gpu.places_info()["count"] == pc.EDGE_TOTAL
    cells = _cells(gpu.places_export()).copy()
    want = np.concatenate([main, np.stack(desc)] + [c for c, _ in blocks])
    assert np.array_equal(_bits(cells), _bits(want))
    kinds = list(kinds) + [("own", b) for b in range(pc.EDGE_BATCH)] + [k for _, ks in blocks for k in ks]
    # the model, once per distinct descriptor
    filled = cells.any(axis=(1, 2))
    d64, cache = [], {}
    for b in range(pc.EDGE_BATCH):
        key = desc[b].tobytes()
        if key not in cache:
            cache[key] = np.full((len(cells), pl.SECTORS), np.inf)          # (a zero entry has no valid shift)
            cache[key][filled] = pl.shift_distances(desc[b], cells[filled])
        d64.append(cache[key])
    distinct = {desc[b].tobytes(): b for b in range(pc.EDGE_BATCH) if desc[b].any()}
    eps = pc.eps_ref([desc[b] for b in distinct.values()], cells[filled], [d64[b][filled] for b in distinct.values()])
    e = SimpleNamespace(gpu=gpu, binding=binding, model=model, desc=desc, cells=cells, kinds=kinds, d64=d64, eps=eps, tol=8 * eps, worst=0.0,
                        edge=(edge_pts, edge_rows, edge_expect), dup=dup)
    assert 0 < e.tol <= 1e-4
    e.bits, e.shift = _readback(e, 0, check=False)           # (checked in the first test)
    yield e
    gpu.close()


def _where(E, name, par=None, lo=0, hi=None):
    hi = len(E.kinds) if hi is None else hi
    return [i for i in range(lo, hi) if E.kinds[i][0] == name and (par is None or E.kinds[i][1] == par)]


# ---- 1. every shift, every wave, every tile ---------------------------------------------------------------------------------------------
def test_every_shift_in_every_wave_and_tile_and_the_same_bits_everywhere(E):
    a = pc.SLOT_A[0]
    # every entry of the store is read back through ranges eight wide, each checked against the model; the bits are those the fixture got
    bits0, shift0 = _readback(E, 0)
    assert np.array_equal(bits0, E.bits) and np.array_equal(shift0, E.shift)
    # an entry comes back exactly when the model gives it a valid shift
    for b in range(pc.EDGE_BATCH):
        assert np.array_equal(E.shift[b] >= 0, np.isfinite(E.d64[b]).any(axis=1)), b
    # a rolled record: the shift is the roll, which the model separates from every other shift by more than 2 tol
    seen = set()
    for i, (name, k) in enumerate(E.kinds):
        if name in ("roll", "noisy", "dup", "scaled"):
            k = pc.SCALED_ROLL if name == "scaled" else k
            d = E.d64[a][i]
            assert int(np.argmin(d)) == k and np.sort(d)[1] - d[k] > 2 * E.tol, (i, name, k)
            for b in pc.SLOT_A:
                assert E.shift[b][i] == k, (b, i, name, k, E.shift[b][i])
            seen.add(k)
    assert seen == set(range(pl.SECTORS))
    # the same record -> the same (distance bits, shift), wherever it is stored, for every query; and the five copies of one sweep agree
    groups = {}
    for i in range(len(E.cells)):
        groups.setdefault(E.cells[i].tobytes(), []).append(i)
    many = [g for g in groups.values() if len(g) > 1 and E.cells[g[0]].any()]
    assert len(many) >= pl.SECTORS + 1 and max(len(g) for g in many) >= 12 + len(pc.Z_DUPS)
    for g in many:
        for b in range(pc.EDGE_BATCH):
            assert len({(int(E.bits[b][i]), int(E.shift[b][i])) for i in g}) == 1, (b, g, [E.kinds[i] for i in g])
    for b in pc.SLOT_A[1:]:
        assert np.array_equal(E.bits[b], E.bits[a]) and np.array_equal(E.shift[b], E.shift[a])
    # a record times a power of two has the same unit columns: the same bits again
    for sign in (-1, 1):
        i, j = _where(E, "scaled", sign * pc.SCALE_LOG2)[0], _where(E, "roll", pc.SCALED_ROLL)[0]
        assert all((E.bits[b][i], E.shift[b][i]) == (E.bits[b][j], E.shift[b][j]) for b in range(pc.EDGE_BATCH))
    # ranges eight wide that start elsewhere give the same table
    bits3, shift3 = _readback(E, 3)
    assert np.array_equal(bits3, E.bits) and np.array_equal(shift3, E.shift)
    # long ranges over the sparse blocks: the valid records come back from every wave and every tile, with the bits of the table
    places = set()
    for base, n, starts in ((pc.Z0, pc.Z_N, (0, 1, 4, 41, 71, 101, 128, 129, 201)), (pc.W0, pc.W_N, (0, 30, 72))):
        for k in range(0, len(starts), 3):
            slots = [pc.SLOT_A[0], pc.SLOT_A[1], pc.SLOT_B][:len(starts[k:k + 3])]
            ranges = [(base + s, base + n) for s in starts[k:k + 3]]
            res = _run(E, slots, ranges)
            for i, (lo, hi) in enumerate(ranges):
                places |= {pc.tile_wave(int(e) - lo) for e in res["entry"][i] if e >= 0}
    assert {w for _, w in places} == {0, 1, 2, 3} and {t for t, _ in places} == {0, 1, 2, 3}, sorted(places)
    assert len(places) >= 10, sorted(places)
    _report(E, "every shift, wave and tile")


# ---- 2. ranges ------------------------------------------------------------------------------------------------------------------------
def test_ranges_of_different_lengths_in_one_call(E):
    N = pc.EDGE_N
    slots = [pc.SLOT_A[0], pc.SLOT_A[1], pc.SLOT_B, pc.SLOT_PERIODIC, pc.SLOT_FEW, pc.SLOT_SINGLE, pc.SLOT_A[2], pc.SLOT_EDGES]
    ranges = [(0, N), (1, 130), (127, 129), (96, 161), (300, N), (N - 1, N), (0, 0), (200, 200)]
    for turn in range(len(slots)):                           # every slot meets every range: the grid is sized by (0, N), the others return early
        sl = slots[turn:] + slots[:turn]
        res = _run(E, sl, ranges, pinned=turn % 2 == 0)
        for i, (lo, hi) in enumerate(ranges):
            assert all(e == -1 or lo <= e < hi for e in res["entry"][i]), (sl[i], lo, hi, res[i])
        assert np.all(res["entry"][6:] == -1)
    # a call whose longest range is two entries long
    short = [(127, 129), (0, 0), (N - 1, N), (200, 200), (5, 6), (384, 386)]
    for turn in range(3):
        sl = (slots[turn:] + slots[:turn])[:len(short)]
        res = _run(E, sl, short)
        for i, (lo, hi) in enumerate(short):
            assert all(e == -1 or lo <= e < hi for e in res["entry"][i]), (sl[i], lo, hi, res[i])
    _report(E, "ranges")


# ---- 3. selection over more than 256 entries -----------------------------------------------------------------------------------------------
def test_selection_over_more_than_256_entries(E):
    a, total = pc.SLOT_A[0], pc.EDGE_TOTAL
    _run(E, list(range(pc.EDGE_BATCH)), [(0, total)] * pc.EDGE_BATCH)
    # 300 zero entries and three valid ones: three results and five fillers, whatever the query (the two empty queries get none)
    slots = [a, pc.SLOT_B, pc.SLOT_PERIODIC, pc.SLOT_FEW, pc.SLOT_LOW]
    res = _run(E, slots, [(pc.W0, pc.W0 + pc.W_N)] * len(slots))
    for i, b in enumerate(slots):
        want = [] if b == pc.SLOT_LOW else sorted(pc.W0 + p for p in pc.W_ROLLS)
        assert sorted(e for e in res["entry"][i] if e >= 0) == want and np.all(res["entry"][i][len(want):] == -1), (b, res[i])
    # duplicates of one record in different waves and tiles of a range: bit-equal distances, ranked by index
    lo, hi = pc.Z0 + 128, pc.Z0 + pc.Z_N
    res = _run(E, [a], [(lo, hi)])[0]
    dups = [pc.Z0 + p for p in pc.Z_DUPS]
    assert sorted(res["entry"][:3].tolist()) == sorted(pc.Z0 + p for p in pc.Z_ROLLS if p >= 128) and res["entry"][3:].tolist() == dups + [-1], res
    assert len(set(_bits(res["distance"][3:7]).tolist())) == 1 and {pc.tile_wave(e - lo) for e in dups} == {(0, 0), (0, 1), (1, 2), (2, 1)}
    # the twelve duplicates of the main block tie bit for bit too (the table), in all four waves and three tiles
    main_dups = _where(E, "dup", hi=pc.EDGE_N)
    assert len(main_dups) == 12 and len({int(E.bits[a][i]) for i in main_dups + dups}) == 1
    # where the model's ranks are separated by more than 2 tol, entry and shift equal the model's: the graded block, alone and at the end
    # of a range of 343 entries
    b = pc.SLOT_B
    for lo in (pc.V0, pc.W0):
        d = E.d64[b][lo:total]
        best = np.sort(d.min(axis=1)[np.isfinite(d.min(axis=1))])[:T + 1]
        assert len(best) == T + 1 and np.all(np.diff(best) > 2 * E.tol), np.diff(best)
        res = _run(E, [b], [(lo, total)])[0]
        ent, sh, di = pl.match(E.desc[b], E.cells[lo:total], T, first=lo)
        assert res["entry"].tolist() == ent.tolist() and res["shift"].tolist() == sh.tolist(), (res, ent, sh)
        assert all(E.kinds[e][0] == "graded" for e in ent)
    assert total - pc.W0 > 256
    _report(E, "selection")


# ---- 4. ties between shifts ---------------------------------------------------------------------------------------------------------------
def test_shifts_that_tie_bit_for_bit_go_to_the_lower_one(E):
    P, b = E.desc[pc.SLOT_PERIODIC], pc.SLOT_PERIODIC
    assert np.array_equal(_bits(P[:, :pc.PERIOD]), _bits(P[:, pc.PERIOD:])) and P.any()       # periodic on the device's own export
    assert [s for s in range(pc.PERIOD) if not P[:, s].any()] == list(pc.EMPTY_COLUMNS)
    halves = set()
    for k in pc.TIE_KS:
        (i,) = _where(E, "periodic", k)
        assert np.array_equal(_bits(E.cells[i]), _bits(np.roll(P, k, axis=1)))
        s = k % pc.PERIOD
        d = E.d64[b][i]
        assert d[s] == d[s + pc.PERIOD] and int(np.argmin(d)) == s and np.sort(d)[2] - d[s] > 2 * E.tol   # the input: an exact tie, the rest far off
        assert E.shift[b][i] == s, (k, i, int(E.shift[b][i]))
        halves.add((pc.h_of_shift(s), pc.h_of_shift(s + pc.PERIOD), s + pc.PERIOD >= 32))
    assert {(0, 0, True), (0, 1, True), (1, 0, True), (1, 1, True)} <= halves and any(not seam for _, _, seam in halves)
    # and in a long range, where these entries sit in all waves and tiles: the same shifts (the table) at the top of the list
    res = _run(E, [b], [(0, pc.EDGE_N)])[0]
    assert all(E.kinds[e][0] == "periodic" and s == E.kinds[e][1] % pc.PERIOD for e, s in zip(res["entry"], res["shift"])), res
    _report(E, "ties between shifts")


# ---- 5. masks and emptiness ---------------------------------------------------------------------------------------------------------------
def test_empty_and_single_column_queries(E):
    total = pc.EDGE_TOTAL
    for b in (pc.SLOT_LOW, pc.SLOT_FAR):
        assert not E.desc[b].any() and np.all(E.shift[b] == -1)
    res = _run(E, [pc.SLOT_LOW, pc.SLOT_FAR, pc.SLOT_A[0], pc.SLOT_SINGLE], [(0, total), (5, 300), (0, total), (0, total)])
    filler = np.zeros(T, E.binding.PLACE_MATCH_DTYPE)
    filler["entry"], filler["shift"] = -1, -1
    assert res[0].tobytes() == filler.tobytes() and res[1].tobytes() == filler.tobytes() and res["entry"][2, 0] >= 0
    res = _run(E, [pc.SLOT_FAR, pc.SLOT_LOW], [(0, 0), (pc.OWN0, pc.OWN0 + pc.EDGE_BATCH)])
    assert res[0].tobytes() == filler.tobytes() and res[1].tobytes() == filler.tobytes()
    # no query finds the entries of the empty sweeps, or any zero entry
    empty = [i for i in range(total) if not E.cells[i].any()]
    assert len(empty) > 700 and np.all(E.shift[:, empty] == -1)
    # one column against one column: cnt = 1, one valid shift, distance = 1 - the cosine of the two columns
    b, S = pc.SLOT_SINGLE, E.desc[pc.SLOT_SINGLE]
    assert np.flatnonzero(S.any(axis=0)).tolist() == [pc.SINGLE_SECTOR]
    for s in pc.SINGLE_SHIFTS:
        (i,) = _where(E, "single", s)
        d = E.d64[b][i]
        assert np.flatnonzero(np.isfinite(d)).tolist() == [s]
        u, v = S[:, pc.SINGLE_SECTOR].astype(np.float64), E.cells[i][:, (pc.SINGLE_SECTOR + s) % pl.SECTORS].astype(np.float64)
        assert abs(d[s] - (1.0 - u @ v / np.sqrt((u @ u) * (v @ v)))) < 1e-12
        assert E.shift[b][i] == s and abs(float(E.bits[b][i:i + 1].view(np.float32)[0]) - d[s]) <= E.tol, (s, i)
    # entries of one, two and three columns, and entries that meet the few-column query at some shifts only: read back within tol (the
    # fixture's check_match); here: the shift the device chose is valid in the model
    for name in ("fewcol", "nomeet"):
        for i in _where(E, name):
            for b in (pc.SLOT_FEW, pc.SLOT_SINGLE, pc.SLOT_A[0]):
                ok = np.isfinite(E.d64[b][i])
                assert (E.shift[b][i] >= 0) == ok.any() and (not ok.any() or ok[E.shift[b][i]])
    some = [np.isfinite(E.d64[pc.SLOT_FEW][i]) for i in _where(E, "nomeet")]
    assert all(o.any() and not o.all() for o in some)
    _report(E, "masks and emptiness")


# ---- 6. descriptor edges ------------------------------------------------------------------------------------------------------------------
def _check_descriptor(binding, gpu, slot, got, pts, rows, expect, max_range, height, empty_ring):
    cloud = gpu.cloud(binding.CLOUD_FULL, slot)
    assert len(cloud) == len(pts)                                                  # scan registration kept every crafted point
    have = {r.tobytes() for r in np.ascontiguousarray(cloud[:, :3])}
    for name, i in rows.items():
        assert np.ascontiguousarray(pts[i]).tobytes() in have, name                # bit for bit, the sign of a zero included
    assert gpu.ring_ranges(slot)[1][empty_ring] == 0
    D = pl.scan_context(cloud, max_range, height)
    lo, hi = pl.scan_context_bounds(cloud, max_range, height)
    assert np.array_equal(lo, hi) and np.array_equal(lo, D)                         # no point near a sector border: nothing to excuse
    assert np.array_equal(_bits(got), _bits(D)), np.argwhere(got != D)
    for name, (c, s, v) in expect.items():
        if v is not None:
            assert got[c, s] == np.float32(v) > 0, (name, c, s, v, got[c, s])
    c, s, _ = expect["z_at_floor"]
    assert got[c, s] == 0 and int((got > 0).sum()) > 60


def test_descriptor_edges_are_bit_exact(E):
    pts, rows, expect = E.edge
    _check_descriptor(E.binding, E.gpu, pc.SLOT_EDGES, E.desc[pc.SLOT_EDGES], pts, rows, expect, 80.0, 2.0, 5)
    # the other crafted sweeps too: one point per cell, in the middle of it
    for b in (pc.SLOT_PERIODIC, pc.SLOT_SINGLE, pc.SLOT_FEW, pc.SLOT_LOW, pc.SLOT_FAR):
        cloud = E.gpu.cloud(E.binding.CLOUD_FULL, b)
        lo, hi = pl.scan_context_bounds(cloud)
        assert np.array_equal(lo, hi) and np.array_equal(_bits(E.desc[b]), _bits(pl.scan_context(cloud))), b


def test_descriptor_edges_with_other_parameters(binding, syn):
    model = syn.sensor_model(MATCH_DRIVE["name"], columns=MATCH_DRIVE["columns"])
    pts, rows, expect = pc.edge_sweep(model, 50.0, 0.0, empty_ring=3)
    gpu = make(binding, model, 1, len(pts) + 64, False)
    gpu.places_enable(2, max_range=50.0, sensor_height=0.0)
    gpu.scan_register([pts], check=True)
    assert gpu.places_add([0]) == 0
    rec = gpu.places_export()
    assert rec["n_points"][0] == len(pts)
    _check_descriptor(binding, gpu, 0, _cells(rec[0]), pts, rows, expect, 50.0, 0.0, 3)
    gpu.close()


# ---- 7. cells at the ends of the f32 range -------------------------------------------------------------------------------------------------
def test_cells_at_the_ends_of_the_f32_range(E):
    """A loaded column of cells near 1e-25 is non-zero, yet its f32 squares underflow: the norm is 0 and the column loses its mask bit.
    Near 1e20 the norm is inf, the unit cells are 0 and the column counts with cosine 0.  aloam_places_load refuses both: positive cells
    lie in [2^-62, 2^60], and at both ends of that range the match equals the model."""
    gpu, binding, total = E.gpu, E.binding, pc.EDGE_TOTAL
    col = E.desc[pc.SLOT_SINGLE][:, pc.SINGLE_SECTOR]
    shape = np.where(col > 0, 1.0 + 0.25 * np.arange(pl.RINGS) / pl.RINGS, 0.0)      # cells within a factor 1.25 of each other
    assert (shape > 0).sum() >= 15
    lowest, highest = (shape / shape[shape > 0].min() * pc.CELL_MIN).astype(np.float32), (shape / shape.max() * pc.CELL_MAX).astype(np.float32)
    below, above = lowest.copy(), highest.copy()
    below[np.argmax(lowest == np.float32(pc.CELL_MIN))] = np.nextafter(np.float32(pc.CELL_MIN), np.float32(0))
    above[np.argmax(highest)] = np.nextafter(np.float32(pc.CELL_MAX), np.float32(np.inf))
    for column in ((shape * 1e-25).astype(np.float32), (shape * 1e20).astype(np.float32), below, above):
        c = np.zeros((2, pl.RINGS, pl.SECTORS), np.float32)
        c[0], c[1][:, 22] = E.cells[0], column
        assert np.all(np.isfinite(c)) and np.all(c >= 0) and c[1].any()
        with pytest.raises(binding.AloamError) as err:
            gpu.places_load(_records(binding, c))
        assert err.value.code == binding.E_ARG and gpu.places_info()["count"] == total, column
    # the ends of the range are accepted and match like any other column
    c = np.zeros((2, pl.RINGS, pl.SECTORS), np.float32)
    c[0][:, 22], c[1][:, 22] = lowest, highest
    assert c[0][c[0] > 0].min() == np.float32(pc.CELL_MIN) and c[1].max() == np.float32(pc.CELL_MAX)
    assert gpu.places_load(_records(binding, c)) == total
    b = pc.SLOT_SINGLE
    d64 = pl.shift_distances(E.desc[b], c)
    assert np.isfinite(d64).sum(axis=1).tolist() == [1, 1] and np.all(np.isfinite(d64[:, 22 - pc.SINGLE_SECTOR]))
    res = gpu.places_match([b], [(total, total + 2)], T)
    E.worst = max(E.worst, pc.check_match(res[0], E.desc[b], c, total, T, E.tol, d64=d64))
    assert sorted(res["entry"][0][:2].tolist()) == [total, total + 1] and res["shift"][0][:2].tolist() == [22 - pc.SINGLE_SECTOR] * 2
    _report(E, "cells at the ends of the f32 range")
