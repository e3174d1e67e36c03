"""What the place-recognition tests share: the drive whose sweeps are stored and queried on the GPU (test_gpu_places.py) and checked on
the model alone (test_places_model.py), and the NaN / range filter of scan registration for the model-only tests."""
import numpy as np

from test_registration_models import ring_from_angle

# The batch of the GPU match tests: slot b registers sweep b of this drive; the even slots are stored, the odd slots are the queries.
MATCH_DRIVE = dict(name="HDL-64", frames=24, seed=7, columns=512, travel=True, step=1.6)
MATCH_T = 4


def db_slots():
    return list(range(0, MATCH_DRIVE["frames"], 2))


def query_slots():
    return list(range(1, MATCH_DRIVE["frames"], 2))


def kept(scan, min_range):
    """The points that pass NaN removal + removeClosedPointCloud (float32 arithmetic).  ALOAM_CLOUD_FULL is a subset of them: scan
    registration also drops the rays whose elevation maps to no ring (src/scanRegistration.cpp:166-205).  Good enough for the model-only tests;
    the GPU tests take the descriptor's input from the device's own full cloud."""
    p = np.asarray(scan, np.float32)[:, :3]
    ok = np.isfinite(p).all(axis=1)
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
    thr = np.float32(min_range) * np.float32(min_range)
    with np.errstate(invalid="ignore"):
        ok &= ~(r2 < thr)
    return p[ok]


# ---- the adversarial store of test_gpu_places_edges.py ---------------------------------------------------------------------------------
# k_place_match deals a range over tiles of 128 entries, four waves of 32 each; position p = entry - lo of a range falls in tile p // 128,
# wave p % 128 // 32.  The store is loaded (aloam_places_load takes any finite non-negative cells), so every kind of record sits where
# the test wants it: EDGE_N entries fill three tiles, one full wave and a wave of five.
RINGS, SECTORS = 20, 60
TILE, WAVE = 128, 32
EDGE_N = 3 * TILE + WAVE + 5
EDGE_STRIDE = TILE + WAVE + 1                              # item j of the list sits at index 161 j mod 421 (421 is prime), which spreads every
                                                           # kind over the tiles and waves; items four apart lie 223 = 128 + 95 (or, wrapped,
                                                           # -198 = -256 + 58) apart: another tile and another wave
EDGE_BATCH = 12                                            # the slots of the module's context, by what they register:
SLOT_A = (0, 1, 2, 3, 11)                                  #   one drive sweep, five times
SLOT_PERIODIC, SLOT_LOW, SLOT_FAR, SLOT_SINGLE, SLOT_EDGES, SLOT_FEW, SLOT_B = 4, 5, 6, 7, 8, 9, 10
DRIVE_FRAME_A, DRIVE_FRAME_B = 0, 6
PERIOD = 30
EMPTY_COLUMNS = (7, 19)                                    # sectors (mod 30) the periodic sweep leaves empty
TIE_KS = (1, 2, 5, 6, 9, 10, 26, 29, 31, 35, 39, 44, 56, 59)      # rolls of the periodic query: shifts k % 30 and k % 30 + 30 tie bit for bit
SINGLE_SECTOR = 17
SINGLE_SHIFTS = (0, 1, 3, 15, 28, 30, 31, 32, 33, 36, 47, 55, 56, 57, 58, 59)
FEW_SECTORS = (3, 4, 40)
SCALE_LOG2 = 50                                            # the "scaled" records: a roll times 2^-50 and 2^50, same unit columns bit for bit
SCALED_ROLL = 7
DUP_ROLL = 33
# aloam_places_load: positive cells lie in [2^-62, 2^60], where the f32 squares and their 20-term sums are normal numbers
CELL_MIN, CELL_MAX = 2.0 ** -62, 2.0 ** 60
# the second block: zero entries around a few valid ones, so that a range returns every valid one wherever it falls (position -> record)
Z_N = 437
Z_ROLLS = {3: 31, 40: 32, 70: 33, 100: 56, 127: 59, 200: 57, 300: 58, 417: 0}
Z_DUPS = (128, 173, 326, 424)
# the third block: 300 zero entries and three valid ones
W_N = 303
W_ROLLS = {71: 1, 171: 34, 288: 55}
# the fourth block: copies of the other drive sweep under growing noise, engineered so that the model's ranks are well separated
V_N = 40
# where the blocks lie in the store: the loaded main block, the queries' own entries, then the loaded blocks Z, W and V
MAIN0, OWN0 = 0, EDGE_N
Z0 = OWN0 + EDGE_BATCH
W0 = Z0 + Z_N
V0 = W0 + W_N
EDGE_TOTAL = V0 + V_N


def tile_wave(p):
    return p // TILE, p % TILE // WAVE


def h_of_shift(s):
    """Which half of the lanes (lane >> 5) holds shift s: row s % 32 of its accumulator, rows 4 h .. 4 h + 3 of every eight."""
    return (s % 32 >> 2) & 1


def _noisy(rng, d, amount=0.1):
    return (d * (1.0 + amount * (2.0 * rng.random(d.shape) - 1.0))).astype(np.float32)


def _columns(d, keep):
    out = np.zeros_like(d)
    out[:, list(keep)] = d[:, list(keep)]
    return out


def edge_store(Qa, P, S, seed=11):
    """(cells [EDGE_N, 20, 60] float32, kinds [EDGE_N] of (name, parameter)) from the exported descriptors of the drive sweep (Qa), the
    periodic sweep (P) and the single-column sweep (S)."""
    rng = np.random.default_rng(seed)
    items = []
    for k0 in range(0, SECTORS, 4):
        items += [(("roll", k), np.roll(Qa, k, axis=1)) for k in range(k0, k0 + 4)] * 2
    for k in range(SECTORS):
        items.append((("noisy", k), _noisy(rng, np.roll(Qa, k, axis=1))))
    for k in TIE_KS:
        items.append((("periodic", k), np.roll(P, k, axis=1)))
    full = np.flatnonzero(Qa.any(axis=0))
    for j in range(24):
        keep = rng.choice(full, 1 + j % 3, replace=False)
        items.append((("fewcol", 1 + j % 3), _columns(Qa, keep)))
    for s in SINGLE_SHIFTS:
        c = np.zeros_like(S)
        c[:, (SINGLE_SECTOR + s) % SECTORS] = _noisy(rng, S[:, SINGLE_SECTOR], 0.3)
        items.append((("single", s), c))
    for j in range(20):
        w = (3 * j) % SECTORS
        items.append((("nomeet", w), _columns(np.roll(Qa, j, axis=1), [(w + i) % SECTORS for i in range(6)])))
    for j in range(40):
        items.append((("zero", j), np.zeros_like(Qa)))
    dup = _noisy(rng, np.roll(Qa, DUP_ROLL, axis=1))
    for j in range(12):
        items.append((("dup", DUP_ROLL), dup))
    for sign in (-1, 1):
        items.append((("scaled", sign * SCALE_LOG2), np.roll(Qa, SCALED_ROLL, axis=1) * np.float32(2.0 ** (sign * SCALE_LOG2))))
    while len(items) < EDGE_N:
        d = (4.0 * rng.random((RINGS, SECTORS))).astype(np.float32)
        d[rng.random((RINGS, SECTORS)) < 0.3] = 0
        d[:, rng.random(SECTORS) < 0.3] = 0
        items.append((("random", len(items)), d))
    assert len(items) == EDGE_N
    cells, kinds = np.zeros((EDGE_N, RINGS, SECTORS), np.float32), [None] * EDGE_N
    for j, (kind, d) in enumerate(items):
        i = j * EDGE_STRIDE % EDGE_N
        cells[i], kinds[i] = d, kind
    return cells, kinds, dup


def sparse_block(n, rolls, dups, Qa, dup):
    """n entries, zero but for np.roll(Qa, k) at the positions of `rolls` and the duplicate record at those of `dups`."""
    cells, kinds = np.zeros((n, RINGS, SECTORS), np.float32), [("zero", i) for i in range(n)]
    for p, k in rolls.items():
        cells[p], kinds[p] = np.roll(Qa, k, axis=1), ("roll", k)
    for p in dups:
        cells[p], kinds[p] = dup, ("dup", DUP_ROLL)
    return cells, kinds


def separated_block(Qb, seed=13):
    """V_N records: record with rank i is a roll of Qb under multiplicative noise of amplitude 0.02 (i + 1), at position 17 i mod V_N."""
    rng = np.random.default_rng(seed)
    cells, kinds = np.zeros((V_N, RINGS, SECTORS), np.float32), [None] * V_N
    for i in range(V_N):
        p, k = 17 * i % V_N, 7 * i % SECTORS
        cells[p], kinds[p] = _noisy(rng, np.roll(Qb, k, axis=1), 0.02 * (i + 1)), ("graded", i)
    return cells, kinds


def shift_distances_f32(q, entries):
    """The documented arithmetic of the device in float32, d[e, shift]: columns divided by their norm (squares summed in ascending ring
    order), the 1200 products of a (entry, shift) pair rounded and summed one after the other in cell order, 1 - sum / cnt.  +inf where
    cnt = 0.  Its distance from the float64 model is the rounding error any f32 evaluation of the definition may show (eps_ref)."""
    f = np.float32

    def unit(d):
        d = np.asarray(d, f)
        ss = np.zeros(d.shape[:-2] + d.shape[-1:], f)
        for r in range(RINGS):
            ss = ss + d[..., r, :] * d[..., r, :]
        n = np.sqrt(ss)[..., None, :]
        return np.divide(d, n, out=np.zeros_like(d), where=n > 0), (n > 0).squeeze(-2)
    qu, qm = unit(q)
    cu, cm = unit(np.asarray(entries).reshape(-1, RINGS, SECTORS))
    acc = np.zeros((len(cu), SECTORS), f)
    shifts = np.arange(SECTORS)
    for j in range(SECTORS):
        for r in range(RINGS):
            acc = acc + cu[:, r, j, None] * qu[r, (j - shifts) % SECTORS][None]
    cnt = np.stack([(cm & np.roll(qm, s)[None]).sum(axis=1) for s in range(SECTORS)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = f(1) - acc / cnt.astype(f)
    return np.where(cnt > 0, d, f(np.inf)).astype(f)


def eps_ref(queries, entries, d64s=None):
    """The largest |shift_distances_f32 - places.shift_distances| over the queries x entries x shifts with a valid shift."""
    import importlib
    pl = importlib.import_module("a-loam_amd.places")
    worst = 0.0
    for i, q in enumerate(queries):
        d64 = pl.shift_distances(q, entries) if d64s is None else d64s[i]
        d32 = shift_distances_f32(q, entries)
        ok = np.isfinite(d64)
        assert np.array_equal(ok, np.isfinite(d32))
        if ok.any():
            worst = max(worst, float(np.abs(d32[ok].astype(np.float64) - d64[ok]).max()))
    return worst


def check_match(result_row, q, entries, lo, T, tol, d64=None):
    """One query's T results (PLACE_MATCH_DTYPE [T]) for the range [lo, lo + len(entries)) against the float64 model, with no separation
    between distances assumed.  d64: shift_distances(q, entries) where the caller has it already.  Returns the device's worst deviation."""
    import importlib
    pl = importlib.import_module("a-loam_amd.places")
    entries = np.asarray(entries).reshape(-1, RINGS, SECTORS)
    hi = lo + len(entries)
    if d64 is None:
        d64 = pl.shift_distances(q, entries) if len(entries) else np.zeros((0, SECTORS))
    best = d64.min(axis=1) if len(entries) else np.zeros(0)
    n_valid = int(np.isfinite(best).sum())
    n = min(T, n_valid)
    ent, sh, di = result_row["entry"], result_row["shift"], result_row["distance"]
    assert len(ent) == T and np.all(result_row["pad"] == 0)
    # (e) as many as the range provides, the rest is the filler
    assert np.all(ent[:n] >= 0) and np.all(ent[n:] == -1) and np.all(sh[n:] == -1) and np.all(di[n:].view(np.uint32) == 0), (lo, hi, n, result_row)
    # (a) sorted by (device distance, index), distinct, inside the range
    keys = [(float(di[k]), int(ent[k])) for k in range(n)]
    assert keys == sorted(keys) and len(set(ent[:n].tolist())) == n, (lo, hi, result_row)
    assert all(lo <= e < hi for e in ent[:n]), (lo, hi, result_row)
    worst = 0.0
    for k in range(n):
        e, s = int(ent[k]) - lo, int(sh[k])
        assert 0 <= s < SECTORS and np.isfinite(d64[e, s]), (lo, hi, result_row[k])
        dev = abs(float(di[k]) - d64[e, s])
        worst = max(worst, dev)
        assert dev <= tol, (lo, hi, result_row[k], d64[e, s], dev, tol)                                     # (b)
        assert d64[e, s] <= best[e] + tol, (lo, hi, result_row[k], d64[e, s], best[e], int(np.argmin(d64[e])))   # (c)
    if n == T:                                                                                             # (d)
        rest = np.setdiff1d(np.flatnonzero(np.isfinite(best)), ent[:n] - lo)
        assert np.all(best[rest] >= float(di[n - 1]) - tol), (lo, hi, result_row, rest[best[rest] < float(di[n - 1]) - tol])
    return worst


# ---- crafted sweeps ---------------------------------------------------------------------------------------------------------------------
def ring_elevations(model):
    """Elevation in degrees of every ring of a synthetic.SensorModel."""
    dirs, ring = model.dirs.numpy(), model.ring.numpy()
    return np.array([np.degrees(np.arcsin(dirs[np.argmax(ring == r), 2])) for r in range(model.n_scans)])


def polar_point(rho, theta_deg, el_deg):
    """A point at horizontal range rho, descriptor angle theta = atan2(y, x) + pi (degrees) and elevation el."""
    az = np.radians(theta_deg) - np.pi
    return [rho * np.cos(az), rho * np.sin(az), rho * np.tan(np.radians(el_deg))]


def inner_rings(el):
    """The rings whose own elevation the front end's ring decision maps back to them, 1e-3 degrees to either side included.  For 64
    rings that leaves out ring 0, which sits on the decision's upper limit of 2 degrees, where the rounding of the f32 angle decides
    whether a point is kept at all, and the rings past 50, which the decision drops."""
    f = np.float32
    return [r for r in range(len(el)) if {ring_from_angle(f(el[r]) + d, len(el)) for d in (f(-1e-3), f(0), f(1e-3))} == {r}]


def usable_rings(el, rho, sensor_height, min_range, avoid=()):
    """The inner rings whose ray at horizontal range rho is kept by scan registration and stands at least 5 cm above the descriptor's floor."""
    z = rho * np.tan(np.radians(el))
    return [r for r in inner_rings(el) if r not in avoid and z[r] + sensor_height > 0.05 and np.hypot(rho, z[r]) > 1.1 * min_range + 0.1]


def cell_sweep(model, cells_of, max_range=80.0, sensor_height=2.0, per_cell=1):
    """One point (or per_cell points side by side) in the middle of each descriptor cell (ring c, sector s) for which cells_of(c, s) gives
    a key; the sensor ring - hence the height - is a function of that key alone."""
    el = ring_elevations(model)
    pts = []
    for c in range(RINGS):
        rho = (c + 0.5) * max_range / RINGS
        ok = usable_rings(el, rho, sensor_height, model.min_range)
        for s in range(SECTORS):
            key = cells_of(c, s)
            if key is None or not ok:
                continue
            z = rho * np.tan(np.radians(el[ok[key % len(ok)]]))
            for i in range(per_cell):
                p = polar_point(rho, (s + (i + 1.0) / (per_cell + 1.0)) * 360.0 / SECTORS, 0.0)
                pts.append([p[0], p[1], z])
    return np.asarray(pts, np.float32)


def periodic_sweep(model):
    return cell_sweep(model, lambda c, s: None if s % PERIOD in EMPTY_COLUMNS else 7 * c + 3 * (s % PERIOD))


def single_column_sweep(model):
    return cell_sweep(model, lambda c, s: c if s == SINGLE_SECTOR else None, per_cell=3)


def few_column_sweep(model):
    return cell_sweep(model, lambda c, s: 5 * c + s if s in FEW_SECTORS else None, per_cell=2)


def low_sweep(model, sensor_height=2.0):
    """Points that scan registration keeps and that all lie at or below the descriptor's floor (z + sensor_height <= 0)."""
    el = ring_elevations(model)
    pts = [polar_point(rho, th, e) for rho in (20.0, 30.0, 40.0) for th in np.arange(1.0, 360.0, 9.0) for e in el[inner_rings(el)]
           if rho * np.tan(np.radians(e)) + sensor_height < -0.05]
    assert len(pts) > 100
    return np.asarray(pts, np.float32)


def far_sweep(model, max_range=80.0, sensor_height=2.0):
    """Points above the floor that all lie beyond max_range."""
    el = ring_elevations(model)
    pts = [polar_point(rho, th, e) for rho in (1.1 * max_range, 1.2 * max_range) for th in np.arange(1.0, 360.0, 9.0) for e in el[inner_rings(el)]
           if rho * np.tan(np.radians(e)) + sensor_height > 0.05]
    assert len(pts) > 100
    return np.asarray(pts, np.float32)


def edge_sweep(model, max_range=80.0, sensor_height=2.0, seed=3, empty_ring=5):
    """The sweep of the descriptor-edge test: (points float32 [N, 3], edges = name -> row index, expect = name -> (ring, sector, value or
    None for "contributes nothing")).  max_range must make 0.6 max_range and 0.8 max_range exact in float32 (80 and 50 do)."""
    f = np.float32
    el = ring_elevations(model)
    h, step = float(sensor_height), max_range / RINGS
    rng = np.random.default_rng(seed)
    pts, edges, expect = [], {}, {}

    def ring_for(rho, want=0):
        ok = usable_rings(el, rho, h, model.min_range, avoid=(empty_ring,))
        return el[ok[want % len(ok)]]

    def add(name, p, cell, value):
        edges[name], expect[name] = len(pts), (cell[0], cell[1], value)
        pts.append([f(p[0]), f(p[1]), f(p[2])])
    # rho == max_range exactly (skipped) and one f32 step below it (ring 19), off the axes
    x, y = f(0.6 * max_range), f(0.8 * max_range)
    z = f(max_range * np.tan(np.radians(ring_for(max_range))))
    sec = int((np.degrees(np.arctan2(float(y), float(x))) + 180.0) / 6.0)
    add("rho_at_max", (x, y, z), (RINGS, sec), None)
    z1 = f(max_range * np.tan(np.radians(ring_for(max_range, 1))))
    yb = y
    while np.sqrt(x * x + yb * yb) == f(max_range):         # (the first steps of y still round to max_range)
        yb = np.nextafter(yb, f(0))
    add("rho_below_max", (x, yb, z1), (RINGS - 1, sec), z1 + f(h))
    # the axes: atan2f is exact there.  (x < 0, +0) -> theta = 2 pi -> sector 60, clamped to 59; (x < 0, -0) -> theta = 0 -> sector 0
    for name, c, xs, y0, s in (("minus_x_plus_zero", 7, -1.0, 0.0, SECTORS - 1), ("minus_x_minus_zero", 8, -1.0, -0.0, 0), ("plus_x", 10, 1.0, 0.0, SECTORS // 2),
                               ("plus_x_minus_zero", 11, 1.0, -0.0, SECTORS // 2)):
        rho = (c + 0.5) * step
        z = f(rho * np.tan(np.radians(ring_for(rho, c))))
        add(name, (f(xs * rho), f(y0), z), (c, s), z + f(h))
    # z == -sensor_height exactly (v = 0: nothing) and just above it (v = the smallest step), each alone in its cell
    if h != 0:
        r_floor = int(np.argmin(np.abs(el + 3.0)))
        rho = h / np.tan(np.radians(-el[r_floor]))
        above = np.nextafter(f(-h), f(np.inf))
    else:
        rho, above = 0.475 * max_range, f(2.0 ** -20)
    c = int(rho / step)
    add("z_at_floor", polar_point(rho, 100.5, 0.0)[:2] + [f(-h)], (c, int(100.5 / 6.0)), None)
    add("z_above_floor", polar_point(rho, 130.5, 0.0)[:2] + [above], (c, int(130.5 / 6.0)), f(above) + f(h))
    # two points in one cell, the higher one last and the higher one first
    for name, s, order in (("two_low_high", 40, (0, 1)), ("two_high_low", 44, (1, 0))):
        rho = 12.5 * step
        zz = sorted(f(rho * np.tan(np.radians(ring_for(rho, w)))) for w in (0, 1))
        assert zz[0] < zz[1]
        for i in order:
            add(f"{name}_{i}", polar_point(rho, (s + 0.5) * 6.0, 0.0)[:2] + [zz[i]], (12, s), zz[1] + f(h))
    # a few points well inside each of some other cells
    taken = {(cc, ss) for cc, ss, _ in expect.values()}
    lowest = 0 if model.min_range < 0.25 * step else 1 + int(model.min_range / step)
    for _ in range(80):
        c, s = int(rng.integers(lowest, RINGS - 1)), int(rng.integers(1, SECTORS - 1))
        if (c, s) in taken or s in (SECTORS // 2 - 1, SECTORS // 2):
            continue
        taken.add((c, s))
        for fr, fs in ((0.5, 0.5), (0.3, 0.7), (0.7, 0.3)):
            rho = (c + fr) * step
            pts.append([f(v) for v in polar_point(rho, (s + fs) * 6.0, ring_for(rho, int(rng.integers(0, 64))))])
    return np.asarray(pts, np.float32), edges, expect
