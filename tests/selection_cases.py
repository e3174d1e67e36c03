"""Rings built for the corner / flat selection of k_ring_features (pick_sector and the second pass), the facts that prove what
each ring forces, and mutants of the selection model: one plausible device mistake each.  No GPU in this file.

Rings with exact arithmetic.  With `ring_from_field=True` the fourth float is the ring id, so a ring's points are free.  Every
ring here is a polyline at y = 8 m:
  * x advances by 2^-3 m per step, or by 5 * 2^-3 m where a gap is wanted (squared step >= 0.39 against the 0.05 threshold);
  * z is a small multiple of 2^-4 m (0, 1 or 2 for spikes, up to 9 in the tents of C7) that changes by at most 2 * 2^-4 m over a plain
    step (squared plain step <= 0.03125).
The three points of C9 alone leave the grid.  All differences, 11-point sums and squares are then exact in f32: the curvature is
(4 dX^2 + dZ^2) / 256 with integers dX (in 2^-3 m) and dZ (in 2^-4 m), independent of the summation order, ties exist by
construction, and a device that disagrees with the oracle on such a ring has a logic error, never a rounding difference.  A lone "spike" z = h gives its point the curvature
100 h^2 / 256 (0.39 or 1.56) and the ten points around it h^2 / 256; a gap gives the five points on either side 0.25 m^2,
m = 1 .. 5.  `random_ring` repairs its draw until no curvature lies in [0.05, 0.2].

`facts(O, ring)` runs the oracle on the ring and the instrumented register-level model (`run`, the same scheme as
selection_model.model over pick_sector_regs, with a log and the mutants) on the oracle's own curvature and gaps.
"""
import numpy as np

from selection_model import INF, THR

RINGS = 8
M32 = 0xffffffff
K6_2048, K6_4096 = 6, 11                                  # registers per sector of the two kernel instances
MUTANTS = {
    "a": "no second pass",
    "b": "the second pass carries the pre-redo spill of the sector in front",
    "c": "carry not passed through sectors shorter than 5 (carry >> len dropped)",
    "d": "carry mask not clipped to len (equivalent: nothing reads the bits at or behind len)",
    "e": "corner ties go to the smallest index",
    "f": "flat ties go to the largest index",
    "g": "within one lane, ties pick the wrong register",
    "h": "a kill is clipped to register kr",
    "i": "a kill into kr + 1 or kr - 1 is off by one lane",
    "j": "the 4th flat marks its neighbours",
    "k": "the 21st corner candidate marks its neighbours",
    "l": "spill taken from 5 instead of fw",
    "m": "the reach window is shifted by one step",
    "n": "the reach bytes of kr >= 8 are read from the packed register in front",
    "o": "the two values next to the threshold: corner needs bits > bits(0.1f), flat takes bits <= bits(0.1f)",
    "p": "the curvature stencil reads one column off at a 256-point chunk border",
}


# ------------------------------------------------------------------------------------------------ builders
def ring(zs, steps=None, ring_id=0):
    """zs: heights in 2^-4 m; steps: n - 1 x steps in 2^-3 m (1 plain, 5 a gap).  -> float32 (n, 4), fourth float the ring id"""
    zs = np.asarray(zs, np.int64)
    n = len(zs)
    steps = np.ones(n - 1, np.int64) if steps is None else np.asarray(steps, np.int64)
    assert len(steps) == n - 1
    xu = np.concatenate([[0], np.cumsum(steps)]) - int(steps.sum()) // 2
    out = np.zeros((n, 4), np.float64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = xu * 0.125, 8.0, zs * 0.0625, ring_id
    return out.astype(np.float32)


def spikes(n, at, gaps=()):
    """flat ring with z spikes {index: height} and gaps behind the steps listed (step s joins points s and s + 1; {step: length in 2^-3 m}
    for a gap that is not 5 long)"""
    zs = np.zeros(n, np.int64)
    for i, h in dict(at).items(): zs[i] = h
    steps = np.ones(n - 1, np.int64)
    for s in gaps: steps[s] = gaps[s] if isinstance(gaps, dict) else 5
    return ring(zs, steps)


def curvature_units(zs, steps):
    """256 * curvature as exact integers (4 dX^2 + dZ^2), zero outside 5 .. n - 6"""
    zs = np.asarray(zs, np.int64); n = len(zs)
    xu = np.concatenate([[0], np.cumsum(np.asarray(steps, np.int64))])
    c = np.zeros(n, np.int64)
    for i in range(5, n - 5):
        dx = xu[i - 5:i + 6].sum() - 11 * xu[i]; dz = zs[i - 5:i + 6].sum() - 11 * zs[i]
        c[i] = 4 * dx * dx + dz * dz
    return c


def random_ring(n, seed, p_spike=0.12, p_gap=0.0):
    """pseudo-random spikes (heights 1, 2) and gaps; spikes around a curvature inside [0.05, 0.2] are taken out again"""
    rng = np.random.default_rng(seed)
    zs = np.where(rng.random(n) < p_spike, rng.integers(1, 3, n), 0).astype(np.int64)
    steps = np.where(rng.random(n - 1) < p_gap, 5, 1).astype(np.int64)
    while True:
        c = curvature_units(zs, steps)
        bad = np.flatnonzero((c >= 13) & (c <= 51))
        if not len(bad): break
        for i in bad: zs[max(0, i - 5):i + 6] = 0
    return ring(zs, steps)


def with_id(r, ring_id):
    out = r.copy(); out[:, 3] = ring_id
    return out


# ------------------------------------------------------------------------------------------------ geometry as the oracle computes it
def curvature_f32(xyz, mut=""):
    """11-point curvature in f32, the sums in the order of src/scanRegistration.cpp:256-266.  Mutant p: a point at a multiple of 256
    takes the stencil one column further on."""
    F = np.float32
    n = len(xyz); c = np.zeros(n, F); p = np.concatenate([xyz.astype(F), np.zeros((1, 3), F)])   # behind the ring the tile holds zeros
    for i in range(5, n - 5):
        k = i + 1 if mut == "p" and i % 256 == 0 else i
        d = np.zeros(3, F)
        for o in (-5, -4, -3, -2, -1): d = d + p[k + o]
        d = d - F(10) * p[k]
        for o in (1, 2, 3, 4, 5): d = d + p[k + o]
        s = d * d
        c[i] = (s[0] + s[1]) + s[2]
    return c


def steps2(xyz):
    """squared steps in f32 ((dx^2 + dy^2) + dz^2)"""
    d = np.diff(xyz.astype(np.float32), axis=0); s = d * d
    return (s[:, 0] + s[:, 1]) + s[:, 2]


def reach_of(gap, n, shift=0):
    """(fw, bk) per point: gap-free steps ahead and behind, at most 5, inside the ring.  shift = 1: the window one step off (mutant m)"""
    g = lambda s: True if s < 0 or s >= n - 1 else bool(gap[s])
    out = []
    for i in range(n):
        fw = bk = 0
        while fw < 5 and not g(i + fw + shift): fw += 1
        while bk < 5 and not g(i - 1 - bk + shift): bk += 1
        out.append((fw, bk))
    return out


# ------------------------------------------------------------------------------------------------ the scheme, instrumented, with mutants
def pick_regs(j, init_marks, L, curv, reach, K=K6_2048, mut="", log=None, W=64):
    """selection_model.pick_sector_regs with K registers as the kernel instance has them, a log entry per pick and the mutants"""
    sp, ln = (L * j) // 6, (L * (j + 1)) // 6 - (L * j) // 6
    first = sp + 5
    cc = np.zeros((K, W), np.int64)
    cc.reshape(-1)[:ln] = np.ascontiguousarray(curv[first:first + ln], np.float32).view(np.uint32).astype(np.int64) + 1
    for pos in range(min(ln, 5)):
        if (init_marks >> pos) & 1: cc[0, pos] = 0
    spill = 0
    lanes = np.arange(W)

    def kill(kr, f, dead, entry):
        nonlocal spill
        kq = kr - 4 if mut == "n" and kr >= 8 else kr
        fw, bk = reach[first + kq * W + f]
        P, lo, w = kr * W + f, f - bk, fw + bk
        cc[kr, ((lanes - lo) & M32) <= w] = dead
        prev = nxt = False
        if (lo & M32) > ((W - 1 - w) & M32) and mut != "h":
            off = 1 if mut == "i" else 0
            if lo < 0 and kr > 0: cc[kr - 1, lanes >= W + lo + off] = dead; prev = True
            if lo >= 0 and kr + 1 < K: cc[kr + 1, lanes <= lo + w - W - off] = dead; nxt = True
        if P + 5 >= ln:
            e = P + (5 if mut == "l" else fw) - (ln - 1)
            if e > 0: spill |= (1 << e) - 1
        if entry is not None: entry.update(fw=fw, bk=bk, prev=prev, next=nxt and (kr + 1) * W < ln)
        return P

    def note(kind, kr, f, ext, tie):
        if log is None: return None
        e = {"sector": j, "kind": kind, "pos": kr * W + f, "kr": kr, "lane": f, "tie_lanes": len(tie),
             "tie_regs": int(max((cc[:, t] == ext).sum() for t in tie)), "fw": None, "bk": None, "prev": False, "next": False}
        log.append(e)
        return e

    corners, flats = [], []
    for count in range(21 if mut == "k" else 20):
        m = cc.max(axis=0)
        krl = np.zeros(W, np.int64)
        if mut in ("e", "g"):
            krl[:] = K - 1
            for r in range(K - 2, -1, -1): krl = np.where(cc[r] == m, r, krl)
        else:
            for r in range(1, K): krl = np.where(cc[r] == m, r, krl)
        cmax = int(m.max())
        lowest = THR + 1 if mut == "o" else THR
        if not (lowest <= ((cmax - 1) & M32) <= INF): break
        tie = np.flatnonzero(m == cmax)
        f = int(tie[0]); kr = int(krl[f])
        if len(tie) != 1:
            if mut == "e": wv = int(np.where(m == cmax, krl * W + lanes, M32).min())
            else: wv = int(np.where(m == cmax, krl * W + lanes, 0).max())
            f, kr = wv % W, wv // W
        if count == 20:
            kill(kr, f, 0, None); break                                      # mutant k only
        corners.append(first + kill(kr, f, 0, note("corner", kr, f, cmax, tie)))
    cc = (cc - 1) & M32
    count = 0
    while True:
        m = cc.min(axis=0)
        if mut in ("f", "g"):
            krl = np.zeros(W, np.int64)
            for r in range(1, K): krl = np.where(cc[r] == m, r, krl)
        else:
            krl = np.full(W, K - 1, np.int64)
            for r in range(K - 2, -1, -1): krl = np.where(cc[r] == m, r, krl)
        cmin = int(m.min())
        if not (cmin <= THR if mut == "o" else cmin < THR): break
        tie = np.flatnonzero(m == cmin)
        f = int(tie[0]); kr = int(krl[f])
        if len(tie) != 1:
            if mut == "f": wv = int(np.where((m == cmin) & (krl * W + lanes < ln), krl * W + lanes, 0).max())
            else: wv = int(np.where(m == cmin, krl * W + lanes, M32).min())
            f, kr = wv % W, wv // W
        entry = note("flat", kr, f, cmin, tie)
        flats.append(first + kr * W + f)
        count += 1
        if count >= 4:
            if mut == "j": kill(kr, f, M32, None)
            break
        kill(kr, f, M32, entry)
    return corners, flats, spill


def run(curv, gap, n, K=K6_2048, mut="", log=None):
    """first pass of all six sectors without incoming marks, then the in-order second pass.  -> labels, picks, per-sector info"""
    L = n - 11
    reach = reach_of(gap, n, 1 if mut == "m" else 0)
    logs = [[] for _ in range(6)]
    first = [pick_regs(j, 0, L, curv, reach, K, mut, logs[j]) for j in range(6)]
    res = list(first)
    info = [{"first": (first[0][0], first[0][1]), "redone": False, "marks": 0, "carried": 0, "len": L // 6}]
    carry = res[0][2]
    for j in range(1, 6):
        sp, ln = (L * j) // 6, (L * (j + 1)) // 6 - (L * j) // 6
        m = carry if ln >= 5 or mut == "d" else carry & ((1 << ln) - 1)
        redone = False
        if m and mut != "a":
            if any(pk - 5 - sp < 5 and (m >> (pk - 5 - sp)) & 1 for pk in res[j][0] + res[j][1]):
                logs[j] = []
                res[j] = pick_regs(j, m, L, curv, reach, K, mut, logs[j]); redone = True
        passed = 0 if ln >= 5 or mut == "c" else carry >> ln
        info.append({"first": (first[j][0], first[j][1]), "redone": redone, "marks": m & ((1 << min(ln, 5)) - 1), "carried": passed, "len": ln})
        carry = passed | (first[j][2] if mut == "b" else res[j][2])
    label = np.zeros(n, np.int8)
    for j, (corners, flats, spill) in enumerate(res):
        for q, ind in enumerate(corners): label[ind] = 2 if q < 2 else 1
        for ind in flats: label[ind] = -1
        info[j].update(final=(corners, flats), spill=spill, first_spill=first[j][2], picks=logs[j])
    if log is not None: log.extend(e for lg in logs for e in lg)
    return label, [(c, f) for c, f, _ in res], info


def oracle_ring(O, r):
    """the oracle on one ring alone -> cloud xyz, curvature, labels, gaps (its own steps against 0.05, compared in double)"""
    orc = O.Oracle(n_scans=RINGS, min_range=0.3, ring_from_field=True)
    fo = orc.scan_register(with_id(r, 0))
    starts, counts = orc.ring_ranges()
    assert starts[0] == 0 and counts[0] == len(r)
    curv, lab, _ = orc.per_point()
    xyz = fo["cloud"][:, :3]
    return xyz, curv, lab, steps2(xyz).astype(np.float64) > 0.05


def lane_class(lane):
    return "lo" if lane < 5 else "hi" if lane > 58 else "mid"


def facts(O, r):
    """what the ring forces, see facts_of"""
    return facts_of(*oracle_ring(O, r)[:3])


def facts_of(xyz, curv, lab):
    """from one ring of the oracle's cloud, its curvature and labels: per sector the first-pass and final picks, redone, incoming marks, marks
    carried on, spill and every final pick's (kr, lane, fw, bk), neighbour registers touched and ties; plus totals over the ring"""
    n = len(xyz)
    gap = steps2(xyz).astype(np.float64) > 0.05
    K = K6_4096 if n > 2059 else K6_2048
    if n - 11 < 6:                                                            # :279: the ring is not looked at
        label, picks, info = np.zeros(n, np.int8), [], []
    else:
        label, picks, info = run(curv, gap, n, K)
    ps = [e for s in info for e in s["picks"]]
    tot = {
        "n": n, "redone": sum(s["redone"] for s in info), "hit_sectors": sum(1 for s in info if s["marks"]),
        "carried": sum(1 for s in info if s["carried"]), "corners": sum(len(s["final"][0]) for s in info), "flats": sum(len(s["final"][1]) for s in info),
        "redo_after_redo": sum(1 for a, b in zip(info, info[1:]) if a["redone"] and b["redone"] and not (a["first_spill"] & b["marks"])),
        "prev_kills": sum(e["prev"] for e in ps), "next_kills": sum(e["next"] for e in ps),
        "lane_ties": {k: sum(1 for e in ps if e["kind"] == k and e["tie_lanes"] > 1) for k in ("corner", "flat")},
        "reg_ties": {k: sum(1 for e in ps if e["kind"] == k and e["tie_regs"] > 1) for k in ("corner", "flat")},
        "by_reg_lane": {}, "reach": {},
    }
    for e in ps:
        key = (e["kr"], lane_class(e["lane"])); tot["by_reg_lane"][key] = tot["by_reg_lane"].get(key, 0) + 1
        if e["fw"] is not None:
            key = (e["fw"], e["bk"]); tot["reach"][key] = tot["reach"].get(key, 0) + 1
    return {"curv": curv, "gap": gap, "labels": lab, "model_labels": label, "picks": picks, "sectors": info, "total": tot, "xyz": xyz}


def mutant_effect(f, mut):
    """labels a mutant of the scheme changes on a ring (facts f); for p: curvature values it changes"""
    n = len(f["curv"])
    if n - 11 < 6: return 0
    if mut == "p":
        return int((curvature_f32(f["xyz"], "p").view(np.uint32) != f["curv"].view(np.uint32))[5:n - 5].sum())
    label, _, _ = run(f["curv"], f["gap"], n, K6_4096 if n > 2059 else K6_2048, mut)
    return int((label != f["model_labels"]).sum())


# ------------------------------------------------------------------------------------------------ scenes
def sector_ring(n, per_sector, gaps=()):
    """spikes given per sector as {position in the sector: height}"""
    L = n - 11
    at = {}
    for j, d in enumerate(per_sector):
        for pos, h in d.items():
            assert 0 <= pos < (L * (j + 1)) // 6 - (L * j) // 6
            at[5 + (L * j) // 6 + pos] = h
    return spikes(n, at, gaps)


def c1_redo():
    """n = 101, sectors of 15: a spike of height 2 at position 13 of every sector marks positions 0 .. 3 of the next one, where a spike of
    height 1 at position 2 is the first pass's second corner: sectors 1 .. 5 are all redone"""
    return sector_ring(101, [{13: 2}] + [{2: 1, 13: 2}] * 5)


def c4_ties(kind):
    """n = 431, sectors of 70 (register 0 and lanes 0 .. 5 of register 1), the same pattern in every sector"""
    pat = {"corner_lanes": {10: 2, 30: 2, 50: 2},                            # one value in three lanes of register 0
           "corner_regs": {3: 1, 67: 1, 30: 1},                               # lane 3 of registers 0 and 1 (and lane 30, so that the order shows in the labels)
           "corner_both": {3: 1, 67: 1, 20: 1, 40: 1},
           "corner_border": {63: 1, 64: 1, 20: 1, 21: 1},                     # lane 63 of register 0 against lane 0 of register 1: adjacent spikes, 81 / 256 each
           "flat_lanes": {66: 2},                                             # register 1 dead after the corner: zeros tie over lanes of register 0 only
           "flat_both": {30: 2},                                              # zeros everywhere: lanes 0 .. 5 tie over both registers
           "flat_border": {2: 2, 13: 2, 24: 2, 35: 2, 46: 2, 57: 2}}[kind]    # positions 0 .. 62 dead: the zeros start at lane 63 of register 0
    return sector_ring(431, [pat] * 6)


def c4_flat_regs():
    """n = 431, sectors of 70.  Five points per sector stand between two gaps (reach 0, nobody can mark them): positions 20, 30, 40 with
    curvature 0, positions 3 and 67 - lane 3 of registers 0 and 1 - with 1 / 256 from a neighbour of height 1; corners kill everything else.
    The 4th flat is decided by a tie over the registers of ONE lane: position 3 is a flat, position 67 is not"""
    at, gaps = {}, []
    for j in range(6):
        b = 5 + 70 * j
        for P in (3, 20, 30, 40, 67): gaps += [b + P - 1, b + P]
        at.update({b + 11: 2, b + 52: 2, b + 58: 1, b + 5: 1, b + 65: 1})
    return spikes(431, at, gaps)


def border_ring(n, regs, mid=None, extra=None, gaps=()):
    """picks at lanes 0 .. 4 and 59 .. 63 of the registers listed (as far as the sector has them), spread over the six sectors so that no
    spike lies within reach of another or of the marks a sector leaves on the next: sector 0 takes lane 0, sector j = 1 .. 4 lanes j and
    58 + j, sector 5 lane 63 (height 1: spikes closer than 11 share neighbours, whose dZ must stay below 4); `mid` adds a lane of
    height 2 to every sector"""
    L = n - 11
    per = []
    for j in range(6):
        ln = (L * (j + 1)) // 6 - (L * j) // 6
        lanes = ([j] if j < 5 else []) + ([58 + j] if j >= 1 else []) + ([mid] if mid is not None else [])
        d = {kr * 64 + ln_: 2 if ln_ == mid else 1 for kr in regs for ln_ in lanes if kr * 64 + ln_ < ln}
        d.update((extra or {}).get(j, {}))
        per.append(d)
    return sector_ring(n, per, gaps)


def c10_long():
    """n = 4107, sectors of 682 / 683 (registers 0 .. 10): picks in registers 0, 3, 4, 7, 8, 10.  In sectors 0 and 3 a gap follows lane 31 of
    registers 4 and 6, and lane 34 of registers 8 and 10 holds a spike of height 1 inside the reach of the pick at lane 31: reading the reach of
    register kr - 4 for kr >= 8 (mutant n) leaves it alive.  Sector 0: a pick at lane 1 of register 9 must kill lane 60 of register 8, sector 5:
    one at lane 62 of register 9 must kill lane 3 of register 10 (c5_victims, behind register 8)"""
    L = 4096
    extra = {j: {8 * 64 + 34: 1, 10 * 64 + 31: 2, 10 * 64 + 34: 1, 6 * 64 + 31: 2} for j in (0, 3)}
    extra[0].update({9 * 64 + 1: 2, 8 * 64 + 60: 1})
    extra[5] = {9 * 64 + 62: 2, 10 * 64 + 3: 1}
    gaps = [5 + (L * j) // 6 + kr * 64 + 31 for j in (0, 3) for kr in (4, 6)]
    return border_ring(4107, (0, 3, 4, 7, 8, 10), mid=31, extra=extra, gaps=gaps)


C3_LENGTHS = (17, 18, 22, 23, 28, 35, 40)                                   # L = 6, 7, 11, 12, 17, 24, 29: sectors of 1 .. 4 (and 5) points
C8_LENGTHS = (17, 18, 22, 256, 261, 262, 266, 267, 272, 512, 517, 523, 1029, 2059)


def c8_ring(n):
    """pseudo-random spikes, and a spike of height 2 right behind every multiple of 256 so that the columns around a chunk border differ"""
    r = random_ring(n, 800 + n, 0.15)
    zs = np.rint(r[:, 2] * 16).astype(np.int64)
    for i in range(256, n - 5, 256):
        zs[max(0, i - 10):i + 12] = 0
        zs[i + 1] = 2
    return ring(zs)


def c5_victims():
    """n = 1163, sectors of 192 (registers 0 .. 2): a spike of height 2 two lanes from a register border and a spike of height 1 five points
    further on, in the neighbouring register: the pick must kill it there, in its last lane of reach.  Sector 0: register 0 -> 1, sector 1:
    1 -> 0, sector 2: 1 -> 2, sector 3: 2 -> 1, sector 4: both directions"""
    return sector_ring(1163, [{62: 2, 67: 1}, {65: 2, 60: 1}, {126: 2, 131: 1}, {129: 2, 124: 1}, {62: 2, 67: 1, 129: 2, 124: 1}, {}])


def c6_isolated():
    """n = 191, sectors of 30, every step a gap and z alternating between 0 and 2: all curvatures are 144 / 256, every reach is (0, 0): 30
    isolated candidates per sector, of which the 20 with the largest indices are picked and the other ten stay unmarked and are no flats"""
    return ring(np.arange(191) % 2 * 2, np.full(190, 5))


def c6_fourth_flat(corner=False):
    """n = 125, sectors of 19, no curvature anywhere: the flats of a sector are its positions 0, 6, 12 and 18, the 4th is the last point and must
    leave position 0 of the next sector alone.  No corner in any sector; `corner`: one spike in sector 2, so that its sharp cloud has one point"""
    return sector_ring(125, [{}, {}, {9: 2} if corner else {}, {}, {}, {}])


# tent height at the picked point for every reach (fw, bk), found by a search over -14 .. 14: the run between the two gaps is a tent of slope
# 2 * 2^-4 m per step with its top at the point, so that the point (dZ = C - 11 z, the same C for the whole run) outranks the run's ends,
# whose curvature the gap beside them already puts at 6.25
C7_TENT = {(0, 0): -1, (0, 1): 1, (0, 2): 2, (0, 3): 3, (0, 4): 4, (0, 5): 0, (1, 0): 2, (1, 1): 2, (1, 2): 3, (1, 3): 5, (1, 4): 6, (1, 5): 0,
           (2, 0): 3, (2, 1): 3, (2, 2): 4, (2, 3): 6, (2, 4): 7, (2, 5): 9, (3, 0): 4, (3, 1): 5, (3, 2): 6, (3, 3): 6, (3, 4): 7, (3, 5): 9,
           (4, 0): 6, (4, 1): 6, (4, 2): 7, (4, 3): 7, (4, 4): 7, (4, 5): 9, (5, 0): 0, (5, 1): 0, (5, 2): 9, (5, 3): 9, (5, 4): 9, (5, 5): 0}
C7_RESIDUES = (-4, -3, -2, -1, 0, 1, 2, 3, 4)               # i mod 32 with (i + 59) & 31 > 22: the 10-bit window leaves its 32-bit word


def c7_points(q):
    """ring q of four: the nine points (index, fw, bk) that must be picked with that reach; every second index lies at a multiple of 64"""
    combos = [(fw, bk) for fw in range(6) for bk in range(6)][9 * q:9 * q + 9]
    return [(32 * (k + 1) + C7_RESIDUES[(k + q) % 9], fw, bk) for k, (fw, bk) in enumerate(combos)]


def c7_ring(q):
    """n = 330: per point a run that ends fw steps ahead and bk steps behind in a gap (no gap within 8 steps where the reach is 5), z a tent
    over the run; a spike on the last point of the last sector"""
    at, gaps = {330 - 7: 2}, {}
    for P, fw, bk in c7_points(q):
        off = C7_TENT[(fw, bk)]
        for i in range(P - (bk if bk < 5 else 8), P + (fw if fw < 5 else 8) + 1):
            z = off - 2 * abs(i - P)
            at[i] = (max(z, 0) if off > 0 else min(z, 0)) if abs(i - P) > 5 else z
        if bk < 5: gaps[P - bk - 1] = 5
        if fw < 5: gaps[P + fw] = 5
    return spikes(330, at, gaps)


C9_INDEX = (27, 42, 57)                                       # position 7 of sectors 1, 2, 3 of a ring of 101
C9_BITS = (THR - 1, THR, THR + 1)
C9_Z_BITS = 0x3D0186BA                                        # z of the three points: dZ = -(10 z) rounded
C9_X_BITS = (0xC077FE67, 0xBF7FF997, 0x3FF00338)              # their x: 409, 1641, 824 ulps off the grid, dX = -(10 x) rounded against the exact sum


def c9_ring():
    """n = 101.  Three points between two gaps each (reach 0, nobody can mark them) whose f32 curvature has the bits of 0.1f - 1 ulp, 0.1f and
    0.1f + 1 ulp: dZ^2 with dZ = -fl(10 z), z near 0.0316, plus dX^2 with x a few hundred ulps off its grid position, found by a search
    over f32 values.  The first is a flat ((double)c < 0.1), the other two are corners ((double)0.1f > 0.1)"""
    r = spikes(101, {}, gaps=[s for i in C9_INDEX for s in (i - 1, i)])
    for i, xb in zip(C9_INDEX, C9_X_BITS):
        r[i, 0] = np.uint32(xb).view(np.float32)
        r[i, 2] = np.uint32(C9_Z_BITS).view(np.float32)
    return r


# ------------------------------------------------------------------------------------------------ the scenes by name
def _scenes():
    s = {"C1_redo": c1_redo(),
         "C2_chain": random_ring(59, 127, 0.2),       # sectors 3 and 4 are hit only by what the redone sector in front spills
         "C2_stop": random_ring(59, 0, 0.2)}          # sector 3: its pick lies under the pre-redo spill of sector 2, not under the final one
    for n in C3_LENGTHS: s["C3_flat_%d" % n] = spikes(n, {})
    for n, seed in zip(C3_LENGTHS, (77, 79, 67, 79, 5, 49, 75)): s["C3_gaps_%d" % n] = random_ring(n, seed, 0.25, 0.1)
    s["C3_none_16"] = spikes(16, {8: 2})
    for k in ("corner_lanes", "corner_regs", "corner_both", "corner_border", "flat_lanes", "flat_both", "flat_border"): s["C4_" + k] = c4_ties(k)
    s["C4_flat_regs"] = c4_flat_regs()
    s["C5_borders"] = border_ring(1163, (0, 1, 2))
    s["C5_victims"] = c5_victims()
    s["C5_gaps"] = random_ring(1163, 2, 0.08, 0.04)
    s["C6_end"] = random_ring(125, 2, 0.1, 0.3)
    s["C6_isolated"] = c6_isolated()
    s["C6_twenty"] = random_ring(251, 209, 0.1, 0.5)     # sector 1: 20 corners, and the 21st candidate has a flat inside its reach
    s["C6_fourth"] = c6_fourth_flat()
    s["C6_one"] = c6_fourth_flat(True)
    for q in range(4): s["C7_window_%d" % q] = c7_ring(q)
    for n in C8_LENGTHS: s["C8_%d" % n] = c8_ring(n)
    s["C9_threshold"] = c9_ring()
    s["C10_long_4107"] = c10_long()
    s["C10_2060"] = random_ring(2060, 2060, 0.1, 0.02)
    return s


_CACHE = {}


def scenes():
    """{name: ring}, built once"""
    if "s" not in _CACHE: _CACHE["s"] = _scenes()
    return _CACHE["s"]


def scene_facts(O, name):
    """facts of a scene, computed once and shared by the tests"""
    if name not in _CACHE: _CACHE[name] = facts(O, scenes()[name])
    return _CACHE[name]


LONG = ("C10_long_4107", "C10_2060")                          # need the <4096> instance
AGAIN_4096 = ("C1_redo", "C4_", "C5_")                        # run in both ring-capacity classes


def sweeps(long_context):
    """the scenes packed into sweeps of RINGS rings (ring ids 0 .. 7 in order): [(float32 (n, 4), [scene names])].  The <4096> context gets
    the long rings, C1, C4 and C5 again, and one sweep with a short-sector ring, an empty ring id and a full-length ring side by side"""
    sc = scenes()
    names = [k for k in sc if (k in LONG or k.startswith(AGAIN_4096)) == long_context or (long_context and k in LONG)] if long_context else [k for k in sc if k not in LONG]
    out = []
    for i in range(0, len(names), RINGS):
        part = names[i:i + RINGS]
        out.append((np.concatenate([with_id(sc[k], r) for r, k in enumerate(part)]), part))
    if long_context:
        out.append((np.concatenate([with_id(sc["C3_none_16"], 0), with_id(sc["C3_flat_17"], 1), with_id(sc["C10_long_4107"], 3), with_id(sc["C3_gaps_22"], 4),
                                    with_id(sc["C10_2060"], 6), with_id(sc["C3_flat_18"], 7)]), ["C3_none_16", "C3_flat_17", None, "C10_long_4107", "C3_gaps_22", None, "C10_2060", "C3_flat_18"]))
    return out
