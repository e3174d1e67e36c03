"""Constructed clouds for the voxel filters of the mapping stage (a-loam_amd/csrc/mapping_kernels.hip: the single-workgroup LDS filter k_vox_lds in its
three instances, and the general tile-sort / rank-merge path k_vox_setup ... k_vox_copyback), with the facts that show which line of a kernel each cloud
is there for.  No GPU in here.

`case(name, leaf)` returns the cloud (`points`, f32 [n, 4], intensity = ring + relative time, fractional), the `leaf` it was built for, `props` - what
properties() finds in it - and `expect` - the subset of those the builder promises; check() asserts the promise.  Builders work in units of the leaf, so
the same name can sit in the corner class (line resolution) or the surf class (plane resolution) of one context.

properties() restates, in numpy and in f32 where the kernels use f32, the conditions the kernels and voxel_device.hpp state: the cell of a point
(floor(p * (1 / leaf))), a run head (cell differs from the predecessor's), the box (PCL's guard on dx * dy * dz, min_b, div_b), the cell index with its
32-bit wrap, key_bits of the radix sort, cell_exact, the list vox_enlist puts a segment of n points on and whether that instance keeps the segment.

plain_filter() is the definition the filters are held to: group the points by cell index, keep first-appearance order inside a cell, add the members
in f32 one at a time starting from 0.f, divide by the count, emit the cells by ascending (unsigned) index; a box beyond PCL's guard returns its input.

One kind of box was suspect and is settled on the CPU (tests/test_voxel_cases.py): dx * dy * dz can pass the guard while div_b[0] * div_b[1] * div_b[2]
does not, because div_b exceeds dx by one where the box's minimum sits late in its cell - it does not take a long axis, 1290 cells a side are enough
(1290^3 <= 2^31 - 1 < 1291^3).  The cell index then passes 2^31 and wraps as a 32-bit integer.  `wrap-3d` and `wrap-2d` are such boxes; the oracle's
filter, plain_filter() with the same unsigned wrap and the reference-compiled mapping node agree on them (no two cells collide below 2^32, and all three
order the cells by the unsigned index), so they stay and are pinned on the GPU.  (The third is the project's stand-in VoxelGrid under the reference's own
node, not PCL itself; like PCL it multiplies ints and sorts on an unsigned index, and the agreement rests on the compiler wrapping those products.)
NOT examined: a div_b product above 2^32, which cell_exact still admits (2^23 x 257 x 2 cells pass the guard as (2^23 - 1) x 256 x 1).  There two cells
share one 32-bit index and PCL itself would merge them; no case here builds such a box, and the model of k_vox_lds in test_mapping_models.py, which
forms the index without the wrap, would not describe it.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

F = np.float32
TILE = 2048                                           # kVoxTile
INSTANCES = {"tiny": (64, 2048, 2048), "small": (256, 8192, 8192), "big": (1024, 24576, 65536)}   # k_vox_lds<NT, CAPR, CAPN>
MAX_CELLS = 2147483647                                # voxel::kMaxCells
EXACT_LIMIT = F(8388608.0)                            # voxel::kExactCellLimit
LEAVES = (0.4, 0.8)                                   # line / plane resolution of the contexts the GPU test opens
CUBE = 50.0                                           # edge of a map cube (reference src/laserMapping.cpp:72-80)


def inverse_leaf(leaf):
    return F(1.0) / F(leaf)


def cells_of(points, leaf):
    """voxel::cell_coord of every point and axis: floorf(p * inv), integer-valued f32."""
    return np.floor(np.asarray(points, F)[:, :3] * inverse_leaf(leaf))


def route(n):
    """vox_enlist: the list a segment of n points is put on."""
    return "none" if n <= 0 else "tiny" if n <= 2048 else "small" if n <= 8192 else "big" if n <= 65536 else "general"


def chunk_of(n, cls):
    """k_vox_lds: the contiguous, 64-aligned stretch of a segment one wave owns."""
    nw = INSTANCES[cls][0] // 64
    return ((n + nw - 1) // nw + 63) & ~63


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def box_of(points, leaf):
    """voxel::make_box: (unfiltered, min_b, div_b) with python integers."""
    p = np.asarray(points, F)[:, :3]
    inv = inverse_leaf(leaf)
    mn, mx = p.min(0), p.max(0)
    d = [int(np.int64((mx[q] - mn[q]) * inv)) + 1 for q in range(3)]
    unfiltered = _wrap64(d[0] * d[1] * d[2]) > MAX_CELLS
    minb = [int(np.floor(mn[q] * inv)) for q in range(3)]
    divb = [int(np.floor(mx[q] * inv)) - minb[q] + 1 for q in range(3)]
    return unfiltered, minb, divb, d


def cell_index(points, leaf, minb, divb):
    """voxel::cell_index: (int)(floorf(p * inv) - (float)min_b) per axis, combined in 32-bit arithmetic, read as unsigned."""
    ijk = (cells_of(points, leaf) - np.array(minb, np.int64).astype(F)).astype(np.int64)
    return (ijk[:, 0] + ijk[:, 1] * divb[0] + ijk[:, 2] * (divb[0] * divb[1] & 0xFFFFFFFF)) & 0xFFFFFFFF


def properties(points, leaf):
    p = np.asarray(points, F)
    n = len(p)
    c = cells_of(p, leaf)
    head = np.ones(n, bool)
    head[1:] = np.any(c[1:] != c[:-1], axis=1)
    starts = np.nonzero(head)[0]
    unfiltered, minb, divb, d = box_of(p, leaf)
    cells = divb[0] * divb[1] * divb[2]
    exact = bool(np.all(np.abs(c) < EXACT_LIMIT))
    cls = route(n)
    if unfiltered:
        vi, voxels, members, span = None, n, 1, 1
    else:
        vi = cell_index(p, leaf, minb, divb)
        val, cnt = np.unique(vi, return_counts=True)
        voxels, members = len(cnt), int(cnt.max())
        at = int(np.searchsorted(np.sort(vi), val[np.argmax(cnt)]))           # where the keys of the largest voxel start once sorted
        span = (at + members - 1) // TILE - at // TILE + 1
    tiles = (n + TILE - 1) // TILE
    return dict(n=n, runs=len(starts), max_run=int(np.diff(np.append(starts, n)).max()), voxels=voxels, max_members=members,
                unfiltered=unfiltered, guard_cells=d[0] * d[1] * d[2], divb=tuple(divb), cells=cells, key_bits=max(1, (cells - 1).bit_length()),
                cell_exact=exact, cls=cls, kept=cls != "general" and exact and len(starts) <= INSTANCES[cls][1],
                wraps=not unfiltered and cells > MAX_CELLS, voxel_tiles=span, tiles=tiles, merge_levels=max(0, (tiles - 1).bit_length()), last_tile=n - (tiles - 1) * TILE,
                index_min=None if vi is None else int(vi.min()), index_max=None if vi is None else int(vi.max()))


def plain_filter(points, leaf):
    """The definition (module docstring).  Summation in input order: the canonical order of DESIGN.md section 5."""
    p = np.ascontiguousarray(points, F)
    unfiltered, minb, divb, _ = box_of(p, leaf)
    if unfiltered:
        return p.copy()
    vi = cell_index(p, leaf, minb, divb)
    order = np.argsort(vi, kind="stable")                                      # ascending cell, input order inside a cell
    bounds = np.append(np.nonzero(np.append(True, np.diff(vi[order]) != 0))[0], len(p))
    out = np.empty((len(bounds) - 1, 4), F)
    zero = np.zeros((1, 4), F)
    for k in range(len(bounds) - 1):
        m = p[order[bounds[k]:bounds[k + 1]]]
        # np.cumsum in f32 adds one element at a time, left to right; the leading zero is Centroid's 0.f (0.f + -0.f = +0.f)
        out[k] = np.cumsum(np.concatenate([zero, m]), axis=0, dtype=F)[-1] / F(len(m))
    return out


# --------------------------------------------------------------------------------------------------------------------------- building blocks
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def place(ijk, leaf, frac):
    """Points inside the cells `ijk` [n, 3], at the fraction `frac` of the cell's edge (scalar or [n, 3]); moved by single ulps where the f32 product
    floor(p * inv) would land in a neighbour."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    want = ijk.astype(F)
    x = ((ijk + frac) * float(F(leaf))).astype(F)
    inv = inverse_leaf(leaf)
    for _ in range(64):
        got = np.floor(x * inv)
        if np.array_equal(got, want):
            return x
        x = np.where(got < want, np.nextafter(x, F(np.inf)), np.where(got > want, np.nextafter(x, F(-np.inf)), x)).astype(F)
    raise AssertionError("cells out of reach of f32")


def cloud(ijk, leaf, rng):
    """One point per row of `ijk`, spread inside its cell, with ring + relative-time intensities in input order."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    xyz = place(ijk, leaf, rng.uniform(0.15, 0.85, ijk.shape))
    return with_intensity(xyz)


def with_intensity(xyz, rings=16):
    n = len(xyz)
    i = np.arange(n)
    w = (i * rings // max(n, 1)) + 0.1 * ((i * 0.6180339887) % 1.0)            # ring + 0.1 relTime-like fraction
    return np.concatenate([np.asarray(xyz, F), w.astype(F)[:, None]], axis=1)


def tiled(points, n):
    """The same cloud over and over up to n points: same box and cells, more members, a size for the general path."""
    reps = (n + len(points) - 1) // len(points)
    return with_intensity(np.tile(points[:, :3], (reps, 1))[:n])


def ring_like(n, leaf, per_cell=2.8):
    """Ring-ordered returns: circles 0.13 leaves apart, 2.8 points per crossed cell - runs of one to five points, every voxel revisited by the next rings."""
    xs = []
    have, j = 0, 0
    while have < n:
        r = 12.0 + 0.13 * j
        m = int(8 * per_cell * r)
        a = 0.37 * j + np.arange(m) * (2 * np.pi / m)
        xs.append(np.stack([r * np.cos(a), r * np.sin(a), np.full(m, 0.3) + 0.2 * np.sin(5 * a)], 1))
        have += m; j += 1
    xyz = (np.concatenate(xs)[:n] * float(F(leaf))).astype(F)
    return with_intensity(xyz)


def runs_of(lengths, cells, leaf, rng):
    """Runs of the given lengths, run k inside cells[k % len(cells)]."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    ijk = np.repeat(cells[np.arange(len(lengths)) % len(cells)], lengths, axis=0)
    return cloud(ijk, leaf, rng)


def boxed(dims, n, leaf, rng, distinct=60, origin=(0, 0, 0)):
    """Two anchors in the first and the last cell of a dims[0] x dims[1] x dims[2] box (cell index 0 and cells - 1), then n - 2 points clustered in
    `distinct` cells drawn over the whole box, so that every digit of the index varies; cells come back many times.  `origin`: the cell the box starts at."""
    dims = np.asarray(dims, np.int64)
    pick = np.stack([rng.integers(0, d, distinct) for d in dims], 1)
    pick[0] = 0; pick[1] = dims - 1                                            # members besides the anchors in the first and the last cell
    seq = rng.integers(0, distinct, n - 2)
    ijk = np.concatenate([[np.zeros(3, np.int64)], pick[seq[: (n - 2) // 2]], [dims - 1], pick[seq[(n - 2) // 2:]]])
    return cloud(ijk + np.asarray(origin, np.int64), leaf, rng)


def far_slab(n, leaf, rng, own=()):
    """A thin slab (x below 3000 cells, three rows of y, one of z) and one point 9 000 000 cells out in x: cell_exact fails, the general path takes the segment
    whatever its size, and the box stays inside PCL's guard.  `own`: (odd cell x, members) of voxels that are to hold many members, spread over the input."""
    m = n - 1 - sum(k for _, k in own)
    ijk = np.stack([2 * rng.integers(0, 1500, m), rng.integers(0, 3, m), np.zeros(m, np.int64)], 1) if m > 0 else np.zeros((0, 3), np.int64)
    for cx, k in own:
        at = np.sort(rng.choice(len(ijk) + k, k, replace=False))
        full = np.empty((len(ijk) + k, 3), np.int64)
        mask = np.zeros(len(full), bool); mask[at] = True
        full[mask] = (cx, 1, 0); full[~mask] = ijk
        ijk = full
    pts = cloud(ijk, leaf, rng)
    far = with_intensity(place([[9_000_000, 1, 0]], leaf, 0.5))
    k = min(len(pts), 1234 % max(n, 1))
    out = np.concatenate([pts[:k], far, pts[k:]])
    out[:, 3] = with_intensity(out[:, :3])[:, 3]
    return out


# --------------------------------------------------------------------------------------------------------------------------- the cases
LIMIT_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 65535, 65536, 65537)
FAR_SIZES = (1, 2047, 2048, 2049, 4096, 4097, 6144, 6145)
KEY_BOXES = {                                        # name -> (dims, key_bits); products 2, 128, 129, 2^14, 2^14 + 1, 2^21, 2^21 + 1, 2^28, > 2^28
    "1d-2": ((2, 1, 1), 1), "1d-128": ((1, 128, 1), 7), "1d-129": ((1, 1, 129), 8), "1d-2^14": ((16384, 1, 1), 14), "1d-2^14+1": ((1, 16385, 1), 15),
    "1d-2^21": ((1, 1, 2097152), 21), "1d-2^21+1": ((2097153, 1, 1), 22),
    "2d-128": ((16, 8, 1), 7), "2d-129": ((3, 1, 43), 8), "2d-2^14": ((1, 128, 128), 14), "2d-2^14+1": ((145, 113, 1), 15), "2d-2^21": ((2048, 1, 1024), 21),
    "2d-2^21+1": ((1, 387, 5419), 22), "2d-2^28": ((16384, 16384, 1), 28),
    "3d-128": ((8, 4, 4), 7), "3d-2^14": ((32, 32, 16), 14), "3d-2^14+1": ((5, 29, 113), 15), "3d-2^21": ((128, 128, 128), 21), "3d-2^21+1": ((9, 43, 5419), 22),
    "3d-2^28": ((1024, 512, 512), 28), "3d-2^28+": ((1025, 512, 512), 29),
}
KEY_SIZES = {"1d-2^14+1": 3000, "2d-2^21+1": 3000, "3d-2^28+": 3000, "3d-2^21+1": 9000, "2d-2^28": 9000, "2d-2^14+1": 9000}   # small / big instance; the rest 400 (tiny)


def _build(name, leaf):
    rng = _rng(name)
    kind, _, arg = name.partition("-")
    if kind == "limits":                              # 1. routing limits
        n = int(arg)
        pts = ring_like(n, leaf)
        ex = dict(n=n, cls=route(n), kept=n <= 65536, cell_exact=True, unfiltered=False)
        return pts, ex
    if kind == "onecell":                             # 2. one run, one voxel, a serial sum of n members
        n = int(arg)
        return cloud(np.tile([[3, -2, 1]], (n, 1)), leaf, rng), dict(n=n, runs=1, voxels=1, max_members=n, key_bits=1, kept=True)
    if kind == "abab":                                # A B A B ...: every point a run, two voxels, one key bit
        n = int(arg)
        return runs_of(np.ones(n, np.int64), [[-1, 0, 0], [0, 0, 0]], leaf, rng), dict(n=n, runs=n, voxels=2, max_members=n // 2, key_bits=1, kept=True)
    if name == "interleave5000":                      # V x V y V z V x ...: 5000 single-point runs of one voxel between those of three others
        cells = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 0]])
        return runs_of(np.ones(10000, np.int64), cells, leaf, rng), dict(n=10000, runs=10000, voxels=4, max_members=5000, key_bits=2, cls="big", kept=True)
    if kind == "runlen":                              # runs as long as a wave's chunk, one shorter, one longer: a run boundary on, before, behind every wave's first point
        cls, d = arg.split("@")
        n = {"tiny": 2048, "small": 8192, "big": 65536}[cls]
        length = chunk_of(n, cls) + int(d)
        k = (n + length - 1) // length
        lengths = np.full(k, length, np.int64); lengths[-1] = n - length * (k - 1)
        return runs_of(lengths, [[0, 0, 0], [2, 1, 0], [1, 0, 1]], leaf, rng), dict(n=n, runs=k, max_run=length, voxels=min(k, 3), cls=cls, kept=True)
    if kind == "runs64" or kind == "runs65":          # runs of exactly one row of a wave, and one more
        n, length = int(arg), int(kind[4:])
        k = (n + length - 1) // length
        lengths = np.full(k, length, np.int64); lengths[-1] = n - length * (k - 1)
        return runs_of(lengths, [[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 1, 1], [2, 0, 1]], leaf, rng), dict(n=n, runs=k, max_run=length, voxels=5, kept=True)
    if kind == "capr":                                # 3. 40 000 points, exactly `arg` runs: an all-distinct line of cells, neighbours merged from the front
        runs, n = int(arg), 40000
        lengths = np.ones(runs, np.int64); lengths[: n - runs] = 2
        ijk = np.zeros((runs, 3), np.int64); ijk[:, 0] = np.arange(runs) % 200; ijk[:, 1] = np.arange(runs) // 200
        return cloud(np.repeat(ijk, lengths, axis=0), leaf, rng), dict(n=n, runs=runs, voxels=runs, cls="big", kept=runs <= 24576, cell_exact=True)
    if kind == "keybits":                             # 4. key width
        dims, bits = KEY_BOXES[arg]
        n = KEY_SIZES.get(arg, 400)
        cells = dims[0] * dims[1] * dims[2]
        return boxed(dims, n, leaf, rng), dict(n=n, divb=tuple(dims), cells=cells, key_bits=bits, index_min=0, index_max=cells - 1, kept=True, cls=route(n))
    if name == "keybits_general-1d-2^28+1":           # a box of 2^28 + 1 cells along x: far beyond exact cells, the general path's 64-bit keys
        inv = inverse_leaf(leaf)
        x = F(268435456.0 * float(F(leaf)))
        cand = [x]
        for _ in range(200):
            cand.append(np.nextafter(cand[-1], F(np.inf)))
        top = next(c for c in cand if np.floor(c * inv) == F(268435456.0))
        pts = boxed((3000, 3, 1), 400, leaf, rng)
        pts[200, 0] = top
        return pts, dict(n=400, divb=(268435457, 3, 1), key_bits=30, cell_exact=False, kept=False, unfiltered=False)
    if name == "lattice":                             # 5. exact multiples of the leaf, both signs, both zeros, one ulp to either side of every face
        lf = float(F(leaf))
        face = np.array([k * lf for k in range(-6, 7)]).astype(F)
        v = np.concatenate([face, np.nextafter(face, F(np.inf)), np.nextafter(face, F(-np.inf)), [F(-0.0), F(0.0)]]).astype(F)
        mid = place(np.array([[1, -2, 0]]), leaf, 0.5)[0]
        rows = []
        for axis in range(3):
            for a in v[rng.permutation(len(v))]:
                q = mid.copy(); q[axis] = a
                rows.append(q)
        rows += [[F(-0.0)] * 3, [F(0.0)] * 3, [F(-0.0), F(0.0), F(-0.0)]]
        return with_intensity(np.array(rows, F)), dict(cell_exact=True, cls="tiny", kept=True, unfiltered=False)
    if name == "minfrac09":                           # the box's minimum 0.9 leaves into its cell: div_b = dx + 1 on every axis
        ijk = np.stack([rng.integers(0, 41, 600), rng.integers(0, 31, 600), rng.integers(0, 6, 600)], 1)
        ijk[::3] = ijk[1::3][: len(ijk[::3])]
        xyz = place(ijk, leaf, rng.uniform(0.2, 0.8, ijk.shape))
        lo, hi = place([[0, 0, 0]], leaf, 0.9)[0], place([[40, 30, 5]], leaf, 0.5)[0]
        xyz[ijk == 0] = np.broadcast_to(lo, xyz.shape)[ijk == 0]              # nothing of cell 0 of an axis lies in front of 0.9
        xyz[7], xyz[311] = lo, hi
        return with_intensity(xyz), dict(divb=(41, 31, 6), guard_cells=40 * 30 * 5, kept=True, unfiltered=False)
    if kind == "guard":                               # PCL's overflow guard at its edge: 1290^3 <= 2^31 - 1 < 1291 * 1290^2
        top = 1289 if arg == "in" else 1290
        pts = boxed((top + 1, 1290, 1290), 500, leaf, rng)
        pts[0, :3] = place([[0, 0, 0]], leaf, 0.1)[0]
        pts[250, :3] = place([[top, 1289, 1289]], leaf, 0.5)[0]
        ex = dict(guard_cells=(top + 1) * 1290 * 1290, unfiltered=arg == "out", cell_exact=True, cls="tiny", kept=True)
        if arg == "in":
            ex.update(divb=(1290, 1290, 1290), wraps=False, key_bits=31)
        return pts, ex
    if kind == "wrap":                                # dx dy dz passes the guard, div_b's product does not: the cell index wraps past 2^31
        dims = (1291, 1291, 1291) if arg == "3d" else (46341, 46341, 1)
        org = np.array([-645, -645, -645] if arg == "3d" else [0, 0, 0])     # (3d: centred, +-258 m at a 0.4 m leaf - inside the 21 x 21 x 11 cube window)
        pts = boxed(dims, 500, leaf, rng, origin=org)
        lo = place([org], leaf, 0.9)[0]
        xyz = pts[:, :3]
        c = cells_of(pts, leaf)
        xyz[c == org] = np.broadcast_to(lo, xyz.shape)[c == org]              # the minimum of every axis sits 0.9 leaves into the box's first cell
        if arg == "2d":
            xyz[:, 2] = place([[0, 0, 0]], leaf, 0.5)[0, 2] + F(0.25 * leaf) * (np.arange(len(xyz)) % 2).astype(F)
        hi = place([org + np.array(dims) - 1], leaf, 0.5)[0]
        xyz[250] = hi if arg == "3d" else [hi[0], hi[1], xyz[250, 2]]
        g = (dims[0] - 1) * (dims[1] - 1) * max(dims[2] - 1, 1)
        return pts, dict(unfiltered=False, guard_cells=g, divb=tuple(dims), wraps=True, key_bits=32, cell_exact=True, kept=True)
    if kind == "general":                             # a cloud of section 5 (or a key box) repeated up to 65 537 points: the same box and cells through the general path
        base, _ = _build(arg, leaf)
        return tiled(base, 65537), dict(n=65537, cls="general", kept=False, last_tile=1, tiles=33, merge_levels=6)
    if kind == "far":                                 # 6. general path at small sizes
        if arg == "v2500":                            # one voxel's 2500 members lie across the first tile edge of the sorted keys
            pts = far_slab(4097, leaf, rng, own=((1501, 2500),))
            ex = dict(n=4097, max_members=2500, voxel_tiles=2, tiles=3, last_tile=1)
        elif arg == "v5000":                          # 5000 members spread over 10 000 points: sorted, they start in tile 0 or 1 and cover two whole tiles more
            pts = far_slab(10000, leaf, rng, own=((1501, 5000),))
            ex = dict(n=10000, max_members=5000, voxel_tiles=3, tiles=5, merge_levels=3)
        elif arg == "65537":                          # the tail tile holds one key: the far point, a voxel of its own
            pts = far_slab(65537, leaf, rng)
            ex = dict(n=65537, tiles=33, last_tile=1, merge_levels=6, cls="general")
        else:
            n = int(arg)
            pts = far_slab(n, leaf, rng)
            ex = dict(n=n, tiles=(n + TILE - 1) // TILE, last_tile=n - (n - 1) // TILE * TILE)
        ex.update(cell_exact=False, kept=False, unfiltered=False)
        return pts, ex
    raise KeyError(name)


RUNS = tuple(f"onecell-{n}" for n in (2048, 8192, 65536)) + ("abab-2048", "abab-8192", "abab-24576", "interleave5000") + \
    ("runlen-tiny@-1",) + tuple(f"runlen-{c}@{d}" for c in ("small", "big") for d in (0, -1, 1)) + ("runs64-2048", "runs65-2048", "runs64-5000", "runs65-5000", "runs64-20000", "runs65-20000")
LIMITS = tuple(f"limits-{n}" for n in LIMIT_SIZES)
CAPR = ("capr-24576", "capr-24577")
KEYBITS = tuple(f"keybits-{k}" for k in KEY_BOXES) + ("keybits_general-1d-2^28+1",)
ARITH = ("lattice", "minfrac09", "guard-in", "guard-out", "wrap-3d", "wrap-2d")
GENERAL = tuple(f"far-{n}" for n in FAR_SIZES) + ("far-v2500", "far-v5000", "far-65537") + tuple(f"general-{a}" for a in ARITH) + ("general-keybits-3d-2^21+1",)
ALL = LIMITS + RUNS + CAPR + KEYBITS + ARITH + GENERAL


@functools.lru_cache(maxsize=None)
def case(name, leaf):
    pts, expect = _build(name, leaf)
    pts = np.ascontiguousarray(pts, F)
    pts.setflags(write=False)
    return SimpleNamespace(name=name, leaf=leaf, points=pts, expect=expect, props=properties(pts, leaf))


def check(c):
    """The builder's promise: every expected property is what properties() finds in the cloud."""
    for k, v in c.expect.items():
        assert c.props[k] == v, (c.name, c.leaf, k, c.props[k], v)
    return c


# --------------------------------------------------------------------------------------------------------------------------- the in-place cube re-filter
def cube_frames(total, leaf, name="cube"):
    """7. Two frames into the centre cube (|x|, |y|, |z| < 25 m).  Frame 1: total // 2 points, each in a voxel of its own.  Frame 2: the rest; every second
    one lands in a voxel frame 1 occupied, the others in new ones, each again alone in its voxel.  Both clouds pass the incoming filter as they are (one
    member per voxel), so the cube's segment holds `total` points when its re-filter starts."""
    rng = _rng(f"{name}-{total}")
    side = int(2 * 24.0 / float(F(leaf)))                                    # cells across 48 m
    n1, n2 = total // 2, total - total // 2
    flat = rng.choice(side ** 3 if side ** 3 < 4_000_000 else 4_000_000, n1 + n2, replace=False)
    ijk = np.stack([flat % side, flat // side % side, flat // (side * side)], 1) - side // 2
    first, new = ijk[:n1], ijk[n1:]
    again = first[rng.permutation(n1)[: n2 // 2]]
    second = new.copy(); second[::2][: len(again)] = again[: len(second[::2])]
    return cloud(first, leaf, rng), cloud(second, leaf, rng)


CUBE_TOTALS = (2048, 2049, 8192, 8193, 65536, 65537)


def unfiltered_cube_frames(leaf=0.03):
    """Points at opposite corners of the centre cube with a leaf of 0.03 m: 1600^3 cells, beyond PCL's guard, for the incoming filter and for the cube's
    re-filter alike - both return what they were given."""
    rng = _rng("unfiltered-cube")
    out = []
    for k in range(2):
        xyz = rng.uniform(-20.0, 20.0, (300, 3)).astype(F)
        xyz[5 + k], xyz[200 + k] = (-24.0, -24.0, -24.0), (24.0, 24.0, 24.0)
        xyz[100:110] = xyz[90:100]                                             # members that a filter would merge
        out.append(with_intensity(xyz))
    return out


# --------------------------------------------------------------------------------------------------------------------------- many segments on the small list
SHEET_CUBES = [(i, j) for i in range(-2, 3) for j in range(-2, 3)]             # the 5 x 5 cubes of the window's middle layer


def sheet_frames(leaf, sizes=(2100, 7000), add=1000):
    """8. Two surf frames over 25 cubes, for batches that put more segments on the small list than its launch has workgroups.  Frame 1 gives cube c
    sizes[c % 2] points on lattice sites of their own (a long segment beside a short one); frame 2 adds `add` points per cube, every second one a point
    of frame 1 moved by less than 0.2 leaves, so the cube's segment holds sizes[c % 2] + add points - above 2048, at most 8192 - before a re-filter that
    merges.  With a leaf of 1e-5 m (sites 20 cells apart, as far as f32 resolves them) the cubes 100 m out hold cells beyond 2^23: the instance hands
    them back, the cubes within 50 m it keeps.  The cloud is thin in z, so the box of the incoming filter stays below 2^63 cells (no 64-bit wrap)."""
    rng = _rng(f"sheet-{leaf}")
    lf = float(F(leaf))
    pitch = max(lf, 2e-4)
    g = np.arange(-10, 11)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    f1, f2 = [], []
    for c, (i, j) in enumerate(SHEET_CUBES):
        m = sizes[c % 2]
        centre = np.array([i, j, 0]) * CUBE
        sites = (np.round(centre / pitch) + lattice[rng.permutation(len(lattice))[: m + add // 2]]) * pitch + 0.5 * lf
        first = sites[:m] + rng.uniform(-0.3, 0.3, (m, 3)) * lf
        again = first[rng.permutation(m)[: add - add // 2]] + rng.uniform(-0.2, 0.2, (add - add // 2, 3)) * lf
        second = np.empty((add, 3))
        second[0::2], second[1::2] = again, sites[m:]
        f1.append(first); f2.append(second)
    return with_intensity(np.concatenate(f1).astype(F)), with_intensity(np.concatenate(f2).astype(F))


def sheet_cube_of(points):
    """Index into SHEET_CUBES of every point (cubes are 50 m wide, centred on multiples of 50 m)."""
    ij = np.floor((np.asarray(points, np.float64)[:, :2] + CUBE / 2) / CUBE).astype(np.int64)
    return (ij[:, 0] + 2) * 5 + ij[:, 1] + 2
