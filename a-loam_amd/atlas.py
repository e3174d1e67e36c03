"""Map tiles on the host (numpy only): the record that the map spill produces (aloam_map_tile), a log that collects drained spills, files,
a model of the window arithmetic - which cubes a shift empties, and the window cut out of a set of tiles at any centre - and the model
of the map assembled from keyframe clouds at the poses of a pose graph (tiles_from_keyframes, aloam_graph_export_map).

A tile is one 50 m cube of one class with ABSOLUTE cube coordinates: window index (i, j, k) minus the window centre (cenW, cenH, cenD),
which is int((t + 25) / 50), minus one when t + 25 < 0, of the coordinates of its points (reference src/laserMapping.cpp:312-321).  The
centre only maps absolute cubes to window indices, so tiles cut from different windows of one map fit together.
"""
from __future__ import annotations

import numpy as np

from .records import MAP_TILE_DTYPE as TILE_DTYPE

W, H, D = 21, 21, 11                                    # reference src/laserMapping.cpp:75-77
DIMS = (W, H, D)
N_CUBES = W * H * D
assert TILE_DTYPE.itemsize == 32


def index_of(i, j, k):
    return i + W * j + W * H * k


def ijk_of(index):
    return index % W, (index // W) % H, index // (W * H)


# ---- the window shift (reference src/laserMapping.cpp:323-507 as k_map_begin runs it) ------------------------------------------------
def shift_of(center):
    """How far the window moves for a centre cube at window index `center` (three ints): per axis +1 while the index is below 3, -1 while it
    is above n - 4, at most 64 shifts per axis (the guard of k_map_begin)."""
    s = []
    for c, n in zip(center, DIMS):
        d = 0
        for _ in range(64):
            step = 1 if c < 3 else (-1 if c >= n - 3 else 0)
            if step == 0:
                break
            c += step
            d += step
        s.append(d)
    return tuple(s)


def survives(index, s):
    """A cube survives a shift by s iff every shifted index stays inside the window (a slab that re-enters is empty)."""
    return all(0 <= x + d < n for x, d, n in zip(ijk_of(index), s, DIMS))


def spill_of(cubes, cen, s, frame=0, room=None, dropped=None):
    """The tiles a shift by `s` of a window centred at `cen` cuts: cubes = [{index: (n, 4) points}] * 2 (corner, surf).  Returns
    (tiles, points) in the order of the device: corner row then surf row, each in ascending window index.  room = [(tiles, points)] * 2:
    what is left of the class rows - a tile that does not fit is left out whole and takes no room; dropped (a list) receives (tiles, points)
    of those."""
    tiles, pts, first, lost = [], [], 0, [0, 0]
    for cls in (0, 1):
        left = list(room[cls]) if room is not None else None
        for index in sorted(cubes[cls]):
            p = cubes[cls][index]
            if len(p) and not survives(index, s):
                if left is not None:
                    if left[0] < 1 or left[1] < len(p):
                        lost[0] += 1
                        lost[1] += len(p)
                        continue
                    left[0] -= 1
                    left[1] -= len(p)
                t = np.zeros((), TILE_DTYPE)
                t["cube"] = np.array(ijk_of(index)) - np.array(cen)
                t["feature_class"], t["count"], t["frame"], t["first_point"] = cls, len(p), frame, first
                tiles.append(t)
                pts.append(np.asarray(p, np.float32).reshape(-1, 4))
                first += len(p)
    if dropped is not None:
        dropped[:] = lost
    return (np.array(tiles, TILE_DTYPE) if tiles else np.zeros(0, TILE_DTYPE)), (np.concatenate(pts) if pts else np.zeros((0, 4), np.float32))


# ---- tiles of a context ------------------------------------------------------------------------------------------------------------------
def tiles_of_window(cubes, cen, frame=0):
    """cubes = [{index: points}] * 2 of a window centred at `cen` -> (tiles, points)."""
    return spill_of(cubes, cen, (64, 64, 64), frame)    # a shift that empties everything


def window_tiles(gpu, seq=0):
    """The current window of sequence `seq` of a binding.Aloam context as tiles (synchronises)."""
    info = gpu.map_info(seq)
    return tiles_of_window([gpu.map_cubes(cls, seq) for cls in (0, 1)], (info["cenW"], info["cenH"], info["cenD"]), info["frame_count"])


def concatenate(parts):
    """[(tiles, points), ...] -> one (tiles, points) with first_point rebased; the order of the parts and of their tiles is kept."""
    tiles, pts, base = [], [], 0
    for t, p in parts:
        t = np.array(t, TILE_DTYPE, copy=True)
        p = np.asarray(p, np.float32).reshape(-1, 4)
        t["first_point"] += base
        base += len(p)
        tiles.append(t)
        pts.append(p)
    return (np.concatenate(tiles) if tiles else np.zeros(0, TILE_DTYPE)), (np.concatenate(pts) if pts else np.zeros((0, 4), np.float32))


class TileLog:
    """Collects drained spills (Aloam.export_map_spill) of one sequence, in the order they were cut."""

    def __init__(self):
        self.parts = []

    def add(self, tiles, points):
        if len(tiles):
            self.parts.append((np.array(tiles, TILE_DTYPE, copy=True), np.array(points, np.float32, copy=True).reshape(-1, 4)))

    def result(self, *more):
        """Everything logged so far, followed by `more` (e.g. window_tiles of the final window)."""
        return concatenate(self.parts + list(more))


def save_atlas(path, tiles, points, places=None):
    """places: the stored places that go with the map (structured array of binding.PLACE_DTYPE, aloam_places_export), kept as raw bytes."""
    extra = {} if places is None else {"places": np.ascontiguousarray(places).view(np.uint8).reshape(-1)}
    np.savez_compressed(path, tiles=np.asarray(tiles, TILE_DTYPE), points=np.asarray(points, np.float32).reshape(-1, 4), **extra)


def load_atlas_places(path):
    """The places of a save_atlas file (binding.PLACE_DTYPE); none when it was written without them."""
    from .binding import PLACE_DTYPE
    with np.load(path) as z:
        raw = np.asarray(z["places"], np.uint8) if "places" in z.files else np.zeros(0, np.uint8)
    return raw.view(PLACE_DTYPE).copy()


def load_atlas(path):
    with np.load(path) as z:
        return np.asarray(z["tiles"], TILE_DTYPE), np.asarray(z["points"], np.float32).reshape(-1, 4)


# ---- the map of a pose graph: keyframe clouds at the graph's poses (aloam_graph_export_map) --------------------------------
CUBE_MIN, CUBE_MAX = -512, 511                          # absolute cubes an atlas holds per axis


def associate_to_map(points, q, t):
    """pointAssociateToMap as the device evaluates it (map_search_device.hpp, lm_device.hpp quat_rotate): q = (x, y, z, w), every product,
    sum and difference a separately rounded f64 operation in this order, each component stored to f32, the intensity kept."""
    p = np.asarray(points, np.float32).reshape(-1, 4)
    q0, q1, q2, q3 = (np.float64(v) for v in q)
    t0, t1, t2 = (np.float64(v) for v in t)
    vx, vy, vz = (p[:, k].astype(np.float64) for k in range(3))
    ux, uy, uz = q1 * vz - q2 * vy, q2 * vx - q0 * vz, q0 * vy - q1 * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    ox = vx + q3 * ux + (q1 * uz - q2 * uy)
    oy = vy + q3 * uy + (q2 * ux - q0 * uz)
    oz = vz + q3 * uz + (q0 * uy - q1 * ux)
    out = np.empty_like(p)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = (ox + t0).astype(np.float32), (oy + t1).astype(np.float32), (oz + t2).astype(np.float32), p[:, 3]
    return out


def cube_coord(v):
    """int((v + 25) / 50), minus one when v + 25 < 0, of f32 coordinates widened to f64 (cube_coord with centre 0): -75 lands in -2."""
    s = np.asarray(v, np.float32).astype(np.float64) + 25.0
    return np.trunc(s / 50.0).astype(np.int64) - (s < 0)


def tiles_from_keyframes(q, t, clouds, leaves, voxel_filter, stats=None):
    """The map of keyframes k = 0 .. K-1 with poses (q[k], t[k]) and sensor-frame clouds clouds[k] = (corner, surf): every point through
    associate_to_map, into the cube of its coordinates; the members of a (cube, class) - node order, then point order inside the node - are
    filtered once with voxel_filter(points, leaves[class]) (the caller's input-order pcl::VoxelGrid), always, also with one contributor.
    Returns (tiles, points): corner tiles, then surf tiles, each ascending in (cube[0], cube[1], cube[2]), frame 0.  Points whose cube
    lies outside -512 .. 511 on some axis are left out.  stats (a dict) receives tiles, points, raw_points (per class) and outside."""
    members = ({}, {})
    outside = 0
    for k, cl in enumerate(clouds):
        for cls in (0, 1):
            w = associate_to_map(cl[cls], q[k], t[k])
            if not len(w):
                continue
            cube = np.stack([cube_coord(w[:, a]) for a in range(3)], 1)
            ok = np.all((cube >= CUBE_MIN) & (cube <= CUBE_MAX), 1)
            outside += int(np.count_nonzero(~ok))
            for key in sorted(set(map(tuple, cube[ok].tolist()))):
                members[cls].setdefault(key, []).append(w[ok & np.all(cube == np.array(key), 1)])
    tiles, pts, first = [], [], 0
    st = {"tiles": [0, 0], "points": [0, 0], "raw_points": [0, 0], "outside": outside}
    for cls in (0, 1):
        for key in sorted(members[cls]):
            raw = np.concatenate(members[cls][key])
            p = np.asarray(voxel_filter(raw, leaves[cls]), np.float32).reshape(-1, 4)
            tl = np.zeros((), TILE_DTYPE)
            tl["cube"] = key
            tl["feature_class"], tl["count"], tl["frame"], tl["first_point"] = cls, len(p), 0, first
            tiles.append(tl)
            pts.append(p)
            first += len(p)
            st["tiles"][cls] += 1
            st["points"][cls] += len(p)
            st["raw_points"][cls] += len(raw)
    if stats is not None:
        stats.update(st)
    return (np.array(tiles, TILE_DTYPE) if tiles else np.zeros(0, TILE_DTYPE)), (np.concatenate(pts) if pts else np.zeros((0, 4), np.float32))


def tiles_from_parts(parts, leaves, voxel_filter, frames=None, stats=None):
    """The map of a group of parts (aloam_graph_export_map_joint).  parts = [(q[k], t[k], clouds[k], frame), ...]: the poses
    and sensor-frame clouds of a run of nodes and the frame they stand under, -1 (or None) for the poses as they are, else an index into
    frames = [(q_A xyzw, t_A) as seven numbers, ...], in which case every pose becomes posegraph.compose(A, X_k), nothing renormalised.  The
    result is tiles_from_keyframes of the concatenation, in part order: that is the whole definition."""
    from .posegraph import compose
    q, t, clouds = [], [], []
    for pq, pt, pc, frame in parts:
        for k in range(len(pc)):
            qk, tk = np.asarray(pq[k], np.float64), np.asarray(pt[k], np.float64)
            if frame is not None and frame >= 0:
                A = np.asarray(frames[frame], np.float64).reshape(7)
                qk, tk = compose(A[:4], A[4:], qk, tk)
            q.append(qk)
            t.append(tk)
            clouds.append(pc[k])
    return tiles_from_keyframes(q, t, clouds, leaves, voxel_filter, stats)


def window_centre(t_w_curr):
    """The window centre that puts the sensor's cube at the middle of the window: (10, 10, 5) - cube of the f64 position."""
    s = np.asarray(t_w_curr, np.float64) + 25.0
    cube = np.trunc(s / 50.0).astype(np.int64) - (s < 0)
    return tuple(int(v) for v in np.array([10, 10, 5]) - cube)


def window_from_keyframes(q, t, clouds, leaves, voxel_filter, cen, stats=None):
    """The window aloam_graph_apply builds: Atlas(*tiles_from_keyframes(...)).cut(cen), [{window index: points}] * 2.  stats (a dict)
    receives tiles_from_keyframes' figures plus cubes and points of the window (per class) and outside_window, the filtered points of the
    tiles that the window leaves out."""
    st = {}
    atlas = Atlas(*tiles_from_keyframes(q, t, clouds, leaves, voxel_filter, st))
    cut = atlas.cut(cen)
    if stats is not None:
        stats.update(st)
        stats["cubes"] = [len(c) for c in cut]
        stats["window_points"] = [sum(len(p) for p in c.values()) for c in cut]
        stats["outside_window"] = sum(st["points"]) - sum(stats["window_points"])
    return cut


# ---- a set of tiles as a map of any extent ---------------------------------------------------------------------------------------------
class Atlas:
    """Tiles keyed by (absolute cube, class).  Several tiles of one key (a cube that left the window, was re-entered and left again) are
    concatenated in array order; no voxel filter is applied here."""

    def __init__(self, tiles, points):
        tiles, points = np.asarray(tiles, TILE_DTYPE), np.asarray(points, np.float32).reshape(-1, 4)
        self.cubes = ({}, {})
        for t in tiles:
            cls, n, f = int(t["feature_class"]), int(t["count"]), int(t["first_point"])
            if cls not in (0, 1) or n < 0 or f < 0 or f + n > len(points):
                raise ValueError("bad tile")
            if n:
                key = tuple(int(v) for v in t["cube"])
                prev = self.cubes[cls].get(key)
                self.cubes[cls][key] = points[f:f + n] if prev is None else np.concatenate([prev, points[f:f + n]])

    def counts(self):
        """(cubes, points) per class."""
        return [(len(c), sum(len(p) for p in c.values())) for c in self.cubes]

    def cut(self, cen):
        """The window centred at `cen`: [{window index: points}] * 2, what Aloam.set_map takes."""
        out = ({}, {})
        for cls in (0, 1):
            for key, p in self.cubes[cls].items():
                ijk = [a + c for a, c in zip(key, cen)]
                if all(0 <= x < n for x, n in zip(ijk, DIMS)):
                    out[cls][index_of(*ijk)] = p
        return out

    def largest_window(self, cls):
        """The largest number of points of class cls that any 21 x 21 x 11 box of cubes holds: sliding sums over the occupied bounding box."""
        c = self.cubes[cls]
        if not c:
            return 0
        keys = np.array(list(c), np.int64)
        lo, hi = keys.min(0), keys.max(0)
        vol = np.zeros(tuple(hi - lo + 1), np.int64)
        for key, p in c.items():
            vol[tuple(np.array(key) - lo)] = len(p)
        for axis, n in enumerate(DIMS):                 # windowed sum along each axis in turn: cumulative sum, then differences n apart
            cs = np.cumsum(vol, axis=axis)
            shifted = np.zeros_like(cs)
            idx = [slice(None)] * 3
            if cs.shape[axis] > n:
                src, dst = list(idx), list(idx)
                src[axis], dst[axis] = slice(0, cs.shape[axis] - n), slice(n, None)
                shifted[tuple(dst)] = cs[tuple(src)]
            vol = cs - shifted                          # vol[x] = sum of the n cubes that end at x
        return int(vol.max())
