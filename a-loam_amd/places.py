"""Place recognition, the numpy model: the Scan Context descriptor of a sweep (Kim & Kim, IROS 2018) as include/aloam_mi355x.h defines it,
the shift-minimised column-cosine distance, the ranked match, and the map <- odometry guess a match stands for.

Nothing here touches the GPU: `scan_context` restates k_place_descriptor operation for operation in float32 (all but atan2f: numpy's is
not glibc's, `scan_context_bounds` says which cells that can touch), `distance` and `match` are the float64 reference the device's f32
matrix-core product is compared with."""
from __future__ import annotations

import math

import numpy as np

from .relocalize import _qmul, _qrot

RINGS, SECTORS = 20, 60
SECTOR_DEG = 360.0 / SECTORS


def _cell_indices(p, max_range, atan_ulps=0):
    """(keep, ring, sector) of float32 points [N, >= 3]: the device's float32 operations in the device's order.  atan_ulps moves the
    azimuth by that many float32 steps before the sector is taken (scan_context_bounds)."""
    p = np.asarray(p, np.float32)
    x, y = p[:, 0], p[:, 1]
    rho = np.sqrt(x * x + y * y)
    ring = (rho * (np.float32(RINGS) / np.float32(max_range))).astype(np.int32)
    az = np.arctan2(y, x).astype(np.float32)
    for _ in range(abs(atan_ulps)):
        az = np.nextafter(az, np.float32(math.copysign(math.inf, atan_ulps)))
    az = np.clip(az, -np.float32(np.pi), np.float32(np.pi))            # (atan2f never leaves [-pi, pi] as float32)
    theta = az + np.float32(np.pi)
    sector = np.minimum((theta * np.float32(60.0 / (2.0 * math.pi))).astype(np.int32), SECTORS - 1)
    return ring < RINGS, ring, sector


def _heights(p, sensor_height):
    v = np.asarray(p, np.float32)[:, 2] + np.float32(sensor_height)
    return np.where(v > 0, v, np.float32(0)).astype(np.float32)


def scan_context(points, max_range=80.0, sensor_height=2.0):
    """The descriptor of a sweep: float32 [RINGS, SECTORS], cell (r, s) = the greatest max(z + sensor_height, 0) of the points whose
    horizontal range falls in ring r (of 20 up to max_range) and whose azimuth atan2(y, x) + pi falls in sector s (of 60); empty cells 0."""
    keep, ring, sector = _cell_indices(points, max_range)
    D = np.zeros((RINGS, SECTORS), np.float32)
    np.maximum.at(D, (ring[keep], sector[keep]), _heights(points, sensor_height)[keep])
    return D


def scan_context_bounds(points, max_range=80.0, sensor_height=2.0, ulps=4):
    """(lo, hi): the descriptor without the points whose azimuth lies within `ulps` float32 steps of a sector border, and with each of them
    counted in both sectors it may fall in.  An atan2f that differs from numpy's by at most that much gives cells between the two; lo == hi
    wherever no such point matters."""
    keep, ring, s0 = _cell_indices(points, max_range)
    _, _, s_dn = _cell_indices(points, max_range, -ulps)
    _, _, s_up = _cell_indices(points, max_range, ulps)
    v = _heights(points, sensor_height)
    sure = keep & (s_dn == s0) & (s_up == s0)
    lo = np.zeros((RINGS, SECTORS), np.float32)
    np.maximum.at(lo, (ring[sure], s0[sure]), v[sure])
    hi = lo.copy()
    edge = keep & ~sure
    for s in (s0, s_dn, s_up):
        np.maximum.at(hi, (ring[edge], s[edge]), v[edge])
    return lo, hi


def _unit_columns(d):
    d = np.asarray(d, np.float64)
    n = np.sqrt((d * d).sum(axis=-2, keepdims=True))
    return np.divide(d, n, out=np.zeros_like(d), where=n > 0), (n > 0).squeeze(-2)


def shift_distances(q, entries):
    """d[e, shift] for every entry [N, RINGS, SECTORS] and every shift 0 .. 59, float64; +inf where no column is non-zero on both sides.
    d(shift) = 1 - mean over the columns j with C[:, j] and Q[:, (j - shift) mod 60] both non-zero of their cosine."""
    qn, qm = _unit_columns(q)
    cn, cm = _unit_columns(np.asarray(entries).reshape(-1, RINGS, SECTORS))
    d = np.full((len(cn), SECTORS), np.inf)
    for s in range(SECTORS):
        qs, ms = np.roll(qn, s, axis=1), np.roll(qm, s)                 # qs[:, j] = qn[:, (j - s) mod 60]
        cos = (cn * qs[None]).sum(axis=1)                               # [N, 60] column cosines (0 where either side is zero)
        cnt = (cm & ms[None]).sum(axis=1)
        ok = cnt > 0
        d[ok, s] = 1.0 - cos[ok].sum(axis=1) / cnt[ok]
    return d


def distance(q, c):
    """(d, shift) of query q against one entry c: the minimum over the 60 shifts, ties to the lower shift; (inf, -1) when no shift is valid."""
    d = shift_distances(q, np.asarray(c)[None])[0]
    s = int(np.argmin(d))
    return (float(d[s]), s) if np.isfinite(d[s]) else (math.inf, -1)


def match(q, entries, T=1, first=0):
    """The T best entries of `entries` [N, RINGS, SECTORS] for query q, ranked by (distance, index): (entry [T] int, shift [T] int,
    distance [T] float64), entry = -1 / shift = -1 / distance 0 where fewer than T entries have a valid shift.  `first` is added to the
    returned indices (a range [first, first + N) of a larger store)."""
    entries = np.asarray(entries).reshape(-1, RINGS, SECTORS)
    ent, sh, di = np.full(T, -1, np.int64), np.full(T, -1, np.int64), np.zeros(T)
    if len(entries) == 0:
        return ent, sh, di
    d = shift_distances(q, entries)
    best_shift = np.argmin(d, axis=1)
    best = d[np.arange(len(d)), best_shift]
    order = [i for i in np.lexsort((np.arange(len(best)), best)) if np.isfinite(best[i])][:T]
    for k, i in enumerate(order):
        ent[k], sh[k], di[k] = first + i, best_shift[i], best[i]
    return ent, sh, di


def guess_from_match(place_q, place_t, shift, odom_q, odom_t):
    """The map <- odometry correction (q_wmap_wodom, t_wmap_wodom) a match stands for: the sensor is taken to be at the stored pose
    (place_q, place_t, in the map frame) turned by +shift * 6 degrees about its own z, while the odometry says it is at (odom_q, odom_t)."""
    h = math.radians(shift * SECTOR_DEG) / 2
    q_map = _qmul(np.asarray(place_q, np.float64), np.array([0.0, 0.0, math.sin(h), math.cos(h)]))
    q_map = q_map / np.linalg.norm(q_map)
    q_c = _qmul(q_map, np.asarray(odom_q, np.float64) * np.array([-1.0, -1.0, -1.0, 1.0]))
    t_c = np.asarray(place_t, np.float64) - _qrot(q_c, np.asarray(odom_t, np.float64))
    return q_c, t_c
