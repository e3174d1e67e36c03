"""Sweeps as 16-bit range images (include/aloam_mi355x.h, aloam_range_decoder): the numpy model of the format.

A spinning LiDAR produces a 16-bit range per laser and firing and a 16-bit azimuth per firing.  The range entry points of the C ABI take
exactly that - 2 bytes per point - and decode it in the front-end kernels; this module holds the definition they are tested against
(`decode_sweep`), the tables for the synthetic sensors (`decoder_from_model`) and the way back from rendered points (`encode_sweep`).
numpy only; nothing here is on a measured path.

One sweep of `n_cols` columns is a blob of uint16:
    az[(n_cols + 7) & ~7]     azimuth code per column (padded so that the ranges start 16-byte aligned)
    range[n_cols * rows]      in the decoder's order
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

COLUMN_MAJOR, ROW_MAJOR = 0, 1
MAX_ROWS, MAX_N_AZ = 128, 65536


@dataclass
class RangeDecoder:
    """The fields of aloam_range_decoder; tables as contiguous float32 / int32 arrays."""
    rows: int
    n_az: int
    order: int
    range_scale: float
    az_x: np.ndarray       # [n_az] f32
    az_y: np.ndarray       # [n_az] f32
    cos_el: np.ndarray     # [rows] f32
    sin_el: np.ndarray     # [rows] f32
    range_off: np.ndarray  # [rows] f32
    z_off: np.ndarray      # [rows] f32
    az_off: np.ndarray     # [rows] i32, |.| < n_az
    ring_id: np.ndarray    # [rows] i32, -1 or 0 .. n_scans-1

    def __post_init__(self):
        for k in ("az_x", "az_y", "cos_el", "sin_el", "range_off", "z_off"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.float32))
        for k in ("az_off", "ring_id"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.int32))


def header_len(n_cols: int) -> int:
    """uint16 entries of the azimuth header: n_cols rounded up to 8."""
    return (int(n_cols) + 7) & ~7


def blob_len(n_cols: int, rows: int) -> int:
    """uint16 entries of one sweep."""
    return header_len(n_cols) + int(n_cols) * int(rows)


def pack_sweep(az, ranges, rows: int) -> np.ndarray:
    """az [n_cols] and ranges [n_cols * rows] (already in the decoder's order) as one blob."""
    az = np.asarray(az, dtype=np.uint16).reshape(-1)
    ranges = np.asarray(ranges, dtype=np.uint16).reshape(-1)
    assert len(ranges) == len(az) * rows
    blob = np.zeros(blob_len(len(az), rows), np.uint16)
    blob[:len(az)] = az
    blob[header_len(len(az)):] = ranges
    return blob


def split_index(i, n_cols: int, dec: RangeDecoder):
    """(column, row) of point i."""
    i = np.asarray(i)
    if dec.order == COLUMN_MAJOR:
        return i // dec.rows, i % dec.rows
    return i % max(n_cols, 1), i // max(n_cols, 1)


def decode_sweep(blob, n_cols: int, dec: RangeDecoder) -> np.ndarray:
    """The definition: [n_cols * rows, 4] float32 (x, y, z, ring), every operation a separately rounded f32 operation, the no-return
    cells (code 0, or an azimuth code >= n_az) as NaN rows in place."""
    blob = np.asarray(blob, dtype=np.uint16).reshape(-1)
    n = int(n_cols) * dec.rows
    az = blob[:n_cols].astype(np.int64)
    code = blob[header_len(n_cols):header_len(n_cols) + n]
    col, row = split_index(np.arange(n, dtype=np.int64), n_cols, dec)
    azc = az[col] if n else np.zeros(0, np.int64)
    hit = (code != 0) & (azc < dec.n_az)
    a = np.where(hit, (azc + dec.az_off[row]) % dec.n_az, 0)
    f = np.float32
    rho = code.astype(f) * f(dec.range_scale) + dec.range_off[row]
    rxy = rho * dec.cos_el[row]
    out = np.empty((n, 4), f)
    out[:, 0] = rxy * dec.az_x[a]
    out[:, 1] = rxy * dec.az_y[a]
    out[:, 2] = rho * dec.sin_el[row] + dec.z_off[row]
    out[:, 3] = dec.ring_id[row].astype(f)
    out[~hit, :3] = np.nan
    assert out.dtype == np.float32 and rho.dtype == np.float32
    return out


def _grid(model):
    """The model's directions as [rows, cols, 3] float64 and whether its message order is ring-major."""
    d = np.asarray(model.dirs.cpu().numpy(), np.float64)
    ring = np.asarray(model.ring.cpu().numpy())
    rows, cols = model.n_scans, model.columns
    ring_major = cols > 1 and ring[1] == ring[0]
    g = d.reshape(rows, cols, 3) if ring_major else d.reshape(cols, rows, 3).transpose(1, 0, 2)
    return g, ring_major


def decoder_from_model(model, range_scale: float = 0.002, az_per_column: int = 1, az_off=None, range_off=None, z_off=None, ring_id=None) -> RangeDecoder:
    """The decoder of a synthetic.SensorModel: tables in f64 from the model's own directions, rounded to f32.  Column k carries azimuth
    code k * az_per_column.  ring_id defaults to the row itself, with rows 51 .. 63 of HDL-64 rejected as the reference's elevation
    formula rejects them (src/scanRegistration.cpp:198)."""
    g, ring_major = _grid(model)
    rows, cols = model.n_scans, model.columns
    n_az = cols * az_per_column
    assert rows <= MAX_ROWS and n_az <= MAX_N_AZ
    hyp = np.hypot(g[:, 0, 0], g[:, 0, 1])                    # cos(elevation) of every row
    ux, uy = g[0, :, 0] / hyp[0], g[0, :, 1] / hyp[0]         # cos / sin of every column's azimuth
    az_x, az_y = np.zeros(n_az), np.zeros(n_az)
    if az_per_column == 1:
        az_x, az_y = ux, uy
    else:                                                    # the codes between two columns: the angle interpolated
        ang = np.unwrap(np.arctan2(uy, ux))
        step = (ang[-1] - ang[0]) / (cols - 1) if cols > 1 else 0.0
        fine = ang[0] + step * (np.arange(n_az) / az_per_column)
        az_x, az_y = np.cos(fine), np.sin(fine)
    if ring_id is None:
        ring_id = np.arange(rows)
        if model.name == "HDL-64":
            ring_id = np.where(ring_id > 50, -1, ring_id)
    zeros = np.zeros(rows)
    return RangeDecoder(rows, n_az, ROW_MAJOR if ring_major else COLUMN_MAJOR, float(range_scale), az_x, az_y, hyp, g[:, 0, 2],
                        zeros if range_off is None else range_off, zeros if z_off is None else z_off,
                        np.zeros(rows, np.int32) if az_off is None else az_off, ring_id)


def quantise(rho, row, dec: RangeDecoder) -> np.ndarray:
    """Range codes of ranges `rho` (metres along the ray; inf / NaN = no return) measured by lasers `row`: nearest code, 0 for no
    return, clamped to 65535."""
    rho = np.asarray(rho, np.float64)
    ok = np.isfinite(rho)
    q = np.rint((np.where(ok, rho, 0.0) - dec.range_off[row].astype(np.float64)) / float(np.float32(dec.range_scale)))
    return np.where(ok, np.clip(q, 0, 65535), 0).astype(np.uint16)


def encode_sweep(points, model, dec: RangeDecoder, az_per_column: int = 1):
    """A rendered sweep (float32 [N, >=3] returns of `model` in any order, no-return rays simply missing, as synthetic.render_scan
    leaves them) on the sensor's grid: every return goes to the cell of the nearest ray (row by elevation, column by azimuth), its range
    along the ray is quantised (`quantise`), cells without a return hold 0.  Returns (blob, n_cols).  Assumes the decoder was made by
    decoder_from_model with az_off = 0 for the same model."""
    p = np.asarray(points, np.float64)[:, :3]
    p = p[np.isfinite(p).all(1)]
    g, _ = _grid(model)
    rows, cols = model.n_scans, model.columns
    el_rows = np.arctan2(g[:, 0, 2], np.hypot(g[:, 0, 0], g[:, 0, 1]))
    az_cols = np.unwrap(np.arctan2(g[0, :, 1], g[0, :, 0]))
    step = (az_cols[-1] - az_cols[0]) / (cols - 1) if cols > 1 else 1.0
    rho = np.linalg.norm(p, axis=1)
    el = np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]))
    row = np.abs(el[:, None] - el_rows[None, :]).argmin(1) if len(p) else np.zeros(0, np.int64)
    turns = (np.arctan2(p[:, 1], p[:, 0]) - az_cols[0]) / step
    col = np.rint(turns).astype(np.int64) % int(round(abs(2 * np.pi / step))) if len(p) else np.zeros(0, np.int64)
    keep = col < cols
    row, col, rho = row[keep], col[keep], rho[keep]
    codes = np.zeros((rows, cols), np.uint16)
    codes[row, col] = quantise(rho, row, dec)
    ranges = codes if dec.order == ROW_MAJOR else codes.T
    return pack_sweep(np.arange(cols) * az_per_column, ranges.reshape(-1), rows), cols
