"""Sweeps as range images for the range-input tests: built once per session, shared, never changed."""
import dataclasses
import functools
import importlib

import numpy as np

ri = importlib.import_module("a-loam_amd.range_input")
syn = importlib.import_module("a-loam_amd.synthetic")

FRAMES = 4


@functools.lru_cache(maxsize=None)
def case(kind):
    """-> dict(model, dec, blobs [FRAMES] uint16, n_cols, decoded [FRAMES] float32 [n, 4] with the NaN rows in place, n_scans, min_range).
    vlp16_403   VLP-16 x 403 columns, column-major: 6448 points = 7 blocks of k_front, the last one partial; the azimuth header is padded (403 -> 408)
    hdl64_row   HDL-64 x 256 columns, row-major: 16 blocks
    hdl64_hard  HDL-64 x 256 columns, column-major, ring_id a permutation of 0 .. 50 over rows 0 .. 50 and -1 on rows 51 .. 63, nonzero az_off
                (negative and wrapping) / range_off / z_off, 7 % random zero codes, the first 20 columns all zero (the first ray has no return)"""
    name, cols = {"vlp16_403": ("VLP-16", 403), "hdl64_row": ("HDL-64", 256), "hdl64_hard": ("HDL-64", 256)}[kind]
    scans, _, _, model = syn.make_sequence(name, FRAMES, seed=21, columns=cols)
    dec = ri.decoder_from_model(model)
    rng = np.random.default_rng(5)
    if kind == "hdl64_hard":
        ring_id = np.full(64, -1, np.int32)
        ring_id[:51] = rng.permutation(51)
        az_off = rng.integers(-3, 4, 64).astype(np.int32)
        az_off[0], az_off[1] = -255, 255                       # wraps either way for most columns
        dec = dataclasses.replace(dec, order=ri.COLUMN_MAJOR, ring_id=ring_id, az_off=az_off,
                                  range_off=rng.uniform(-0.05, 0.05, 64).astype(np.float32), z_off=rng.uniform(-0.1, 0.1, 64).astype(np.float32))
    blobs, decoded = [], []
    for s in scans:
        blob, n_cols = ri.encode_sweep(s.numpy(), model, dec)
        if kind == "hdl64_hard":
            codes = blob[ri.header_len(n_cols):].reshape(n_cols, 64)
            codes[rng.random(codes.shape) < 0.07] = 0
            codes[:20] = 0
        blobs.append(blob)
        decoded.append(ri.decode_sweep(blob, n_cols, dec))
    return dict(model=model, dec=dec, blobs=blobs, n_cols=cols, decoded=decoded, n_scans=model.n_scans, min_range=model.min_range)
