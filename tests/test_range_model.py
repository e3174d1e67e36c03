"""The numpy model of range-image input (a-loam_amd/range_input.py) against the definition written out point by point, and the
encode -> decode round trip on a rendered sweep.  No GPU."""
import dataclasses
import importlib

import numpy as np
import pytest

ri = importlib.import_module("a-loam_amd.range_input")
f32 = np.float32


def loop_decode(blob, n_cols, d):
    """The definition of include/aloam_mi355x.h, one point at a time, every operation an np.float32 operation."""
    n = n_cols * d.rows
    hdr = (n_cols + 7) // 8 * 8
    out = np.zeros((n, 4), f32)
    for i in range(n):
        col, row = (i // d.rows, i % d.rows) if d.order == ri.COLUMN_MAJOR else (i % n_cols, i // n_cols)
        code, azc = int(blob[hdr + i]), int(blob[col])
        out[i, 3] = f32(int(d.ring_id[row]))
        if code == 0 or azc >= d.n_az:
            out[i, :3] = np.nan
            continue
        a = (azc + int(d.az_off[row])) % d.n_az
        rho = f32(f32(code) * f32(d.range_scale)) + d.range_off[row]
        rxy = f32(rho * d.cos_el[row])
        out[i, 0] = f32(rxy * d.az_x[a])
        out[i, 1] = f32(rxy * d.az_y[a])
        out[i, 2] = f32(f32(rho * d.sin_el[row]) + d.z_off[row])
    return out


def random_decoder(rng, rows, n_az, order):
    ang = rng.uniform(-np.pi, np.pi, n_az)
    el = rng.uniform(-0.5, 0.3, rows)
    ring_id = rng.permutation(rows).astype(np.int32)
    ring_id[rng.random(rows) < 0.2] = -1
    az_off = rng.integers(-(n_az - 1), n_az, rows).astype(np.int32)             # negative and wrapping ones
    return ri.RangeDecoder(rows, n_az, order, 0.002, np.cos(ang), np.sin(ang), np.cos(el), np.sin(el), rng.uniform(-0.3, 0.3, rows),
                           rng.uniform(-0.2, 0.2, rows), az_off, ring_id)


@pytest.mark.parametrize("order", [ri.COLUMN_MAJOR, ri.ROW_MAJOR])
@pytest.mark.parametrize("rows,n_cols,n_az", [(16, 37, 360), (5, 8, 7), (64, 3, 36000), (1, 11, 1), (7, 0, 100)])
def test_decode_equals_the_per_point_definition(order, rows, n_cols, n_az):
    rng = np.random.default_rng(rows * 1000 + n_cols)
    d = random_decoder(rng, rows, n_az, order)
    az = rng.integers(0, n_az, n_cols)
    codes = rng.integers(1, 65536, n_cols * rows)
    if n_cols:
        codes[rng.random(len(codes)) < 0.1] = 0                                  # no return
        codes[0], codes[-1] = 65535, 0
        az[rng.integers(0, n_cols)] = min(65535, n_az)                           # a code off the table (not representable when n_az = 65536)
    blob = ri.pack_sweep(az, codes, rows)
    assert len(blob) == (n_cols + 7) // 8 * 8 + n_cols * rows and (2 * ri.header_len(n_cols)) % 16 == 0
    got, want = ri.decode_sweep(blob, n_cols, d), loop_decode(blob, n_cols, d)
    assert got.shape == want.shape == (n_cols * rows, 4) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if n_cols:
        assert np.isnan(got[:, 0]).any() and np.isfinite(got[:, 0]).any()


def test_encode_then_decode_moves_no_point_by_more_than_half_a_code_along_its_ray(syn):
    """A rendered VLP-16 sweep through encode_sweep and decode_sweep.  In real arithmetic the decoded point lies on the same ray, at most
    range_scale / 2 from the rendered one.  In f32, with s = the spacing of float32 at the largest range of the sweep (no coordinate and no
    intermediate exceeds it), each rounding moves a coordinate by at most s / 2: the rendered point is rounded once; the decoded coordinate
    goes through the rounded scale, code * scale, + range_off, the rounded cos_el (or sin_el), the product, the rounded az_x (az_y) and the
    last product - seven roundings.  Eight half-spacings per coordinate, three coordinates: 4 * sqrt(3) * s in distance."""
    scans, _, _, model = syn.make_sequence("VLP-16", 1, seed=9)
    p = scans[0].numpy()
    dec = ri.decoder_from_model(model, range_scale=0.002)
    blob, n_cols = ri.encode_sweep(p, model, dec)
    assert n_cols == model.columns and dec.order == ri.COLUMN_MAJOR and dec.rows == 16
    out = ri.decode_sweep(blob, n_cols, dec)
    hit = np.isfinite(out[:, 0])
    assert hit.sum() == len(p)                                                 # every return found its own cell
    q = out[hit, :3].astype(np.float64)
    p64 = p[:, :3].astype(np.float64)                                          # both in storage order: the render keeps the firing order
    rmax = np.linalg.norm(p64, axis=1).max()
    bound = float(np.float32(dec.range_scale)) / 2 + 4 * np.sqrt(3.0) * float(np.spacing(np.float32(rmax)))
    moved = np.linalg.norm(q - p64, axis=1)
    ray = p64 / np.linalg.norm(p64, axis=1, keepdims=True)
    across = np.linalg.norm((q - p64) - ((q - p64) * ray).sum(1, keepdims=True) * ray, axis=1)
    print("largest move", moved.max(), "bound", bound, "across the ray", across.max())
    assert moved.max() <= bound
    assert across.max() <= 4 * np.sqrt(3.0) * float(np.spacing(np.float32(rmax)))      # the quantisation acts along the ray only
    assert np.array_equal(out[:, 3], np.tile(np.arange(16, dtype=np.float32), n_cols))


def test_quantise_rounds_to_nearest_clamps_and_marks_no_return():
    dec = dataclasses.replace(random_decoder(np.random.default_rng(1), 4, 10, ri.COLUMN_MAJOR), range_off=np.zeros(4, np.float32))
    s = float(np.float32(0.002))
    got = ri.quantise(np.array([np.inf, np.nan, 1.4 * s, 1.6 * s, 1e6, 100 * s]), np.zeros(6, np.int64), dec)
    assert got.tolist() == [0, 0, 1, 2, 65535, 100] and got.dtype == np.uint16


def test_hdl64_decoder_rejects_the_rows_the_reference_rejects(syn):
    """Rows 51 .. 63 of HDL-64 get scanID > 50 from src/scanRegistration.cpp:193-198 and are cut there; the decoder says -1."""
    dec = ri.decoder_from_model(syn.sensor_model("HDL-64", columns=64))
    assert dec.order == ri.ROW_MAJOR and dec.ring_id[:51].tolist() == list(range(51)) and (dec.ring_id[51:] == -1).all()
    over = ri.decoder_from_model(syn.sensor_model("VLP-16", columns=40), az_per_column=3, ring_id=np.arange(16)[::-1], z_off=np.full(16, 0.1))
    assert over.n_az == 120 and over.ring_id[0] == 15 and over.z_off[3] == np.float32(0.1) and over.order == ri.COLUMN_MAJOR
