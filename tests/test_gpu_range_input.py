"""Range-image input on the GPU.  The yardstick is a TWIN context with ring_from_field = 1 that is fed range_input.decode_sweep's array as
16-byte records through the existing entry points, NaN rows in place: by the definition of the format the two contexts agree bit for bit
on every getter.  No tolerance exists in this file except the oracle's pose bound, which is test_gpu_parity.py's."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import bits_equal
from range_cases import FRAMES, case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ri = importlib.import_module("a-loam_amd.range_input")
FEATURES = ("cloud", "sharp", "less_sharp", "flat", "less_flat")
POSE_KEYS = ("q_w", "t_w", "q_lc", "t_lc")


def _pair(binding, c, batch=1, max_points=None, **kw):
    """(range context with its decoder set, twin)."""
    mp = max_points or c["n_cols"] * c["dec"].rows
    rng = binding.Aloam(n_scans=c["n_scans"], min_range=c["min_range"], ring_from_field=False, batch=batch, max_points=mp, **kw)
    twin = binding.Aloam(n_scans=c["n_scans"], min_range=c["min_range"], ring_from_field=True, batch=batch, max_points=mp, **kw)
    rng.set_range_decoder(c["dec"])
    return rng, twin


def _device(blob):
    import torch
    return torch.from_numpy(np.ascontiguousarray(blob).view(np.int16)).cuda()


def _record(binding, g, seq=0):
    """The sequence record with the saving context's ring_from_field blanked: SeqMeta (n_in, first / last kept, half index, start / end
    azimuth, cloud sizes, error bits), the odometry state and the last clouds, byte for byte."""
    blob, off = g.save_sequences([seq])
    rec = np.array(blob[off[0]:off[1]], copy=True)
    o = binding.AloamSeqRecordHeader.ring_from_field.offset
    rec[o:o + 4] = 0
    return rec


def _same_everywhere(binding, a, b, seq=0, ctx=""):
    fa, fb = a.features(seq), b.features(seq)
    for k in FEATURES:
        assert fa[k].shape == fb[k].shape and bits_equal(fa[k], fb[k]), (ctx, k, fa[k].shape, fb[k].shape)
    (sa, ca), (sb, cb) = a.ring_ranges(seq), b.ring_ranges(seq)
    assert np.array_equal(sa, sb) and np.array_equal(ca, cb), ctx
    for w in (binding.CLOUD_CORNER_LAST, binding.CLOUD_SURF_LAST):
        assert bits_equal(a.cloud(w, seq), b.cloud(w, seq)), (ctx, w)
    pa, pb = a.pose(seq), b.pose(seq)
    for k in POSE_KEYS:
        assert np.array_equal(pa[k], pb[k]), (ctx, k, pa[k], pb[k])
    assert a.odom_stats(seq) == b.odom_stats(seq) or str(a.odom_stats(seq)) == str(b.odom_stats(seq)), ctx   # (costs may be NaN before the first solve)


@pytest.mark.parametrize("kind", ["vlp16_403", "hdl64_row", "hdl64_hard"])
def test_range_context_equals_its_twin_on_every_getter(binding, kind):
    c = case(kind)
    rng, twin = _pair(binding, c)
    assert c["n_cols"] * c["dec"].rows > 1024                                           # more than one block of k_front
    for k in range(FRAMES):
        d = _device(c["blobs"][k])
        rng.scan_register_range_device(d.data_ptr(), 0, [c["n_cols"]])
        twin.scan_register(c["decoded"][k])
        rng.synchronize()
        ca, la = rng.per_point(); cb, lb = twin.per_point()
        assert bits_equal(ca, cb) and np.array_equal(la, lb), (kind, k)
        rng.odometry_step(); twin.odometry_step()
        _same_everywhere(binding, rng, twin, 0, (kind, k))
        ra, rb = _record(binding, rng), _record(binding, twin)
        assert np.array_equal(ra, rb), (kind, k, np.nonzero(ra != rb)[0][:8])
    meta = _record(binding, rng)[128:128 + 64].view(np.int32)
    assert meta[0] == c["n_cols"] * c["dec"].rows and meta[7] == 0                      # n_in, no error bit
    if kind == "hdl64_hard":
        assert meta[1] >= 20 * 64                                                       # the first kept point lies behind the 20 empty columns
    assert np.linalg.norm(rng.pose()["t_w"]) > 0.5                                      # the odometry moved
    rng.close(); twin.close()


def test_throughput_entries_over_four_frames(binding):
    """aloam_process_range_device against the twin's aloam_process_device on the decoded records: poses, statistics and last clouds."""
    import torch
    c = case("hdl64_row")
    rng, twin = _pair(binding, c)
    n = c["n_cols"] * 64
    for k in range(FRAMES):
        d = _device(c["blobs"][k])
        x = torch.from_numpy(c["decoded"][k]).cuda()
        rng.process_range_device(d.data_ptr(), 0, [c["n_cols"]])
        twin.process_device(x.data_ptr(), 0, [n], 16)
        rng.synchronize(); twin.synchronize()
    _same_everywhere(binding, rng, twin, 0, "process")
    assert np.array_equal(_record(binding, rng), _record(binding, twin))
    rng.close(); twin.close()


def test_batch_with_unequal_sweeps_an_empty_one_and_an_idle_one(binding):
    """Batch 3: 403 columns, 0 columns (kErrEmpty, as in the twin) and the first 200 columns; then a frame in which sequence 2 sits out."""
    c = case("vlp16_403")
    rows = c["dec"].rows
    rng, twin = _pair(binding, c, batch=3, max_points=403 * rows)

    def part(k, cols):
        b = c["blobs"][k]
        return ri.pack_sweep(b[:cols], b[ri.header_len(403):ri.header_len(403) + cols * rows], rows), c["decoded"][k][:cols * rows]

    def frame(k, cols):
        blobs, recs = zip(*(part(k, n) for n in cols))
        out = []
        for g, call in ((rng, lambda: rng.scan_register_range(list(blobs), list(cols))), (twin, lambda: twin.scan_register(list(recs)))):
            try:
                call()
                out.append(0)
            except binding.AloamError as e:
                out.append(e.code)
        return out

    assert frame(0, (403, 0, 200)) == [binding.E_EMPTY, binding.E_EMPTY]
    for b in (0, 2):
        _same_everywhere(binding, rng, twin, b, ("frame 0", b))
    assert rng.cloud(binding.CLOUD_FULL, 1).shape[0] == 0
    rng.odometry_step(); twin.odometry_step()
    rng.set_active([1, 1, 0]); twin.set_active([1, 1, 0])
    assert frame(1, (403, 0, 77)) == [binding.E_EMPTY, binding.E_EMPTY]
    rng.odometry_step(); twin.odometry_step()
    for b in (0, 2):
        _same_everywhere(binding, rng, twin, b, ("frame 1", b))
    assert bits_equal(rng.cloud(binding.CLOUD_SURF_LAST, 2), twin.cloud(binding.CLOUD_SURF_LAST, 2)) and len(rng.cloud(binding.CLOUD_SURF_LAST, 2)) > 0
    rng.close(); twin.close()


def test_one_case_against_the_oracle(O, binding):
    """The decoded points with their rings through the oracle, as test_gpu_parity.py compares ring_from_field input: discrete results equal,
    poses within that file's bound."""
    from test_gpu_parity import _assert_features_equal, _assert_pose_close
    c = case("hdl64_hard")
    rng, _twin = _pair(binding, c)
    _twin.close()
    orc = O.Oracle(n_scans=c["n_scans"], min_range=c["min_range"], ring_from_field=True)
    for k in range(FRAMES):
        fo = orc.scan_register(c["decoded"][k])
        rng.scan_register_range([c["blobs"][k]], [c["n_cols"]])
        _assert_features_equal(fo, rng.features(), ("range", k))
        so, co = orc.ring_ranges(); sg, cg = rng.ring_ranges()
        assert np.array_equal(so, sg) and np.array_equal(co, cg)
        po = orc.odometry_step()
        rng.odometry_step()
        _assert_pose_close(po, rng.pose(), ("range", k))
        so_, sg_ = orc.odom_stats(), rng.odom_stats()
        for key in ("corner_corr", "plane_corr", "lm_iterations", "lm_successful", "termination"):
            assert so_[key] == sg_[key], (k, key, so_, sg_)
    rng.close()


def test_host_path_from_pinned_and_pageable_memory(binding):
    """aloam_process_range_host from pinned memory: two calls back to back from two buffers with nothing in between, then
    aloam_input_consumed - the bits of the device entry.  Once from pageable memory as well."""
    import torch
    c = case("vlp16_403")
    nc = c["n_cols"]
    g_host, g_dev = _pair(binding, c, batch=2)
    g_dev.set_range_decoder(c["dec"])                                     # (two range contexts: the second one's ring_from_field plays no part)
    stride = c["blobs"][0].nbytes + 32                                    # (rows are not packed back to back)
    bufs = []
    for k in (0, 1):
        h = torch.zeros(2 * stride, dtype=torch.uint8).pin_memory()
        for b in (0, 1):
            h[b * stride:b * stride + c["blobs"][k + b].nbytes] = torch.from_numpy(c["blobs"][k + b].view(np.uint8))
        bufs.append(h)
    g_host.process_range_host(bufs[0].data_ptr(), stride, [nc, nc])
    g_host.process_range_host(bufs[1].data_ptr(), stride, [nc, nc])
    g_host.input_consumed()
    devs = [b.cuda() for b in bufs]
    for d in devs:
        g_dev.process_range_device(d.data_ptr(), stride, [nc, nc])
    g_host.synchronize(); g_dev.synchronize()
    for b in (0, 1):
        _same_everywhere(binding, g_host, g_dev, b, ("pinned", b))
    assert np.linalg.norm(g_host.pose(0)["t_lc"]) > 0.1
    pageable = np.concatenate([np.frombuffer(bufs[1].numpy().tobytes(), np.uint8)])
    g_host.process_range_host(pageable.ctypes.data, stride, [nc, nc])
    g_dev.process_range_device(devs[1].data_ptr(), stride, [nc, nc])
    g_host.input_consumed()
    g_host.synchronize(); g_dev.synchronize()
    for b in (0, 1):
        _same_everywhere(binding, g_host, g_dev, b, ("pageable", b))
    g_host.close(); g_dev.close()


def test_one_context_alternates_between_float_records_and_range_images(binding):
    c = case("hdl64_row")
    mixed, twin = _pair(binding, c)
    mixed.close()
    mixed = binding.Aloam(n_scans=64, min_range=c["min_range"], ring_from_field=True, max_points=c["n_cols"] * 64)   # its float frames carry the ring too
    mixed.set_range_decoder(c["dec"])
    for k in range(FRAMES):
        if k % 2:
            mixed.scan_register(c["decoded"][k])
        else:
            mixed.scan_register_range([c["blobs"][k]], [c["n_cols"]])
        twin.scan_register(c["decoded"][k])
        mixed.odometry_step(); twin.odometry_step()
        _same_everywhere(binding, mixed, twin, 0, ("alternating", k))
    mixed.close(); twin.close()


def test_with_mapping_and_places_enabled(binding):
    """Two frames with the mapping step and a place descriptor behind the range front end: map pose and Scan Context cells equal the twin's."""
    c = case("vlp16_403")
    rng, twin = _pair(binding, c)
    for g in (rng, twin):
        g.mapping_enable(0.2, 0.4, pool_points=65536)
        g.places_enable(8)
    for k in range(2):
        rng.scan_register_range([c["blobs"][k]], [c["n_cols"]])
        twin.scan_register(c["decoded"][k])
        for g in (rng, twin):
            g.odometry_step(); g.mapping_step(); g.places_add([0]); g.synchronize()
        ma, mb = rng.map_pose(), twin.map_pose()
        for key in ma:
            assert np.array_equal(ma[key], mb[key]), (k, key)
    pa, pb = rng.places_export(), twin.places_export()
    assert len(pa) == 2 and pa.tobytes() == pb.tobytes() and np.count_nonzero(pa["cells"]) > 0
    assert rng.map_info() == twin.map_info()
    rng.close(); twin.close()


def test_errors_name_the_field_and_queue_nothing(binding):
    c = case("vlp16_403")
    dec = c["dec"]
    g = binding.Aloam(n_scans=16, min_range=0.3, max_points=403 * 16)
    blob = c["blobs"][0]

    def fails(call, code, word):
        with pytest.raises(binding.AloamError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))

    for entry in (g.scan_register_range_host, g.process_range_host):
        fails(lambda: entry(blob.ctypes.data, 0, [403]), binding.E_STATE, "aloam_set_range_decoder")
    d = _device(blob)
    for entry in (g.scan_register_range_device, g.process_range_device):
        fails(lambda: entry(d.data_ptr(), 0, [403]), binding.E_STATE, "aloam_set_range_decoder")

    def broken(**kw):
        s, keep = binding.range_decoder_struct(dec)
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keep[k] = v
                v = v.ctypes.data_as(type(getattr(s, k)))
            setattr(s, k, v)
        return s, keep

    ring_bad = dec.ring_id.copy(); ring_bad[3] = 16
    az_bad = dec.az_off.copy(); az_bad[5] = -dec.n_az
    for kw, word in (({"rows": 129}, "rows"), ({"rows": 0}, "rows"), ({"n_az": 65537}, "n_az"), ({"n_az": 0}, "n_az"), ({"ring_id": ring_bad}, "ring_id"),
                     ({"az_off": az_bad}, "az_off"), ({"order": 2}, "order")):
        s, keep = broken(**kw)
        fails(lambda: g.set_range_decoder(s), binding.E_ARG, word)
    for name in ("az_x", "cos_el", "ring_id"):
        s, keep = binding.range_decoder_struct(dec)
        setattr(s, name, type(getattr(s, name))())                           # NULL
        fails(lambda: g.set_range_decoder(s), binding.E_ARG, "null table")
    fails(lambda: g.scan_register_range_host(blob.ctypes.data, 0, [403]), binding.E_STATE, "aloam_set_range_decoder")   # a refused decoder changes nothing
    g.set_range_decoder(dec)
    fails(lambda: g.scan_register_range_host(blob.ctypes.data, 0, [404]), binding.E_CAPACITY, "max_points")
    fails(lambda: g.scan_register_range_device(d.data_ptr(), 0, [-1]), binding.E_ARG, "n_cols")
    with pytest.raises(binding.AloamError) as e:                                # nothing was queued by any of them
        g.odometry_step()
    assert e.value.code == binding.E_STATE
    g.scan_register_range([blob], [403])                                        # and the context works
    assert len(g.cloud(binding.CLOUD_FULL)) > 5000
    g.close()


def test_run_kitti_range_input_passes_the_bounds_of_the_float_run(tmp_path):
    """tools/run_kitti.py --selftest --mapping --range-input: the bounds test_kitti_io.py applies to the float run (the 2 mm quantisation sits
    under the drive's 2 cm range noise)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--selftest", "--mapping", "--range-input", "--out", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    ate = {m.group(1): float(m.group(2)) for m in re.finditer(r"(odometry|mapped): \d+ sweeps, ATE \(RMSE, no alignment\) = ([0-9.]+) m", r.stdout)}
    print(ate)
    assert ate["odometry"] < 0.5 and ate["mapped"] < 0.05 and ate["mapped"] < ate["odometry"], ate
