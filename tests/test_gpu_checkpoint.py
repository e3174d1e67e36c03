"""Sequence records on the MI355X (aloam_save_sequences / aloam_load_sequences): a sequence saved from one context and loaded into a slot of
another - other batch, other max_points, smaller pool, other slot, through device memory, pinned host memory or a file - continues bit for
bit as if it had never left; stream order, the capacity rules and the argument / state rules."""
import ctypes as C
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_sequence_lifecycle import NAN_ROW, _drives, diff, snap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xAB


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _torch():
    import torch
    return torch


def make(binding, model, B, mp, mapping, pool=1 << 17, ref_order=False, pool_limit=None, **kw):
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=mp, **kw)
    if ref_order:
        gpu.set_voxel_sum_order(True)
    if mapping:
        gpu.mapping_enable(0.4, 0.8, pool_points=pool, pool_limit=pool_limit)
    return gpu


def step(gpu, scans, mapping):
    """One frame; scans[slot] = a sweep, or None (the slot sits the step out)."""
    mask = [s is not None for s in scans]
    gpu.set_active(mask)
    gpu.scan_register([s if s is not None else NAN_ROW for s in scans], check=False)
    gpu.odometry_step()
    if mapping:
        gpu.mapping_step()


def last_sizes(binding, gpu, b):
    return tuple(binding.lib().aloam_cloud_size(gpu.h, b, w) for w in (binding.CLOUD_CORNER_LAST, binding.CLOUD_SURF_LAST))


def full(binding, gpu, b, mapping, prev=None):
    """snap() of the lifecycle tests, with the pool compaction count left out (the only field a load may change).  prev = the last-cloud
    sizes before the step: after an odometry step the LESS_SHARP / LESS_FLAT getters read the swapped row, whose content is the previous last
    clouds - what lies past them is residue of older sweeps, which no record carries, so only that content is compared."""
    s = snap(binding, gpu, b, mapping)
    if prev is not None:
        s["less_sharp"] = _sha(gpu.cloud(binding.CLOUD_LESS_SHARP, b)[:prev[0]])
        s["less_flat"] = _sha(gpu.cloud(binding.CLOUD_LESS_FLAT, b)[:prev[1]])
    if mapping:
        info = gpu.map_info(b)
        info.pop("compactions")
        s["map_info"] = repr(info)
    return s


def persistent(binding, gpu, b, mapping):
    """The getters of what a record holds (no per-step scratch): right after a load they equal the source's."""
    s = {"pose": _sha(np.concatenate(list(gpu.pose(b).values()))), "stats": repr(gpu.odom_stats(b)),
         "corner_last": _sha(gpu.cloud(binding.CLOUD_CORNER_LAST, b)), "surf_last": _sha(gpu.cloud(binding.CLOUD_SURF_LAST, b))}
    torch = _torch()
    rec = torch.zeros(gpu.batch * C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)
    gpu.export_poses(rec.data_ptr())
    gpu.synchronize()
    n = C.sizeof(binding.AloamPoseRecord)
    s["export_pose"] = _sha(rec.numpy()[b * n:(b + 1) * n])
    if mapping:
        s["map_pose"] = _sha(np.concatenate(list(gpu.map_pose(b).values())))
        info = gpu.map_info(b)
        info.pop("compactions")
        s["map_info"] = repr(info)
        s["cubes"] = [{c: _sha(p) for c, p in gpu.map_cubes(cls, b).items()} for cls in (0, 1)]
        s["surround"] = _sha(gpu.map_cloud(binding.MAP_SURROUND, b))
        s["full_map"] = _sha(gpu.map_cloud(binding.MAP_FULL, b))
    return s


def header(binding, blob, off, i=0):
    raw = bytes(np.asarray(blob[int(off[i]):int(off[i]) + 128]).tobytes()) if not hasattr(blob, "cpu") else blob[int(off[i]):int(off[i]) + 128].cpu().numpy().tobytes()
    return binding.AloamSeqRecordHeader.from_buffer_copy(raw)


def _mp(drives):
    return max(len(x) for d in drives for x in d) + 64


def round_trip(binding, sequence, mapping, ref_order=False, F=6, G=6):
    drives, model = _drives(sequence, 4, F + G)
    mp = _mp(drives)
    A = make(binding, model, 4, mp, mapping, ref_order=ref_order)
    for k in range(F):
        step(A, [d[k] for d in drives], mapping)
    blob, off = A.save_sequences(range(4), pinned=False)
    assert isinstance(blob, _torch().Tensor) and blob.is_cuda
    assert all(int(off[i + 1] - off[i]) % 256 == 0 for i in range(4))
    B = make(binding, model, 5, mp + 3000, mapping, pool=4096, ref_order=ref_order)
    perm = [3, 0, 4, 1]                                                # drive i -> slot perm[i] of B; slot 2 stays empty
    before_growths = B.map_pool_info()["growths"] if mapping else 0
    B.load_sequences(perm, blob, off)
    B.synchronize()
    if mapping:
        assert B.map_pool_info()["growths"] > before_growths            # the map did not fit B's initial pool: the load grew it
    for i in range(4):
        a, b = persistent(binding, A, i, mapping), persistent(binding, B, perm[i], mapping)
        assert not diff(a, b), (i, diff(a, b))
    for k in range(F, F + G):
        prev = [last_sizes(binding, A, i) for i in range(4)]
        step(A, [d[k] for d in drives], mapping)
        row = [None] * 5
        for i in range(4):
            row[perm[i]] = drives[i][k]
        step(B, row, mapping)
        A.synchronize(); B.synchronize()
        for i in range(4):
            a, b = full(binding, A, i, mapping, prev[i]), full(binding, B, perm[i], mapping, prev[i])
            assert not diff(a, b), (k, i, diff(a, b))
    A.close(); B.close()


@pytest.mark.parametrize("mapping", [False, True])
def test_round_trip_across_contexts_continues_bit_for_bit(binding, sequence, mapping):
    round_trip(binding, sequence, mapping)


def test_round_trip_in_reference_order(binding, sequence):
    round_trip(binding, sequence, True, ref_order=True, F=4, G=3)


def _schedule_sliced():
    spec = importlib.util.spec_from_file_location("run_kitti", os.path.join(ROOT, "tools", "run_kitti.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.schedule_sliced


@pytest.mark.parametrize("mapping, graph", [(False, "0"), (True, "0"), (True, "8")])
def test_preemption_equals_no_preemption(binding, sequence, monkeypatch, mapping, graph):
    monkeypatch.setenv("ALOAM_GRAPH_MAX_BATCH", graph)
    F = 5
    drives, model = _drives(sequence, 4, F)
    mp = _mp(drives)
    gpu = make(binding, model, 2, mp, mapping)
    parked, got = {}, {}
    for active, resets, frames, saves, loads in _schedule_sliced()([F] * 4, 2, 2):
        if saves:
            blob, off = gpu.save_sequences([s for s, _ in saves], pinned=True)
            for j, (_, i) in enumerate(saves):
                parked[i] = (blob[off[j]:off[j + 1]], np.array([0, off[j + 1] - off[j]], np.int64))
        for s, i in loads:
            gpu.load_sequences([s], *parked.pop(i))
        if resets:
            gpu.reset_sequences(resets)
        row = [None, None]
        for s, (i, k) in frames.items():
            row[s] = drives[i][k]
        gpu.synchronize()
        prev = {s: last_sizes(binding, gpu, s) for s in frames}
        step(gpu, row, mapping)
        gpu.synchronize()
        for s, (i, k) in frames.items():
            got[(i, k)] = full(binding, gpu, s, mapping, prev[s])
    gpu.close()
    assert len(got) == 4 * F
    for i in range(4):
        alone = make(binding, model, 1, mp, mapping)
        for k in range(F):
            prev = last_sizes(binding, alone, 0)
            step(alone, [drives[i][k]], mapping)
            alone.synchronize()
            want = full(binding, alone, 0, mapping, prev)
            assert not diff(got[(i, k)], want), (i, k, diff(got[(i, k)], want))
        alone.close()


def test_file_round_trip_from_pageable_memory(binding, sequence, tmp_path):
    F, G = 4, 3
    drives, model = _drives(sequence, 2, F + G)
    mp = _mp(drives)
    A = make(binding, model, 2, mp, True)
    for k in range(F):
        step(A, [d[k] for d in drives], True)
    blob, off = A.save_sequences([0, 1], pinned=True)
    path = tmp_path / "seqs.bin"
    blob.tofile(path)
    np.save(tmp_path / "offsets.npy", off)
    data = np.fromfile(path, dtype=np.uint8)                           # pageable host memory, as read from a file
    C2 = make(binding, model, 2, mp, True)
    C2.load_sequences([1, 0], data, np.load(tmp_path / "offsets.npy"))
    for k in range(F, F + G):
        prev = [last_sizes(binding, A, i) for i in (0, 1)]
        step(A, [d[k] for d in drives], True)
        step(C2, [drives[1][k], drives[0][k]], True)
        A.synchronize(); C2.synchronize()
        for i, s in ((0, 1), (1, 0)):
            a, b = full(binding, A, i, True, prev[i]), full(binding, C2, s, True, prev[i])
            assert not diff(a, b), (k, i, diff(a, b))
    A.close(); C2.close()


class DeviceInput:
    """The sweeps of one frame in device memory, for steps queued with no host synchronisation (aloam_scan_register_device)."""

    def __init__(self, scans, cap):
        torch = _torch()
        self.cap = cap
        self.buf = torch.zeros((len(scans), cap, 4), dtype=torch.float32, device="cuda")
        for b, s in enumerate(scans):
            self.buf[b, :len(s)] = torch.from_numpy(np.ascontiguousarray(s, np.float32)).cuda()
        torch.cuda.synchronize()
        self.nin = [len(s) for s in scans]

    def step(self, gpu, mapping):
        gpu.set_active(None)
        gpu.scan_register_device(self.buf.data_ptr(), self.cap * 16, self.nin, 16)
        gpu.odometry_step()
        if mapping:
            gpu.mapping_step()


@pytest.mark.parametrize("mapping", [False, True])
def test_save_and_load_are_stream_ordered(binding, sequence, mapping):
    torch = _torch()
    k = 4
    drives, model = _drives(sequence, 2, k + 2)
    mp = _mp(drives)
    nxt = DeviceInput([d[k] for d in drives], mp)
    A = make(binding, model, 2, mp, mapping)
    for f in range(k):
        step(A, [d[f] for d in drives], mapping)
    off = torch.zeros(3, dtype=torch.int64, device="cuda")
    A.save_sequences_into([0, 1], 0, 0, off.data_ptr())                # size query
    A.synchronize()
    total = int(off[-1])
    at_k = [persistent(binding, A, b, mapping) for b in (0, 1)]
    prev = [last_sizes(binding, A, b) for b in (0, 1)]
    blob = torch.empty(total, dtype=torch.uint8, device="cuda")
    A.save_sequences_into([0, 1], blob.data_ptr(), total, off.data_ptr())
    nxt.step(A, mapping)                                               # step k + 1 queued right behind the save: no synchronisation
    A.synchronize()
    after = [full(binding, A, b, mapping, prev[b]) for b in (0, 1)]
    D = make(binding, model, 2, mp, mapping)
    D.load_sequences([0, 1], blob, off.cpu().numpy())
    D.synchronize()
    for b in (0, 1):
        got = persistent(binding, D, b, mapping)
        assert not diff(got, at_k[b]), (b, diff(got, at_k[b]))          # the record holds step k's state
        assert got["pose"] != persistent(binding, A, b, mapping)["pose"]
    E = make(binding, model, 2, mp, mapping)
    E.load_sequences([0, 1], blob, off.cpu().numpy())
    nxt.step(E, mapping)                                               # a step queued right behind the load
    E.synchronize()
    for b in (0, 1):
        got = full(binding, E, b, mapping, prev[b])
        assert not diff(got, after[b]), (b, diff(got, after[b]))
    for g in (A, D, E):
        g.close()


def test_capacity_rules(binding, sequence):
    torch = _torch()
    drives, model = _drives(sequence, 3, 6)
    mp = _mp(drives)
    A = make(binding, model, 3, mp, True)
    for k in range(6):
        step(A, [d[k] for d in drives], True)
    ref_blob, ref_off = A.save_sequences([0, 1, 2], pinned=True)
    total = int(ref_off[-1])
    # cap 0: the offsets only
    off = torch.full((4,), -7, dtype=torch.int64, pin_memory=True)
    A.save_sequences_into([0, 1, 2], 0, 0, off.data_ptr())
    A.synchronize()
    assert np.array_equal(off.numpy(), ref_off)
    # a cap inside record 1: record 0 whole, nothing at or past the cap
    guard = 4096
    dst = torch.full((total + guard,), SENTINEL, dtype=torch.uint8, pin_memory=True)
    cap = int(ref_off[1]) + 256
    A.save_sequences_into([0, 1, 2], dst.data_ptr(), cap, off.data_ptr())
    A.synchronize()
    d = dst.numpy()
    assert np.array_equal(off.numpy(), ref_off)
    assert np.array_equal(d[:ref_off[1]], ref_blob[:ref_off[1]])
    assert (d[ref_off[1]:] == SENTINEL).all()
    # last clouds above the target's max_points, a map above the target's pool limit: ALOAM_E_CAPACITY, the target unchanged
    h = header(binding, ref_blob, ref_off, 0)
    assert h.n_surf_last > 64 and max(h.map_points) > 4096, (h.n_surf_last, list(h.map_points))
    rec, roff = ref_blob[:ref_off[1]], np.array([0, ref_off[1]], np.int64)
    for small_mp, pool_limit in ((h.n_surf_last - 1, None), (mp, 4096)):
        T = make(binding, model, 2, small_mp, True, pool=4096, pool_limit=pool_limit)
        if pool_limit is None:                                         # (a map step at the pool limit could drop points: that target stays fresh)
            step(T, [drives[2][0][:small_mp], drives[2][0][:small_mp]], True)
            T.synchronize()
        before, pool = full(binding, T, 1, True), T.map_pool_info()
        with pytest.raises(binding.AloamError) as e:
            T.load_sequences([1], rec, roff)
        assert e.value.code == binding.E_CAPACITY, str(e.value)
        assert not diff(full(binding, T, 1, True), before)
        assert T.map_pool_info() == pool
        T.close()
    A.close()


def test_argument_and_state_rules(binding, sequence):
    torch = _torch()
    drives, model = _drives(sequence, 2, 4)
    mp = _mp(drives)
    A = make(binding, model, 2, mp, True)
    for k in range(3):
        step(A, [d[k] for d in drives], True)
    blob, off = A.save_sequences([0, 1], pinned=True)
    rec, roff = np.array(blob[:off[1]]), np.array([0, off[1]], np.int64)
    off_pin = torch.zeros(3, dtype=torch.int64, pin_memory=True)
    before = [full(binding, A, b, True) for b in (0, 1)]

    def refused(code, fn, *args, name=None):
        with pytest.raises(binding.AloamError) as e:
            fn(*args)
        assert e.value.code == code, str(e.value)
        if name:
            assert name in str(e.value), str(e.value)

    pageable = np.zeros(int(off[-1]), np.uint8)
    refused(binding.E_ARG, A.save_sequences_into, [0, 1], pageable.ctypes.data, len(pageable), off_pin.data_ptr())
    refused(binding.E_ARG, A.save_sequences_into, [0, 1], 0, 1024, off_pin.data_ptr())                 # NULL dst
    refused(binding.E_ARG, A.save_sequences_into, [0, 1], 0, 0, np.zeros(3, np.int64).ctypes.data)   # pageable offsets
    refused(binding.E_ARG, A.save_sequences_into, [0, 1], 0, 0, 0)                                   # NULL offsets
    refused(binding.E_ARG, A.save_sequences_into, [0, 0], 0, 0, off_pin.data_ptr())
    refused(binding.E_ARG, A.save_sequences_into, [2], 0, 0, off_pin.data_ptr())
    refused(binding.E_ARG, A.load_sequences, [1, 1], blob, off)
    refused(binding.E_ARG, A.load_sequences, [-1], rec, roff)
    # compatibility: each field in turn
    for kw, mapping, res, ref_order, name in (({"n_scans": 32}, True, (0.4, 0.8), False, "n_scans"), ({"distortion": True}, True, (0.4, 0.8), False, "distortion"),
                                              ({}, False, None, False, "map part"), ({}, True, (0.2, 0.8), False, "mapping_line_resolution"),
                                              ({}, True, (0.4, 0.8), True, "voxel sum order")):
        T = binding.Aloam(n_scans=kw.get("n_scans", model.n_scans), min_range=model.min_range, batch=2, max_points=mp, distortion=kw.get("distortion", False))
        if ref_order:
            T.set_voxel_sum_order(True)
        if mapping:
            T.mapping_enable(*res, pool_points=1 << 17)
        t_before = full(binding, T, 0, mapping)
        refused(binding.E_ARG, T.load_sequences, [0], rec, roff, name=name)
        assert not diff(full(binding, T, 0, mapping), t_before)
        T.close()
    # corrupted magic, version, length
    for field, value in (("magic", 0x12345678), ("version", 2), ("bytes", int(roff[1]) + 256)):
        bad = rec.copy()
        h = binding.AloamSeqRecordHeader.from_buffer(bad)
        setattr(h, field, value)
        del h
        refused(binding.E_ARG, A.load_sequences, [0], bad, roff, name="record 0")
    assert [full(binding, A, b, True) for b in (0, 1)] == before
    # between a registration and its odometry step
    A.set_active(None)
    A.scan_register([drives[0][3], drives[1][3]], check=False)
    refused(binding.E_STATE, A.save_sequences_into, [0], 0, 0, off_pin.data_ptr())
    refused(binding.E_STATE, A.load_sequences, [0], rec, roff)
    A.odometry_step()
    A.mapping_step()
    A.synchronize()
    # a loaded slot may not map before its next odometry step; the other slot may
    A.load_sequences([0], rec, roff)
    A.synchronize()
    loaded = full(binding, A, 0, True)
    refused(binding.E_STATE, A.mapping_step)
    assert not diff(full(binding, A, 0, True), loaded)
    A.set_active([False, True])
    A.mapping_step()                                                   # slot 0 sits this mapping step out
    A.set_active(None)
    A.scan_register([drives[0][3], drives[1][3]], check=False)
    A.odometry_step()
    A.mapping_step()
    A.synchronize()
    A.close()


def test_kitti_runner_time_slices_like_the_unsliced_run(tmp_path):
    seqs = ["00", "01", "02"]
    for tag, extra in (("plain", []), ("sliced", ["--slice", "2"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--selftest", "--mapping", "--seqs", *seqs, "--batch", "2",
                            "--out", str(tmp_path / tag), *extra], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
    for s in seqs:
        for kind in ("odometry", "mapped"):
            assert (tmp_path / "sliced" / f"{s}_{kind}.txt").read_bytes() == (tmp_path / "plain" / f"{s}_{kind}.txt").read_bytes(), (s, kind)
