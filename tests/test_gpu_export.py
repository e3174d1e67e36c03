"""Batched export on the MI355X (aloam_export_poses / aloam_export_clouds): the poses and clouds of every sequence written in one stream-ordered call
into device or pinned host memory, bit for bit what the per-sequence getters return; the surround and full map in the reference's order
(src/laserMapping.cpp:803-834); the capacity and argument rules."""
import ctypes as C
import glob
import hashlib
import os

import numpy as np
import pytest

from conftest import bits_equal


pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = np.uint32(0x7FBADBAD)                         # a NaN no export writes


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _torch():
    import torch
    return torch


def all_ids(binding, mapping=True):
    ids = list(range(7))
    if mapping:
        ids += [binding.EXPORT_MAP + w for w in (binding.MAP_REGISTERED, binding.MAP_CORNER_STACK, binding.MAP_SURF_STACK, binding.MAP_SURROUND, binding.MAP_FULL)]
    return ids


def getter(binding, gpu, which, b):
    return gpu.cloud(which, b) if which < binding.EXPORT_MAP else gpu.map_cloud(which - binding.EXPORT_MAP, b)


class Dest:
    """Export destinations in device memory (torch tensor on the context's device) or pinned host memory, filled with a sentinel."""

    def __init__(self, batch, n_ids, cap_points, pinned, guard=256):
        torch = _torch()
        kw = {"pin_memory": True} if pinned else {"device": "cuda"}
        self.cap, self.guard = cap_points, guard
        self.pts = torch.full(((cap_points + guard) * 4,), int(SENTINEL), dtype=torch.int32, **kw)
        self.off = torch.full((n_ids * batch + 1,), -7, dtype=torch.int64, **kw)
        self.recs = torch.zeros(batch * C.sizeof(_binding().AloamPoseRecord), dtype=torch.uint8, **kw)

    def host(self):
        return self.pts.cpu().numpy().view(np.float32).reshape(-1, 4), self.off.cpu().numpy(), self.recs.cpu().numpy()


def _binding():
    import importlib
    return importlib.import_module("a-loam_amd.binding")


def export_into(binding, gpu, ids, dest, cap=None):
    gpu.export_clouds(ids, dest.pts.data_ptr(), dest.cap if cap is None else cap, dest.off.data_ptr())
    gpu.export_poses(dest.recs.data_ptr())


def records(binding, raw, batch):
    return (binding.AloamPoseRecord * batch).from_buffer_copy(raw.tobytes())


def check_against_getters(binding, gpu, ids, pts, off, recs, mapping, seqs=None):
    B = gpu.batch
    for i, which in enumerate(ids):
        for b in (range(B) if seqs is None else seqs):
            want = getter(binding, gpu, which, b)
            got = pts[off[i * B + b]:off[i * B + b + 1]]
            assert _sha(got) == _sha(want), (which, b, got.shape, want.shape)
    for b in (range(B) if seqs is None else seqs):
        p, r = gpu.pose(b), recs[b]
        for key, field in (("q_w", "q_w"), ("t_w", "t_w"), ("q_lc", "q_last_curr"), ("t_lc", "t_last_curr")):
            assert _sha(np.array(getattr(r, field))) == _sha(p[key]), (b, field)
        if mapping:
            m = gpu.map_pose(b)
            for key, field in (("q_w", "map_q_w"), ("t_w", "map_t_w"), ("q_wmap_wodom", "q_wmap_wodom"), ("t_wmap_wodom", "t_wmap_wodom")):
                assert _sha(np.array(getattr(r, field))) == _sha(m[key]), (b, field)
            assert r.map_frames == gpu.map_info(b)["frame_count"]
        else:
            assert r.map_frames == -1 and not any(r.map_q_w) and not any(r.t_wmap_wodom)


def _drives(sequence, n, frames):
    out = []
    for i in range(n):
        scans, R, t, model = sequence("HDL-64", frames, seed=61 + 5 * i, columns=512, travel=True, step=1.6)
        out.append([x[40:] if i % 2 else x for x in scans])        # odd drives: the first rays of the first ring have no return (nearly ring-sorted clouds)
    return out, model


@pytest.mark.parametrize("pinned", [False, True])
def test_export_equals_the_getters(binding, sequence, pinned):
    F, B = 4, 6
    drives, model = _drives(sequence, B, F)
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=max(len(x) for d in drives for x in d) + 64)
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 17)
    for k in range(F):
        last = k == F - 1
        gpu.set_active([not (last and b == 4) for b in range(B)])            # sequence 4 sits out the last step
        gpu.scan_register([drives[b][k] if not (last and b == 4) else np.full((10, 4), np.nan, np.float32) for b in range(B)], check=False)
        gpu.odometry_step()
        gpu.set_active([not (last and b in (4, 5)) for b in range(B)])       # sequence 5 drops the last frame in mapping only
        gpu.mapping_step()
    gpu.synchronize()
    gpu.set_active(None)
    gpu.set_full_cloud(drives[3][0][:777], seq=3)                            # a cloud injected from outside
    ids = all_ids(binding)
    sizes = [sum(len(getter(binding, gpu, w, b)) for b in range(B)) for w in ids]
    assert all(sizes), sizes
    dest = Dest(B, len(ids), sum(sizes), pinned)
    export_into(binding, gpu, ids, dest)
    gpu.synchronize()
    pts, off, raw = dest.host()
    assert off[-1] == sum(sizes)
    recs = records(binding, raw, B)
    check_against_getters(binding, gpu, ids, pts, off, recs, mapping=True)
    assert [r.inited for r in recs] == [1] * B
    gpu.close()


@pytest.mark.parametrize("graph", ["0", "8"])
def test_exports_are_stream_ordered(binding, sequence, monkeypatch, graph):
    """Context A queues four steps, each followed by exports into that step's own buffers, with no host synchronisation in between; context B
    runs the same inputs and reads the getters after every step."""
    torch = _torch()
    monkeypatch.setenv("ALOAM_GRAPH_MAX_BATCH", graph)
    F, B = 4, 3
    drives, model = _drives(sequence, B, F)
    NP = max(len(x) for d in drives for x in d) + 64
    data = torch.zeros((B, F, NP, 4), dtype=torch.float32)
    for b in range(B):
        for k in range(F):
            data[b, k, :len(drives[b][k])] = torch.from_numpy(drives[b][k])
    data = data.cuda()
    stride = F * NP * 16
    masks = [None, None, [True, False, True], None]                     # sequence 1 sits out step 2
    ids = all_ids(binding)
    cap = 16 * B * NP                                                    # room for all twelve clouds of a step
    A = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=NP)
    A.mapping_enable(0.4, 0.8, pool_points=1 << 18)
    Bc = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=NP)
    Bc.mapping_enable(0.4, 0.8, pool_points=1 << 18)
    dests = [Dest(B, len(ids), cap, pinned=k % 2 == 1) for k in range(F)]
    torch.cuda.synchronize()
    for k in range(F):
        A.set_active(masks[k])
        A.process_device(data.data_ptr() + k * NP * 16, stride, [len(drives[b][k]) for b in range(B)])
        A.mapping_step()
        export_into(binding, A, ids, dests[k])
    A.synchronize()
    for k in range(F):
        Bc.set_active(masks[k])
        Bc.process_device(data.data_ptr() + k * NP * 16, stride, [len(drives[b][k]) for b in range(B)])
        Bc.mapping_step()
        Bc.synchronize()
        pts, off, raw = dests[k].host()
        check_against_getters(binding, Bc, ids, pts, off, records(binding, raw, B), mapping=True)
    A.close()
    Bc.close()


def window_of(map_pose_before, t_odom, cen):
    """laserCloudSurroundInd (reference src/laserMapping.cpp:512-529) rebuilt from aloam_get_map_info: the centre cube of
    transformAssociateToMap's t_w_curr (:142-146, :318-320) against the window origin after the step's shifts."""
    q, t = map_pose_before["q_wmap_wodom"], map_pose_before["t_wmap_wodom"]
    u = np.cross(q[:3], t_odom) * 2
    tw = t_odom + q[3] * u + np.cross(q[:3], u) + t
    c = [int((tw[a] + 25.0) / 50.0) + cen[a] - (1 if tw[a] + 25.0 < 0 else 0) for a in range(3)]
    return [i + 21 * j + 441 * k for i in range(c[0] - 2, c[0] + 3) for j in range(c[1] - 2, c[1] + 3) for k in range(c[2] - 1, c[2] + 2)
            if 0 <= i < 21 and 0 <= j < 21 and 0 <= k < 11]


def concat(cubes_corner, cubes_surf, order):
    parts = [p for c in order for p in (cubes_corner.get(c), cubes_surf.get(c)) if p is not None]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def _check_map_clouds(binding, gpu, O_cubes, seq, window, exact):
    """Getter, export and the cube concatenation in the reference's order agree bit for bit; the oracle's cubes within the voxel tolerance."""
    ids = [binding.EXPORT_MAP + binding.MAP_SURROUND, binding.EXPORT_MAP + binding.MAP_FULL]
    cc, cs = gpu.map_cubes(0, seq), gpu.map_cubes(1, seq)
    want = {ids[0]: concat(cc, cs, window), ids[1]: concat(cc, cs, range(4851))}
    dest = Dest(gpu.batch, 2, 8 * sum(len(v) for v in want.values()) * gpu.batch + 4096, pinned=False)   # (the other sequence's map is of the same frames)
    gpu.export_clouds(ids, dest.pts.data_ptr(), dest.cap, dest.off.data_ptr())
    gpu.synchronize()
    pts, off, _ = dest.host()
    for i, w in enumerate(ids):
        got_get = gpu.map_cloud(w - binding.EXPORT_MAP, seq)
        got_exp = pts[off[i * gpu.batch + seq]:off[i * gpu.batch + seq + 1]]
        assert bits_equal(got_get, want[w]) and bits_equal(got_exp, want[w]), (w, seq, got_get.shape, got_exp.shape, want[w].shape)
    oc, os_ = O_cubes
    for w, order in ((ids[0], window), (ids[1], range(4851))):
        o = concat(oc, os_, order)
        assert o.shape == want[w].shape, (w, o.shape, want[w].shape)
        if exact:
            assert bits_equal(o, want[w])
        else:
            tol = 2 * np.spacing(np.maximum(np.abs(o), np.abs(want[w])).astype(np.float32)).astype(np.float64) + 1e-12
            assert np.all(np.abs(o.astype(np.float64) - want[w]) <= tol)
    return len(want[ids[0]])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "refmap_hdl64_c256_seed13.npz"))))
def test_surround_and_full_map_in_reference_order_golden(O, binding, path):
    g = np.load(path)
    orc = O.Oracle(n_scans=int(g["n_scans"]), min_range=float(g["min_range"]))
    orc.map_config(float(g["line_res"]), float(g["plane_res"]))
    gpu = binding.Aloam(n_scans=int(g["n_scans"]), min_range=float(g["min_range"]), max_points=40000)
    gpu.mapping_enable(float(g["line_res"]), float(g["plane_res"]), pool_points=65536)
    assert len(gpu.map_cloud(binding.MAP_SURROUND)) == 0                 # no mapping step yet: an empty surround
    for k in range(int(g["frames"])):
        q, t, c, s, f = g[f"odom_q{k}"], g[f"odom_t{k}"], g[f"corner_last{k}"], g[f"surf_last{k}"], g[f"full{k}"]
        before = gpu.map_pose()
        orc.mapping_step(q, t, c, s, f)
        gpu.mapping_step_inputs(q, t, c, s, f)
        gpu.synchronize()
        info = gpu.map_info()
        window = window_of(before, np.asarray(t, np.float64), (info["cenW"], info["cenH"], info["cenD"]))
        assert _check_map_clouds(binding, gpu, (orc.map_cubes(0), orc.map_cubes(1)), 0, window, exact=False) > 0
    gpu.close()


def test_surround_and_full_map_follow_the_window_shifts(O, binding):
    """Poses that cross several 50 m cubes (the window shifts of src/laserMapping.cpp:323-507), solver off: bit-exact against the oracle."""
    rng = np.random.default_rng(5)
    orc = O.Oracle(16, 0.3, lm_max_iterations=0)
    orc.map_config(0.4, 0.8)
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=8192, lm_max_iterations=0)
    gpu.mapping_enable(0.4, 0.8, pool_points=131072)
    track = [(0, 0, 0), (120, -60, 0), (390, -380, 30), (420, -100, 160), (200, 30, 170), (-40, 390, -120), (-380, 395, -130), (-395, 0, 0)]
    cens = set()
    for k, (tx, ty, tz) in enumerate(track):
        pts = rng.uniform(-60, 60, (1500, 4)).astype(np.float32); pts[:, 3] = rng.integers(0, 16, 1500)
        surf = rng.uniform(-60, 60, (4000, 4)).astype(np.float32); surf[:, 2] *= 0.05; surf[:, 3] = rng.integers(0, 16, 4000)
        q = np.array([0, 0, np.sin(0.1 * k), np.cos(0.1 * k)]); t = np.array([tx, ty, tz], float)
        before = gpu.map_pose(0)
        orc.mapping_step(q, t, pts, surf, surf[:100])
        for seq in (0, 1):
            gpu.set_last(pts, surf, seq); gpu.set_full_cloud(surf[:100], seq); gpu.set_state([0, 0, 0, 1], [0, 0, 0], q, t, seq)
        gpu.set_active([True, k % 3 != 2])                                # sequence 1 drops some frames: its window is that of its last step
        gpu.mapping_step()
        gpu.synchronize()
        info = gpu.map_info(0)
        cens.add((info["cenW"], info["cenH"], info["cenD"]))
        window = window_of(before, t, (info["cenW"], info["cenH"], info["cenD"]))
        _check_map_clouds(binding, gpu, (orc.map_cubes(0), orc.map_cubes(1)), 0, window, exact=True)
    assert len(cens) > 3                                                  # the window did shift
    gpu.close()


def test_capacity_rules(binding, sequence):
    F, B = 3, 2
    drives, model = _drives(sequence, B, F)
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=max(len(x) for d in drives for x in d) + 64)
    for k in range(F):
        gpu.scan_register([drives[b][k] for b in range(B)])
        gpu.odometry_step()
    gpu.synchronize()
    ids = [binding.CLOUD_SHARP, binding.CLOUD_LESS_FLAT, binding.CLOUD_FLAT, binding.CLOUD_CORNER_LAST]
    want = [gpu.cloud(w, b) for w in ids for b in range(B)]
    total = sum(len(x) for x in want)
    ref_off = np.concatenate([[0], np.cumsum([len(x) for x in want])])
    seg = 1 + int(np.argmax([len(x) for x in want[1:]]))                 # a long segment that is not the first
    cases = {"size query": 0, "mid-segment": int(ref_off[seg] + len(want[seg]) // 2), "exact": total}
    for name, cap in cases.items():
        dest = Dest(B, len(ids), total, pinned=False, guard=512)
        gpu.export_clouds(ids, dest.pts.data_ptr(), cap, dest.off.data_ptr())
        gpu.synchronize()
        pts, off, _ = dest.host()
        assert np.array_equal(off, ref_off), name
        raw = pts.view(np.uint32)
        assert (raw[total:] == SENTINEL).all(), name                      # the guard region is never touched
        for s, x in enumerate(want):
            got = pts[ref_off[s]:ref_off[s + 1]]
            if ref_off[s + 1] <= cap:
                assert bits_equal(got, x), (name, s)
            else:
                assert (got.view(np.uint32) == SENTINEL).all(), (name, s)
        assert (raw[cap:] == SENTINEL).all(), name                        # nothing past cap_points
    gpu.close()


def test_argument_rules(binding, sequence):
    torch = _torch()
    F, B = 2, 2
    drives, model = _drives(sequence, B, F)
    NP = max(len(x) for d in drives for x in d) + 64
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=NP)
    for k in range(F):
        gpu.scan_register([drives[b][k] for b in range(B)])
        gpu.odometry_step()
    gpu.synchronize()
    L = binding.lib()
    dest = Dest(B, 4, 4 * B * NP, pinned=False)

    def call(ids, pts_ptr, cap, off_ptr):
        a = (C.c_int * max(1, len(ids)))(*ids)
        return L.aloam_export_clouds(gpu.h, a, len(ids), C.c_void_p(pts_ptr) if pts_ptr else None, cap, C.c_void_p(off_ptr))

    assert call([99], dest.pts.data_ptr(), dest.cap, dest.off.data_ptr()) == binding.E_ARG                 # unknown id
    assert call([binding.CLOUD_SHARP, binding.CLOUD_SHARP], dest.pts.data_ptr(), dest.cap, dest.off.data_ptr()) == binding.E_ARG   # repeated
    assert call(list(range(13)), dest.pts.data_ptr(), dest.cap, dest.off.data_ptr()) == binding.E_ARG      # more than ALOAM_EXPORT_MAX_IDS
    assert call([binding.EXPORT_MAP + binding.MAP_SURROUND], dest.pts.data_ptr(), dest.cap, dest.off.data_ptr()) == binding.E_STATE   # no mapping
    pageable = np.zeros(4 * 1024, np.float32)
    assert call([binding.CLOUD_SHARP], pageable.ctypes.data, 0, dest.off.data_ptr()) == binding.E_ARG    # pageable points (cap 0: nothing could be written)
    if torch.cuda.device_count() > 1:
        other = torch.zeros(4 * 1024, dtype=torch.float32, device="cuda:1")
        assert call([binding.CLOUD_SHARP], other.data_ptr(), 1024, dest.off.data_ptr()) == binding.E_ARG
        assert L.aloam_export_poses(gpu.h, C.c_void_p(other.data_ptr())) == binding.E_ARG
    gpu.synchronize()
    _, off, _ = dest.host()
    assert (off == -7).all() and (dest.pts.cpu().numpy().view(np.uint32) == SENTINEL).all()   # nothing was queued
    # a stage the context was created without
    mo = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=NP, stages=binding.STAGE_MAPPING)
    mo.mapping_enable(0.4, 0.8, pool_points=1 << 16)
    for w in (binding.CLOUD_SHARP, binding.CLOUD_FLAT, binding.CLOUD_LESS_SHARP, binding.CLOUD_LESS_FLAT):
        a = (C.c_int * 1)(w)
        assert L.aloam_export_clouds(mo.h, a, 1, C.c_void_p(dest.pts.data_ptr()), dest.cap, C.c_void_p(dest.off.data_ptr())) == binding.E_STATE, w
    ok = (C.c_int * 2)(binding.CLOUD_CORNER_LAST, binding.EXPORT_MAP + binding.MAP_SURROUND)   # what a mapping-only context holds
    assert L.aloam_export_clouds(mo.h, ok, 2, C.c_void_p(dest.pts.data_ptr()), dest.cap, C.c_void_p(dest.off.data_ptr())) == 0
    mo.synchronize()
    assert dest.off.cpu().numpy()[:2 * B + 1].tolist() == [0] * (2 * B + 1)
    mo.close()
    # a following export is unaffected
    ids = [binding.CLOUD_SHARP, binding.CLOUD_FULL, binding.CLOUD_SURF_LAST, binding.CLOUD_LESS_SHARP]
    export_into(binding, gpu, ids, dest)
    gpu.synchronize()
    pts, off, raw = dest.host()
    check_against_getters(binding, gpu, ids, pts, off, records(binding, raw, B), mapping=False)
    # n_ids = 0: only the total
    assert call([], dest.pts.data_ptr(), dest.cap, dest.off.data_ptr()) == 0
    gpu.synchronize()
    assert int(dest.off.cpu()[0]) == 0
    gpu.close()


def test_benchmark_size(binding, syn):
    """Batch 256 of 64 x 2048 sweeps (the headline sensor): the offsets of every sequence are the getters' sizes; a seeded sample of 8 sequences
    is bit-identical."""
    torch = _torch()
    B, F, distinct = 256, 3, 8
    model = syn.sensor_model("HDL-64", device="cuda")
    NP = model.dirs.shape[0]
    data = torch.zeros((B, F, NP, 4), dtype=torch.float32, device="cuda")
    counts = np.zeros((B, F), np.int32)
    world = syn.make_world(101).to("cuda")
    for d in range(distinct):
        R, t = syn.trajectory(F, step=1.0, seed=d, start_angle=0.37 * d)
        gen = torch.Generator(device="cuda").manual_seed(9000 + d)
        for k in range(F):
            s = syn.render_scan(world, model, R[k], t[k], 0.02, gen)
            counts[d::distinct, k] = s.shape[0]
            data[d::distinct, k, :s.shape[0]] = s
    gpu = binding.Aloam(n_scans=64, min_range=model.min_range, batch=B, max_points=NP, max_ring_points=2059)
    for k in range(F):
        gpu.process_device(data.data_ptr() + k * NP * 16, F * NP * 16, counts[:, k])
    ids = list(range(7))
    off_t = torch.zeros(len(ids) * B + 1, dtype=torch.int64, device="cuda")
    gpu.export_clouds(ids, 0, 0, off_t.data_ptr())                        # size query
    gpu.synchronize()
    off = off_t.cpu().numpy()
    L = binding.lib()
    sizes = np.array([[L.aloam_cloud_size(gpu.h, b, w) for b in range(B)] for w in ids]).reshape(-1)
    assert np.array_equal(np.diff(off), sizes)
    pts_t = torch.empty((int(off[-1]), 4), dtype=torch.float32, device="cuda")
    recs = torch.zeros(B * C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, device="cuda")
    gpu.export_clouds(ids, pts_t.data_ptr(), int(off[-1]), off_t.data_ptr())
    gpu.export_poses(recs.data_ptr())
    gpu.synchronize()
    assert np.array_equal(off_t.cpu().numpy(), off)
    sample = sorted(np.random.default_rng(2024).choice(B, 8, replace=False).tolist())
    check_against_getters(binding, gpu, ids, pts_t.cpu().numpy(), off, records(binding, recs.cpu().numpy(), B), mapping=False, seqs=sample)
    gpu.close()
