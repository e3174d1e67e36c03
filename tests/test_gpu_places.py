"""Place recognition on the MI355X (aloam_places_*): the scan-context descriptor against the numpy model, distances, shifts and ranks of
the matrix-core match against the float64 model, determinism across call shapes, stream order, export / load round trips, the errors, a
twin context that never enables places, and the chain match -> grid search -> frozen steps from no prior at all."""
import importlib
import math

import numpy as np
import pytest
import torch

from places_common import MATCH_DRIVE, MATCH_T, db_slots, kept, query_slots
from test_gpu_checkpoint import make
from test_gpu_localization import SECOND_PASS_BOUND_M, cubes, frame
from test_gpu_sequence_lifecycle import NAN_ROW, diff, snap

pytestmark = pytest.mark.gpu
pl = importlib.import_module("a-loam_amd.places")
rl = importlib.import_module("a-loam_amd.relocalize")


def _cells(rec):
    """[20, 60] descriptor(s) of exported place record(s) (the store keeps them sector-major)."""
    return np.swapaxes(rec["cells"], -1, -2)


# ---- descriptor against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cols,seed", [("HDL-64", 2048, 31), ("VLP-16", 600, 5)])
def test_descriptor_equals_the_model_in_a_mixed_batch(binding, sequence, name, cols, seed):
    scans, R, t, model = sequence(name, 2, seed=seed, columns=cols)
    gpu = make(binding, model, 3, max(len(s) for s in scans) + 64, False)
    gpu.profile_enable(True)
    gpu.places_enable(8)
    gpu.scan_register([scans[0]] * 3, check=False)
    gpu.odometry_step()
    gpu.set_active([True, False, True])                                   # slot 1 sits the second sweep out and keeps the first
    gpu.scan_register([scans[1], NAN_ROW, scans[1]], check=False)
    gpu.odometry_step()
    gpu.synchronize()
    dense = gpu.profile()["k_dense_cloud"]["launches"]
    assert gpu.places_add([2, 1, 0]) == 0
    rec = gpu.places_export()
    assert gpu.profile()["k_dense_cloud"]["launches"] == dense            # made from the ring slabs: the dense cloud is not assembled for it
    assert rec["slot"].tolist() == [2, 1, 0] and rec["frame"].tolist() == [-1, -1, -1]
    n_exc = []
    for i, b in enumerate((2, 1, 0)):
        cloud = gpu.cloud(binding.CLOUD_FULL, b)
        # the full cloud is what scan registration keeps: the NaN / range filter, then the rays whose elevation maps to no ring are dropped too
        assert rec["n_points"][i] == len(cloud) and 0 < len(cloud) <= len(kept(scans[0 if b == 1 else 1], model.min_range))
        p = gpu.pose(b)
        assert np.array_equal(rec["q"][i], p["q_w"]) and np.array_equal(rec["t"][i], p["t_w"])   # without mapping: the odometry pose
        D, got = pl.scan_context(cloud), _cells(rec[i])
        lo, hi = pl.scan_context_bounds(cloud)
        exc = lo != hi
        n_exc.append(int(exc.sum()))
        assert n_exc[-1] <= 12, n_exc
        assert np.array_equal(got[~exc].view(np.uint32), D[~exc].view(np.uint32)), (b, int((got != D).sum()))
        assert np.all((got[exc] >= lo[exc]) & (got[exc] <= hi[exc]))
    print(f"{name} x {cols}: cells under the border exception per sweep {n_exc}")
    assert np.array_equal(rec["cells"][0], rec["cells"][2]) and not np.array_equal(rec["cells"][0], rec["cells"][1])
    gpu.close()


# ---- the store of the match tests ------------------------------------------------------------------------------------------------------
def _drive(sequence):
    kw = dict(MATCH_DRIVE)
    return sequence(kw.pop("name"), kw.pop("frames"), **kw)


def _registered(binding, sequence, capacity=64):
    scans, R, t, model = _drive(sequence)
    gpu = make(binding, model, len(scans), max(len(s) for s in scans) + 64, False)
    gpu.places_enable(capacity)
    gpu.scan_register(scans, check=False)
    gpu.odometry_step()
    return gpu


@pytest.fixture(scope="module")
def store(binding, sequence):
    """Slot b holds sweep b of the drive; entries 0 .. 11 are the even slots, 12 .. 23 the odd ones (the queries, stored only so that their
    descriptors can be exported and handed to the model)."""
    gpu = _registered(binding, sequence)
    assert gpu.places_add(db_slots()) == 0
    assert gpu.places_add(query_slots()) == len(db_slots())
    rec = gpu.places_export()
    desc = {b: _cells(rec[i]) for i, b in enumerate(db_slots() + query_slots())}
    yield gpu, rec, desc
    gpu.close()


def _model(desc, b, lo, hi, T):
    db = np.stack([desc[s] for s in db_slots()[lo:hi]]) if hi > lo else np.zeros((0, pl.RINGS, pl.SECTORS), np.float32)
    return pl.match(desc[b], db, T, first=lo)


def test_distances_shifts_and_ranks_equal_the_model(store):
    """The device sums 1200 f32 products per (entry, shift) as an fmaf chain: its error is at most 1.5e-7 * sum |a b| <= 1.5e-7 * 60, divided
    by cnt - near 1e-5 at worst; 1e-4 leaves a decade."""
    gpu, rec, desc = store
    N, Q = len(db_slots()), query_slots()
    res = gpu.places_match(Q, [(0, N)] * len(Q), MATCH_T)
    worst = 0.0
    for i, b in enumerate(Q):
        ent, sh, di = _model(desc, b, 0, N, MATCH_T)
        gaps = np.diff(np.sort(pl.shift_distances(desc[b], np.stack([desc[s] for s in db_slots()])).min(axis=1))[:MATCH_T + 1])
        assert gaps.min() > 2e-4, (b, gaps)                               # the input check of test_places_model, on the device's own descriptors
        worst = max(worst, float(np.abs(res["distance"][i] - di).max()))
        assert res["entry"][i].tolist() == ent.tolist() and res["shift"][i].tolist() == sh.tolist(), (b, res[i], ent, sh, di)
        assert np.all(np.diff(res["distance"][i]) >= 0)
        assert abs(2 * int(res["entry"][i][0]) - b) == 1                   # the best stored place is a neighbouring sweep of the drive
    print(f"max |distance - f64 model| over {len(Q)} x {MATCH_T} results: {worst:.3e}")
    assert worst <= 1e-4
    assert np.all(res["pad"] == 0)


def test_ranges_are_respected(store):
    gpu, rec, desc = store
    Q = query_slots()[:4]
    ranges = [(3, 9), (0, 2), (5, 5), (11, 12)]
    res = gpu.places_match(Q, ranges, MATCH_T)
    for i, (b, (lo, hi)) in enumerate(zip(Q, ranges)):
        ent, sh, di = _model(desc, b, lo, hi, MATCH_T)
        assert res["entry"][i].tolist() == ent.tolist() and res["shift"][i].tolist() == sh.tolist(), (b, lo, hi, res[i])
        assert all(e == -1 or lo <= e < hi for e in res["entry"][i])
        assert np.abs(res["distance"][i] - di).max() <= 1e-4
        assert len(set(e for e in res["entry"][i] if e >= 0)) == min(MATCH_T, hi - lo)   # each entry at most once, -1 fills the rest
    # a query may be matched against its own entry: distance 0 up to rounding, shift 0
    own = gpu.places_match([query_slots()[0]], [(len(db_slots()), len(db_slots()) + 1)], 1)
    assert own["entry"][0, 0] == len(db_slots()) and own["shift"][0, 0] == 0 and abs(float(own["distance"][0, 0])) <= 1e-5


def test_a_pair_has_the_same_bits_in_every_call_shape(store):
    gpu, rec, desc = store
    N, Q = len(db_slots()), query_slots()
    seen = {}

    def run(seqs, ranges, T, pinned=True):
        res = gpu.places_match(seqs, ranges, T, pinned=pinned)
        for i, b in enumerate(seqs):
            for k in range(T):
                if res["entry"][i, k] >= 0:
                    key, val = (b, int(res["entry"][i, k])), res[i, k].tobytes()
                    assert seen.setdefault(key, val) == val, (key, seqs, ranges, T)
    run(Q, [(0, N)] * len(Q), 8)
    run(Q[::-1], [(0, N)] * len(Q), 3)
    run([Q[5]], [(0, N)], 1)
    run([Q[5], Q[0]], [(2, N), (1, 7)], 8, pinned=False)
    run(Q[:3], [(0, N + len(Q))] * 3, 8)                                   # other tile contents: the queries' own entries are in range too
    assert len(seen) >= len(Q) * 8


def test_add_then_match_needs_no_synchronise_and_a_loaded_store_matches_alike(binding, sequence, store):
    ref, rec, desc = store
    N, Q = len(db_slots()), query_slots()
    want = ref.places_match(Q, [(0, N)] * len(Q), MATCH_T)
    gpu = _registered(binding, sequence)
    dst = torch.zeros(len(Q) * MATCH_T * 16, dtype=torch.uint8).pin_memory()
    gpu.places_add(db_slots())                                             # queued: nothing waits between the add and the match
    gpu.places_match_into(Q, [(0, N)] * len(Q), MATCH_T, dst.data_ptr())
    gpu.synchronize()
    assert dst.numpy().tobytes() == want.tobytes()
    assert gpu.places_export().tobytes() == rec[:N].tobytes()
    # round trip: the exported records loaded from pageable memory, and again from device memory behind them
    gpu.places_clear()
    assert gpu.places_info()["count"] == 0
    assert gpu.places_load(rec[:N]) == 0
    assert gpu.places_match(Q, [(0, N)] * len(Q), MATCH_T).tobytes() == want.tobytes()
    dev = torch.from_numpy(rec[:N].copy().view(np.uint8)).cuda()
    assert gpu.places_load(dev) == N and gpu.places_info()["count"] == 2 * N
    again = gpu.places_match(Q, [(N, 2 * N)] * len(Q), MATCH_T)
    assert np.array_equal(again["entry"] - N, want["entry"]) and again["distance"].tobytes() == want["distance"].tobytes()
    assert gpu.places_export(N, N, pinned=False).tobytes() == rec[:N].tobytes()
    # a record with a negative or non-finite cell is refused and nothing changes
    bad = rec[:2].copy()
    bad["cells"][1, 3, 4] = -1.0
    with pytest.raises(binding.AloamError) as e:
        gpu.places_load(bad)
    assert e.value.code == binding.E_ARG
    bad["cells"][1, 3, 4] = np.nan
    with pytest.raises(binding.AloamError) as e:
        gpu.places_load(bad)
    assert e.value.code == binding.E_ARG and gpu.places_info()["count"] == 2 * N
    # so is a positive cell outside [2^-62, 2^60]: the f32 norm of its column would underflow to 0 or overflow to inf
    for cell in (1e-25, 1e20):
        bad["cells"][1, 3, 4] = cell
        with pytest.raises(binding.AloamError) as e:
            gpu.places_load(bad)
        assert e.value.code == binding.E_ARG and gpu.places_info()["count"] == 2 * N
    gpu.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _code(binding, fn, *a, **kw):
    with pytest.raises(binding.AloamError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors(binding, sequence):
    scans, R, t, model = sequence("VLP-16", 2, seed=5, columns=600)
    gpu = make(binding, model, 2, max(len(s) for s in scans) + 64, False)
    assert _code(binding, gpu.places_add, [0]) == binding.E_STATE          # not enabled
    assert _code(binding, gpu.places_enable, 0) == binding.E_ARG
    assert _code(binding, gpu.places_enable, 4, max_range=0.0) == binding.E_ARG
    gpu.places_enable(3)
    assert _code(binding, gpu.places_enable, 3) == binding.E_STATE
    assert _code(binding, gpu.places_add, [0]) == binding.E_STATE          # no sweep registered yet
    gpu.set_active([True, False])
    gpu.scan_register([scans[0], NAN_ROW], check=False)
    gpu.odometry_step()
    gpu.set_active(None)
    assert _code(binding, gpu.places_add, [0, 1]) == binding.E_STATE and gpu.places_info()["count"] == 0   # slot 1 has sat every registration out
    gpu.scan_register([scans[1], scans[0]], check=False)                   # two different sweeps: each slot's best place is its own
    gpu.odometry_step()
    assert gpu.places_add([0, 1]) == 0
    assert _code(binding, gpu.places_add, [0, 1]) == binding.E_CAPACITY and gpu.places_info()["count"] == 2   # full: nothing was queued
    assert _code(binding, gpu.places_add, [0, 0]) == binding.E_ARG
    assert _code(binding, gpu.places_match, [0], [(0, 2)], 0) == binding.E_ARG
    assert _code(binding, gpu.places_match, [0], [(0, 2)], 9) == binding.E_ARG
    assert _code(binding, gpu.places_match, [0], [(2, 1)]) == binding.E_ARG     # reversed
    assert _code(binding, gpu.places_match, [0], [(0, 3)]) == binding.E_ARG     # past the entries stored so far
    assert _code(binding, gpu.places_match, [2], [(0, 2)]) == binding.E_ARG
    pageable = np.zeros(16, np.uint8)
    assert _code(binding, gpu.places_match_into, [0], [(0, 2)], 1, pageable.ctypes.data) == binding.E_ARG
    assert _code(binding, gpu.places_export_into, 0, 2, np.zeros(2, binding.PLACE_DTYPE).ctypes.data) == binding.E_ARG
    assert _code(binding, gpu.places_export_into, 1, 2, 0) == binding.E_ARG
    ok = gpu.places_match([0, 1], [(0, 2), (0, 2)], 2)
    assert ok["entry"][:, 0].tolist() == [0, 1]
    # a reset or loaded slot holds no sweep until it registers one; the store itself is left alone
    blob, off = gpu.save_sequences([0])
    gpu.reset_sequences([1])
    assert _code(binding, gpu.places_match, [1], [(0, 2)]) == binding.E_STATE
    gpu.load_sequences([0], blob, off)
    assert _code(binding, gpu.places_add, [0]) == binding.E_STATE
    assert gpu.places_info()["count"] == 2 and gpu.places_export()["slot"].tolist() == [0, 1]
    gpu.close()
    odo = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=1, max_points=4096, stages=binding.STAGE_ODOMETRY)
    assert _code(binding, odo.places_enable, 4) == binding.E_STATE         # no registration stage: no sweeps to describe
    odo.close()


# ---- a twin that never enables places -----------------------------------------------------------------------------------------------
def test_a_twin_without_places_returns_the_same_bits(binding, sequence):
    F = 4
    scans, R, t, model = sequence("HDL-64", F, seed=41, columns=512)
    ctx = [make(binding, model, 2, max(len(s) for s in scans) + 64, True) for _ in range(2)]
    ctx[0].places_enable(16)
    for k in range(F):
        for g in ctx:
            frame(g, [scans[k], scans[k] if k % 2 == 0 else None])
        ctx[0].places_add([0, 1])
        m = ctx[0].places_match([1, 0], [(0, 2 * k + 2)] * 2, 2)
        assert m["entry"][0, 0] >= 0
        for g in ctx:
            g.synchronize()
        for b in range(2):
            a, c = snap(binding, ctx[0], b, True), snap(binding, ctx[1], b, True)
            assert not diff(a, c), (k, b, diff(a, c))
    rec = ctx[0].places_export()
    assert rec["frame"].tolist() == [1, 1, 2, 1, 3, 2, 4, 2]               # map_frames of the slot when each place was stored
    p = ctx[0].map_pose(0)
    assert np.array_equal(rec["q"][-2], p["q_w"]) and np.array_equal(rec["t"][-2], p["t_w"])   # with mapping: the map pose
    for g in ctx:
        g.close()


# ---- end to end: match -> guess -> frozen step -> grid search -> frozen steps -----------------------------------------------------------
def _rz(deg):
    a = math.radians(deg)
    return torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


def test_fresh_sequences_localize_with_no_prior(binding, sequence, syn):
    """DESIGN.md §7h.  The drive of test_second_pass_localizes_in_the_first_pass_map is mapped with a place every
    second frame; then fresh sequences start mid-drive from an identity odometry pose: slot 0 on the drive's heading, 1.5 m aside and 30 deg
    turned; slot 1 driving it backwards, 2 m aside.  Slots 2 and 3 are the same starts without the match (the identity correction)."""
    F, G = 30, 5
    scans, R, t, model = sequence("HDL-64", F, seed=43, columns=512)
    R, t = torch.from_numpy(R), torch.from_numpy(t)
    mp = max(len(s) for s in scans) + 4096
    A = make(binding, model, 1, mp, True)
    A.places_enable(F)
    for k in range(F):
        frame(A, [scans[k]])
        if k % 2 == 0:
            assert A.places_add([0]) == k // 2
    A.synchronize()
    m, info, places = cubes(A, 0), A.map_info(0), A.places_export()
    A.close()
    assert places["frame"].tolist() == list(range(1, F + 1, 2))

    world, gen = syn.make_world(43), torch.Generator().manual_seed(4343)
    starts = [[(R[k] @ _rz(30.0), t[k] + R[k] @ torch.tensor([0.0, 1.5, 0.0], dtype=torch.float64)) for k in range(12, 12 + G)],
              [(R[k] @ _rz(180.0), t[k] + R[k] @ torch.tensor([0.0, -2.0, 0.0], dtype=torch.float64)) for k in range(20, 20 - G, -1)]]
    sweeps = [[syn.render_scan(world, model, Rq, tq, 0.02, gen).numpy() for Rq, tq in s] for s in starts]
    truth = [[(R[0].T @ (tq - t[0])).numpy() for Rq, tq in s] for s in starts]

    B = make(binding, model, 4, mp, True)
    B.places_enable(len(places))
    B.places_load(places)
    cen = (info["cenW"], info["cenH"], info["cenD"])
    for b in range(4):
        for cls in (0, 1):
            B.set_map(m[cls], cls, seq=b)
    frozen = [True] * 4
    for j in range(G):
        batch = [sweeps[0][j], sweeps[1][j], sweeps[0][j], sweeps[1][j]]
        if j > 0:
            frame(B, batch, frozen=frozen)
            continue
        B.set_active(None)
        B.scan_register(batch, check=False)
        B.odometry_step()
        match = B.places_match([0, 1])
        for b in range(4):
            if b < 2:
                e, s = int(match["entry"][b, 0]), int(match["shift"][b, 0])
                odom = B.pose(b)
                q, tt = pl.guess_from_match(places["q"][e], places["t"][e], s, odom["q_w"], odom["t_w"])
                print(f"slot {b}: matched place {e} (frame {2 * e}) shift {s} distance {float(match['distance'][b, 0]):.3f}; guess off by "
                      f"{np.linalg.norm(tt - truth[b][0]):.2f} m")
            else:
                q, tt = (0, 0, 0, 1), (0, 0, 0)
            B.set_map_frame(cen, q, tt, 0, seq=b)
        B.set_map_frozen(frozen)
        B.mapping_step()
        rl.relocalize(B, [0, 1, 2, 3])
    B.synchronize()
    err = [float(np.linalg.norm(B.map_pose(b)["t_w"] - truth[b % 2][G - 1])) for b in range(4)]
    print(f"final |t - gt|: with the match {err[0]:.4f} m, {err[1]:.4f} m; without {err[2]:.2f} m, {err[3]:.2f} m")
    assert max(err[:2]) < SECOND_PASS_BOUND_M, err
    assert min(err[2:]) > 1.0, err                                         # the grid of relocalize() alone does not reach: these never converge
    B.close()


def test_kitti_runner_relocalizes_globally_from_the_places_in_the_atlas_file(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    atlas = importlib.import_module("a-loam_amd.atlas")
    tool = [sys.executable, os.path.join(root, "tools", "run_kitti.py"), "--selftest"]
    a = tmp_path / "atlas.npz"
    r = subprocess.run(tool + ["--mapping", "--out", str(tmp_path / "out"), "--save-atlas", str(a), "--place-spacing", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and " places (" in r.stdout, r.stdout + r.stderr
    stored = atlas.load_atlas_places(a)
    assert 2 <= len(stored) <= 3 and stored["frame"][0] == 1 and np.all(np.diff(stored["frame"]) >= 2)   # six sweeps 1 m apart, a place every 2 m
    r = subprocess.run(tool + ["--out", str(tmp_path / "loc"), "--prior-atlas", str(a), "--global-relocalize"], capture_output=True, text=True)
    assert r.returncode == 0 and "matched place 0 of" in r.stdout and "shift 0 " in r.stdout and " relocalized: " in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if " localized: " in l and "final error" in l]
    assert line and float(line[0].split("final error = ")[1].split()[0]) < SECOND_PASS_BOUND_M, r.stdout
