"""Per-sequence lifecycle on the MI355X (aloam_set_active, aloam_reset_sequences): a sequence of a batch sits out steps with its state kept
bit for bit, drops frames in mapping only, or restarts in place as a fresh context would - while the other sequences run on undisturbed."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest


pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_ROW = np.full((100, 4), np.nan, np.float32)      # what an idle row holds: its points must never be read


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def snap(binding, gpu, b, mapping):
    """Everything a getter returns for sequence b, as comparable values."""
    s = {k: _sha(v) for k, v in gpu.features(b).items()}
    for name, which in (("corner_last", binding.CLOUD_CORNER_LAST), ("surf_last", binding.CLOUD_SURF_LAST)):
        s[name] = _sha(gpu.cloud(which, b))
    s["pose"] = _sha(np.concatenate(list(gpu.pose(b).values())))
    s["stats"] = repr(gpu.odom_stats(b))
    s["corr"] = [_sha(x) for x in gpu.correspondences(b)]
    s["rings"] = [_sha(x) for x in gpu.ring_ranges(b)]
    s["order"] = gpu.last_cloud_order(b)
    if mapping:
        s["map_pose"] = _sha(np.concatenate(list(gpu.map_pose(b).values())))
        s["map_info"] = repr(gpu.map_info(b))
        s["cubes"] = [{c: _sha(p) for c, p in gpu.map_cubes(cls, b).items()} for cls in (0, 1)]
        s["registered"] = _sha(gpu.map_cloud(binding.MAP_REGISTERED, b))
    return s


def diff(a, b):
    """Names of the getters whose values differ between two snapshots (empty: bit-identical)."""
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def run(binding, model, drives, plan, mapping=False, pool=1 << 17, max_points=None, ref_order=False, snap_steps=None, on_step=None):
    """One batch context.  plan: per step a list over the slots of (drive, frame, map) or None (idle); map False = the frame is
    registered and odometry runs, but the slot is idle in mapping.  plan entries ('reset', [slots]) queue a reset.  Returns
    {(slot, step): snapshot} after every step (or the steps in snap_steps) for the active slots and {(slot, step): snapshot} of the idle ones."""
    B = len(next(p for p in plan if not isinstance(p, tuple)))
    mp = max_points or max(len(x) for d in drives for x in d) + 64
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=mp)
    if ref_order:
        gpu.set_voxel_sum_order(True)
    if mapping:
        gpu.mapping_enable(0.4, 0.8, pool_points=pool)
    active_snaps, idle_snaps, step = {}, {}, 0
    for entry in plan:
        if isinstance(entry, tuple):
            gpu.reset_sequences(entry[1])
            continue
        mask = [e is not None for e in entry]
        gpu.set_active(mask)
        gpu.scan_register([drives[e[0]][e[1]] if e is not None else NAN_ROW for e in entry], check=False)
        gpu.odometry_step()
        if mapping:
            gpu.set_active([e is not None and e[2] for e in entry])
            gpu.mapping_step()
        if on_step:
            on_step(gpu, step)
        if snap_steps is None or step in snap_steps:
            gpu.synchronize()
            for b, e in enumerate(entry):
                (active_snaps if e is not None else idle_snaps)[(b, step)] = snap(binding, gpu, b, mapping)
        step += 1
    gpu.close()
    return active_snaps, idle_snaps


def alone(binding, model, drive, frames, mapping=False, map_on=None, **kw):
    """Batch-1 reference: the frames of one drive with no gap; map_on[k] False = no mapping step on frame k."""
    plan = [[(0, k, True if map_on is None else map_on[k])] for k in frames]
    snaps, _ = run(binding, model, [drive], plan, mapping=mapping, **kw)
    return [snaps[(0, i)] for i in range(len(frames))]


def _drives(sequence, n, frames, name="HDL-64", cols=512):
    out = []
    for i in range(n):
        scans, R, t, model = sequence(name, frames, seed=41 + 7 * i, **({"columns": cols} if name == "HDL-64" else {}))
        out.append(scans)
    return out, model


@pytest.mark.parametrize("idle_seq", [1, 0])
@pytest.mark.parametrize("mapping", [False, True])
def test_idle_sequence_keeps_its_state_and_resumes_as_if_never_paused(binding, sequence, idle_seq, mapping):
    F = 7
    drives, model = _drives(sequence, 3, F)
    gap = (2, 3, 4)                                                      # the idle sequence sits out these steps, then takes its next sweep
    plan, nxt, growth = [], [0, 0, 0], {}
    for step in range(F + len(gap)):
        row = []
        for b in range(3):
            if (b == idle_seq and step in gap) or nxt[b] >= F:
                row.append(None)
            else:
                row.append((b, nxt[b], True)); nxt[b] += 1
        plan.append(row + [None])                                        # slot 3 never runs: a map injected there forces a pool growth

    def grow_pool(gpu, step):
        if step == gap[0]:                                               # a map one point larger than the pool: every pool is doubled and moved
            n = gpu.map_pool_info()["pool_points"] + 1
            gpu.set_map({0: np.zeros((n, 4), np.float32)}, 0, seq=3)
        growth[step] = gpu.map_pool_info()["growths"]
    act, idle = run(binding, model, drives, plan, mapping=mapping, on_step=grow_pool if mapping else None)
    if mapping:
        assert growth[gap[0]] > growth[gap[0] - 1], growth               # the pools grew while the sequence was idle: its map came through the move
    before = act[(idle_seq, gap[0] - 1)]
    for step in gap:
        assert not diff(idle[(idle_seq, step)], before), (step, diff(idle[(idle_seq, step)], before))                    # every getter: the same bits as before the idle steps
    for b in range(3):
        ref = alone(binding, model, drives[b], range(F), mapping=mapping)
        got = [act[k] for k in sorted(k for k in act if k[0] == b)]
        assert len(got) == F
        for k in range(F):
            assert not diff(got[k], ref[k]), (b, k, diff(got[k], ref[k]))
    # the others are also those of the all-active batch (no sequence idle)
    full, _ = run(binding, model, drives, [[(b, k, True) for b in range(3)] for k in range(F)], mapping=mapping, snap_steps={F - 1})
    for b in range(3):
        if b != idle_seq:
            assert not diff(full[(b, F - 1)], act[(b, F - 1)]), (b, diff(full[(b, F - 1)], act[(b, F - 1)]))


def test_mapping_drops_frames_of_one_sequence(O, binding, sequence):
    F = 7
    drives, model = _drives(sequence, 2, F)
    dropped = {2, 3, 5}                                                  # sequence 1 skips mapping on these frames; odometry runs on all of them
    plan = [[(0, k, True), (1, k, k not in dropped)] for k in range(F)]
    act, _ = run(binding, model, drives, plan, mapping=True)
    map_on = [k not in dropped for k in range(F)]
    for b, mo in ((0, None), (1, map_on)):
        ref = alone(binding, model, drives[b], range(F), mapping=True, map_on=mo)
        for k in range(F):
            assert not diff(act[(b, k)], ref[k]), (b, k, diff(act[(b, k)], ref[k]))
    # and the chained oracle with mappingProcess skipped on the same frames
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=2, max_points=max(len(x) for d in drives for x in d) + 64)
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 17)
    orc = O.Oracle(n_scans=model.n_scans, min_range=model.min_range)
    orc.map_config(0.4, 0.8)
    for k in range(F):
        gpu.set_active(None)
        gpu.scan_register([drives[0][k], drives[1][k]], check=False)
        gpu.odometry_step()
        gpu.set_active([True, map_on[k]])
        gpu.mapping_step()
        orc.scan_register(drives[1][k])
        po = orc.odometry_step()
        if map_on[k]:
            pm = orc.mapping_step(po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
            mg = gpu.map_pose(1)
            for key in ("q_w", "t_w"):
                assert np.abs(pm[key] - mg[key]).max() < 1e-8, (k, key, pm[key], mg[key])
    gpu.close()


@pytest.mark.parametrize("graph", ["0", "8"])
def test_slot_recycling_restarts_as_a_fresh_context(binding, sequence, monkeypatch, graph):
    monkeypatch.setenv("ALOAM_GRAPH_MAX_BATCH", graph)
    drives, model = _drives(sequence, 3, 8)
    A, Bd, C = 0, 1, 2
    plan = [[(A, k, True), (Bd, k, True)] for k in range(5)]
    plan.append([None, (Bd, 5, True)])                                  # drive A has ended: slot 0 sits a step out (the mask changes)
    plan.append(("reset", [0]))                                         # queued with no synchronisation in between
    plan += [[(C, k, True), (Bd, 6 + k, True)] for k in range(2)]
    plan += [[(C, 2 + k, True), None] for k in range(4)]                # drive B has ended
    act, _ = run(binding, model, drives, plan, mapping=True, snap_steps=set(range(6, 12)) | {4})
    refC = alone(binding, model, drives[C], range(6), mapping=True)
    for k in range(6):
        assert not diff(act[(0, 6 + k)], refC[k]), (k, diff(act[(0, 6 + k)], refC[k]))                            # the first frame too: no solve, cubes, cen, frame_count, map pose
    refB = alone(binding, model, drives[Bd], range(8), mapping=True)
    assert not diff(act[(1, 4)], refB[4])
    for k in range(2):
        assert not diff(act[(1, 6 + k)], refB[6 + k]), (k, diff(act[(1, 6 + k)], refB[6 + k]))


def test_reference_order_idle_and_reset(binding, sequence):
    drives, model = _drives(sequence, 3, 5, name="VLP-16")
    plan = [[(0, 0, True), (1, 0, True)], [None, (1, 1, True)], [(0, 1, True), (1, 2, True)], ("reset", [0]),
            [(2, 0, True), (1, 3, True)], [(2, 1, True), None], [(2, 2, True), (1, 4, True)]]
    act, _ = run(binding, model, drives, plan, mapping=True, ref_order=True)
    ref0 = alone(binding, model, drives[0], range(2), mapping=True, ref_order=True)
    ref1 = alone(binding, model, drives[1], range(5), mapping=True, ref_order=True)
    ref2 = alone(binding, model, drives[2], range(3), mapping=True, ref_order=True)
    for got, want in [(act[(0, 0)], ref0[0]), (act[(0, 2)], ref0[1])] + list(zip([act[(1, s)] for s in (0, 1, 2, 3, 5)], ref1)) + \
            list(zip([act[(0, s)] for s in (3, 4, 5)], ref2)):
        assert not diff(got, want), diff(got, want)


def test_argument_and_state_rules(binding, sequence):
    scans, R, t, model = sequence("VLP-16", 3, seed=5)
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=2, max_points=max(len(x) for x in scans) + 64)
    for bad in ([2], [-1], [0, 0]):
        with pytest.raises(binding.AloamError) as e:
            gpu.reset_sequences(bad)
        assert e.value.code == binding.E_ARG
    gpu.scan_register([scans[0], scans[0]])
    with pytest.raises(binding.AloamError) as e:                         # the registration is waiting for its odometry step
        gpu.set_active([True, False])
    assert e.value.code == binding.E_STATE
    gpu.odometry_step()
    gpu.scan_register([scans[1], scans[1]])
    gpu.odometry_step()
    before = [snap(binding, gpu, b, False) for b in (0, 1)]
    gpu.set_active([False, False])                                       # an all-idle step changes nothing
    gpu.scan_register([NAN_ROW, NAN_ROW])
    gpu.odometry_step()
    assert [snap(binding, gpu, b, False) for b in (0, 1)] == before
    gpu.set_active([False, True])                                        # an ACTIVE empty sweep still fails
    with pytest.raises(binding.AloamError) as e:
        gpu.scan_register([NAN_ROW, NAN_ROW])
    assert e.value.code == binding.E_EMPTY
    gpu.close()


def test_kitti_runner_batches_unequal_sequences_like_single_runs(tmp_path):
    seqs = ["00", "01", "02"]
    outs = {}
    for tag, extra in (("batched", ["--seqs", *seqs, "--batch", "2"]), ("single", None)):
        if extra is None:
            for s in seqs:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--dataset", str(tmp_path / "batched" / "selftest_dataset"),
                                    "--seq", s, "--mapping", "--out", str(tmp_path / "single")], capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stdout + r.stderr
        else:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--selftest", "--mapping", "--out", str(tmp_path / tag), *extra],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = tmp_path / tag
    lengths = set()
    for s in seqs:
        for kind in ("odometry", "mapped"):
            a = (outs["batched"] / f"{s}_{kind}.txt").read_bytes()
            assert a == (outs["single"] / f"{s}_{kind}.txt").read_bytes(), (s, kind)
        lengths.add(len(np.loadtxt(outs["batched"] / f"{s}_odometry.txt")))
    assert len(lengths) == 3                                             # the sequences are of unequal length
