"""Localization against a frozen prior map on the MI355X (aloam_set_map_frozen): a frozen sequence's mapping step computes the pose of a
normal step and leaves its map untouched (moved only by the window shifts); its submap grid is kept while the submap is unchanged and gives
the results of a rebuilt one; the grid is rebuilt after every event that replaces the map, the frame or the pools; mixed batches, pool
sizing, records and the reference summation order; a second pass over a mapped drive, several pose guesses of one map, and the KITTI runner."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_checkpoint import full, last_sizes, make
from test_gpu_sequence_lifecycle import NAN_ROW, _drives, diff, snap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mp(drives):
    return max(len(x) for d in drives for x in d) + 64


def frame(gpu, scans, map_mask=None, frozen=None):
    """One frame: registration + odometry of the slots with a sweep (None = idle), then the mapping step with map_mask (default: the same
    slots) and the frozen mask `frozen` (None = none)."""
    gpu.set_active([s is not None for s in scans])
    gpu.scan_register([s if s is not None else NAN_ROW for s in scans], check=False)
    gpu.odometry_step()
    gpu.set_active(map_mask if map_mask is not None else [s is not None for s in scans])
    gpu.set_map_frozen(frozen)
    gpu.mapping_step()


def cubes(gpu, b):
    return [gpu.map_cubes(cls, b) for cls in (0, 1)]


def same_cubes(a, b):
    return all(set(a[c]) == set(b[c]) and all(np.array_equal(a[c][i].view(np.uint32), b[c][i].view(np.uint32)) for i in a[c]) for c in (0, 1))


def pose_part(binding, gpu, b):
    """What a frozen step must compute exactly as a normal one: pose, statistics (the compaction count apart: it belongs to the insert) and
    the registered cloud."""
    info = gpu.map_info(b)
    info.pop("compactions")
    return {"map_pose": _sha(np.concatenate(list(gpu.map_pose(b).values()))), "map_info": repr(info),
            "registered": _sha(gpu.map_cloud(binding.MAP_REGISTERED, b))}


def world_cube(gpu, b):
    """The 50 m cube the refined pose lies in, in map coordinates (int((t + 25) / 50) per axis, rounded down)."""
    t = gpu.map_pose(b)["t_w"]
    return tuple(int(math.floor((v + 25.0) / 50.0)) for v in t)


def test_frozen_step_computes_the_pose_of_a_normal_step_and_keeps_the_map(binding, sequence):
    F, G = 4, 3
    drives, model = _drives(sequence, 1, F + G)
    gpu = make(binding, model, 2, _mp(drives), True)
    for k in range(F + G):
        before = cubes(gpu, 0), cubes(gpu, 1), gpu.map_info(0)["compactions"]
        frame(gpu, [drives[0][k]] * 2, frozen=[k >= F, False])
        gpu.synchronize()
        if k <= F:                                                        # (after frame F the maps differ: the twin has inserted frame F)
            a, b = pose_part(binding, gpu, 0), pose_part(binding, gpu, 1)
            assert not diff(a, b), (k, diff(a, b))                        # the same pose, statistics and registered cloud as the growing twin
        if k >= F:
            assert same_cubes(cubes(gpu, 0), before[0]), k                 # every cube: the same points, order and bits
            assert gpu.map_info(0)["compactions"] == before[2]
            grown = cubes(gpu, 1)
            assert sum(len(p) for c in grown for p in c.values()) != sum(len(p) for c in before[1] for p in c.values()), k
    # the surround / full-map clouds show the unchanged map
    full_map = gpu.map_cloud(binding.MAP_FULL, 0)
    assert len(full_map) == sum(len(p) for c in cubes(gpu, 0) for p in c.values())
    gpu.close()


@pytest.mark.parametrize("cen,roll", [((2, 10, 5), (1, 0, 0)), ((10, 18, 8), (0, -1, -1))])
def test_window_shift_of_a_frozen_map_is_a_pure_permutation(binding, sequence, cen, roll):
    F = 4
    drives, model = _drives(sequence, 1, F + 1)
    gpu = make(binding, model, 1, _mp(drives), True)
    for k in range(F):
        frame(gpu, [drives[0][k]])
    p = gpu.map_pose(0)
    gpu.set_map_frame(cen, p["q_wmap_wodom"], p["t_wmap_wodom"], gpu.map_info(0)["frame_count"])   # the next step's centre cube is at the edge
    gpu.synchronize()
    before = cubes(gpu, 0)
    frame(gpu, [drives[0][F]], frozen=[True])
    gpu.synchronize()
    after = cubes(gpu, 0)
    info = gpu.map_info(0)
    assert (info["cenW"], info["cenH"], info["cenD"]) == tuple(c + r for c, r in zip(cen, roll))
    dims = (21, 21, 11)
    for cls in (0, 1):
        want = {}
        for idx, pts in before[cls].items():
            ijk = [idx % 21, (idx // 21) % 21, idx // 441]
            ijk = [x + r for x, r in zip(ijk, roll)]
            # the slab that falls off re-enters emptied at the other end
            if all(0 <= x < n for x, n in zip(ijk, dims)) and not any((r > 0 and x == 0) or (r < 0 and x == n - 1) for x, r, n in zip(ijk, roll, dims)):
                want[ijk[0] + 21 * ijk[1] + 441 * ijk[2]] = pts
        assert set(after[cls]) == set(want), cls
        for idx in want:
            assert np.array_equal(after[cls][idx].view(np.uint32), want[idx].view(np.uint32)), (cls, idx)
    gpu.close()


def test_reused_grid_equals_a_rebuilt_grid(binding, sequence):
    F0, F = 8, 22                                                         # normal steps, then frozen steps past the 25 m cube boundary
    scans, R, t, model = sequence("HDL-64", F, seed=41, columns=512, travel=True, step=2.0)
    gpu = make(binding, model, 2, max(len(s) for s in scans) + 64, True)
    for k in range(F0):
        frame(gpu, [scans[k], None])
    gpu.synchronize()
    cube_seen, reused, rebuilt = world_cube(gpu, 0), 0, 0
    for k in range(F0, F):
        blob, off = gpu.save_sequences([0])
        gpu.load_sequences([1], blob, off)                                # slot B: the same sequence, its grid invalidated by the load
        frame(gpu, [scans[k], scans[k]], frozen=[True, True])
        gpu.synchronize()
        a, b = pose_part(binding, gpu, 0), pose_part(binding, gpu, 1)
        assert not diff(a, b), (k, diff(a, b))
        assert same_cubes(cubes(gpu, 0), cubes(gpu, 1)), k
        c = world_cube(gpu, 0)
        reused += c == cube_seen
        rebuilt += c != cube_seen
        cube_seen = c
    assert reused >= 3 and rebuilt >= 1, (reused, rebuilt)                # both kinds of frame were compared
    gpu.close()


def _map_of(binding, model, drive, frames):
    g = make(binding, model, 1, max(len(s) for s in drive) + 64, True)
    for k in range(frames):
        frame(g, [drive[k]])
    g.synchronize()
    m = cubes(g, 0)
    g.close()
    return m


def test_frozen_steps_skip_the_grid_build(binding, sequence):
    """The grid of an unchanged submap is kept: the map_grid stage of a frozen step is a fraction of one that rebuilds (every slot's grid
    invalidated by aloam_set_map_frame with the values it already holds)."""
    F, B = 8, 16
    drives, model = _drives(sequence, 1, F, cols=2048)                   # full-resolution sweeps: a submap whose build is well above a launch
    m = _map_of(binding, model, drives[0], F)
    gpu = make(binding, model, B, _mp(drives), True)
    for b in range(B):
        for cls in (0, 1):
            gpu.set_map(m[cls], cls, seq=b)
    grid, window = {}, {}
    for k in range(F):
        if k % 2 == 0:
            for b in range(B):
                p, i = gpu.map_pose(b), gpu.map_info(b)
                gpu.set_map_frame((i["cenW"], i["cenH"], i["cenD"]), p["q_wmap_wodom"], p["t_wmap_wodom"], i["frame_count"], seq=b)
        gpu.profile_enable(True)
        frame(gpu, [drives[0][k]] * B, frozen=[True] * B)
        grid[k] = gpu.profile()["map_grid"]["total_ms"]
        gpu.profile_enable(False)
        window[k] = world_cube(gpu, 0)
    kept = [grid[k] for k in range(1, F, 2) if window[k] == window[k - 1]]     # (a frame that enters another 50 m cube rebuilds)
    built = [grid[k] for k in range(0, F, 2)]
    print("map_grid ms per step: kept", [round(x, 4) for x in kept], "rebuilt", [round(x, 4) for x in built])
    assert len(kept) >= 2 and np.median(kept) < 0.5 * np.median(built), (kept, built)   # measured: 6 - 8 us against 33 us
    gpu.close()


def test_invalidation_events_rebuild_the_grid(binding, sequence):
    F = 12
    drives, model = _drives(sequence, 1, F)
    d = drives[0]
    mp = _mp(drives)
    m1 = _map_of(binding, model, d, 6)
    # the same cubes with the same populations, every point moved: the (off, cnt) signature cannot tell the two maps apart, only the
    # invalidation by aloam_set_map / by the reset inside aloam_load_sequences can
    moved = [{c: p + np.array([0.15, -0.1, 0.05, 0.0], np.float32) for c, p in m1[cls].items()} for cls in (0, 1)]
    X = make(binding, model, 2, mp, True, pool=1 << 15)
    for cls in (0, 1):
        X.set_map(m1[cls], cls, seq=0)
    # set_map_frame: an unchanged window would keep an exact grid, a moved one changes the signature; the step is compared all the same
    events = {3: "set_map", 5: "set_map_frame", 7: "pool_growth", 9: "load"}
    start = 0
    for k in range(F):
        ev = events.get(k)
        if ev == "set_map":
            for cls in (0, 1):
                X.set_map(moved[cls], cls, seq=0)
        elif ev == "set_map_frame":
            p = X.map_pose(0)
            X.set_map_frame((10, 10, 5), p["q_wmap_wodom"], p["t_wmap_wodom"] + np.array([0.05, -0.03, 0.0]), X.map_info(0)["frame_count"])
        elif ev == "pool_growth":
            g0 = X.map_pool_info()["growths"]
            X.set_map({0: np.zeros((X.map_pool_info()["pool_points"] + 1, 4), np.float32)}, 0, seq=1)
            assert X.map_pool_info()["growths"] > g0
        elif ev == "load":                                                # a record of the same cube layout (m1 in slot 1): a fresh sequence
            for cls in (0, 1):
                X.set_map(m1[cls], cls, seq=1)
            blob, off = X.save_sequences([1])
            X.load_sequences([0], blob, off)
            start = k
        if ev:
            X.synchronize()
            inj, p, info = cubes(X, 0), X.map_pose(0), X.map_info(0)
        frame(X, [d[k], None], frozen=[True, False])
        if not ev:
            continue
        X.synchronize()
        got = snap(binding, X, 0, True)
        # a fresh context: the same sweeps from the same start, idle in mapping until the injected map and frame, then one frozen step
        Y = make(binding, model, 1, mp, True)
        for j in range(start, k):
            frame(Y, [d[j]], map_mask=[False])
        for cls in (0, 1):
            Y.set_map(inj[cls], cls)
        Y.set_map_frame((info["cenW"], info["cenH"], info["cenD"]), p["q_wmap_wodom"], p["t_wmap_wodom"], info["frame_count"])
        frame(Y, [d[k]], frozen=[True])
        Y.synchronize()
        want = snap(binding, Y, 0, True)
        Y.close()
        assert not diff(got, want), (ev, diff(got, want))
    X.close()


def test_mixed_batch_and_asynchronous_mask_changes(binding, sequence):
    F = 7
    drives, model = _drives(sequence, 3, F)
    mp = _mp(drives)

    def run(frozen_plan, idle_plan, sync):
        g = make(binding, model, 3, mp, True)
        out = {}
        for k in range(F):
            scans = [drives[b][k] for b in range(3)]
            frame(g, scans, map_mask=[b not in idle_plan.get(k, ()) for b in range(3)], frozen=frozen_plan(k))
            if sync:
                g.synchronize()
                out[k] = [snap(binding, g, b, True) for b in range(3)]
        g.synchronize()
        out["end"] = [snap(binding, g, b, True) for b in range(3)]
        g.close()
        return out

    plain = run(lambda k: None, {}, True)
    mixed = run(lambda k: [False, True, False], {4: (1,)}, True)
    for k in range(F):
        for b in (0, 2):
            assert not diff(mixed[k][b], plain[k][b]), (k, b, diff(mixed[k][b], plain[k][b]))
    m3 = mixed[3][1]
    idle = {k: v for k, v in mixed[4][1].items() if k in ("map_pose", "map_info", "cubes")}
    assert not diff(idle, {k: m3[k] for k in idle}), diff(idle, {k: m3[k] for k in idle})   # an idle frozen slot is untouched
    plan = lambda k: [False, k % 2 == 1, k >= 3]
    a, s = run(plan, {}, False), run(plan, {}, True)
    for b in range(3):
        assert not diff(a["end"][b], s["end"][b]), (b, diff(a["end"][b], s["end"][b]))


def test_all_frozen_steps_never_size_the_pools(binding, sequence):
    F = 22
    drives, model = _drives(sequence, 2, F)
    mp = _mp(drives)
    m = _map_of(binding, model, drives[0], 2)
    gpu = make(binding, model, 2, mp, True, pool=4096)
    for b in range(2):
        for cls in (0, 1):
            gpu.set_map(m[cls], cls, seq=b)
    g0 = gpu.map_pool_info()["growths"]
    for k in range(F):
        frame(gpu, [drives[0][k], drives[1][k]], frozen=[True, True])
    gpu.synchronize()                                                     # no ALOAM_E_CAPACITY (raises)
    assert gpu.map_pool_info()["growths"] == g0
    assert same_cubes(cubes(gpu, 0), m) and same_cubes(cubes(gpu, 1), m)
    gpu.close()


# Measured on the MI355X: over this 30-frame drive the second pass stays within 5.1 cm of ground truth (mean 3.1 cm).
SECOND_PASS_BOUND_M = 0.08


def test_second_pass_localizes_in_the_first_pass_map(binding, sequence):
    F = 30
    scans, R, t, model = sequence("HDL-64", F, seed=43, columns=512)
    mp = max(len(s) for s in scans) + 64
    A = make(binding, model, 1, mp, True)
    for k in range(F):
        frame(A, [scans[k]])
    A.synchronize()
    m, info = cubes(A, 0), A.map_info(0)
    A.close()
    B = make(binding, model, 1, mp, True)
    for cls in (0, 1):
        B.set_map(m[cls], cls)
    B.set_map_frame((info["cenW"], info["cenH"], info["cenD"]), (0, 0, 0, 1), (0, 0, 0), 0)
    err = []
    for k in range(F):
        frame(B, [scans[k]], frozen=[True])
        B.synchronize()
        gt = R[0].T @ (t[k] - t[0])
        err.append(float(np.linalg.norm(B.map_pose(0)["t_w"] - gt)))
    assert same_cubes(cubes(B, 0), m)
    print(f"second pass: max |t - gt| = {max(err):.4f} m, mean {np.mean(err):.4f} m over {F} frames")
    assert max(err) < SECOND_PASS_BOUND_M, err
    B.close()


def _quat_of(Rm):
    w = math.sqrt(max(0.0, 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])) / 2.0
    return np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w), w])


def _qmul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def _qrot(q, v):
    return _qmul(_qmul(q, np.array([*v, 0.0])), q * np.array([-1, -1, -1, 1]))[:3]


# (dx, dy, dyaw in degrees) of the map <- odometry guess around the true correction, one per slot: the +-3 m / +-10 deg spread.  Measured
# on the MI355X: after five frozen frames the guesses within 1 m and 2.5 deg of the truth converge to within 5 cm and 0.5 deg,
# the others do not (and score fewer factors).
BASIN_M, BASIN_DEG = 1.0, 2.5
GUESSES = [(0, 0, 0), (0.5, 0, 0), (0, -0.5, 0), (1, 0, 0), (0, 1, 0), (-1, -1, 0), (2, 0, 0), (0, -2, 0), (3, 0, 0), (-3, 3, 0),
           (0, 0, 2.5), (0, 0, -5), (0, 0, 10), (0.5, 0.5, 2.5), (1, -1, -5), (3, -3, 10)]


def test_multi_hypothesis_best_score_is_the_truth(binding, sequence):
    F, G = 12, 5
    scans, R, t, model = sequence("HDL-64", F + G, seed=44, columns=512)
    mp = max(len(s) for s in scans) + 64
    A = make(binding, model, 1, mp, True)
    for k in range(F):
        frame(A, [scans[k]])
    blob, off = A.save_sequences([0])
    truth = A.map_pose(0)
    A.close()
    K = len(GUESSES)
    B = make(binding, model, K, mp, True)
    B.load_sequences(list(range(K)), np.concatenate([blob] * K), np.concatenate([[0], np.cumsum([off[1] - off[0]] * K)]).astype(np.int64))
    B.set_active([True] * K)
    B.scan_register([scans[F]] * K)                                       # the odometry step every loaded slot takes before it maps
    B.odometry_step()
    info = B.map_info(0)
    for s, (dx, dy, dyaw) in enumerate(GUESSES):
        dq = np.array([0.0, 0.0, math.sin(math.radians(dyaw) / 2), math.cos(math.radians(dyaw) / 2)])
        q = _qmul(dq, truth["q_wmap_wodom"])
        c = truth["t_w"]                                                  # the guess turns about the sensor, then moves it
        tt = _qrot(dq, truth["t_wmap_wodom"] - c) + c + np.array([dx, dy, 0.0])
        B.set_map_frame((info["cenW"], info["cenH"], info["cenD"]), q, tt, info["frame_count"], seq=s)
    B.set_map_frozen([True] * K)
    B.mapping_step()
    for k in range(F + 1, F + G):
        B.scan_register([scans[k]] * K)
        B.odometry_step()
        B.mapping_step()
    B.synchronize()
    k = F + G - 1
    gt_t, gt_q = R[0].T @ (t[k] - t[0]), _quat_of(R[0].T @ R[k])
    score, err = [], []
    for s in range(K):
        i = B.map_info(s)
        score.append(i["corner_num1"] + i["surf_num1"])
        p = B.map_pose(s)
        ang = 2 * math.degrees(math.acos(min(1.0, abs(float(np.dot(p["q_w"], gt_q))))))
        err.append((float(np.linalg.norm(p["t_w"] - gt_t)), ang))
    best = int(np.argmax(score))
    converged = [GUESSES[s] for s in range(K) if err[s][0] < 0.05 and err[s][1] < 0.5]
    print("multi-hypothesis: scores", score, "errors", [(round(a, 3), round(b, 2)) for a, b in err], "converged", converged)
    assert err[best][0] < 0.05 and err[best][1] < 0.5, (best, err[best], score)
    inside = [g for g in GUESSES if math.hypot(g[0], g[1]) <= BASIN_M and abs(g[2]) <= BASIN_DEG]
    assert set(inside) <= set(converged), (inside, converged)
    B.close()


def test_record_of_a_frozen_slot_continues_unfrozen(binding, sequence):
    F, G = 5, 4
    drives, model = _drives(sequence, 1, F + G)
    d = drives[0]
    gpu = make(binding, model, 2, _mp(drives), True)
    for k in range(F):
        frame(gpu, [d[k], None], frozen=[k >= 2, False])
    blob, off = gpu.save_sequences([0])
    gpu.load_sequences([1], blob, off)
    gpu.set_map_frozen(None)                                              # the source continues unfrozen, and so does the loaded slot
    for k in range(F, F + G):
        prev = [last_sizes(binding, gpu, b) for b in range(2)]
        frame(gpu, [d[k], d[k]])
        gpu.synchronize()
        a, b = full(binding, gpu, 0, True, prev[0]), full(binding, gpu, 1, True, prev[1])
        assert not diff(a, b), (k, diff(a, b))
    # the mask survives a load
    gpu.set_map_frozen([False, True])
    blob, off = gpu.save_sequences([0])
    gpu.load_sequences([1], blob, off)
    gpu.set_active([True, True])
    gpu.scan_register([d[F + G - 1]] * 2)
    gpu.odometry_step()
    gpu.synchronize()
    before = cubes(gpu, 1)
    gpu.mapping_step()                                                    # no set_map_frozen since the load
    gpu.synchronize()
    assert same_cubes(cubes(gpu, 1), before)
    gpu.close()


def test_reference_order_frozen_map_is_untouched(binding, sequence):
    F = 4
    drives, model = _drives(sequence, 1, F + 2)
    gpu = make(binding, model, 2, _mp(drives), True, ref_order=True)
    for k in range(F + 2):
        before = cubes(gpu, 0)
        frame(gpu, [drives[0][k]] * 2, frozen=[k >= F, False])
        gpu.synchronize()
        if k <= F:
            a, b = pose_part(binding, gpu, 0), pose_part(binding, gpu, 1)
            assert not diff(a, b), (k, diff(a, b))
        if k >= F:
            assert same_cubes(cubes(gpu, 0), before), k
    gpu.close()


def test_kitti_runner_localizes_against_a_saved_map(tmp_path):
    m = tmp_path / "m.npz"

    def run(out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--selftest", "--out", str(tmp_path / out), *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    run("map", "--mapping", "--save-map", str(m))
    digest = _sha(np.frombuffer(m.read_bytes(), np.uint8))
    mapped = np.loadtxt(tmp_path / "map" / "00_mapped.txt")
    for out, extra in (("loc", []), ("loc_offset", ["--initial-pose", "0.4", "-0.3", "0", "0.02"])):
        stdout = run(out, "--prior-map", str(m), *extra)
        loc, odo = np.loadtxt(tmp_path / out / "00_localized.txt"), np.loadtxt(tmp_path / out / "00_odometry.txt")
        assert loc.shape == odo.shape == mapped.shape
        assert "00 localized:" in stdout and "ATE" in stdout, stdout
        line = next(x for x in stdout.splitlines() if "factors per sweep" in x)
        assert int(line.split(" min ")[1].split(",")[0]) > 50, line               # every sweep was fitted to the map
        # the map was used: not the odometry pushed through the guess, but the poses of the mapping run
        assert np.abs(loc[:, 1:4] - odo[:, 1:4]).max() > 0, out
        err = np.linalg.norm(loc[:, 1:4] - mapped[:, 1:4], axis=1)
        assert err[-1] < 0.1 and (extra or err.max() < 0.1), (out, err)         # the offset guess (0.5 m off) is pulled onto the map
        assert _sha(np.frombuffer(m.read_bytes(), np.uint8)) == digest
