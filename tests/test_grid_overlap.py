"""The search grids of the next odometry step are built beside the association and the solve of the current one (ALOAM_GRID_OVERLAP, default on:
two grid sets per sequence, one per cloud buffer; a grid stream forked from and joined into the context's stream inside aloam_odometry_step).
With ALOAM_GRID_OVERLAP=0 a context builds the grids of the last clouds at the start of every step, one chain on one stream.  Both schedules run the
same kernels on the same clouds, positions inside a bucket are never looked at in order and the association takes exact minima with index
tie-breaks, so every pose, correspondence, last cloud and cloud-order flag must agree bit for bit, after every step."""
import numpy as np
import pytest
from conftest import bits_equal
from test_gpu_parity import _mk

pytestmark = pytest.mark.gpu


def _snap(binding, gpu, b):
    p = gpu.pose(b)
    e, pl, eq, pq = gpu.correspondences(b)
    return (np.concatenate([p["q_w"], p["t_w"], p["q_lc"], p["t_lc"]]), e, eq, pl, pq, gpu.cloud(binding.CLOUD_SURF_LAST, b),
            gpu.cloud(binding.CLOUD_CORNER_LAST, b), np.array(gpu.last_cloud_order(b)))


def _snap_all(binding, gpu):
    return [_snap(binding, gpu, b) for b in range(gpu.batch)]


def _assert_same(run_a, run_b, what):
    assert len(run_a) == len(run_b) and len(run_a) > 0
    for step, (sa, sb) in enumerate(zip(run_a, run_b)):
        assert len(sa) == len(sb)
        for b, (a, c) in enumerate(zip(sa, sb)):
            for i, (x, y) in enumerate(zip(a, c)):
                assert bits_equal(x, y), (what, "step", step, "sequence", b, "array", i)


def _both(monkeypatch, run, overlap_env=None):
    """run() under ALOAM_GRID_OVERLAP=1 (plus overlap_env) and under =0: the two lists of per-step snapshots."""
    out = []
    for overlap in ("1", "0"):
        monkeypatch.setenv("ALOAM_GRID_OVERLAP", overlap)
        for k, v in (overlap_env or {}).items():
            monkeypatch.setenv(k, v) if overlap == "1" else monkeypatch.delenv(k, raising=False)
        out.append(run())
    return out


def _feeds(scans):
    """Two different sequences from one list of sweeps: forwards and backwards."""
    return [[scans[k], scans[len(scans) - 1 - k]] for k in range(len(scans))]


def _free_running(binding, model, feeds, max_points, orders=None):
    gpu = _mk(binding, model, batch=len(feeds[0]), max_points=max_points)
    rec = []
    for xs in feeds:
        gpu.scan_register(xs)
        gpu.odometry_step()
        rec.append(_snap_all(binding, gpu))
        if orders is not None:
            orders.append([gpu.last_cloud_order(b) for b in range(gpu.batch)])
    gpu.close()
    return rec


def test_free_running_matches_serial_build(binding, sequence, monkeypatch):
    """Six sweeps, batch 2: both cloud buffers and both grid sets of every sequence are used three times."""
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    cap = max(len(x) for x in scans) + 64
    a, b = _both(monkeypatch, lambda: _free_running(binding, model, _feeds(scans), cap))
    assert len(a) == 6
    _assert_same(a, b, "free running")
    assert any(len(s[0][1]) > 100 for s in a[1:]), "no correspondences: the comparison would be empty"


def test_process_device_entry_matches_serial_build(binding, sequence, monkeypatch):
    """The same sweeps resident on the device through aloam_process_device, the path the benchmark times."""
    import torch
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    feeds = _feeds(scans)
    T, NP = len(feeds), max(len(x) for x in scans)
    host = np.zeros((2, T, NP, 4), np.float32)
    for k, xs in enumerate(feeds):
        for b, x in enumerate(xs):
            w = min(4, x.shape[1])
            host[b, k, :len(x), :w] = x[:, :w]
    data = torch.from_numpy(host).cuda()

    def run():
        gpu = _mk(binding, model, batch=2, max_points=NP + 64)
        rec = []
        for k, xs in enumerate(feeds):
            gpu.process_device(data.data_ptr() + k * NP * 16, T * NP * 16, [len(x) for x in xs])
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    _assert_same(a, b, "process_device")
    assert any(len(s[0][1]) > 100 for s in a[1:])


def _order_of(cloud):
    """0 = ring keys ascending, 1 = no key more than 2 below an earlier one, 2 = anything else (aloam_get_last_cloud_order)."""
    key = cloud[:, 3].astype(np.int32)
    return 0 if not (np.diff(key) < 0).any() else (1 if (np.maximum.accumulate(key) - key).max() <= 2 else 2)


def test_nearly_sorted_clouds_through_the_next_build(binding, sequence, monkeypatch):
    """Sweeps whose first ray has no return leave nearly ring-sorted last clouds: the walk tables and the order flag come from the build that ran
    beside the previous step.  Both schedules must report, for every step, the order of the clouds that step searched, and order 1 for the surf
    cloud wherever its keys say so (the sweeps hold such clouds: at least two of the three searched ones)."""
    scans, R, t, model = sequence("HDL-64", 4, seed=7, columns=512)
    cut = [x[40:] for x in scans]
    cap = max(len(x) for x in scans) + 64
    reported, searched = [], []

    def run():
        gpu = _mk(binding, model, max_points=cap)
        rec = []
        for k, x in enumerate(cut):
            gpu.scan_register(x)
            if k > 0:
                searched.append((_order_of(gpu.cloud(binding.CLOUD_CORNER_LAST)), _order_of(gpu.cloud(binding.CLOUD_SURF_LAST))))
            gpu.odometry_step()
            rec.append(_snap_all(binding, gpu))
            if k > 0:
                reported.append(gpu.last_cloud_order())
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    _assert_same(a, b, "nearly sorted")
    assert len(reported) == 6 and reported == searched, (reported, searched)
    assert reported[:3] == reported[3:] and sum(1 for o in reported[:3] if o[1] == 1) >= 2, reported


@pytest.mark.parametrize("mode", ["unsorted", "far"])
def test_injected_last_clouds_take_the_serial_build(binding, sequence, monkeypatch, mode):
    """aloam_set_last replaces the last clouds: the grids built beside the previous step no longer describe them, so the step builds them
    first.  Clouds that are not ring-sorted / hold far coordinates, then one ordinary step that searches the grids built beside the injected one."""
    scans, R, t, model = sequence("HDL-64", 3, seed=8, columns=1024)
    monkeypatch.setenv("ALOAM_GRID_OVERLAP", "0")
    src = _mk(binding, model, max_points=70000)
    feats = []
    for x in scans:
        src.scan_register(x)
        feats.append(src.features())
        src.odometry_step()
    src.close()
    rng = np.random.default_rng(3)
    corner, surf = feats[1]["less_sharp"].copy(), feats[1]["less_flat"].copy()
    if mode == "unsorted":
        for c in (corner, surf):
            k = len(c) // 2
            c[:] = np.concatenate([c[k:], c[:k]])
    else:
        surf[rng.integers(len(surf))][:3] = (5000.0, 10.0, 1.0)
        corner[rng.integers(len(corner))][:3] = (-4200.0, 0.0, 0.0)
    para_q, para_t = np.array([0.0, 0.0, 0.01, 1.0]), np.array([0.95, 0.02, 0.0])
    para_q /= np.linalg.norm(para_q)

    def run():
        gpu = _mk(binding, model, max_points=70000)
        rec = []
        gpu.scan_register(scans[0])                            # a first frame: its "next" build leaves grids that set_last makes stale
        gpu.odometry_step()
        gpu.set_features(feats[2])
        gpu.set_last(corner, surf)
        gpu.set_state(para_q, para_t, [0, 0, 0, 1.0], [0, 0, 0.0], inited=True)
        gpu.odometry_step()
        rec.append(_snap_all(binding, gpu))
        gpu.scan_register(scans[1])
        gpu.odometry_step()
        rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    _assert_same(a, b, mode)
    assert tuple(a[0][0][7]) == ((2, 2) if mode == "unsorted" else (-1, -1)), a[0][0][7]
    assert len(a[0][0][3]) > 100


def test_invalidation_set_last_sit_out_and_reload(binding, sequence, monkeypatch):
    """Batch of 3 over 6 sweeps: sequence 1 gets another sweep's last clouds before step 3, sequence 2 sits out steps 2 and 3 and resumes, after
    step 4 all three are saved, reset and loaded, and two more steps run.  A stale or wrongly addressed grid set shows here."""
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    cap = max(len(x) for x in scans) + 64
    feeds = [[scans[k], scans[k], scans[5 - k]] for k in range(6)]

    def run():
        gpu = _mk(binding, model, batch=3, max_points=cap)
        rec = []
        for k, xs in enumerate(feeds):                         # step k + 1
            if k == 2:
                gpu.set_last(gpu.cloud(binding.CLOUD_CORNER_LAST, 2), gpu.cloud(binding.CLOUD_SURF_LAST, 2), seq=1)
            gpu.set_active([1, 1, 0] if k in (1, 2) else None)
            gpu.scan_register(xs)
            gpu.odometry_step()
            rec.append(_snap_all(binding, gpu))
            if k == 3:
                blob, off = gpu.save_sequences([0, 1, 2])
                gpu.reset_sequences([0, 1, 2])
                gpu.load_sequences([0, 1, 2], blob, off)
                gpu.synchronize()
                rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 7
    _assert_same(a, b, "invalidation")
    assert all(len(s[b][1]) > 50 for s in a[5:] for b in range(3))


def test_per_grid_kernel_matches_serial_build(binding, sequence, monkeypatch):
    """max_points = 170000 gives the surf table 32768 buckets, beyond the fused kernel: its grids go through k_build_grids in both forms."""
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    a, b = _both(monkeypatch, lambda: _free_running(binding, model, _feeds(scans)[:4], 170000))
    assert len(a) == 4
    _assert_same(a, b, "per-grid kernel")
    assert any(len(s[0][3]) > 100 for s in a[1:])


def test_graph_replay_takes_precedence_over_overlap(binding, sequence, monkeypatch):
    """A context that replays the step as a hipGraph keeps the serial chain whatever ALOAM_GRID_OVERLAP says."""
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    cap = max(len(x) for x in scans) + 64
    a, b = _both(monkeypatch, lambda: _free_running(binding, model, _feeds(scans), cap), overlap_env={"ALOAM_GRAPH_MAX_BATCH": "8"})
    _assert_same(a, b, "graph replay")
