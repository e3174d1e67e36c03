"""aloam_process_device / aloam_process_host build the search grids of a step beside the scan registration of the same call: the mask of the step
is staged before anything is queued, a persistent "last"-form build (k_build_grids_fused_last, then the per-grid launch) is forked onto the grid
stream behind k_front, runs beside k_ring_features and is joined in front of the first k_transform_queries.  Such a step builds nothing for the next
one, so no sequence leaves it with grid_built; aloam_scan_register* + aloam_odometry_step keep the build beside the association.  With
ALOAM_GRID_OVERLAP=0 every step builds serially on one stream.  All schedules run the same code on the same clouds: every pose, correspondence with
its query index, last cloud and cloud-order flag must agree bit for bit after every step."""
import numpy as np
import pytest
from test_gpu_parity import _mk
from test_grid_overlap import _assert_same, _both, _feeds, _snap_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sweeps(sequence):
    scans, R, t, model = sequence("HDL-64", 6, seed=31, columns=512)
    return scans, model


def _resident(feeds, floats=4, pinned=False):
    """feeds[k][b] -> one [B, T, NP, floats] buffer (device, or pinned host) and NP; sweep k of sequence b starts at element (b, k, 0, 0)."""
    import torch
    B, T, NP = len(feeds[0]), len(feeds), max(len(x) for xs in feeds for x in xs)
    host = np.zeros((B, T, NP, floats), np.float32)
    for k, xs in enumerate(feeds):
        for b, x in enumerate(xs):
            w = min(floats, x.shape[1])
            host[b, k, :len(x), :w] = x[:, :w]
    t = torch.from_numpy(host)
    return (t.pin_memory() if pinned else t.cuda()), NP


def _process(gpu, data, NP, feeds, k, floats=4, host=False):
    call = gpu.process_host if host else gpu.process_device
    call(data.data_ptr() + k * NP * floats * 4, len(feeds) * NP * floats * 4, [len(x) for x in feeds[k]], floats * 4)


@pytest.mark.parametrize("first", ["process", "separate"])
def test_hand_over_between_the_two_overlapped_schedules(binding, sweeps, monkeypatch, first):
    """Steps alternate between aloam_process_device and aloam_scan_register + aloam_odometry_step: a step of the first kind leaves no grids behind, so
    the separate step after it builds serially and builds the next ones beside its solve; the process step after that finds them built."""
    scans, model = sweeps
    feeds = _feeds(scans)
    data, NP = _resident(feeds)

    def run():
        gpu = _mk(binding, model, batch=2, max_points=NP + 64)
        rec = []
        for k, xs in enumerate(feeds):
            if (k % 2 == 0) == (first == "process"):
                _process(gpu, data, NP, feeds, k)
            else:
                gpu.scan_register(xs)
                gpu.odometry_step()
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 6
    _assert_same(a, b, "hand-over, first = " + first)
    assert all(len(s[q][1]) > 100 for s in a[1:] for q in range(2)), "no correspondences: the comparison would be empty"


def test_the_staged_mask_is_read_on_the_grid_stream(binding, sweeps, monkeypatch):
    """Batch 3: sequence 2 sits out steps 2 - 3 and resumes, sequence 1 is reset before step 4 - a first frame in the middle of a solving batch.
    The build reads who solves from the mask staged at the start of the call, in front of the fork."""
    scans, model = sweeps
    feeds = [[scans[k], scans[5 - k], scans[k]] for k in range(6)]
    data, NP = _resident(feeds)

    def run():
        gpu = _mk(binding, model, batch=3, max_points=NP + 64)
        rec = []
        for k in range(6):                                     # step k + 1
            gpu.set_active([1, 1, 0] if k in (1, 2) else None)
            if k == 3:
                gpu.reset_sequences([1])
            _process(gpu, data, NP, feeds, k)
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 6
    _assert_same(a, b, "masked")
    assert len(a[4][1][1]) > 100, "sequence 1: a first frame in step 4, a solve in step 5"
    assert len(a[3][2][1]) > 0 and all(len(a[k][2][1]) > 100 for k in (4, 5)), "sequence 2 solves again once it resumes"
    assert all(len(a[k][0][1]) > 100 for k in range(1, 6))


@pytest.mark.parametrize("mode", ["unsorted", "far"])
def test_injected_last_clouds_before_a_process_call(binding, sweeps, monkeypatch, mode):
    """aloam_set_last directly before aloam_process_device: the build beside the registration covers the injected clouds, flags them (not
    ring-sorted / coordinates out of range) and the association takes the matching kernel, as with the serial build."""
    scans, model = sweeps
    monkeypatch.setenv("ALOAM_GRID_OVERLAP", "0")
    cap = max(len(x) for x in scans) + 64
    src = _mk(binding, model, max_points=cap)
    src.scan_register(scans[1])
    feats = src.features()
    src.close()
    rng = np.random.default_rng(3)
    corner, surf = feats["less_sharp"].copy(), feats["less_flat"].copy()
    if mode == "unsorted":
        for c in (corner, surf):
            k = len(c) // 2
            c[:] = np.concatenate([c[k:], c[:k]])
    else:
        surf[rng.integers(len(surf))][:3] = (5000.0, 10.0, 1.0)
        corner[rng.integers(len(corner))][:3] = (-4200.0, 0.0, 0.0)
    para_q, para_t = np.array([0.0, 0.0, 0.01, 1.0]), np.array([0.95, 0.02, 0.0])
    para_q /= np.linalg.norm(para_q)
    feeds = [[scans[0]], [scans[2]], [scans[3]]]
    data, NP = _resident(feeds)

    def run():
        gpu = _mk(binding, model, max_points=cap)
        rec = []
        _process(gpu, data, NP, feeds, 0)                      # a first frame
        gpu.set_last(corner, surf)
        gpu.set_state(para_q, para_t, [0, 0, 0, 1.0], [0, 0, 0.0], inited=True)
        for k in (1, 2):                                       # the step that searches the injected clouds, then an ordinary one
            _process(gpu, data, NP, feeds, k)
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    _assert_same(a, b, mode)
    assert tuple(a[0][0][7]) == ((2, 2) if mode == "unsorted" else (-1, -1)), a[0][0][7]
    assert len(a[0][0][3]) > 100


@pytest.mark.parametrize("floats", [4, 3])
def test_process_host_runs_copy_build_and_registration_side_by_side(binding, sweeps, monkeypatch, floats):
    """aloam_process_host from pinned memory, records of 16 and of 12 bytes: the H2D copy on the copy stream, the build on the grid stream and the
    registration on the main stream."""
    scans, model = sweeps
    feeds = _feeds(scans)
    data, NP = _resident(feeds, floats, pinned=True)

    def run():
        gpu = _mk(binding, model, batch=2, max_points=NP + 64)
        rec = []
        for k in range(6):
            _process(gpu, data, NP, feeds, k, floats, host=True)
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 6
    _assert_same(a, b, "process_host, %d floats" % floats)
    assert all(len(s[q][1]) > 100 for s in a[1:] for q in range(2))


def test_per_grid_kernel_behind_the_persistent_build(binding, sweeps, monkeypatch):
    """max_points = 170000 gives the surf table 32768 buckets, beyond the fused kernels: the surf grids come from the k_build_grids launch that
    follows the persistent kernel on the grid stream."""
    scans, model = sweeps
    feeds = _feeds(scans)[:4]
    data, NP = _resident(feeds)

    def run():
        gpu = _mk(binding, model, batch=2, max_points=170000)
        rec = []
        for k in range(4):
            _process(gpu, data, NP, feeds, k)
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 4
    _assert_same(a, b, "per-grid kernel")
    assert any(len(s[0][3]) > 100 for s in a[1:])


def test_more_clouds_than_workgroups(binding, sequence, monkeypatch):
    """Batch 160: 320 clouds, more than the persistent build has workgroups, so the walk reaches its second round and the flipped class bit.
    Every sequence is compared with the serial build."""
    import torch
    scans, R, t, model = sequence("HDL-64", 3, seed=31, columns=256)
    B = 160
    two, NP = _resident([[scans[k], scans[2 - k]] for k in range(3)])
    data = two[torch.arange(B, device=two.device) % 2].contiguous()     # even sequences run forwards, odd ones backwards
    counts = [[len(scans[k]) if b % 2 == 0 else len(scans[2 - k]) for b in range(B)] for k in range(3)]

    def run():
        gpu = _mk(binding, model, batch=B, max_points=NP + 64)
        rec = []
        for k in range(3):
            gpu.process_device(data.data_ptr() + k * NP * 16, 3 * NP * 16, counts[k])
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        gpu.close()
        return rec

    a, b = _both(monkeypatch, run)
    assert len(a) == 3 and len(a[0]) == B
    _assert_same(a, b, "two rounds")
    assert all(len(a[2][q][1]) > 50 for q in range(B))


def test_profile_slot_counts_one_build_per_solving_step(binding, sweeps):
    """With the profile on, k_build_grids is the one build of a step, timed on the grid stream: three solving steps of four, and the same results."""
    scans, model = sweeps
    feeds = _feeds(scans)[:4]
    data, NP = _resident(feeds)

    def run(profiled):
        gpu = _mk(binding, model, batch=2, max_points=NP + 64)
        gpu.profile_enable(profiled)
        rec = []
        for k in range(4):
            _process(gpu, data, NP, feeds, k)
            gpu.synchronize()
            rec.append(_snap_all(binding, gpu))
        prof = gpu.profile() if profiled else None
        gpu.close()
        return rec, prof

    (a, prof), (b, _) = run(True), run(False)
    _assert_same(a, b, "profiled")
    assert prof["k_build_grids"]["launches"] == 3 and prof["k_build_grids"]["total_ms"] > 0, prof["k_build_grids"]
    assert prof["k_find_ends"]["launches"] == 4 and prof["k_advance"]["launches"] == 4
