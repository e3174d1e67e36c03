"""aloam_export_pose_information on the GPU against the numpy model (a-loam_amd/information.py) evaluated on the factor records and the pose
the getters return for the same state; status and lifecycle; the shape of the call; a corridor and an open world."""
import importlib

import numpy as np
import pytest

import information_cases as cases

info = importlib.import_module("a-loam_amd.information")

pytestmark = pytest.mark.gpu

COLUMNS = 512
MAX_POINTS = 16 * COLUMNS + 1024


def _ctx(binding, model, batch, mapping=True, **kw):
    g = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=batch, max_points=MAX_POINTS, device=0, **kw)
    if mapping:
        g.mapping_enable(0.2, 0.4, pool_points=65536)
    return g


def _rec_bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).tobytes()


def _check_against_model(rec, want, label):
    """The tolerances of the issue: |dH_ij| <= 1e-10 sqrt(H_ii H_jj) (each of <= 1e4 terms is bounded by Cauchy-Schwarz and carries a few ulp),
    |dg_i| <= 1e-10 sqrt(2 cost H_ii) (the same argument over the weighted residuals), cost 1e-12 relative."""
    H, Hm = rec["info"], want["info"]
    dia = np.sqrt(np.diag(Hm))
    dH = np.abs(H - Hm) / np.outer(dia, dia)
    dg = np.abs(rec["gradient"] - want["gradient"]) / np.sqrt(2.0 * want["cost"] * np.diag(Hm))
    dc = abs(rec["cost"] - want["cost"]) / want["cost"]
    print(f"{label}: factors {rec['n_line']} + {rec['n_plane']}, max |dH| / sqrt(HiiHjj) {dH.max():.3g}, max |dg| / sqrt(2 cost Hii) {dg.max():.3g}, cost rel {dc:.3g}")
    assert (int(rec["n_line"]), int(rec["n_plane"]), int(rec["rows"])) == (want["n_line"], want["n_plane"], want["rows"])
    assert dH.max() <= 1e-10 and dg.max() <= 1e-10 and dc <= 1e-12
    assert np.array_equal(H, H.T)


def _check_decomposition(rec, label):
    """Eigenpairs against the device's own matrix, marginals against decompose() of it."""
    H = rec["info"]
    lam, V = rec["eigenvalues"], rec["eigenvectors"]
    top = lam[5]
    res = np.linalg.norm(H @ V - V * lam, axis=0).max()
    dl = np.abs(lam - np.linalg.eigvalsh(H)).max()
    print(f"{label}: eigen residual / lambda_max {res / top:.3g}, eigenvalue difference / lambda_max {dl / top:.3g}, status {rec['status']}")
    assert np.all(np.diff(lam) >= 0) and res <= 1e-10 * top and dl <= 1e-10 * top
    assert np.abs(V.T @ V - np.eye(6)).max() <= 1e-12
    d = info.decompose(H)
    assert int(rec["status"]) == d["status"]
    for name in ("trans", "rot"):
        M, lam3, V3 = rec[name + "_info"], rec[name + "_eigenvalues"], rec[name + "_eigenvectors"]
        scale = d[name + "_eigenvalues"][2]
        assert np.abs(M - d[name + "_info"]).max() <= 1e-9 * scale, name
        assert np.abs(lam3 - d[name + "_eigenvalues"]).max() <= 1e-9 * scale, name
        assert np.linalg.norm(M @ V3 - V3 * lam3, axis=0).max() <= 1e-10 * scale, name
    for W in (V, rec["trans_eigenvectors"], rec["rot_eigenvectors"]):
        for k in range(W.shape[1]):
            assert W[int(np.argmax(np.abs(W[:, k]))), k] > 0                    # the sign rule


@pytest.fixture(scope="module")
def sweeps(sequence):
    a = sequence("VLP-16", 4, seed=4, columns=COLUMNS)
    b = sequence("VLP-16", 4, seed=9, columns=COLUMNS)
    return a[0], b[0], a[3]


def test_odometry_against_the_model(binding, sweeps):
    """Batch 3 (two seeds, and one sequence idle in the last step), 4 sweeps."""
    sa, sb, model = sweeps
    g = _ctx(binding, model, 3, mapping=False)
    before = None
    for k in range(4):
        if k == 3:
            before = g.export_pose_information(binding.INFO_ODOMETRY, [2])[0]
            g.set_active([1, 1, 0])
        g.scan_register([sa[k], sb[k], sa[k]])
        g.odometry_step()
    recs = g.export_pose_information(binding.INFO_ODOMETRY, [0, 1, 2])
    assert _rec_bytes(recs[2]) == _rec_bytes(before)                           # an idle step changes nothing
    for b in range(3):
        e, p, _, _ = g.correspondences(b)
        pose, st = g.pose(b), g.odom_stats(b)
        want = info.information_from_factors(e, p, pose["q_lc"], pose["t_lc"])
        assert int(recs[b]["status"]) == binding.INFO_OK and int(recs[b]["frame"]) == -1
        assert (int(recs[b]["n_line"]), int(recs[b]["n_plane"])) == (st["corner_corr"][1], st["plane_corr"][1])
        _check_against_model(recs[b], want, f"odometry seq {b}")
        _check_decomposition(recs[b], f"odometry seq {b}")
    assert _rec_bytes(recs[0]) != _rec_bytes(recs[2])                          # (one sweep apart)
    g.close()


def test_odometry_with_distortion_against_the_model(binding, sweeps):
    """distortion = 1, one 3-sweep sequence: s from the intensity of the query feature that edge_query / plane_query names."""
    sa, _, model = sweeps
    g = _ctx(binding, model, 1, mapping=False, distortion=True)
    for k in range(3):
        g.scan_register(sa[k])
        g.odometry_step()
    rec = g.export_pose_information(binding.INFO_ODOMETRY, [0])[0]
    e, p, eq, pq = g.correspondences(0)
    ratio = lambda w: (w - np.trunc(w).astype(np.float32)).astype(np.float64) / 0.1      # f32 difference, divided by the double 0.1
    s = (ratio(g.cloud(binding.CLOUD_SHARP, 0)[eq, 3]), ratio(g.cloud(binding.CLOUD_FLAT, 0)[pq, 3]))
    assert s[0].min() >= -0.1 and s[0].max() <= 1.1 and np.ptp(s[1]) > 0.5
    pose = g.pose(0)
    want = info.information_from_factors(e, p, pose["q_lc"], pose["t_lc"], s)
    assert int(rec["status"]) == binding.INFO_OK
    _check_against_model(rec, want, "odometry with distortion")
    _check_decomposition(rec, "odometry with distortion")
    g.close()


def test_mapping_against_the_model(binding, sweeps):
    """Batch 3 (one normal, one frozen after its second step, one idle in the last step), 3 mapping steps."""
    sa, sb, model = sweeps
    g = _ctx(binding, model, 3)
    before = None
    for k in range(3):
        if k == 2:
            before = g.export_pose_information(binding.INFO_MAPPING, [2])[0]
            g.set_map_frozen([0, 1, 0])
            g.set_active([1, 1, 0])
        g.scan_register([sa[k], sb[k], sa[k]])
        g.odometry_step()
        g.mapping_step()
    recs = g.export_pose_information(binding.INFO_MAPPING, [0, 1, 2])
    assert _rec_bytes(recs[2]) == _rec_bytes(before)                           # an idle step changes nothing
    for b in range(3):
        lines, planes = g.map_factors(b)
        mp, mi = g.map_pose(b), g.map_info(b)
        assert (len(lines), len(planes)) == (mi["corner_num1"], mi["surf_num1"])
        assert (int(recs[b]["n_line"]), int(recs[b]["n_plane"])) == (mi["corner_num1"], mi["surf_num1"]) and int(recs[b]["frame"]) == mi["frame_count"]
        assert mi["corner_num1"] > 20 and mi["surf_num1"] > 200
        want = info.information_from_factors(lines, planes, mp["q_w"], mp["t_w"])
        assert int(recs[b]["status"]) == binding.INFO_OK
        _check_against_model(recs[b], want, f"mapping seq {b}")
        _check_decomposition(recs[b], f"mapping seq {b}")
    assert g.map_info(1)["frame_count"] == 3 and g.map_info(2)["frame_count"] == 2
    g.close()


def _status(g, which, seqs):
    return [int(v) for v in g.export_pose_information(which, seqs)["status"]]


def test_status_and_lifecycle(binding, sweeps):
    sa, sb, model = sweeps
    B = binding
    g = _ctx(binding, model, 2)
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_NONE] * 2 and _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_NONE] * 2
    rec = g.export_pose_information(B.INFO_MAPPING, [1])[0]
    assert not rec["info"].any() and rec["cost"] == 0 and int(rec["rows"]) == 0 and int(rec["frame"]) == 0

    def frame(k, mapping=True):
        g.scan_register([sa[k], sb[k]])
        g.odometry_step()
        if mapping:
            g.mapping_step()

    frame(0)
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_NONE] * 2                    # a first frame solves nothing
    rec = g.export_pose_information(B.INFO_MAPPING, [0, 1])
    assert [int(v) for v in rec["status"]] == [B.INFO_NO_FACTORS] * 2                  # an empty map: the gate is false
    assert not rec["info"].any() and [int(v) for v in rec["frame"]] == [1, 1] and g.map_factors(0)[0].shape == (0, 9)
    frame(1)
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_OK] * 2 and _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_OK] * 2
    g.scan_register([sa[2], sb[2]])
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_NONE] * 2                    # the new sweep's counts, the old sweep's records
    assert _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_OK] * 2
    g.odometry_step()
    g.mapping_step()
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_OK] * 2
    # each of these leaves NONE until the next step
    g.reset_sequences([0])
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_NONE, B.INFO_OK] and _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_NONE, B.INFO_OK]
    mp = g.map_pose(1)
    g.set_map_frame([10, 10, 5], mp["q_wmap_wodom"], mp["t_wmap_wodom"], 3, seq=1)
    assert _status(g, B.INFO_MAPPING, [1]) == [B.INFO_NONE] and _status(g, B.INFO_ODOMETRY, [1]) == [B.INFO_OK]
    frame(3)
    assert _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_NO_FACTORS, B.INFO_OK] and _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_NONE, B.INFO_OK]
    g.apply_map_corrections([1], B.map_corrections([mp["q_wmap_wodom"]], [mp["t_wmap_wodom"]]), [0])
    assert _status(g, B.INFO_MAPPING, [0, 1]) == [B.INFO_NO_FACTORS, B.INFO_NONE]
    blob, off = g.save_sequences([1])
    g.load_sequences([1], blob, off)
    assert _status(g, B.INFO_MAPPING, [1]) == [B.INFO_NONE] and _status(g, B.INFO_ODOMETRY, [1]) == [B.INFO_NONE]
    g.scan_register([sa[2], sb[2]])
    g.odometry_step()
    g.mapping_step()
    assert _status(g, B.INFO_ODOMETRY, [0, 1]) == [B.INFO_OK] * 2 and _status(g, B.INFO_MAPPING, [1]) == [B.INFO_OK]
    g.close()


def test_call_shape(binding, sweeps):
    import torch
    sa, sb, model = sweeps
    B = binding
    size = B.POSE_INFORMATION_DTYPE.itemsize
    g = _ctx(binding, model, 3)
    for k in range(2):
        g.scan_register([sa[k], sb[k], sa[k + 1]])
        g.odometry_step()
        g.mapping_step()
    for which in (B.INFO_ODOMETRY, B.INFO_MAPPING):
        alone = _rec_bytes(g.export_pose_information(which, [1])[0])
        assert _rec_bytes(g.export_pose_information(which, [1, 0, 2])[0]) == alone
        assert _rec_bytes(g.export_pose_information(which, [2, 0, 1])[2]) == alone
        assert _rec_bytes(g.export_pose_information(which, [0, 1], pinned=False)[1]) == alone
        assert len(g.export_pose_information(which, [])) == 0                        # n = 0 is legal
    # a step queued after the call, before the synchronise, does not change what it wrote
    want = _rec_bytes(g.export_pose_information(B.INFO_ODOMETRY, [0, 1, 2]))
    dst = torch.zeros(3 * size, dtype=torch.uint8).pin_memory()
    g.export_pose_information_into(B.INFO_ODOMETRY, [0, 1, 2], dst.data_ptr())
    g.scan_register([sa[2], sb[2], sa[3]])
    g.odometry_step()
    g.synchronize()
    assert dst.numpy().tobytes() == want
    assert _rec_bytes(g.export_pose_information(B.INFO_ODOMETRY, [0, 1, 2])) != want
    # refused calls write nothing
    dst.fill_(0xAB)
    pageable = np.zeros(3 * size, np.uint8)
    for call in (lambda: g.export_pose_information_into(B.INFO_ODOMETRY, [0], pageable.ctypes.data),
                 lambda: g.export_pose_information_into(B.INFO_ODOMETRY, [0], 0),
                 lambda: g.export_pose_information_into(B.INFO_ODOMETRY, [0, 0], dst.data_ptr()),
                 lambda: g.export_pose_information_into(B.INFO_ODOMETRY, [0, 3], dst.data_ptr()),
                 lambda: g.export_pose_information_into(2, [0], dst.data_ptr())):
        with pytest.raises(B.AloamError) as e:
            call()
        assert e.value.code == B.E_ARG
    g.synchronize()
    assert bool((dst == 0xAB).all()) and not pageable.any()
    g.close()
    g = _ctx(binding, model, 1, mapping=False)
    with pytest.raises(B.AloamError) as e:
        g.export_pose_information_into(B.INFO_MAPPING, [0], dst.data_ptr())
    assert e.value.code == B.E_STATE
    g.close()
    g = _ctx(binding, model, 1, mapping=False, stages=B.STAGE_REGISTRATION)
    with pytest.raises(B.AloamError) as e:
        g.export_pose_information_into(B.INFO_ODOMETRY, [0], dst.data_ptr())
    assert e.value.code == B.E_STATE
    g.close()


def test_a_corridor_shows_in_the_mapping_record(binding):
    """The corridor and the open world of the model test, 3 sweeps 0.5 m apart with mapping steps; the third step's mapping record.  The
    model on the device's own factors is the reference and has to satisfy the thresholds too.  Nothing is asserted about the odometry."""
    cs, _, _, axis, model = cases.corridor_scans(3, 0.01, columns=COLUMNS)
    os_, _, _, _ = cases.open_scans(3, 0.01, columns=COLUMNS)
    g = _ctx(binding, model, 2)
    for k in range(3):
        g.scan_register([cs[k].numpy(), os_[k].numpy()])
        g.odometry_step()
        g.mapping_step()
    recs = g.export_pose_information(binding.INFO_MAPPING, [0, 1])
    out = []
    for b in range(2):
        lines, planes = g.map_factors(b)
        mp = g.map_pose(b)
        want = info.information_from_factors(lines, planes, mp["q_w"], mp["t_w"])
        want.update(info.decompose(want["info"]))
        assert int(recs[b]["status"]) == binding.INFO_OK and int(recs[b]["frame"]) == 3
        out.append((info.degeneracy(recs[b]), info.degeneracy(want)))
        print("corridor" if b == 0 else "open", "factors", len(lines), len(planes), "trans eigenvalues", recs[b]["trans_eigenvalues"],
              "device ratio", out[b][0][0], "model ratio", out[b][1][0], "map t", mp["t_w"])
    for ratio, direction in out[0]:
        print("corridor |cos|", abs(direction @ axis))
        assert abs(direction @ axis) >= cases.AXIS_COS_MIN and ratio <= cases.CORRIDOR_RATIO_MAX
    for ratio, _ in out[1]:
        assert ratio >= cases.OPEN_RATIO_MIN
    g.close()
