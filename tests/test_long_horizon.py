"""Long horizon on a travelling sensor: hundreds of free-running sweeps of registration -> odometry -> mapping.

The short fixtures hold 3 - 6 sweeps on a 30 m circle that never leaves the centre cube.  Here the sensor drives ~445 m down a street
without returning (a-loam_amd/synthetic.py `travel`), so that
  * the pose chain integrates without renormalisation for 300 frames (reference src/laserOdometry.cpp:504-505),
  * the submap is gathered from changing cubes (src/laserMapping.cpp:509-539) and the cubes grow / are re-filtered frame after frame (:737-801),
  * the cube window really shifts, twice, because the sensor is 375 m and then 425 m from where it started (:323-507),
  * the device map outgrows the pool it was created with (aloam_mapping_step doubles it, no point dropped).

tests/golden/reflong_hdl64_c512_seed51.npz (tools/make_ref_golden.py --long) holds what the reference's OWN three translation units produce end
to end on 300 sweeps of 64 x 512, plus the same run with one coordinate of one input point in a hundred moved by ONE ulp (`ulp_*`).

What can be asked of a free-running comparison over this horizon.  The pipeline is a chain of discrete decisions on float bits (which points are
features, which neighbours pass a gate, which voxel a centroid falls into), so two runs that differ in ANY last bit part ways and never meet again:
the reference against itself with 1 % of its input moved by one ulp differs by > 1e-4 m in frame 1 and by 8 cm after 300 frames.  The oracle in the
reference's literal order has no such difference and reproduces all 300 frames BIT FOR BIT (poses, window, every cube by sha256).  The HIP path (and the
oracle in "canonical" order) sums the members of a voxel in input order where pcl::VoxelGrid sums them in the order an unstable std::sort leaves them:
<= 4 ulp in some less-flat centroids.  Its odometry chain stays within 2e-7 m of the reference for all 300 frames; its scan-to-map poses stay within
1e-4 m / rad until the first decision flips - frame 35, the line test `eigenvalue ratio > 3` (src/laserMapping.cpp:611) of one corner point, 1.01213 against
1.01212 on either side of 1.01213 - and then drift to 2 cm, a quarter of the reference's own one-ulp sensitivity.  So the tests assert: bit-exactness
where it exists (literal order; the HIP path against the canonical oracle on IDENTICAL map state, every 25 frames at full map depth), the 1e-4 tolerance
on the odometry chain throughout and on the refined poses until the first flipped decision, and the reference's own one-ulp envelope afterwards.
With the reference's summation order switched on (aloam_set_voxel_sum_order) the device reproduces the reference's run itself: tests/test_reference_order.py.
"""
import hashlib
import json
import os

import numpy as np
import pytest
from conftest import bits_equal, quat_angle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reflong_hdl64_c512_seed51.npz")
POSE_TOL_M = POSE_TOL_RAD = 1e-4          # BASELINE.json north_star
FIRST_FLIP_FRAME = 35                     # canonical vs literal order: first flipped decision (tools/long_horizon_flips.py), measured
ENVELOPE_FACTOR = 2.0                     # a free-running run may differ from the reference by twice what ONE one-ulp run of the reference differs from it
                                          # (one realisation of a chaotic divergence is a yardstick, not a bound: the canonical oracle reaches 1.07 x at frame 253)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _checkpoints(g):
    n, c = int(g["frames"]), int(g["check"])
    return sorted(set(range(0, n, c)) | {n - 1})


def _scans(g, sequence):
    scans, R, t, model = sequence(str(g["sensor"]), int(g["frames"]), seed=int(g["seed"]), **json.loads(str(g["kwargs"])))
    assert [len(x) for x in scans] == [int(v) for v in g["scan_n"]]
    for k in _checkpoints(g):
        assert _sha(scans[k]) == str(g[f"scan_sha{k}"]), "the synthetic generator no longer reproduces the sweeps the fixture was made from"
    return scans


def _envelope(g):
    """Running maximum of |refined pose of the one-ulp run - refined pose| of the reference's own code, per frame (m, rad)."""
    dt = np.linalg.norm(g["ulp_t_w"] - g["t_w"], axis=1)
    dr = np.array([quat_angle(a, b) for a, b in zip(g["ulp_q_w"], g["q_w"])])
    return np.maximum.accumulate(dt), np.maximum.accumulate(dr)


def _check_free_running(g, k, t_w, q_w, t_odom, q_odom, env, ctx):
    """The assertions every free-running run in this repo's summation order must pass against the reference's own run."""
    assert np.linalg.norm(t_odom - g["odom_t"][k]) < POSE_TOL_M and quat_angle(q_odom, g["odom_q"][k]) < POSE_TOL_RAD, (ctx, k, "odometry chain")
    dt, dr = np.linalg.norm(t_w - g["t_w"][k]), quat_angle(q_w, g["q_w"][k])
    if k < FIRST_FLIP_FRAME:
        assert dt < POSE_TOL_M and dr < POSE_TOL_RAD, (ctx, k, dt, dr)
    else:
        assert dt <= max(POSE_TOL_M, ENVELOPE_FACTOR * env[0][k]) and dr <= max(POSE_TOL_RAD, ENVELOPE_FACTOR * env[1][k]), (ctx, k, dt, dr, env[0][k], env[1][k])
    return dt, dr


def test_long_golden_present():
    assert os.path.exists(GOLDEN), "tests/golden/reflong_*.npz missing: run tools/make_ref_golden.py --long where /root/reference exists"
    g = np.load(GOLDEN)
    assert int(g["frames"]) >= 300 and np.linalg.norm(g["t_w"][-1]) > 400.0                       # a drive, not a lap
    assert len({tuple(c) for c in g["cen"]}) >= 3                                                   # the cube window shifted (twice) by real motion
    assert int(g["map_total"][-1].sum()) > 300000                                                   # and the map is deep
    env = _envelope(g)
    assert env[0][1] > POSE_TOL_M and env[0][-1] > 0.05                                             # the reference's one-ulp sensitivity (see the module docstring)


def test_oracle_long_run_is_bit_exact_with_reference_code(O, sequence):
    """300 frames, literal order: every odometry pose, refined pose, map<-odom transform, window centre and class total of every frame, and at every
    25th frame each cube's population and the sha256 of each class's points and of the registered cloud - the reference's bits."""
    g = np.load(GOLDEN)
    scans = _scans(g, sequence)
    orc = O.Oracle(n_scans=int(g["n_scans"]), min_range=float(g["min_range"]), canonical_order=False)
    orc.map_config(float(g["line_res"]), float(g["plane_res"]))
    check = set(_checkpoints(g))
    cnt = np.zeros(21 * 21 * 11, np.int32)
    for k, x in enumerate(scans):
        orc.scan_register(x)
        po = orc.odometry_step()
        assert np.abs(po["q_w"] - g["odom_q"][k]).max() < 1e-12 and np.abs(po["t_w"] - g["odom_t"][k]).max() < 1e-12, k
        assert orc.odom_stats()["corner_corr"][1] == int(g["corr"][k][0]) and orc.odom_stats()["plane_corr"][1] == int(g["corr"][k][1]), k
        pm = orc.mapping_step(po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
        for key in ("q_w", "t_w", "q_wmap_wodom", "t_wmap_wodom"):
            assert np.abs(pm[key] - g[key][k]).max() < 1e-12, (k, key)
        info = orc.map_info()
        assert (info["cenW"], info["cenH"], info["cenD"]) == tuple(int(v) for v in g["cen"][k]), k
        for cls in (0, 1):
            O.lib().orc_map_cube_counts(orc.h, cls, O._p(cnt))
            assert int(cnt.sum()) == int(g["map_total"][k][cls]) and int((cnt > 0).sum()) == int(g["map_cubes"][k][cls]), (k, cls)
        if k in check:
            for cls, name in ((0, "corner_map"), (1, "surf_map")):
                cubes = orc.map_cubes(cls)
                ids = [int(i) for i in g[f"{name}_ids{k}"]]
                assert sorted(cubes) == ids and [len(cubes[c]) for c in ids] == [int(c) for c in g[f"{name}_cnt{k}"]], (k, name)
                assert _sha(np.concatenate([cubes[c] for c in ids])) == str(g[f"{name}_sha{k}"]), (k, name)
            reg = orc.map_cloud(O.MAP_REGISTERED)
            assert len(reg) == int(g[f"registered_n{k}"]) and _sha(reg) == str(g[f"registered_sha{k}"]), k


def test_canonical_order_long_run_stays_inside_the_reference_envelope(O, sequence):
    """The summation order of the HIP path, on the CPU: odometry chain within 1e-4 of the reference for all 300 frames (measured 1.7e-7 m), refined
    poses within 1e-4 until the first flipped decision and within the reference's own one-ulp envelope afterwards, same cubes occupied."""
    g = np.load(GOLDEN)
    scans = _scans(g, sequence)
    env = _envelope(g)
    orc = O.Oracle(n_scans=int(g["n_scans"]), min_range=float(g["min_range"]))
    orc.map_config(float(g["line_res"]), float(g["plane_res"]))
    check = set(_checkpoints(g))
    worst_odom = 0.0
    O.decision_log(True)                                                                           # every threshold decision of the 300 frames (below)
    for k, x in enumerate(scans):
        orc.scan_register(x)
        po = orc.odometry_step()
        pm = orc.mapping_step(po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
        _check_free_running(g, k, pm["t_w"], pm["q_w"], po["t_w"], po["q_w"], env, "canonical oracle")
        worst_odom = max(worst_odom, np.linalg.norm(po["t_w"] - g["odom_t"][k]))
        info = orc.map_info()
        assert (info["cenW"], info["cenH"], info["cenD"]) == tuple(int(v) for v in g["cen"][k]), k
        if k in check:
            for cls, name in ((0, "corner_map"), (1, "surf_map")):
                assert sorted(orc.map_cubes(cls)) == [int(i) for i in g[f"{name}_ids{k}"]], (k, name)
    assert worst_odom < 1e-5, worst_odom
    # The decision margins of tests/test_decision_margins.py over THIS run (32 M decisions): what a third-party routine that differs in the last bits
    # from this repo's stand-ins (Eigen's eigen solver / QR behind the line and plane tests, the dense solve behind the trust-region loop) could flip.
    # Measured: closest Eigen-dependent decision 2.3e-6 (relative), closest trust-region decision 4e-5 - the flips this run does see (frame 35 on)
    # come from the f32 summation order of the voxel filters, a 1e-7 effect, not from anything of relative size 1e-12.
    import test_decision_margins as tdm
    kinds, values, thresholds = O.decisions()
    O.decision_log(False)
    assert len(kinds) > 20_000_000
    rows = tdm.margin_table(O, kinds, values, thresholds)
    print(f"\ndecision margins over the {len(scans)}-frame drive, {len(kinds)} decisions; bins of the relative margin: <1e-12, <1e-9, <1e-6, <1e-3, >=1e-3")
    for name, n, mn, hist in rows:
        print(f"  {name:34s} n = {n:9d}  min relative margin {mn if mn is None else format(mn, '.3g')}  {hist}")
    for kind in tdm.F64_KINDS:
        name, n, mn, hist = rows[kind]
        assert n > 1_000_000 and hist[0] == 0 and hist[1] == 0 and mn > tdm.PERTURBATION, (name, n, mn, hist)
    for kind in tdm.LM_KINDS:
        name, n, mn, hist = rows[kind]
        assert n > 3000 and mn > 1e-6, (name, n, mn)


# ---- the HIP path ---------------------------------------------------------------------------------------------------------------------------------
def _inject_oracle_map(gpu, orc, O, frame_count):
    for cls in (0, 1):
        gpu.set_map(orc.map_cubes(cls), cls)
    info, pose = orc.map_info(), orc.map_pose()
    gpu.set_map_frame((info["cenW"], info["cenH"], info["cenD"]), pose["q_wmap_wodom"], pose["t_wmap_wodom"], frame_count)


def _compare_cubes(got, want, ctx, max_points_off=0):
    """Same cubes; populations equal; points bit-equal except for `max_points_off` points in total (a map point is q p + t rounded to f32 with
    refined poses that agree to ~1e-10: a coordinate on a rounding boundary lands one ulp away now and then)."""
    assert sorted(got) == sorted(want), (ctx, sorted(set(got) ^ set(want)))
    off = 0
    for c in want:
        assert got[c].shape == want[c].shape, (ctx, c, got[c].shape, want[c].shape)
        if not bits_equal(got[c], want[c]):
            d = (got[c].view(np.uint32) != want[c].view(np.uint32)).any(axis=1)
            assert np.abs(got[c].astype(np.float64) - want[c]).max() < 2e-5, (ctx, c)
            off += int(d.sum())
    assert off <= max_points_off, (ctx, off)
    return off


@pytest.mark.gpu
def test_gpu_long_run_vs_reference_code_and_oracle(binding, O, sequence):
    """300 free-running sweeps on the device (64 x 512, pool 131 072 points to start with) beside the canonical-order oracle, against the reference's own run:
      (a) free-running, every frame: odometry chain within 1e-4 m / rad of the reference; refined pose within 1e-4 until the first flipped decision,
          inside the reference's one-ulp envelope afterwards; window centre equal; the same cubes occupied at every 25th frame;
      (b) identical inputs at full map depth, every 25th frame: a second context is given the ORACLE's map, window and map<-odom transform as they
          are before that frame and the frame's inputs; its step must reproduce the oracle's - stacks bit for bit, factor counts equal, pose to 1e-8,
          every cube's population equal and all but a handful of map points bit-equal;
      (c) the pools grew (no point was dropped: aloam_synchronize raises ALOAM_E_CAPACITY otherwise) and report it."""
    g = np.load(GOLDEN)
    scans = _scans(g, sequence)
    env = _envelope(g)
    n_scans, min_range, lr, pr = int(g["n_scans"]), float(g["min_range"]), float(g["line_res"]), float(g["plane_res"])
    orc = O.Oracle(n_scans=n_scans, min_range=min_range)
    orc.map_config(lr, pr)
    gpu = binding.Aloam(n_scans=n_scans, min_range=min_range, max_points=int(g["max_points"]) + 256)
    gpu.mapping_enable(lr, pr, pool_points=131072)
    forced = binding.Aloam(n_scans=n_scans, min_range=min_range, max_points=int(g["max_points"]) + 256)
    forced.mapping_enable(lr, pr, pool_points=131072)
    check = set(_checkpoints(g))
    first_gap, drift, points_off = None, [], 0
    for k, x in enumerate(scans):
        if k in check and k > 0:
            _inject_oracle_map(forced, orc, O, k)
        orc.scan_register(x)
        po = orc.odometry_step()
        inputs = (po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
        pm = orc.mapping_step(*inputs)
        if k in check and k > 0:                                                                       # (b)
            pf = forced.mapping_step_inputs(*inputs)
            forced.synchronize()
            io, ig = orc.map_info(), forced.map_info()
            for key in ("cenW", "cenH", "cenD", "from_map_corner", "from_map_surf", "corner_stack", "surf_stack", "corner_num0", "corner_num1", "surf_num0", "surf_num1",
                        "lm_iterations0", "lm_iterations1", "termination0"):
                assert io[key] == ig[key], (k, key, io, ig)
            assert bits_equal(orc.map_cloud(O.MAP_CORNER_STACK), forced.map_cloud(binding.MAP_CORNER_STACK)), k
            assert bits_equal(orc.map_cloud(O.MAP_SURF_STACK), forced.map_cloud(binding.MAP_SURF_STACK)), k
            for key in ("q_w", "t_w", "q_wmap_wodom", "t_wmap_wodom"):
                assert np.abs(pm[key] - pf[key]).max() < 1e-8, (k, key, pm[key], pf[key])
            for cls in (0, 1):
                points_off += _compare_cubes(forced.map_cubes(cls), orc.map_cubes(cls), ("identical inputs", k, cls), max_points_off=8)
        gpu.scan_register(x)                                                                           # (a)
        gpu.odometry_step()
        gpu.mapping_step()
        gpu.synchronize()
        pg, og = gpu.map_pose(), gpu.pose()
        dt, dr = _check_free_running(g, k, pg["t_w"], pg["q_w"], og["t_w"], og["q_w"], env, "HIP path")
        d_orc = np.linalg.norm(pg["t_w"] - pm["t_w"])
        if k < 20:
            assert d_orc < 1e-7, (k, d_orc)
        assert d_orc <= max(POSE_TOL_M, ENVELOPE_FACTOR * env[0][k]), (k, d_orc)
        info = gpu.map_info()
        assert (info["cenW"], info["cenH"], info["cenD"]) == tuple(int(v) for v in g["cen"][k]), k
        if first_gap is None and d_orc > 1e-7:
            first_gap = k
        if k in check:
            gap = []
            for cls, name in ((0, "corner_map"), (1, "surf_map")):
                cnt = np.zeros(21 * 21 * 11, np.int32)
                binding.lib().aloam_map_cube_counts(gpu.h, 0, cls, binding._p(cnt))
                assert sorted(int(i) for i in np.nonzero(cnt)[0]) == [int(i) for i in g[f"{name}_ids{k}"]], (k, name)
                gap.append(int(cnt.sum()) - int(g["map_total"][k][cls]))
            drift.append((k, dt, dr, d_orc, gap))
    pool = gpu.map_pool_info()                                                                          # (c)
    assert pool["growths"] >= 1 and pool["pool_points"] > 131072 and pool["live_max"] >= int(g["map_total"][-1].max()) - 1000, pool
    assert pool["live_max"] <= pool["pool_points"]
    print("\nframe  |t - t_ref| m   angle rad   |t - t_oracle| m   map population gap (corner, surf) vs the reference")
    for k, dt, dr, do, gap in drift:
        print(f"{k:5d}  {dt:.3e}      {dr:.3e}   {do:.3e}          {gap}")
    print("first frame whose refined pose differs from the canonical oracle's by > 1e-7 m:", first_gap, "; map points off by an ulp under identical inputs:", points_off, "; pool:", pool)
    gpu.close(); forced.close()


@pytest.mark.gpu
def test_gpu_long_run_at_benchmark_size(binding, O, syn):
    """260 free-running sweeps of 64 x 2048 (the benchmarked size; rendered on the device) through registration -> odometry -> mapping, beside the
    canonical-order oracle: the odometry chain within 1e-4 m / rad throughout; refined poses within 1e-4 for as long as every discrete result of the two
    runs agrees (stack sizes, factor counts, every cube's population) and a sanity bound afterwards (both runs then follow their own decisions, see the
    module docstring); identical inputs at depth every 50th frame as in the 64 x 512 test; trajectory error against the ground truth equal to the oracle's
    within 10 %; the window shifts; the pools grow."""
    import torch
    frames, seed, step = 260, 61, 1.6
    dev = "cuda"
    model = syn.sensor_model("HDL-64", device=dev)
    world = syn.make_street_world(seed).to(dev)
    R, t = syn.trajectory_travel(frames, step=step, seed=seed)
    gen = torch.Generator(device=dev).manual_seed(77 + seed)
    orc = O.Oracle(n_scans=64, min_range=5.0)
    orc.map_config(0.4, 0.8)
    gpu = binding.Aloam(n_scans=64, min_range=5.0, max_points=131072 + 256)
    gpu.mapping_enable(0.4, 0.8, pool_points=131072)
    forced = binding.Aloam(n_scans=64, min_range=5.0, max_points=131072 + 256)
    forced.mapping_enable(0.4, 0.8, pool_points=131072)
    agree_until, worst_agree, worst_after, est_g, est_o, cens = None, 0.0, 0.0, [], [], set()
    keys = ("cenW", "cenH", "cenD", "from_map_corner", "from_map_surf", "corner_stack", "surf_stack", "corner_num0", "corner_num1", "surf_num0", "surf_num1")
    for k in range(frames):
        x = syn.render_scan(world, model, R[k], t[k], 0.02, gen, max_range=syn.STREET_MAX_RANGE, cull=True).cpu().numpy()
        forcing = k > 0 and k % 50 == 0
        if forcing:
            _inject_oracle_map(forced, orc, O, k)
        orc.scan_register(x)
        po = orc.odometry_step()
        inputs = (po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
        pm = orc.mapping_step(*inputs)
        io = orc.map_info()
        if forcing:
            pf = forced.mapping_step_inputs(*inputs)
            forced.synchronize()
            ig = forced.map_info()
            assert all(io[key] == ig[key] for key in keys + ("lm_iterations0", "lm_iterations1", "termination0")), (k, io, ig)
            assert bits_equal(orc.map_cloud(O.MAP_SURF_STACK), forced.map_cloud(binding.MAP_SURF_STACK)), k
            for key in ("q_w", "t_w", "q_wmap_wodom", "t_wmap_wodom"):
                assert np.abs(pm[key] - pf[key]).max() < 1e-8, (k, key)
            for cls in (0, 1):
                _compare_cubes(forced.map_cubes(cls), orc.map_cubes(cls), ("identical inputs", k, cls), max_points_off=16)
        gpu.scan_register(x)
        gpu.odometry_step()
        gpu.mapping_step()
        gpu.synchronize()
        pg, og, ig = gpu.map_pose(), gpu.pose(), gpu.map_info()
        assert np.linalg.norm(og["t_w"] - po["t_w"]) < POSE_TOL_M and quat_angle(og["q_w"], po["q_w"]) < POSE_TOL_RAD, (k, "odometry chain")
        d = np.linalg.norm(pg["t_w"] - pm["t_w"])
        if agree_until is None:
            same = all(io[key] == ig[key] for key in keys)
            if same:
                co, cg = np.zeros(21 * 21 * 11, np.int32), np.zeros(21 * 21 * 11, np.int32)
                for cls in (0, 1):
                    O.lib().orc_map_cube_counts(orc.h, cls, O._p(co)); binding.lib().aloam_map_cube_counts(gpu.h, 0, cls, binding._p(cg))
                    same = same and np.array_equal(co, cg)
            if same:
                worst_agree = max(worst_agree, d)
                assert d < POSE_TOL_M and quat_angle(pg["q_w"], pm["q_w"]) < POSE_TOL_RAD, (k, d)
            else:
                agree_until = k
        if agree_until is not None:
            worst_after = max(worst_after, d)
            assert d < 0.1, (k, d)                                               # sanity only: two runs of a chaotic pipeline (module docstring)
            assert (io["cenW"], io["cenH"], io["cenD"]) == (ig["cenW"], ig["cenH"], ig["cenD"]), k
        cens.add((ig["cenW"], ig["cenH"], ig["cenD"]))
        gt = R[0].numpy().T @ (t[k].numpy() - t[0].numpy())
        est_g.append(np.linalg.norm(pg["t_w"] - gt)); est_o.append(np.linalg.norm(pm["t_w"] - gt))
    ate_g, ate_o = float(np.sqrt(np.mean(np.square(est_g)))), float(np.sqrt(np.mean(np.square(est_o))))
    pool = gpu.map_pool_info()
    print(f"\n64 x 2048, {frames} sweeps: every discrete result equal to the oracle's until frame {agree_until} (worst pose gap there {worst_agree:.2e} m), "
          f"worst gap afterwards {worst_after:.2e} m; ATE vs ground truth {ate_g:.4f} m (device) / {ate_o:.4f} m (oracle); window centres {sorted(cens)}; pool {pool}; "
          f"map {gpu.map_info()['from_map_corner']} / {gpu.map_info()['from_map_surf']} submap points")
    assert agree_until is None or agree_until >= 20, agree_until
    assert abs(ate_g - ate_o) <= 0.1 * ate_o + 1e-3, (ate_g, ate_o)
    assert len(cens) >= 2 and pool["growths"] >= 1, (cens, pool)
    gpu.close(); forced.close()
