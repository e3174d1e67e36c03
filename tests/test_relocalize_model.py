"""The numpy model of the hypothesis score (tests/relocalize_model.py) against the oracle's own mapping step, and the geometry of the
correction grid (a-loam_amd/relocalize.py).  No GPU: the GPU tests then compare the kernel with this model."""
import importlib
import math

import numpy as np
import pytest

import relocalize_model as M


@pytest.fixture(scope="module")
def reloc():
    return importlib.import_module("a-loam_amd.relocalize")


def _oracle_drive(O, sequence, name, frames, seed, res, **kw):
    """Oracle registration + odometry + mapping over a synthetic drive.  Returns what the LAST mapping step started from (cubes, cen,
    correction, odometry pose) and what it counted (stacks, factor counts of iteration 0)."""
    scans, R, t, model = sequence(name, frames, seed=seed, **kw)
    orc = O.Oracle(n_scans=model.n_scans, min_range=model.min_range)
    orc.map_config(*res)
    before = None
    for k, x in enumerate(scans):
        orc.scan_register(x)
        po = orc.odometry_step()
        if k == frames - 1:
            i, p = orc.map_info(), orc.map_pose()
            before = {"cubes": [orc.map_cubes(0), orc.map_cubes(1)], "cen": (i["cenW"], i["cenH"], i["cenD"]),
                      "q_corr": p["q_wmap_wodom"].copy(), "t_corr": p["t_wmap_wodom"].copy(), "q_wodom": po["q_w"].copy(), "t_wodom": po["t_w"].copy()}
        orc.mapping_step(po["q_w"], po["t_w"], orc.cloud(O.CLOUD_CORNER_LAST), orc.cloud(O.CLOUD_SURF_LAST), orc.cloud(O.CLOUD_FULL))
    info = orc.map_info()
    assert (info["cenW"], info["cenH"], info["cenD"]) == before["cen"]      # no window shift: the cube indices captured before still hold
    return before, orc.map_cloud(3), orc.map_cloud(4), info


@pytest.mark.parametrize("name,frames,seed,res", [("VLP-16", 4, 3, (0.2, 0.4)), ("VLP-16", 3, 7, (0.4, 0.8))])
def test_model_counts_what_the_oracle_mapping_step_counts(O, sequence, name, frames, seed, res):
    b, stack_c, stack_s, info = _oracle_drive(O, sequence, name, frames, seed, res)
    par = M.start_pose(b["q_wodom"], b["t_wodom"], b["q_corr"], b["t_corr"])
    center = M.center_cube(par, b["cen"])
    sub_c, sub_s = M.submap(b["cubes"][0], center), M.submap(b["cubes"][1], center)
    assert (len(sub_c), len(sub_s)) == (info["from_map_corner"], info["from_map_surf"])
    assert info["corner_num0"] > 0 and info["surf_num0"] > 50                # a frame that was fitted, not a gated-out one
    (s,) = M.score_model(stack_c, stack_s, sub_c, sub_s, b["q_wodom"], b["t_wodom"], [(b["q_corr"], b["t_corr"])])
    assert (s["corner_factors"], s["surf_factors"]) == (info["corner_num0"], info["surf_num0"]), (s, info)
    assert s["corner_found"] >= s["corner_factors"] and s["surf_found"] >= s["surf_factors"] and s["cost"] >= 0.0
    # a displaced correction is another question with another answer (the model is not insensitive to its candidate)
    (d,) = M.score_model(stack_c, stack_s, sub_c, sub_s, b["q_wodom"], b["t_wodom"], [(b["q_corr"], b["t_corr"] + np.array([1.5, -1.0, 0.0]))])
    assert d["cost"] != s["cost"]
    assert M.best_of([d, s, s]) == 1                                         # more factors or lower cost first; ties: the lower index


# Check 2: the ranking rule on a score surface nobody had seen, without a GPU.  The seed-44 HDL-64 drive of
# test_multi_hypothesis_best_score_is_the_truth, shortened to 256 columns and 6 mapped frames (frame 7 is scored) so that one guess takes
# under a minute; the grid is the full one, 15 x 15 x 11 = 2475 nodes.  BASIN_*: what DESIGN 7e measured the frozen steps to converge from.
BASIN_M, BASIN_DEG = 1.0, 2.5
RANK_GUESSES = [(2.8, -1.3, 7.0), (-3.0, 3.0, -10.0), (0.7, 2.2, -4.0)]         # displaced guesses that are no grid multiples


@pytest.fixture(scope="module")
def seed44(O, sequence):
    b, stack_c, stack_s, info = _oracle_drive(O, sequence, "HDL-64", 7, 44, (0.4, 0.8), columns=256)
    par = M.start_pose(b["q_wodom"], b["t_wodom"], b["q_corr"], b["t_corr"])
    center = M.center_cube(par, b["cen"])
    return dict(b=b, par=par, stack_c=stack_c, stack_s=stack_s, sub_c=M.submap(b["cubes"][0], center), sub_s=M.submap(b["cubes"][1], center), info=info)


def _displaced(reloc, s, dx, dy, dyaw):
    """The correction the step started from, turned by dyaw degrees about the sensor and moved by (dx, dy); the sensor under that guess."""
    h = math.radians(dyaw) / 2
    dq, sensor = np.array([0.0, 0.0, math.sin(h), math.cos(h)]), s["par"][4:7]
    shift = np.array([dx, dy, 0.0])
    return reloc._qmul(dq, s["b"]["q_corr"]), reloc._qrot(dq, s["b"]["t_corr"] - sensor) + sensor + shift, sensor + shift


@pytest.mark.parametrize("guess", RANK_GUESSES)
def test_most_factors_then_lower_cost_puts_the_best_node_inside_the_basin(reloc, seed44, guess):
    s = seed44
    gq, gt, sensor = _displaced(reloc, s, *guess)
    q, t, nodes = reloc.correction_grid(gq, gt, sensor, 3.5, 0.5, 12.5, 2.5)
    assert len(q) == 2475
    w, score, fitted = M.best_model(s["stack_c"], s["stack_s"], s["sub_c"], s["sub_s"], s["b"]["q_wodom"], s["b"]["t_wodom"], list(zip(q, t)))
    got = M.start_pose(s["b"]["q_wodom"], s["b"]["t_wodom"], q[w], t[w])
    err_m = float(np.linalg.norm(got[4:7] - s["par"][4:7]))
    err_deg = 2 * math.degrees(math.acos(min(1.0, abs(float(np.dot(got[:4], s["par"][:4]))))))
    print(f"guess {guess}: best node {tuple(nodes[w])}, {score}, {fitted} candidate(s) fitted exactly; start pose {err_m:.3f} m and {err_deg:.2f} deg from the truth "
          f"(truth: {s['info']['corner_num0']} + {s['info']['surf_num0']} factors)")
    assert err_m <= BASIN_M and err_deg <= BASIN_DEG, (guess, nodes[w], err_m, err_deg)


def test_pruned_argmax_equals_the_plain_one(reloc, seed44):
    """best_model prunes with bounds; on a handful of candidates it must name the candidate best_of(score_model(...)) names, and its bounds
    must bracket the exact count."""
    s = seed44
    gq, gt, sensor = _displaced(reloc, s, 0.3, -0.2, 1.0)
    q, t, nodes = reloc.correction_grid(gq, gt, sensor, 0.5, 0.5, 2.5, 2.5)          # 3 x 3 x 3 = 27 nodes
    pick = [0, 4, 9, 13, 14, 17, 22, 26]
    cand = [(q[k], t[k]) for k in pick]
    args = (s["stack_c"], s["stack_s"], s["sub_c"], s["sub_s"], s["b"]["q_wodom"], s["b"]["t_wodom"])
    plain = M.score_model(*args, cand)
    w, score, fitted = M.best_model(*args, cand)
    assert w == M.best_of(plain) and score == plain[w] and 1 <= fitted <= len(cand)
    for (cq, ct), p in zip(cand, plain):
        lo, hi, found = M.factor_bounds(s["stack_c"], s["stack_s"], s["sub_c"], s["sub_s"], M.start_pose(s["b"]["q_wodom"], s["b"]["t_wodom"], cq, ct))
        assert lo <= p["corner_factors"] + p["surf_factors"] <= hi <= found == p["corner_found"] + p["surf_found"]


def test_gated_out_submap_scores_zeros(O):
    z = np.zeros((0, 4), np.float32)
    pts = np.random.default_rng(0).normal(size=(40, 4)).astype(np.float32)
    (s,) = M.score_model(pts, pts, pts[:10], pts, (0, 0, 0, 1), (0, 0, 0), [((0, 0, 0, 1), (0, 0, 0))])   # 10 corner points: not > 10
    assert s == {"corner_factors": 0, "surf_factors": 0, "corner_found": 0, "surf_found": 0, "cost": 0.0}
    (s,) = M.score_model(z, z, pts, np.concatenate([pts, pts]), (0, 0, 0, 1), (0, 0, 0), [((0, 0, 0, 1), (0, 0, 0))])
    assert s["corner_found"] == 0 and s["surf_found"] == 0


def test_correction_grid_geometry(reloc):
    gq = np.array([0.01, -0.02, 0.3, 0.0])
    gq[3] = math.sqrt(1 - float(gq[:3] @ gq[:3]))
    gt, sensor = np.array([1.5, -0.0, 0.25]), np.array([4.0, 2.0, 0.5])
    q, t, nodes = reloc.correction_grid(gq, gt, sensor, 3.5, 0.5, 12.5, 2.5)
    assert q.shape == (2475, 4) and t.shape == (2475, 3) and nodes.shape == (2475, 3)      # 15 x 15 x 11
    assert sorted(set(nodes[:, 0])) == [-3.5 + 0.5 * k for k in range(15)] and sorted(set(nodes[:, 2])) == [-12.5 + 2.5 * k for k in range(11)]
    (mid,) = np.nonzero((nodes == 0).all(axis=1))[0:1]
    assert len(mid) == 1 and q[mid[0]].tobytes() == gq.tobytes() and t[mid[0]].tobytes() == gt.tobytes()   # the guess itself, bit for bit (-0.0 too)
    # every node keeps the sensor where the shift puts it: turning about the sensor does not move it
    for k in (0, 7, 1237, 2474):
        moved = reloc._qrot(q[k], reloc._qrot(gq * np.array([-1, -1, -1, 1.0]), sensor - gt)) + t[k]
        assert np.allclose(moved, sensor + np.array([nodes[k, 0], nodes[k, 1], 0.0]), atol=1e-12), k
        dq = reloc._qmul(q[k], gq * np.array([-1, -1, -1, 1.0]))
        assert abs(2 * math.degrees(math.atan2(dq[2], dq[3])) - nodes[k, 2]) < 1e-9 and abs(dq[0]) < 1e-12 and abs(dq[1]) < 1e-12
    # any displacement inside the searched box has a node within half a cell of it
    lin, yaw = reloc.grid_axes(3.5, 0.5, 12.5, 2.5)
    for dx, dy, dyaw in ((2.8, -1.3, 7.0), (-3.0, 3.0, -10.0), (0.7, 2.2, -4.0)):
        assert math.hypot(min(abs(lin - dx)), min(abs(lin - dy))) <= 0.36 and min(abs(yaw - dyaw)) <= 1.25
    q1, t1, n1 = reloc.correction_grid(gq, gt, sensor, 0.0, 0.5, 0.0, 2.5)
    assert len(q1) == 1 and q1[0].tobytes() == gq.tobytes()
