"""Worlds and factor sets shared by the pose-information tests: the corridor and the open world of DESIGN §7j, and scan-to-map factors built
from the search and the fits of relocalize_model / the oracle (imported, not copied)."""
import importlib
import math

import numpy as np
import torch

import oracle_py
import relocalize_model as rm

syn = importlib.import_module("a-loam_amd.synthetic")

CORRIDOR_YAW = 0.3            # the sensor looks 0.3 rad off the corridor axis
CORRIDOR_STEP = 0.5           # metres between sweeps, along the axis
CORRIDOR_RANGE = 60.0         # render_scan max_range in the corridor
# The thresholds of the corridor tests, a factor of two off what the model measures on these worlds (test_information_model.py):
# |cos| 0.99995 / 0.99999 and lambda0 / lambda1 0.059 / 0.103 in the corridor (noise 0 / 0.01), 0.526 / 0.572 in the open world.
AXIS_COS_MIN, CORRIDOR_RATIO_MAX, OPEN_RATIO_MIN = 0.99, 0.21, 0.26


def corridor_world():
    """Two walls 12 m apart and 1000 m long, as two boxes, and one pole out of sight (render_scan cannot take zero poles).  The enclosing
    walls of the world are beyond the sensor's range."""
    f = lambda v: torch.tensor(v, dtype=torch.float64)
    h = 6.0
    return syn.World(2000.0, f([[0.0, 6.5, -syn.SENSOR_HEIGHT + h], [0.0, -6.5, -syn.SENSOR_HEIGHT + h]]), f([[500.0, 0.5, h], [500.0, 0.5, h]]),
                     f([[1.0, 0.0], [1.0, 0.0]]), f([[1500.0, 1500.0]]), f([0.2]), f([-syn.SENSOR_HEIGHT + 4.0]))


def corridor_poses(n):
    """Sensor poses (R [n, 3, 3], t [n, 3]) of n sweeps CORRIDOR_STEP apart along the axis, yawed CORRIDOR_YAW, and the axis in the frame of
    sweep 0 (the map frame of a run that starts there)."""
    c, s = math.cos(CORRIDOR_YAW), math.sin(CORRIDOR_YAW)
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    t = torch.stack([torch.tensor([CORRIDOR_STEP * k, 0.0, 0.0], dtype=torch.float64) for k in range(n)])
    return R[None].repeat(n, 1, 1), t, np.array([c, -s, 0.0])


def corridor_scans(n, noise_sigma, columns=512, seed=5):
    model = syn.sensor_model("VLP-16", columns=columns)
    R, t, axis = corridor_poses(n)
    gen = torch.Generator().manual_seed(seed)
    world = corridor_world()
    return [syn.render_scan(world, model, R[k], t[k], noise_sigma, gen, max_range=CORRIDOR_RANGE) for k in range(n)], R, t, axis, model


def open_scans(n, noise_sigma, columns=512, seed=5):
    """make_world(1), n sweeps CORRIDOR_STEP apart on the usual circle."""
    model = syn.sensor_model("VLP-16", columns=columns)
    R, t = syn.trajectory(n, step=CORRIDOR_STEP, seed=1)
    gen = torch.Generator().manual_seed(seed)
    world = syn.make_world(1)
    return [syn.render_scan(world, model, R[k], t[k], noise_sigma, gen) for k in range(n)], R, t, model


def relative_par(R, t, k):
    """par = (q xyzw, t) of sweep k in the frame of sweep 0."""
    Rr = (R[0].T @ R[k]).numpy()
    tr = (R[0].T @ (t[k] - t[0])).numpy()
    w = math.sqrt(max(0.0, 1.0 + Rr[0, 0] + Rr[1, 1] + Rr[2, 2])) / 2.0
    q = np.array([(Rr[2, 1] - Rr[1, 2]) / (4 * w), (Rr[0, 2] - Rr[2, 0]) / (4 * w), (Rr[1, 0] - Rr[0, 1]) / (4 * w), w])
    return np.concatenate([q, tr])


def map_factors_model(stack_corner, stack_surf, submap_corner, submap_surf, par):
    """The scan-to-map factors of one pose, built as relocalize_model.score_one builds them (its transform, the oracle's 5-NN search, line
    and plane fits, the same validity tests): lines [n, 9] (cp, a, b) and planes [m, 7] (cp, n, d), float64."""
    sc, ss = np.asarray(stack_corner, np.float32), np.asarray(stack_surf, np.float32)
    mc, ms = np.ascontiguousarray(submap_corner, np.float32), np.ascontiguousarray(submap_surf, np.float32)
    lines, planes = [], []
    if not (len(mc) > 10 and len(ms) > 50):
        return np.zeros((0, 9)), np.zeros((0, 7))
    if len(sc):
        idx, d2 = oracle_py.knn_search(mc, rm.associate_to_map(sc, par), 5)
        for i in np.nonzero((idx[:, 4] >= 0) & (d2[:, 4] < np.float32(1.0)))[0]:
            near = mc[idx[i], :3].astype(np.float64)
            c = np.zeros(3)
            for j in range(5):
                c = c + near[j]
            c = c / 5.0
            cov = np.zeros((3, 3))
            for j in range(5):
                z = near[j] - c
                cov = cov + np.outer(z, z)
            vals, vecs = oracle_py.sym_eigen3(cov)
            if vals[2] > 3 * vals[1]:
                d = vecs[:, 2]
                lines.append(np.concatenate([sc[i, :3].astype(np.float64), 0.1 * d + c, -0.1 * d + c]))
    if len(ss):
        idx, d2 = oracle_py.knn_search(ms, rm.associate_to_map(ss, par), 5)
        for i in np.nonzero((idx[:, 4] >= 0) & (d2[:, 4] < np.float32(1.0)))[0]:
            near = ms[idx[i], :3].astype(np.float64)
            x = oracle_py.lstsq_5x3(near, -np.ones(5))
            ln = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
            d, n = 1 / ln, x / ln
            if all(abs(n[0] * p[0] + n[1] * p[1] + n[2] * p[2] + d) <= 0.2 for p in near):
                planes.append(np.concatenate([ss[i, :3].astype(np.float64), n, [d]]))
    return np.array(lines).reshape(-1, 9), np.array(planes).reshape(-1, 7)
