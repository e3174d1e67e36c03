"""Coarse relocalization in a prior map: a grid of map <- odometry corrections around a guess, scored on the device against the state one
frozen mapping step has left (aloam_score_map_corrections), the best one installed in stream order (aloam_apply_map_corrections).

The grid is pure numpy.  A frozen step refines a guess within about 1 m and 2.5 deg of yaw of the truth; the grid's job is to
put one node inside that basin, the score's job to find it."""
from __future__ import annotations

import math

import numpy as np


def _qmul(a, b):
    """Hamilton product a * b, (x, y, z, w) storage; a and b broadcast over leading axes."""
    x1, y1, z1, w1 = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    x2, y2, z2, w2 = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=-1)


def _qrot(q, v):
    q = np.asarray(q, np.float64)
    v = np.asarray(v, np.float64)
    vq = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], axis=-1)
    return _qmul(_qmul(q, vq), q * np.array([-1.0, -1.0, -1.0, 1.0]))[..., :3]


def grid_axes(radius_m, step_m, yaw_deg, yaw_step_deg):
    """The node values of the grid: (offsets along x and along y in metres, yaw offsets in degrees), each symmetric about 0."""
    m = int(math.floor(radius_m / step_m + 1e-9)) if step_m > 0 else 0
    a = int(math.floor(yaw_deg / yaw_step_deg + 1e-9)) if yaw_step_deg > 0 else 0
    return np.arange(-m, m + 1) * float(step_m), np.arange(-a, a + 1) * float(yaw_step_deg)


def correction_grid(guess_q, guess_t, sensor_t, radius_m, step_m, yaw_deg, yaw_step_deg):
    """Corrections (q [K, 4], t [K, 3], nodes [K, 3] = dx, dy in metres and dyaw in degrees) that turn the guess (guess_q, guess_t:
    map <- odometry) by dyaw about the vertical through the sensor position sensor_t (in the map frame) and then shift it by (dx, dy, 0).
    Order: yaw outermost, then y, then x.  The node (0, 0, 0) is the guess itself, bit for bit.  Roll, pitch and z are not searched."""
    guess_q, guess_t, c = np.asarray(guess_q, np.float64), np.asarray(guess_t, np.float64), np.asarray(sensor_t, np.float64)
    lin, yaw = grid_axes(radius_m, step_m, yaw_deg, yaw_step_deg)
    qs, ts, nodes = [], [], []
    for dyaw in yaw:
        if dyaw == 0.0:
            q, base = guess_q.copy(), guess_t.copy()
        else:
            h = math.radians(float(dyaw)) / 2
            dq = np.array([0.0, 0.0, math.sin(h), math.cos(h)])
            q, base = _qmul(dq, guess_q), _qrot(dq, guess_t - c) + c
        for dy in lin:
            for dx in lin:
                t = base.copy()
                if dx != 0.0:
                    t[0] += dx
                if dy != 0.0:
                    t[1] += dy
                qs.append(q); ts.append(t); nodes.append((dx, dy, dyaw))
    return np.array(qs), np.array(ts), np.array(nodes)


def relocalize(gpu, seqs, radius_m=3.5, step_m=0.5, yaw_deg=12.5, yaw_step_deg=2.5, guesses=None):
    """Search around each listed sequence's guess and install the best node.  Every sequence must have just taken a frozen mapping step
    (that step's stacks, odometry pose and submap are what is scored).  guesses: {seq: (q_wmap_wodom, t_wmap_wodom)}; a sequence without
    one is searched around the correction it holds now.  Each sequence has a grid of its own (the grid turns about its sensor), so one
    scoring call and one apply are queued per sequence, the apply reading `best` on the device; one synchronise at the end.
    Returns {seq: {"nodes", "q", "t", "scores", "best"}}."""
    import torch

    from . import binding
    out, keep = {}, []
    for s in seqs:
        if guesses is not None and s in guesses:
            gq, gt = (np.asarray(v, np.float64) for v in guesses[s])
        else:
            p = gpu.map_pose(s)
            gq, gt = p["q_wmap_wodom"], p["t_wmap_wodom"]
        sensor = _qrot(gq, gpu.pose(s)["t_w"]) + gt                       # where the guess puts the sensor: transformAssociateToMap
        q, t, nodes = correction_grid(gq, gt, sensor, radius_m, step_m, yaw_deg, yaw_step_deg)
        cand = binding.map_corrections(q, t)
        sc = torch.zeros(len(cand) * 32, dtype=torch.uint8).pin_memory()
        best = torch.zeros(1, dtype=torch.int32).pin_memory()
        gpu.score_map_corrections_into([s], cand.ctypes.data, len(cand), sc.data_ptr(), best.data_ptr())
        gpu.apply_map_corrections_from([s], cand.ctypes.data, len(cand), best.data_ptr())
        keep.append(cand)
        out[s] = {"nodes": nodes, "q": q, "t": t, "_sc": sc, "_best": best}
    gpu.synchronize()
    for s, r in out.items():
        r["scores"] = r.pop("_sc").numpy().view(binding.MAP_SCORE_DTYPE).copy()
        r["best"] = int(r.pop("_best")[0])
    return out
