"""tools/graph_trim_rate.py — what one aloam_graph_trim call costs, beside a device-to-device copy of the bytes it moves.

    python tools/graph_trim_rate.py [--repeats 3] [--cases 2048x256,512x1024,1x4096] [--points 8,32] [--out FILE.json]

Every graph is the same chain of laps (40 nodes per lap of a 10 m circle, the ground truth of posegraph.drifted_laps) with an odometry edge
per node and a loop edge to the node one lap earlier, and every node holds --points corner and surf points.  The graphs are entered with one
aloam_graph_load of records made by graph_records.pack, and entered again (aloam_graph_clear, aloam_graph_load; not timed) before every
timed call, since a trim changes them.  Shapes: batch x nodes, the three of tools/pose_graph_rate.py, every sequence listed in one call.  Two
trims per shape: `half` drops the older half of the nodes (the head kernel moves every point, the tail kernel exits at once), `tenth`
drops a tenth (the head moves a ninth of the points that stay, the tail's one workgroup per row the rest).  Each alternates, in one process,
the call with a device-to-device copy of half the call's algorithmic bytes (a copy reads and writes each of its bytes once, like the trim).
Milliseconds per call: `call` is the host time of the whole call (it synchronises once), `stream` the hipEvent interval of the pose_graph
profiling slot (the three kernels), `queue` their difference - the host's share: checks, staging, queueing and the wake-up behind the
synchronise, which cannot be told apart from outside the call; `copy_stream` the event interval of the copy.  Prints one JSON object.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LAP = 40


def laps_graph(pg, n, points):
    k = np.arange(n)
    ang = 2.0 * np.pi * k / LAP
    nodes = np.zeros(n, pg.NODE_DTYPE)
    nodes["t"] = nodes["t_opt"] = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), 0.002 * k], 1)
    yaw = ang + 0.5 * np.pi
    nodes["q"] = nodes["q_opt"] = np.stack([np.zeros(n), np.zeros(n), np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    nodes["frame"] = k
    i = np.concatenate([k[:-1], k[LAP:] - LAP])
    j = np.concatenate([k[1:], k[LAP:]])
    qz, tz = pg.relative_pose(nodes["q"][i], nodes["t"][i], nodes["q"][j], nodes["t"][j])
    edges = pg.make_edges(0, i, j, qz, tz, np.eye(6) * 100.0)
    rng = np.random.default_rng(1)
    kf = tuple((rng.uniform(-20, 20, (n * p, 4)).astype(np.float32), p * np.arange(n + 1, dtype=np.int64)) for p in points)
    return nodes, edges, kf


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def shape(mods, batch, nodes, points, repeats):
    torch, binding, pg, gr = mods
    n, e, kf = laps_graph(pg, nodes, points)
    rec = gr.pack(n, e, kf, (0.4, 0.8))
    blob, off = np.tile(rec, batch), len(rec) * np.arange(batch + 1, dtype=np.int64)
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024)
    gpu.mapping_enable(0.4, 0.8, pool_points=1 << 12)      # the least it admits: the keyframe store needs mapping enabled, the tool maps nothing
    gpu.graph_enable(nodes, len(e))
    gpu.graph_keyframes_enable(max(1, nodes * points[0]), max(1, nodes * points[1]))
    seqs = list(range(batch))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {"batch": batch, "nodes": nodes, "edges": len(e), "points_per_node": list(points), "record_bytes": len(rec), "trims": {}}
    for name, first in (("half", nodes // 2), ("tenth", max(1, nodes // 10))):
        rows, copies, result, moved = [], [], None, 0
        for p in range(repeats + 1):                   # (pass 0 allocates the item ring and is not reported)
            gpu.graph_clear(seqs)
            gpu.graph_load(seqs, blob, off)
            gpu.synchronize()
            gpu.profile_enable(True)
            t0 = time.perf_counter()
            result = gpu.graph_trim(seqs, first)
            t1 = time.perf_counter()
            prof = gpu.profile()["pose_graph"]
            gpu.profile_enable(False)
            moved = int(prof["bytes_per_launch"])
            a = torch.zeros(max(64, moved // 2), dtype=torch.uint8, device="cuda")
            b = torch.zeros_like(a)
            torch.cuda.synchronize()
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            if p:
                rows.append((1e3 * (t1 - t0), prof["total_ms"]))
                copies.append(e0.elapsed_time(e1))
            del a, b
        assert (result == result[0]).all()
        out["trims"][name] = {"first": first, "result": result[0].tolist(), "algorithmic_bytes": moved,
                              "ms": {"queue": spread([r[0] - r[1] for r in rows]), "call": spread([r[0] for r in rows]), "stream": spread([r[1] for r in rows])}, "copy_stream_ms": spread(copies)}
    gpu.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048x256,512x1024,1x4096", help="batch x nodes, comma-separated; every sequence is trimmed in one call")
    ap.add_argument("--points", default="8,32", help="corner,surf points every node holds")
    ap.add_argument("--repeats", type=int, default=3, help="timed passes per shape and trim")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    gr = importlib.import_module("a-loam_amd.graph_records")
    points = tuple(int(v) for v in args.points.split(","))
    res = {"shapes": []}
    for case in [c for c in args.cases.split(",") if c]:
        batch, nodes = (int(v) for v in case.split("x"))
        res["shapes"].append(shape((torch, binding, pg, gr), batch, nodes, points, args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
