"""tools/graph_propose_rate.py — what one aloam_graph_propose_loops call costs, beside a device-to-device copy of the bytes its scan reads.

    python tools/graph_propose_rate.py [--repeats 5] [--cases 2048x256,512x1024,1x4096] [--all-nodes 4096] [--longest 1048576] [--host-nodes 4096] [--out FILE.json]

Every graph is the same chain of laps (40 nodes per lap of a 10 m circle with a slow climb, the ground truth of posegraph.drifted_laps),
entered with one aloam_graph_load of records made by graph_records.pack.  Shapes:
  - batch x nodes, the shapes of tools/pose_graph_rate.py, with one query per graph, its last node: the live case;
  - one graph of --all-nodes nodes with every node queried: the re-detection after a solve;
  - one query, the last node, on a graph of --longest nodes (default: the most aloam_graph_enable admits): a single long scan.
Parameters: radius 3 m, no growth, min_gap 20, half_window 3, separation 6, K = 4.  Each shape alternates, in one process, the call with a
device-to-device copy of 64 B per eligible node (a 128-byte node record is read for its 24 bytes of t: half of it is the least a scan can
fetch).  Milliseconds per call: `queue` is the host time of the call itself (it returns without waiting), `call` the host time until
aloam_synchronize returns, `stream` the hipEvent interval of the pose_graph profiling slot; `copy_stream` the event interval of the copy.
The host time of posegraph.propose_loops for one query on the --host-nodes chain stands beside them.  Prints one JSON object.
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

PARAMS = dict(radius_m=3.0, growth_m_per_node=0.0, min_gap=20, half_window=3, separation=6, K=4)


def laps_nodes(pg, n):
    k = np.arange(n)
    ang = 2.0 * np.pi * k / 40
    nodes = np.zeros(n, pg.NODE_DTYPE)
    nodes["t"] = nodes["t_opt"] = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), 0.002 * k], 1)
    yaw = ang + 0.5 * np.pi
    nodes["q"] = nodes["q_opt"] = np.stack([np.zeros(n), np.zeros(n), np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    nodes["frame"] = -1
    return nodes


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def shape(mods, name, batch, nodes, queries, repeats):
    torch, binding, pg, gr = mods
    rec = gr.pack(laps_nodes(pg, nodes), np.zeros(0, pg.EDGE_DTYPE))
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024)
    gpu.graph_enable(nodes, 1)
    gpu.graph_load(list(range(batch)), np.tile(rec, batch), len(rec) * np.arange(batch + 1, dtype=np.int64))
    gpu.synchronize()
    qs = np.ascontiguousarray(queries, np.int32)
    n, K = len(qs), PARAMS["K"]
    eligible = int(np.maximum(0, qs[:, 1] - PARAMS["min_gap"] + 1).sum())
    dst = torch.zeros(n * K * 96, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    d2 = torch.zeros(n * K, dtype=torch.float64, device="cuda")
    a = torch.zeros(max(64, 64 * eligible), dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows, copies = [], []
    for p in range(repeats + 1):                   # (pass 0 allocates the query ring and is not reported)
        gpu.synchronize()
        gpu.profile_enable(True)
        t0 = time.perf_counter()
        gpu.graph_propose_loops_into(qs, dst.data_ptr(), cnt.data_ptr(), d2.data_ptr(), **PARAMS)
        t1 = time.perf_counter()
        gpu.synchronize()
        t2 = time.perf_counter()
        prof = gpu.profile()["pose_graph"]
        gpu.profile_enable(False)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if p:
            rows.append((1e3 * (t1 - t0), 1e3 * (t2 - t0), prof["total_ms"]))
            copies.append(e0.elapsed_time(e1))
    counts = cnt.cpu().numpy()
    gpu.close()
    return {"shape": name, "batch": batch, "nodes": nodes, "queries": n, "eligible_nodes": eligible, "scan_bytes": 64 * eligible,
            "ms": {"queue": spread([r[0] for r in rows]), "call": spread([r[1] for r in rows]), "stream": spread([r[2] for r in rows])},
            "copy_stream_ms": spread(copies), "taken": {"min": int(counts.min()), "max": int(counts.max())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048x256,512x1024,1x4096", help="batch x nodes, comma-separated; one query per graph (the last node)")
    ap.add_argument("--all-nodes", type=int, default=4096, help="nodes of the one graph whose every node is queried (0 = skip)")
    ap.add_argument("--longest", type=int, default=1 << 20, help="nodes of the one graph whose last node is queried (0 = skip)")
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per shape")
    ap.add_argument("--host-nodes", type=int, default=4096, help="nodes of the chain posegraph.propose_loops is timed on (0 = skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    gr = importlib.import_module("a-loam_amd.graph_records")
    mods = (torch, binding, pg, gr)
    res = {"parameters": PARAMS, "shapes": []}
    for case in [c for c in args.cases.split(",") if c]:
        batch, nodes = (int(v) for v in case.split("x"))
        res["shapes"].append(shape(mods, "one query per graph", batch, nodes, [(s, nodes - 1) for s in range(batch)], args.repeats))
    if args.all_nodes:
        res["shapes"].append(shape(mods, "every node of one graph", 1, args.all_nodes, [(0, j) for j in range(args.all_nodes)], args.repeats))
    if args.longest:
        res["shapes"].append(shape(mods, "one query on the longest graph", 1, args.longest, [(0, args.longest - 1)], args.repeats))
    if args.host_nodes:
        nodes = laps_nodes(pg, args.host_nodes)
        t0 = time.perf_counter()
        _, count, _ = pg.propose_loops(nodes["q_opt"], nodes["t_opt"], args.host_nodes - 1, **PARAMS)
        res["host_propose_loops"] = {"nodes": args.host_nodes, "queries": 1, "taken": int(count), "ms": 1e3 * (time.perf_counter() - t0)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
