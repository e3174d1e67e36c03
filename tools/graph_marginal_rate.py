"""tools/graph_marginal_rate.py — what one aloam_graph_marginals call costs.

    python tools/graph_marginal_rate.py [--shapes 256x2,1024x5,4096x8] [--requests 1,256,2048] [--repeats 3] [--host-nodes 1024] [--out FILE.json]

Per shape (nodes x loop edges, the graphs of tools/pose_graph_rate.py): one drifted_laps graph (a-loam_amd/posegraph.py) is entered into
sequence 0 of a batch-1 context as a caller would and solved once with aloam_graph_optimize.  The requests all name that sequence - a
(seq, i, j) may be listed any number of times, and every request linearises the graph for itself, so n requests cost what n sequences would:
candidate loop edges (i, j) drawn with a seeded generator, measured on the ground truth with the graph's information, mode MEASURED.  Per
request count, milliseconds per call, median of --repeats after one untimed call (which allocates the scratch rows):
    queueing  the host time of the call, which returns once its rounds are queued
    whole     the same call followed by aloam_synchronize
    stream    the hipEvent interval of the graph_marginals profiling slot
with the rounds the call took, the PCG iterations of the first request and the largest chi2.  The host time of posegraph.marginals (dense,
one request, graphs of up to --host-nodes nodes) stands beside them.  Prints one JSON object.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2,1024x5,4096x8", help="nodes x loops, comma-separated")
    ap.add_argument("--requests", default="1,256,2048", help="requests per call, comma-separated")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per request count")
    ap.add_argument("--host-nodes", type=int, default=1024, help="largest graph posegraph.marginals is timed on (0 = skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    ident, zero = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    res = {"shapes": []}
    for shape in args.shapes.split(","):
        nodes, loops = (int(v) for v in shape.split("x"))
        d = pg.drifted_laps(1, nodes, loops)
        gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=1024)
        gpu.graph_enable(nodes, nodes + loops)
        for k in range(nodes):
            gpu.set_state(ident, zero, d["q"][k], d["t"][k], seq=0)
            gpu.graph_add_nodes([0], d["info"])
        gpu.graph_add_edges(d["loop"])
        solve = gpu.graph_optimize([0])[0]
        rng = np.random.default_rng(nodes)
        row = 8 * (200 * nodes + 115 * (nodes - 1 + loops)) + 4 * (3 * nodes + 1 + 2 * (nodes - 1 + loops))
        entry = {"nodes": nodes, "loops": loops, "solve_status": int(solve["status"]), "scratch_row_bytes": row, "calls": []}
        for n in (int(v) for v in args.requests.split(",")):
            i = rng.integers(0, nodes, n)
            j = (i + rng.integers(1, nodes, n)) % nodes
            zq, zt = pg.relative_pose(d["q_true"][i], d["t_true"][i], d["q_true"][j], d["t_true"][j])
            req = pg.marginal_request(0, i, j, zq, zt, np.tile(d["info"], (n, 1, 1)))
            dst = torch.zeros(n * binding.GRAPH_MARGINAL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            gpu.graph_marginals_into(req, dst.data_ptr())                       # allocates the rows
            gpu.synchronize()
            queue, whole, stream = [], [], []
            for _ in range(args.repeats):
                gpu.profile_enable(True)
                t0 = time.perf_counter()
                gpu.graph_marginals_into(req, dst.data_ptr())
                t1 = time.perf_counter()
                gpu.synchronize()
                t2 = time.perf_counter()
                prof = gpu.profile()["graph_marginals"]
                queue.append(1e3 * (t1 - t0)); whole.append(1e3 * (t2 - t0)); stream.append(prof["total_ms"] / prof["launches"])
            gpu.profile_enable(False)
            rec = dst.cpu().numpy().view(binding.GRAPH_MARGINAL_RESULT_DTYPE)
            rows = max(1, min(n, 1024, (1 << 30) // row))
            entry["calls"].append({"requests": n, "rounds": -(-n // rows), "queueing_ms": float(np.median(queue)), "whole_call_ms": float(np.median(whole)),
                                   "stream_ms": float(np.median(stream)), "stream_ms_min_max": [min(stream), max(stream)],
                                   "statuses": sorted(set(int(s) for s in rec["status"])), "pcg_iterations_first": int(rec[0]["pcg_iterations"]),
                                   "chi2_max": float(rec["chi2"].max())})
        if args.host_nodes and nodes <= args.host_nodes:
            out = gpu.graph_export(0)
            edges = gpu.graph_export(0, edges=True)
            t0 = time.perf_counter()
            m = pg.marginals(out["q_opt"], out["t_opt"], edges, req["edge"][:1])
            entry["host_marginals_one_request_s"] = time.perf_counter() - t0
            entry["host_chi2_first"] = float(m["chi2"][0])
            entry["device_chi2_first"] = float(rec[0]["chi2"])
        gpu.close()
        res["shapes"].append(entry)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
