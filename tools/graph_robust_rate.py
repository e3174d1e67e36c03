"""tools/graph_robust_rate.py — what one aloam_graph_optimize_robust call costs, beside aloam_graph_optimize on the same graphs without
the false loops.

    python tools/graph_robust_rate.py [--false-loops 4] [--repeats 1] [--cases 2048x256x2,512x1024x5,1x4096x8] [--host-nodes 60] [--out FILE.json]

Per case (batch x nodes x loop edges, the shapes of tools/pose_graph_rate.py): every sequence gets the same drifted_laps graph
(a-loam_amd/posegraph.py), entered as a caller would.  A pass enters the graphs with their loops flagged robust and K false loops
(posegraph.false_loops) and times one robust call, then clears them, enters them again without the false loops and times one
aloam_graph_optimize: the two alternate in one process, and every timed solve starts from the drifted estimates.  Entering dominates the
tool's run time.  Milliseconds per call: `queue` is the host time of the call itself (it returns without waiting), `call` the host time
until aloam_synchronize returns, `stream` the hipEvent interval of the pose_graph profiling slot, which times both calls.  Outer, LM and
PCG iterations, the weights of the flagged edges and the status are those of sequence 0.  The host time of posegraph.optimize_robust
(dense numpy steps, one graph) on the --host-nodes graph with 3 false loops is the only baseline there is.  Prints one JSON object.
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


def enter(gpu, d, extra, batch):
    ids = list(range(batch))
    gpu.graph_clear(ids)
    ident, zero = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    for k in range(len(d["q"])):
        for b in ids:
            gpu.set_state(ident, zero, d["q"][k], d["t"][k], seq=b)
        gpu.graph_add_nodes(ids, d["info"])
    rows = []
    for b in ids:
        e = extra.copy()
        e["seq"] = b
        rows.append(e)
    gpu.graph_add_edges(np.concatenate(rows))


def timed(gpu, queue):
    """(queue ms, call ms, stream ms) of one queued call."""
    gpu.synchronize()
    gpu.profile_enable(True)
    t0 = time.perf_counter()
    queue()
    t1 = time.perf_counter()
    gpu.synchronize()
    t2 = time.perf_counter()
    prof = gpu.profile()["pose_graph"]
    gpu.profile_enable(False)
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0), prof["total_ms"] / prof["launches"]


def spread(rows, k):
    v = [r[k] for r in rows]
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048x256x2,512x1024x5,1x4096x8", help="batch x nodes x loops, comma-separated")
    ap.add_argument("--false-loops", type=int, default=4, help="K: false loops per graph, flagged robust beside the true ones")
    ap.add_argument("--repeats", type=int, default=1, help="timed passes per case (each enters the graphs twice)")
    ap.add_argument("--host-nodes", type=int, default=60, help="nodes of the graph posegraph.optimize_robust is timed on (0 = skip)")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    res = {"false_loops": args.false_loops, "cases": []}
    for case in args.cases.split(","):
        batch, nodes, loops = (int(v) for v in case.split("x"))
        d = pg.drifted_laps(1, nodes, loops)
        true = d["loop"].copy()
        true["flags"] = pg.EDGE_ROBUST
        false = pg.false_loops(d, args.false_loops, 101)
        E = nodes - 1 + loops + args.false_loops
        gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024)
        gpu.graph_enable(nodes, E)
        ids = list(range(batch))
        dst = torch.zeros(batch * 128, dtype=torch.uint8, device="cuda")
        wts = torch.zeros((batch, E), dtype=torch.float64, device="cuda")
        plain_dst = torch.zeros(batch * 64, dtype=torch.uint8, device="cuda")
        opt = gpu.graph_options(max_iterations=args.max_iterations)
        robust, plain, rec, prec, w0 = [], [], None, None, None
        for p in range(args.repeats + 1):          # (pass 0 allocates the scratch rows and is not reported)
            enter(gpu, d, np.concatenate([true, false]), batch)
            r = timed(gpu, lambda: gpu.graph_optimize_robust_into(ids, dst.data_ptr(), opt, None, wts.data_ptr(), E))
            rec = dst.cpu().numpy().view(binding.GRAPH_ROBUST_RESULT_DTYPE)
            w0 = wts[0].cpu().numpy()
            enter(gpu, d, d["loop"], batch)
            q = timed(gpu, lambda: gpu.graph_optimize_into(ids, plain_dst.data_ptr(), opt))
            prec = plain_dst.cpu().numpy().view(binding.GRAPH_RESULT_DTYPE)
            if p:
                robust.append(r); plain.append(q)
        same = bool(all(rec[b].tobytes() == rec[0].tobytes() for b in range(batch)))
        res["cases"].append({"batch": batch, "nodes": nodes, "loops": loops,
                             "robust_ms": {"queue": spread(robust, 0), "call": spread(robust, 1), "stream": spread(robust, 2)},
                             "plain_ms": {"queue": spread(plain, 0), "call": spread(plain, 1), "stream": spread(plain, 2)},
                             "outer_iterations": int(rec[0]["outer_iterations"]), "lm_iterations": int(rec[0]["solve"]["lm_iterations"]),
                             "pcg_iterations": int(rec[0]["solve"]["pcg_iterations"]), "status": int(rec[0]["solve"]["status"]),
                             "inliers": int(rec[0]["inliers"]), "outliers": int(rec[0]["outliers"]), "weights": w0[nodes - 1:].tolist(),
                             "plain_lm_iterations": int(prec[0]["lm_iterations"]), "plain_pcg_iterations": int(prec[0]["pcg_iterations"]),
                             "all_records_equal": same})
        gpu.close()
    if args.host_nodes:
        d = pg.drifted_laps(7, args.host_nodes, 2)
        true = d["loop"].copy()
        true["flags"] = pg.EDGE_ROBUST
        edges = np.concatenate([d["odom"], true, pg.false_loops(d, 3, 107)])
        t0 = time.perf_counter()
        _, _, r = pg.optimize_robust(d["q"], d["t"], edges, max_iterations=args.max_iterations)
        res["host_optimize_robust"] = {"nodes": args.host_nodes, "loops": 2, "false_loops": 3, "seconds": time.perf_counter() - t0,
                                       "outer_iterations": r["outer_iterations"], "lm_iterations": r["lm_iterations"]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
