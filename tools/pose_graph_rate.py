"""tools/pose_graph_rate.py — what one aloam_graph_optimize call costs.

    python tools/pose_graph_rate.py [--repeats 1] [--cases 2048x256x2,512x1024x5,1x4096x8] [--host-nodes 256] [--out FILE.json]

Per case (batch x nodes x loop edges): every sequence gets the same drifted_laps graph (a-loam_amd/posegraph.py), entered as a caller
would: the pose of a keyframe injected with aloam_set_state, one aloam_graph_add_nodes per keyframe for the whole batch, the loop edges
with one aloam_graph_add_edges.  Entering dominates the tool's run time (a set_state per sequence and keyframe); a pass clears the graphs
and enters them again, so that every timed solve starts from the drifted estimates.  Milliseconds per call are hipEvent intervals of the
pose_graph profiling slot (allocations happen before it); LM and PCG iterations are those of sequence 0's result record.  The host time of posegraph.optimize (dense numpy LM, one graph) on the
--host-nodes graph is the only baseline there is.  Prints one JSON object.
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


def enter(gpu, pg, d, batch):
    ids = list(range(batch))
    gpu.graph_clear(ids)
    ident, zero = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    for k in range(len(d["q"])):
        for b in ids:
            gpu.set_state(ident, zero, d["q"][k], d["t"][k], seq=b)
        gpu.graph_add_nodes(ids, d["info"])
    loops = []
    for b in ids:
        e = d["loop"].copy()
        e["seq"] = b
        loops.append(e)
    gpu.graph_add_edges(np.concatenate(loops))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048x256x2,512x1024x5,1x4096x8", help="batch x nodes x loops, comma-separated")
    ap.add_argument("--repeats", type=int, default=1, help="timed passes per case (each enters the graphs again)")
    ap.add_argument("--host-nodes", type=int, default=256, help="nodes of the graph posegraph.optimize is timed on (0 = skip)")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    res = {"cases": []}
    for case in args.cases.split(","):
        batch, nodes, loops = (int(v) for v in case.split("x"))
        d = pg.drifted_laps(1, nodes, loops)
        gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024)
        gpu.graph_enable(nodes, nodes + loops)
        dst = torch.zeros(batch * 64, dtype=torch.uint8, device="cuda")
        opt = gpu.graph_options(max_iterations=args.max_iterations)
        ms, rec = [], None
        for p in range(args.repeats):
            enter(gpu, pg, d, batch)
            gpu.profile_enable(True)
            gpu.graph_optimize_into(list(range(batch)), dst.data_ptr(), opt)
            prof = gpu.profile()["pose_graph"]
            ms.append(prof["total_ms"] / prof["launches"])
            rec = dst.cpu().numpy().view(binding.GRAPH_RESULT_DTYPE)
        gpu.profile_enable(False)
        same = bool(all(rec[b].tobytes() == rec[0].tobytes() for b in range(batch)))
        res["cases"].append({"batch": batch, "nodes": nodes, "loops": loops, "ms_per_call": {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)},
                             "lm_iterations": int(rec[0]["lm_iterations"]), "accepted_steps": int(rec[0]["accepted_steps"]),
                             "pcg_iterations": int(rec[0]["pcg_iterations"]), "termination": int(rec[0]["termination"]), "status": int(rec[0]["status"]),
                             "initial_cost": float(rec[0]["initial_cost"]), "final_cost": float(rec[0]["final_cost"]), "all_records_equal": same})
        gpu.close()
    if args.host_nodes:
        d = pg.drifted_laps(1, args.host_nodes, 2)
        edges = np.concatenate([d["odom"], d["loop"]])
        t0 = time.perf_counter()
        _, _, r = pg.optimize(d["q"], d["t"], edges, max_iterations=args.max_iterations)
        res["host_optimize"] = {"nodes": args.host_nodes, "loops": 2, "seconds": time.perf_counter() - t0, "lm_iterations": r["lm_iterations"]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
