"""tools/graph_apply_rate.py — what one aloam_graph_apply call costs, beside aloam_graph_export_map of the same nodes.

    python tools/graph_apply_rate.py [--cases 64x256,8x2048,1x8192] [--repeats 5] [--out FILE.json]

The shapes and the keyframes are those of tools/graph_map_rate.py (sequences x keyframes; every sequence drives a straight line, one
synthetic HDL-64 stack of about 1.5 k corner and 6 k surf points every --spacing metres).  Then, in one process and alternated, --repeats
times each:
  export_ms  host clock around aloam_graph_export_map of all nodes of every sequence at the optimised poses into device memory + aloam_synchronize
  apply_ms   host clock around aloam_graph_apply of the same nodes (pose and map) + aloam_synchronize
An apply rebases the nodes and replaces the window, so every apply after the first finds D = identity and the same map: the same work.
The first apply, which also grows the map pools to the window's size, is timed on its own (first_apply_ms).  Prints one JSON object.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from graph_map_rate import stack_inputs  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default="64x256,8x2048,1x8192", help="sequences x keyframes, comma-separated")
    ap.add_argument("--repeats", type=int, default=5, help="timed calls of each kind per case, alternated (median, min and max are reported)")
    ap.add_argument("--spacing", type=float, default=2.0, help="metres between keyframes")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    res = {"cases": []}
    ident, zero = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    for case in args.cases.split(","):
        batch, frames = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(batch)
        gpu = binding.Aloam(n_scans=64, min_range=0.3, batch=batch, max_points=8192, lm_max_iterations=0)
        gpu.mapping_enable(0.4, 0.8, pool_points=1 << 16)
        gpu.graph_enable(frames, frames)
        gpu.graph_keyframes_enable(frames * 1600, frames * 6100)
        gpu.set_map_frozen([1] * batch)                     # the steps only make the stacks: nothing is inserted into the window maps
        ids = list(range(batch))
        for b in ids:
            corner, surf = stack_inputs(rng)
            gpu.set_last(corner, surf, b)
            gpu.set_full_cloud(surf[:4], b)
        x0 = -0.5 * args.spacing * frames
        for k in range(frames):
            for b in ids:
                gpu.set_state(ident, zero, ident, np.array([x0 + args.spacing * k, 60.0 * b, 0.0]), seq=b)
            gpu.mapping_step()
            gpu.graph_add_nodes(ids, np.eye(6) * 100.0)
        gpu.set_map_frozen(None)                            # an apply replaces the map: it has to be the sequence's own
        gpu.synchronize()
        reqs = gpu.graph_map_requests([(b, 0, frames, binding.GRAPH_POSE_OPTIMIZED) for b in ids])
        areqs = gpu.graph_apply_requests([(b, 0, frames, binding.GRAPH_APPLY_POSE | binding.GRAPH_APPLY_MAP) for b in ids])
        off = torch.zeros(2 * (batch + 1), dtype=torch.int64, pin_memory=True)
        gpu.graph_export_map_into(reqs, 0, 0, 0, 0, off.data_ptr())          # the size query (also allocates the scratch)
        gpu.synchronize()
        nt, npts = int(off[batch]), int(off[2 * batch + 1])
        tiles = torch.zeros(max(1, nt) * 32, dtype=torch.uint8, device="cuda")
        pts = torch.zeros((max(1, npts), 4), dtype=torch.float32, device="cuda")
        out = torch.zeros(batch * binding.GRAPH_APPLY_RESULT_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        t0 = time.perf_counter()
        gpu.graph_apply_into(areqs, out.data_ptr())
        gpu.synchronize()
        first_ms = 1e3 * (time.perf_counter() - t0)
        export_ms, apply_ms = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            gpu.graph_export_map_into(reqs, tiles.data_ptr(), nt, pts.data_ptr(), npts, off.data_ptr())
            gpu.synchronize()
            export_ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            gpu.graph_apply_into(areqs, out.data_ptr())
            gpu.synchronize()
            apply_ms.append(1e3 * (time.perf_counter() - t0))
        r = out.numpy().view(binding.GRAPH_APPLY_RESULT_DTYPE)
        pool = gpu.map_pool_info()
        res["cases"].append({"sequences": batch, "keyframes": frames, "tiles": nt, "points": npts, "applied": int((r["status"] == binding.GRAPH_APPLIED).sum()),
                             "window_cubes": int(r["cubes"].sum()), "window_points": int(r["points"].sum()), "outside_window": int(r["outside_window"].sum()),
                             "first_apply_ms": first_ms, "export_ms": spread(export_ms), "apply_ms": spread(apply_ms),
                             "pool_points": pool["pool_points"], "pool_growths": pool["growths"]})
        gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
