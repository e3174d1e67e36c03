"""tools/graph_map_rate.py — what one aloam_graph_export_map call costs.

    python tools/graph_map_rate.py [--cases 64x256,8x2048,1x8192] [--repeats 5] [--host-keyframes 64] [--joint M] [--out FILE.json]

Per case (sequences x keyframes): every sequence drives a straight line, one keyframe every --spacing metres; each keyframe is a synthetic
HDL-64 stack of about 1.5 k corner and 6 k surf points (random returns in an 80 m square, fed with aloam_set_last, down-sampled by a frozen
mapping step with the solver off), entered with aloam_graph_add_nodes.  Then one request per sequence for all of its nodes at the entered
poses, into device memory: a size query, and --repeats timed calls.  Reported per case, in milliseconds:
  call_ms    host clock around aloam_graph_export_map + aloam_synchronize (the whole call, its one synchronisation and read-back included)
  stream_ms  hipEvent intervals of the graph_map profiling slot: the stream-ordered parts (transform; grouping, voxel filter and emit)
  hbm_ms     the call's algorithmic bytes at the 8 TB/s HBM peak
With --joint M the sequences are also taken M at a time as one group of M parts (aloam_graph_export_map_joint, frame -1; the last group
takes what is left), timed the same way and alternated, call by call, with the per-request call over the same nodes: the pieces are the
same, so the two differ by the filter seeing merged cubes (neighbouring sequences drive 60 m apart and share cubes).  Reported under "joint".
The host time of the model (atlas.tiles_from_keyframes with a numpy voxel filter) on --host-keyframes keyframes of one sequence is printed
beside them.  Prints one JSON object.
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

HBM_PEAK = 8.0e12
LEAF = (0.4, 0.8)


def stack_inputs(rng, n_corner=1500, n_surf=6000):
    def make(n):
        p = np.zeros((n, 4), np.float32)
        p[:, 0:2] = rng.uniform(-40.0, 40.0, (n, 2))
        p[:, 2] = rng.uniform(-2.0, 4.0, n)
        p[:, 3] = np.sort(rng.integers(0, 64, n))
        return p
    return make(n_corner), make(n_surf)


def numpy_voxel_filter(p, leaf):
    """Centroid per occupied leaf, leaves ascending: what the model is timed with (not the oracle's bits)."""
    cell = np.floor(p[:, :3] / np.float32(leaf)).astype(np.int64)
    cell -= cell.min(0)
    dim = cell.max(0) + 1
    key = cell[:, 0] + dim[0] * (cell[:, 1] + dim[1] * cell[:, 2])
    order = np.argsort(key, kind="stable")
    _, start, count = np.unique(key[order], return_index=True, return_counts=True)
    return (np.add.reduceat(p[order].astype(np.float64), start, 0) / count[:, None]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default="64x256,8x2048,1x8192", help="sequences x keyframes, comma-separated")
    ap.add_argument("--repeats", type=int, default=5, help="timed calls per case (median, min and max are reported)")
    ap.add_argument("--spacing", type=float, default=2.0, help="metres between keyframes")
    ap.add_argument("--host-keyframes", type=int, default=64, help="keyframes of one sequence the numpy model is timed on (0 = skip)")
    ap.add_argument("--joint", type=int, default=0, metavar="M", help="also time aloam_graph_export_map_joint with the sequences taken M at a time as one group of M parts (0 = off)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    atlas = importlib.import_module("a-loam_amd.atlas")
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
        gpu.synchronize()
        held = gpu.graph_keyframe_info(0)
        reqs = gpu.graph_map_requests([(b, 0, frames, binding.GRAPH_POSE_ENTERED) for b in ids])
        calls = [("request", batch, lambda *dst: gpu.graph_export_map_into(reqs, *dst))]
        if args.joint > 0:
            lists = gpu.graph_map_groups([([(b, 0, frames, -1) for b in ids[g:g + args.joint]], binding.GRAPH_POSE_ENTERED) for g in range(0, batch, args.joint)])
            calls.append(("joint", len(lists[1]), lambda *dst: gpu.graph_export_map_joint_into(lists, *dst)))
        sized = []
        for name, n, call in calls:                         # a size query each, then the destinations in device memory
            off = torch.zeros(2 * (n + 1), dtype=torch.int64, pin_memory=True)
            t0 = time.perf_counter()
            call(0, 0, 0, 0, off.data_ptr())
            gpu.synchronize()
            query_ms = 1e3 * (time.perf_counter() - t0)     # (the first call also allocates the scratch)
            nt, npts = int(off[n]), int(off[2 * n + 1])
            sized.append({"name": name, "n": n, "call": call, "off": off, "query_ms": query_ms, "nt": nt, "npts": npts,
                          "tiles": torch.zeros(max(1, nt) * 32, dtype=torch.uint8, device="cuda"), "pts": torch.zeros((max(1, npts), 4), dtype=torch.float32, device="cuda"),
                          "stats": torch.zeros(n * 32, dtype=torch.uint8, pin_memory=True), "call_ms": [], "stream_ms": [], "bytes": 0.0})
        for _ in range(args.repeats):                       # alternated, call by call, in this one process
            for c in sized:
                gpu.profile_enable(True)
                t0 = time.perf_counter()
                c["call"](c["tiles"].data_ptr(), c["nt"], c["pts"].data_ptr(), c["npts"], c["off"].data_ptr(), c["stats"].data_ptr())
                gpu.synchronize()
                c["call_ms"].append(1e3 * (time.perf_counter() - t0))
                prof = gpu.profile()["graph_map"]
                c["stream_ms"].append(prof["total_ms"])
                c["bytes"] = prof["bytes_per_launch"]
        gpu.profile_enable(False)

        def figures(c):
            st = c["stats"].numpy().view(binding.GRAPH_MAP_STATS_DTYPE)
            return {"raw_points": int(st["raw_points"].sum()), "tiles": c["nt"], "points": c["npts"], "written": int(st["written"].sum()), "size_query_ms": c["query_ms"],
                    "call_ms": {"median": float(np.median(c["call_ms"])), "min": min(c["call_ms"]), "max": max(c["call_ms"])},
                    "stream_ms": {"median": float(np.median(c["stream_ms"])), "min": min(c["stream_ms"]), "max": max(c["stream_ms"])},
                    "algorithmic_bytes": c["bytes"], "hbm_ms": 1e3 * c["bytes"] / HBM_PEAK}
        row = {"sequences": batch, "keyframes": frames, "points_per_keyframe": [held["points"][0] / frames, held["points"][1] / frames]}
        row.update(figures(sized[0]))
        if args.joint > 0:
            row["joint"] = dict(figures(sized[1]), groups=sized[1]["n"], parts_per_group=min(args.joint, batch))
        row["pool_points"] = gpu.map_pool_info()["pool_points"]
        res["cases"].append(row)
        if args.host_keyframes and "host_model" not in res:
            n = min(args.host_keyframes, frames)
            nodes = gpu.graph_export(0, 0, n)
            clouds = []
            for cls in (0, 1):
                p, o = gpu.graph_export_keyframes(0, 0, n, cls)
                clouds.append([p[o[k]:o[k + 1]] for k in range(n)])
            t0 = time.perf_counter()
            mt, mp = atlas.tiles_from_keyframes(nodes["q"], nodes["t"], list(zip(*clouds)), LEAF, numpy_voxel_filter)
            res["host_model"] = {"keyframes": n, "seconds": time.perf_counter() - t0, "tiles": len(mt), "points": len(mp)}
        gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
