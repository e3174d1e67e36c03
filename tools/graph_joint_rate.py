"""tools/graph_joint_rate.py — what one aloam_graph_optimize_joint call costs, beside aloam_graph_optimize of the same graph held as one
sequence and beside a device-to-device copy of the bytes the gather moves.

    python tools/graph_joint_rate.py [--repeats 3] [--cases 2048x256x2,512x1024x5,1x4096x8] [--members 2,8] [--max-iterations 20] [--out FILE.json]

Per case (batch x nodes x loop edges, the three shapes of tools/pose_graph_rate.py) and per member count M: `batch` groups, each the
drifted_laps graph of `nodes` nodes cut into M sessions of nodes / M nodes; every session after the first is expressed in a frame of its
own (rotated by 2 rad, moved by 100 m times its index), the edges that cross a cut are the group's links, the cut odometry edges first.  A
second context holds the uncut graph once per group.  Graphs are entered with one aloam_graph_load of records made by graph_records.pack
and entered again (not timed) before every timed call, since a solve changes them.  In one process, alternating per pass:
  joint     aloam_graph_optimize_joint with align set for every member but the first
  in_frame  the same with every session entered in the first one's frame and no align (the iterations without an alignment)
  single    aloam_graph_optimize of the uncut graphs
  moves     the joint call and the single call with max_iterations = 0; their difference is the gather and the scatter alone
  copy      a device-to-device copy of 128 B per node and 240 B per joined edge
Milliseconds per call: `queue` is the host time until the C call returns (checks, staging, the launches; the four lists are built
once, outside it), `call` until the stream has drained, `stream` the hipEvent interval of the pose_graph profiling slot (gather, solve,
scatter).  LM and PCG iterations are those of group 0.  Prints one JSON object.
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


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def sessions(pg, g, M, moved):
    """The graph g cut into M sessions: [(nodes, edges)] and the links with seq_i / seq_j = the session's index.  moved: every session
    after the first in a frame of its own."""
    N = len(g["q"])
    cuts = [N * m // M for m in range(M + 1)]
    of = np.searchsorted(cuts, np.arange(N), side="right") - 1
    edges = np.concatenate([g["odom"], g["loop"]])
    si, sj = of[edges["i"]], of[edges["j"]]
    axis = np.array([0.3, -1.1, 2.0]) / np.linalg.norm([0.3, -1.1, 2.0])
    members = []
    for m in range(M):
        q, t = g["q"][cuts[m]:cuts[m + 1]], g["t"][cuts[m]:cuts[m + 1]]
        if moved and m:
            q, t = pg.compose(pg.qexp(2.0 * axis), np.array([100.0 * m, -40.0, 7.0]), q, t)
        e = edges[(si == m) & (sj == m)].copy()
        e["i"] -= cuts[m]; e["j"] -= cuts[m]
        members.append((pg.graph_nodes(q, t, frame=np.arange(cuts[m], cuts[m + 1])), e))
    cross = np.flatnonzero(si != sj)
    cross = np.concatenate([cross[edges["j"][cross] - edges["i"][cross] == 1], cross[edges["j"][cross] - edges["i"][cross] != 1]]).astype(np.int64)
    x = edges[cross]
    starts = np.array(cuts)
    links = pg.make_links(of[x["i"]], x["i"] - starts[of[x["i"]]], of[x["j"]], x["j"] - starts[of[x["j"]]], x["q"], x["t"], x["info"], x["flags"] != 0)
    return members, links, (pg.graph_nodes(g["q"], g["t"], frame=np.arange(N)), edges)


def timed(gpu, fn):
    gpu.synchronize()
    gpu.profile_enable(True)
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    gpu.synchronize()
    t2 = time.perf_counter()
    prof = gpu.profile()["pose_graph"]
    gpu.profile_enable(False)
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0), prof["total_ms"]


def shape(mods, batch, nodes, loops, M, repeats, max_iterations):
    torch, binding, pg, gr = mods
    g = pg.drifted_laps(1, nodes, loops)
    versions = {name: sessions(pg, g, M, moved) for name, moved in (("joint", True), ("in_frame", False))}
    members, links, whole = versions["joint"]
    most_nodes, most_edges = max(len(n) for n, _ in members), max(1, max(len(e) for _, e in members))
    parts = binding.Aloam(n_scans=16, min_range=0.3, batch=batch * M, max_points=1024)
    parts.graph_enable(most_nodes, most_edges)
    one = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024)
    one.graph_enable(nodes, len(whole[1]))
    blobs = {}
    for name, (mem, _, _) in versions.items():
        recs = [gr.pack(n, e) for n, e in mem]
        blob = np.concatenate(recs * batch)
        blobs[name] = blob, np.concatenate([[0], np.cumsum([len(r) for r in recs] * batch)]).astype(np.int64)
    rec = gr.pack(*whole)
    whole_blob = np.tile(rec, batch), len(rec) * np.arange(batch + 1, dtype=np.int64)

    def groups_of(lk, align):
        out = []
        for b in range(batch):
            l = lk.copy()
            l["seq_i"] += b * M; l["seq_j"] += b * M
            out.append((list(range(b * M, b * M + M)), l, [0] + [1] * (M - 1) if align else None))
        return out
    lists = {name: binding.Aloam.joint_lists(groups_of(versions[name][1], name == "joint")) for name in versions}   # built once: the timed region is the C call
    dst = torch.zeros(batch * 64, dtype=torch.uint8, device="cuda")
    joined_edges = sum(len(e) for _, e in members) + len(links)
    copy_bytes = batch * (128 * nodes + 240 * joined_edges)
    a = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = {k: [] for k in ("joint", "in_frame", "single", "joint_moves", "single_moves")}
    copies, records = [], {}
    for p in range(repeats + 1):                       # (pass 0 allocates the rings and the scratch rows and is not reported)
        for name, iters in (("joint", max_iterations), ("in_frame", max_iterations), ("joint_moves", 0)):
            which = "in_frame" if name == "in_frame" else "joint"
            parts.graph_clear(list(range(batch * M)))
            parts.graph_load(list(range(batch * M)), *blobs[which])
            opt = parts.graph_options(max_iterations=iters)
            r = timed(parts, lambda: parts.graph_optimize_joint_into(lists[which], dst.data_ptr(), opt))
            records[name] = dst.cpu().numpy().view(binding.GRAPH_RESULT_DTYPE).copy()
            if p: rows[name].append(r)
        for name, iters in (("single", max_iterations), ("single_moves", 0)):
            one.graph_clear(list(range(batch)))
            one.graph_load(list(range(batch)), *whole_blob)
            opt = one.graph_options(max_iterations=iters)
            r = timed(one, lambda: one.graph_optimize_into(list(range(batch)), dst.data_ptr(), opt))
            records[name] = dst.cpu().numpy().view(binding.GRAPH_RESULT_DTYPE).copy()
            if p: rows[name].append(r)
        torch.cuda.synchronize()
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        if p: copies.append(e0.elapsed_time(e1))
    parts.close(); one.close()

    def ms(name):
        return {"queue": spread([r[0] for r in rows[name]]), "call": spread([r[1] for r in rows[name]]), "stream": spread([r[2] for r in rows[name]])}

    def its(name):
        r = records[name][0]
        return {k: int(r[k]) for k in ("status", "termination", "lm_iterations", "accepted_steps", "pcg_iterations")} | {"final_cost": float(r["final_cost"])}
    moves = [j[2] - s[2] for j, s in zip(rows["joint_moves"], rows["single_moves"])]
    return {"batch": batch, "nodes": nodes, "loops": loops, "members": M, "links": len(links), "joined_edges": joined_edges, "gathered_bytes": copy_bytes,
            "ms": {k: ms(k) for k in rows}, "gather_scatter_stream_ms": spread(moves), "copy_stream_ms": spread(copies),
            "iterations": {k: its(k) for k in ("joint", "in_frame", "single")},
            "all_groups_equal": bool(all(x.tobytes() == records["joint"][0].tobytes() for x in records["joint"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048x256x2,512x1024x5,1x4096x8", help="batch x nodes x loops, comma-separated: `batch` groups of one graph each")
    ap.add_argument("--members", default="2,8", help="members per group, comma-separated")
    ap.add_argument("--repeats", type=int, default=3, help="timed passes per shape and member count")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    mods = (torch, importlib.import_module("a-loam_amd.binding"), importlib.import_module("a-loam_amd.posegraph"), importlib.import_module("a-loam_amd.graph_records"))
    res = {"shapes": []}
    for case in [c for c in args.cases.split(",") if c]:
        batch, nodes, loops = (int(v) for v in case.split("x"))
        for M in [int(v) for v in args.members.split(",") if v]:
            res["shapes"].append(shape(mods, batch, nodes, loops, M, args.repeats, args.max_iterations))
            print(json.dumps(res["shapes"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
