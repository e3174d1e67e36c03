"""tools/graph_record_rate.py — what saving and loading pose graphs with their keyframe clouds costs (aloam_graph_save / aloam_graph_load).

    python tools/graph_record_rate.py [--repeats 5] [--cases 2048x256x2,512x1024x5,1x4096x8] [--points 64x256] [--out FILE.json]

Per case (batch x nodes x loop edges, the shapes of tools/pose_graph_rate.py), once with the keyframe store and once without: one sequence's
graph is entered as a caller would in a context of batch 1 (the pose of a keyframe injected with aloam_set_state, hand-made clouds of
--points corner x surf points through aloam_set_last and aloam_mapping_step, aloam_graph_add_nodes, the loop edges with one
aloam_graph_add_edges), saved, and its record forked into every slot of the batch context with one aloam_graph_load.  Then, --repeats
times and alternated: a save of every slot into device memory, a device-to-device hipMemcpyAsync of the same byte count, a load of every
slot (the graphs cleared before it, outside the clock) and the copy again.

Milliseconds per call, medians: `queue` is the host time of the call itself (the save returns without waiting; the load holds its one
wait and the check), `call` ends in a stream synchronise, `stream` is the hipEvent interval of the profiling slot the kernels run in
(save_sequences / load_sequences; for a load the check and the unpack together).  copy_vs_save / copy_vs_load: the plain copy's
milliseconds over the call's.  Prints one JSON object.
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


def one_graph(torch, binding, pg, nodes, loops, points, keyframes):
    """The record of one sequence's graph (device memory) and its byte length."""
    d = pg.drifted_laps(1, nodes, loops)
    rng = np.random.default_rng(11)
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=max(1024, points[1] + 64), lm_max_iterations=0)
    gpu.graph_enable(nodes, nodes + loops)
    if keyframes:
        gpu.mapping_enable(0.4, 0.8, pool_points=1 << 16)
        gpu.graph_keyframes_enable(nodes * points[0], nodes * points[1])
    ident, zero = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    for k in range(nodes):
        if keyframes:
            cl = []
            for n, half in ((points[0], (10.0, 10.0, 2.0)), (points[1], (20.0, 20.0, 3.0))):
                p = np.zeros((n, 4), np.float32)
                p[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) * half
                p[:, 3] = np.sort(rng.integers(0, 16, n))
                cl.append(p)
            gpu.set_last(cl[0], cl[1], 0)
            gpu.set_full_cloud(cl[1][:4], 0)
        gpu.set_state(ident, zero, d["q"][k], d["t"][k], seq=0)
        if keyframes:
            gpu.mapping_step()
        gpu.graph_add_nodes([0], d["info"])
    gpu.graph_add_edges(d["loop"])
    blob, off = gpu.graph_save([0], pinned=False)
    rec = blob.clone()
    torch.cuda.synchronize()
    gpu.close()
    return rec, int(off[1])


def median_ms(ts):
    return 1e3 * float(np.median(ts))


def case(torch, binding, pg, batch, nodes, loops, points, keyframes, repeats):
    rec, size = one_graph(torch, binding, pg, nodes, loops, points, keyframes)
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=batch, max_points=1024, lm_max_iterations=0)
    gpu.graph_enable(nodes, nodes + loops)
    if keyframes:
        gpu.mapping_enable(0.4, 0.8, pool_points=1 << 12)
        gpu.graph_keyframes_enable(nodes * points[0], nodes * points[1])
    ids = list(range(batch))
    total = size * batch
    src = rec[:size].repeat(batch)                          # the record once per slot: a fork
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    other = torch.empty(total, dtype=torch.uint8, device="cuda")   # the plain copy's destination
    offsets = np.arange(batch + 1, dtype=np.int64) * size
    off_dev = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                # torch filled src on its own stream: the context's stream must not run ahead of it
    gpu.graph_load(ids, src, offsets)
    gpu.synchronize()
    t = {k: [] for k in ("save_queue", "save_call", "save_stream", "load_queue", "load_call", "load_stream", "copy_after_save", "copy_after_load")}

    def copy():
        t0 = time.perf_counter()
        other.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def stream_ms(slot):
        p = gpu.profile()[slot]
        return p["total_ms"] * 1e-3

    for r in range(repeats + 1):                            # the first pass warms up (allocations) and is dropped
        gpu.profile_enable(True)
        t0 = time.perf_counter()
        gpu.graph_save_into(ids, dst.data_ptr(), total, off_dev.data_ptr())
        t1 = time.perf_counter()
        gpu.synchronize()
        t2 = time.perf_counter()
        row = {"save_queue": t1 - t0, "save_call": t2 - t0, "save_stream": stream_ms("save_sequences"), "copy_after_save": copy()}
        gpu.graph_clear(ids)
        gpu.synchronize()
        gpu.profile_enable(True)
        t0 = time.perf_counter()
        gpu.graph_load(ids, dst, offsets)
        t1 = time.perf_counter()
        gpu.synchronize()
        t2 = time.perf_counter()
        row.update({"load_queue": t1 - t0, "load_call": t2 - t0, "load_stream": stream_ms("load_sequences"), "copy_after_load": copy()})
        if r:
            for k, v in row.items():
                t[k].append(v)
    gpu.profile_enable(False)
    same = bool(torch.equal(dst[:size], src[:size])) and off_dev.cpu().numpy().tolist() == offsets.tolist()   # slot 0 saved again is the record it was loaded from
    gpu.close()
    ms = {k: median_ms(v) for k, v in t.items()}
    copy_ms = 0.5 * (ms["copy_after_save"] + ms["copy_after_load"])
    return {"batch": batch, "nodes": nodes, "loops": loops, "keyframes": bool(keyframes), "points_per_node": list(points) if keyframes else [0, 0],
            "record_bytes": size, "total_bytes": total, "repeats": repeats,
            "save_ms": {"queue": ms["save_queue"], "call": ms["save_call"], "stream": ms["save_stream"]},
            "load_ms": {"queue": ms["load_queue"], "call": ms["load_call"], "stream": ms["load_stream"]},
            "memcpy_d2d_same_bytes_ms": copy_ms, "copy_vs_save": copy_ms / ms["save_call"], "copy_vs_load": copy_ms / ms["load_call"],
            "save_stream_tb_s": 2.0 * total / (ms["save_stream"] * 1e-3) / 1e12, "load_stream_tb_s": 2.0 * total / (ms["load_stream"] * 1e-3) / 1e12,
            "records_round_trip_equal": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default="2048x256x2,512x1024x5,1x4096x8", help="batch x nodes x loops, comma-separated (the shapes of tools/pose_graph_rate.py)")
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per case (save, copy, load, copy)")
    ap.add_argument("--points", default="64x256", help="corner x surf points of a keyframe's clouds")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    points = tuple(int(v) for v in args.points.split("x"))
    res = {"cases": []}
    for c in args.cases.split(","):
        batch, nodes, loops = (int(v) for v in c.split("x"))
        for keyframes in (True, False):
            res["cases"].append(case(torch, binding, pg, batch, nodes, loops, points, keyframes, args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
