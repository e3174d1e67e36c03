"""tools/loop_register_rate.py — what one aloam_graph_register_loops call costs.

    python tools/loop_register_rate.py [--shapes 1,256,2048] [--sequences 16] [--repeats 5] [--search R STEP YAW YAWSTEP] [--links] [--out FILE.json]

Every sequence holds 14 hand-made keyframes of a room (loopreg.room_sample: a floor, two walls, four poles, two edges; about 300 corner and 1500 surf points fed
per keyframe, VLP-16-sized, down-sampled by a mapping step with the solver off): 13 target nodes along 8 m and one source node entered
about 0.4 m and 4 degrees off.  A shape of n requests lists the sequences round-robin (a sequence may be listed more than once), each
request registering node 13 against nodes 0 .. 12 in the frame of node 6, into device memory.  Reported per shape, in milliseconds:
  queue_ms   host clock around aloam_graph_register_loops alone (the call does not synchronise)
  call_ms    host clock around the call + aloam_synchronize
  stream_ms  hipEvent interval of the loop_register profiling slot: everything the call queued
with the statuses, the mean factor counts and the mean translation error before and after, and scratch_bytes: the device memory
aloam_graph_loops_enable took for the largest shape.  The spare-slot route of one edge is timed by
tools/loop_closure_drive.py --device-loops, in the same process as the call it replaces.  For a per-kernel profile run this tool under
rocprofv3 --kernel-trace --stats.  Prints one JSON object.

--search R STEP YAW YAWSTEP: the same shapes with FAR guesses (the truth moved by (2.2, -1.6, 0.08) m and turned by 11 degrees) through
aloam_graph_search_loops with that grid (metres, metres, degrees, degrees).  Per shape, under "search": queue_ms, call_ms and stream_ms of
the searched call, nodes per request, us_per_request_node, the mean error, and beside them ("plain") the plain call from the same far
guesses.

--links: the same shapes with every source node in ANOTHER sequence (request r: target and frame in sequence r mod B, source node 13 of
sequence (r + 1) mod B) through aloam_graph_register_links.  The per-sequence call and the link call alternate in one process, repeat by
repeat; per shape, under "loops" and "links": queue_ms, call_ms and stream_ms side by side, the statuses, the mean factor counts and the
mean error.
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LEAF = (0.2, 0.4)
TARGETS = 13


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="1,256,2048", help="requests per call, comma-separated")
    ap.add_argument("--sequences", type=int, default=16, help="sequences the requests are spread over")
    ap.add_argument("--repeats", type=int, default=5, help="timed calls per shape (median, min and max are reported)")
    ap.add_argument("--search", nargs=4, type=float, metavar=("R", "STEP", "YAW", "YAWSTEP"), default=None,
                    help="time aloam_graph_search_loops with this grid (m, m, deg, deg) from far guesses, the plain call beside it")
    ap.add_argument("--links", action="store_true",
                    help="time aloam_graph_register_links (every source node in another sequence) alternated with the per-sequence call")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    pg = importlib.import_module("a-loam_amd.posegraph")
    lr = importlib.import_module("a-loam_amd.loopreg")
    shapes = [int(v) for v in args.shapes.split(",")]
    B = args.sequences
    rng = np.random.default_rng(B)

    def yaw(a):
        return np.array([0.0, 0.0, math.sin(0.5 * a), math.cos(0.5 * a)])
    q_true = [yaw(0.03 * (k - TARGETS // 2)) for k in range(TARGETS)] + [yaw(0.3)]
    t_true = [np.array([8.0 * k / (TARGETS - 1), 0.3 * math.sin(2.0 * k / (TARGETS - 1)), 1.2]) for k in range(TARGETS)] + [np.array([4.35, -0.4, 1.25])]
    q_in, t_in = list(q_true), list(t_true)
    q_in[-1], t_in[-1] = pg.qmul(yaw(math.radians(4.0)), q_true[-1]), t_true[-1] + np.array([0.3, -0.25, 0.08])

    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=B, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(*LEAF, pool_points=1 << 16)
    gpu.graph_enable(TARGETS + 3, TARGETS + 3)
    gpu.graph_keyframes_enable((TARGETS + 1) * 512, (TARGETS + 1) * 2048)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    gpu.graph_loops_enable(max(shapes), TARGETS * 512, TARGETS * 2048)
    scratch = free0 - torch.cuda.mem_get_info()[0]             # what the feature's scratch of max(shapes) slots takes of the device
    ids = list(range(B))
    for k in range(TARGETS + 1):
        for b in ids:
            clouds = [lr.sensor_cloud(w, q_true[k], t_true[k], rng) for w in lr.room_sample(rng)]
            gpu.set_last(clouds[0], clouds[1], b)
            gpu.set_full_cloud(clouds[1][:4], b)
            gpu.set_state([0, 0, 0, 1], [0, 0, 0], q_in[k], t_in[k], seq=b)
        gpu.mapping_step()
        gpu.graph_add_nodes(ids, np.eye(6) * 100.0)
    gpu.synchronize()
    held = gpu.graph_keyframe_info(0)
    i, j = TARGETS // 2, TARGETS
    qg, tg = pg.relative_pose(q_in[i], t_in[i], q_in[j], t_in[j])
    qz, tz = pg.relative_pose(q_true[i], t_true[i], q_true[j], t_true[j])
    res = {"sequences": B, "target_nodes": TARGETS, "points_per_keyframe": [held["points"][0] / (TARGETS + 1), held["points"][1] / (TARGETS + 1)],
           "guess_error_m": float(np.linalg.norm(tg - tz)), "scratch_slots": max(shapes), "scratch_bytes": int(scratch), "shapes": []}
    size = binding.GRAPH_LOOP_RESULT_DTYPE.itemsize
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}

    def timed(call):
        call()                                                             # (warm-up: the first launch of every kernel, the scratch)
        gpu.synchronize()
        queue_ms, call_ms, stream_ms = [], [], []
        for _ in range(args.repeats):
            gpu.profile_enable(True)
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            gpu.synchronize()
            t2 = time.perf_counter()
            queue_ms.append(1e3 * (t1 - t0))
            call_ms.append(1e3 * (t2 - t0))
            stream_ms.append(gpu.profile()["loop_register"]["total_ms"])
        gpu.profile_enable(False)
        return {"queue_ms": stat(queue_ms), "call_ms": stat(call_ms), "stream_ms": stat(stream_ms)}

    if args.search:
        grid = gpu.graph_loop_search(radius_m=args.search[0], step_m=args.search[1], yaw_deg=args.search[2], yaw_step_deg=args.search[3])
        K = len(lr.search_grid(qz, tz, *args.search)[0])
        qf = pg.qmul(yaw(math.radians(11.0)), qz)
        qf, tf = qf / np.linalg.norm(qf), tz + np.array([2.2, -1.6, 0.08])
        res.update(search=list(args.search), nodes_per_request=K, far_guess_error_m=float(np.linalg.norm(tf - tz)))
        ssize = binding.GRAPH_LOOP_SEARCH_RESULT_DTYPE.itemsize
        for n in shapes:
            reqs = gpu.graph_loop_requests([(r % B, i, j, 0, TARGETS, binding.GRAPH_POSE_ENTERED, qf, tf) for r in range(n)])
            dst = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
            sdst = torch.zeros(n * ssize, dtype=torch.uint8, device="cuda")
            opt = gpu.graph_loop_options()
            plain = timed(lambda: gpu.graph_register_loops_into(reqs, dst.data_ptr(), opt))
            plain["error_m"] = float(np.linalg.norm(dst.cpu().numpy().view(binding.GRAPH_LOOP_RESULT_DTYPE)["t"] - tz, axis=1).mean())
            found = timed(lambda: gpu.graph_search_loops_into(reqs, dst.data_ptr(), sdst.data_ptr(), 0, grid, opt))
            out, sout = dst.cpu().numpy().view(binding.GRAPH_LOOP_RESULT_DTYPE), sdst.cpu().numpy().view(binding.GRAPH_LOOP_SEARCH_RESULT_DTYPE)
            found.update(error_m=float(np.linalg.norm(out["t"] - tz, axis=1).mean()), nodes=K, us_per_request_node=1e3 * found["stream_ms"]["median"] / (n * K),
                         best=sorted({int(b) for b in sout["best"]}), statuses={int(s): int(c) for s, c in zip(*np.unique(out["status"], return_counts=True))},
                         factors=[float(out["n_line"].mean()), float(out["n_plane"].mean())])
            res["shapes"].append({"requests": n, "search": found, "plain": plain})
        shapes = []
    if args.links:
        assert B >= 2, "--links needs two sequences"
        for n in shapes:
            loops = gpu.graph_loop_requests([(r % B, i, j, 0, TARGETS, binding.GRAPH_POSE_ENTERED, qg, tg) for r in range(n)])
            links = gpu.graph_link_requests([(r % B, i, 0, TARGETS, (r + 1) % B, j, binding.GRAPH_POSE_ENTERED, qg, tg) for r in range(n)])
            dst = {k: torch.zeros(n * size, dtype=torch.uint8, device="cuda") for k in ("loops", "links")}
            opt = gpu.graph_loop_options()
            calls = {"loops": lambda: gpu.graph_register_loops_into(loops, dst["loops"].data_ptr(), opt),
                     "links": lambda: gpu.graph_register_links_into(links, dst["links"].data_ptr(), opt)}
            for call in calls.values():                                    # (warm-up: the first launch of every kernel, the link staging)
                call()
            gpu.synchronize()
            times = {k: {"queue_ms": [], "call_ms": [], "stream_ms": []} for k in calls}
            for _ in range(args.repeats):
                for k, call in calls.items():                              # alternated: both see the same clocks and the same neighbours
                    gpu.profile_enable(True)
                    t0 = time.perf_counter()
                    call()
                    t1 = time.perf_counter()
                    gpu.synchronize()
                    t2 = time.perf_counter()
                    times[k]["queue_ms"].append(1e3 * (t1 - t0)); times[k]["call_ms"].append(1e3 * (t2 - t0))
                    times[k]["stream_ms"].append(gpu.profile()["loop_register"]["total_ms"])
            gpu.profile_enable(False)
            shape = {"requests": n}
            for k in calls:
                out = dst[k].cpu().numpy().view(binding.GRAPH_LOOP_RESULT_DTYPE)
                shape[k] = {m: stat(v) for m, v in times[k].items()}
                shape[k].update(statuses={int(s): int(c) for s, c in zip(*np.unique(out["status"], return_counts=True))},
                                factors=[float(out["n_line"].mean()), float(out["n_plane"].mean())], error_m=float(np.linalg.norm(out["t"] - tz, axis=1).mean()),
                                ms_per_request=float(np.median(times[k]["stream_ms"])) / n)
            shape["links_over_loops_stream"] = shape["links"]["stream_ms"]["median"] / shape["loops"]["stream_ms"]["median"]
            res["shapes"].append(shape)
        shapes = []
    for n in shapes:
        reqs = gpu.graph_loop_requests([(r % B, i, j, 0, TARGETS, binding.GRAPH_POSE_ENTERED, qg, tg) for r in range(n)])
        dst = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
        opt = gpu.graph_loop_options()
        gpu.graph_register_loops_into(reqs, dst.data_ptr(), opt)          # (warm-up: the first launch of every kernel)
        gpu.synchronize()
        queue_ms, call_ms, stream_ms = [], [], []
        for _ in range(args.repeats):
            gpu.profile_enable(True)
            t0 = time.perf_counter()
            gpu.graph_register_loops_into(reqs, dst.data_ptr(), opt)
            t1 = time.perf_counter()
            gpu.synchronize()
            t2 = time.perf_counter()
            queue_ms.append(1e3 * (t1 - t0))
            call_ms.append(1e3 * (t2 - t0))
            stream_ms.append(gpu.profile()["loop_register"]["total_ms"])
        gpu.profile_enable(False)
        out = dst.cpu().numpy().view(binding.GRAPH_LOOP_RESULT_DTYPE)
        res["shapes"].append({"requests": n, "statuses": {int(s): int(c) for s, c in zip(*np.unique(out["status"], return_counts=True))},
                              "target_raw": out["target_raw"].mean(0).tolist(), "target_points": out["target_points"].mean(0).tolist(),
                              "factors": [float(out["n_line"].mean()), float(out["n_plane"].mean())],
                              "error_m": float(np.linalg.norm(out["t"] - tz, axis=1).mean()),
                              "queue_ms": stat(queue_ms), "call_ms": stat(call_ms), "stream_ms": stat(stream_ms),
                              "ms_per_request": float(np.median(stream_ms)) / n})
    gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
