"""tools/relocalization_rate.py — what scoring a map-pose hypothesis costs (aloam_score_map_corrections) next to the data association of a
mapping step, on the same state: bench.py's configs[2] workload (512 travelling sequences, synthetic HDL-64) is brought to steady-state map
depth with normal mapping steps, saved (aloam_save_sequences), loaded frozen, and one frozen mapping step is profiled (map_associate: both
iterations of every sequence); then the scoring call is timed for (n, K) = (1, 2048), (16, 256), (512, 8) - host clock around the call and a
synchronise, median of --repeats - and its score_corrections slot read.

    python tools/relocalization_rate.py [--batch 512] [--frames 100] [--warmup 80] [--repeats 5] [--out relocalization_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/relocalization_rate.py --repeats 3     (per-kernel times)

The candidates are the identity correction shifted and turned a little (--spread-m, --spread-deg about the origin: within the basin of the frozen steps, so
that a scored candidate finds neighbours for about as many stack points as the step does and the two costs compare like for like; the share
of points with five neighbours is printed for both).  A score does the search and the fit of ONE association of a step, so the yardstick is
map_associate / (2 x sequences).  Prints one JSON object.
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

SHAPES = ((1, 2048), (16, 256), (512, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512, help="sequences (configs[2]: 512)")
    ap.add_argument("--frames", type=int, default=100, help="distinct sweeps per sequence")
    ap.add_argument("--warmup", type=int, default=80, help="normal mapping steps before the state is saved (steady-state map depth)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spread-m", type=float, default=0.25)
    ap.add_argument("--spread-deg", type=float, default=0.1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.warmup + 2 <= args.frames

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    wl = bench.TravelWorkload(syn, torch, args.batch, args.frames, 0, "cuda")
    gpu = wl.ctx(binding, wl.B, 0)
    gpu.mapping_enable(0.4, 0.8, 262144)
    B = wl.B

    def sweep(k):
        gpu.process_device(wl.data.data_ptr() + k * wl.NP * 16, wl.seq_stride, wl.nin(k))

    for k in range(args.warmup):
        sweep(k)
        gpu.mapping_step()
    gpu.synchronize()
    blob, off = gpu.save_sequences(range(B), pinned=False)
    k0 = args.warmup
    gpu.set_map_frozen([True] * B)
    gpu.load_sequences(range(B), blob, off)
    sweep(k0)
    gpu.mapping_step()                                                    # builds the grids after the load
    sweep(k0 + 1)
    gpu.synchronize()
    gpu.profile_enable(True)
    gpu.mapping_step()
    p = gpu.profile()
    gpu.profile_enable(False)
    assoc_ms = p["map_associate"]["total_ms"]                             # both iterations, every sequence
    per_assoc_us = 1e3 * assoc_ms / (2 * B)
    infos = [gpu.map_info(b) for b in range(0, B, max(1, B // 16))]
    res = {"workload": wl.describe(True) + f", state saved after {args.warmup} normal steps, one frozen step", "batch": B,
           "map_associate_ms_per_step": assoc_ms, "map_associate_us_per_association": per_assoc_us,
           "stack_points_mean": float(np.mean([i["corner_stack"] + i["surf_stack"] for i in infos])),
           "step_factor_share": float(np.mean([(i["corner_num0"] + i["surf_num0"]) / max(1, i["corner_stack"] + i["surf_stack"]) for i in infos]))}

    rng = np.random.default_rng(1)
    kmax = max(K for _, K in SHAPES)
    q, t = [], []
    for _ in range(kmax):                                                 # shared by every sequence, so turned about the origin: far out a degree is metres
        h = np.radians(rng.uniform(-args.spread_deg, args.spread_deg)) / 2
        q.append([0.0, 0.0, np.sin(h), np.cos(h)])
        t.append([rng.uniform(-args.spread_m, args.spread_m), rng.uniform(-args.spread_m, args.spread_m), 0.0])
    cand = torch.from_numpy(binding.map_corrections(q, t).view(np.uint8)).cuda()
    res["shapes"] = []
    for n, K in SHAPES:
        n = min(n, B)
        seqs = list(range(0, B, B // n))[:n]
        sc = torch.zeros(n * K * 32, dtype=torch.uint8, device="cuda")
        best = torch.zeros(n, dtype=torch.int32, device="cuda")
        call = lambda: gpu.score_map_corrections_into(seqs, cand.data_ptr(), K, sc.data_ptr(), best.data_ptr())
        call()                                                            # warm: code object, scratch
        gpu.synchronize()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            call()
            gpu.synchronize()
            times.append(time.perf_counter() - t0)
        gpu.profile_enable(True)
        call()
        slot = gpu.profile()["score_corrections"]
        gpu.profile_enable(False)
        s = sc.cpu().numpy().view(binding.MAP_SCORE_DTYPE)
        stack = float(np.mean([gpu.map_info(b)["corner_stack"] + gpu.map_info(b)["surf_stack"] for b in seqs[:16]]))
        us = 1e6 * float(np.median(times)) / (n * K)
        res["shapes"].append({"n": n, "K": K, "call_ms": {"median": 1e3 * float(np.median(times)), "min": 1e3 * min(times), "max": 1e3 * max(times), "repeats": args.repeats},
                              "slot_ms": slot["total_ms"], "slot_bytes": slot["bytes_per_launch"], "us_per_sequence_candidate": us,
                              "slot_us_per_sequence_candidate": 1e3 * slot["total_ms"] / (n * K), "vs_map_associate": us / per_assoc_us,
                              "slot_vs_map_associate": 1e3 * slot["total_ms"] / (n * K) / per_assoc_us,
                              "score_factor_share": float(np.mean((s["corner_factors"] + s["surf_factors"]) / max(1.0, stack)))})
    gpu.set_map_frozen(None)
    gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
