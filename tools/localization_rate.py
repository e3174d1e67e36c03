"""tools/localization_rate.py — what a mapping step costs when every sequence localizes against a frozen map (aloam_set_map_frozen) instead of
extending it: bench.py's configs[2] workload (512 travelling sequences, synthetic HDL-64) is brought to steady-state map depth with normal
mapping steps, saved (aloam_save_sequences), and from that same state frozen and normal steps are timed against each other.

    python tools/localization_rate.py [--batch 512] [--frames 100] [--warmup 80] [--repeats 5] [--out localization_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/localization_rate.py --repeats 3     (per-kernel times)

One repeat: load the saved state into every slot, run frame k (registration + odometry + mapping step, untimed: a frozen run builds its grids
after the load), then frame k + 1 with the mapping step timed alone (host clock around aloam_mapping_step and a synchronise).  Medians of
--repeats.  The profiled pass (aloam_profile_get) reports map_grid, map_insert and map_voxel[cubes] per step of the timed frame.  Prints one
JSON object.
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

SLOTS = ("map_begin", "map_voxel[stacks]", "map_grid", "map_associate", "map_solve", "map_insert", "map_voxel[cubes]", "map_register")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512, help="sequences (configs[2]: 512)")
    ap.add_argument("--frames", type=int, default=100, help="distinct sweeps per sequence")
    ap.add_argument("--warmup", type=int, default=80, help="normal mapping steps before the state is saved (steady-state map depth)")
    ap.add_argument("--repeats", type=int, default=5)
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

    def timed_step(frozen, profile=False):
        """Load the saved state, frame k0 untimed, frame k0 + 1 with its mapping step timed."""
        gpu.set_map_frozen([True] * B if frozen else None)
        gpu.load_sequences(range(B), blob, off)
        sweep(k0)
        gpu.mapping_step()
        sweep(k0 + 1)
        gpu.synchronize()
        if profile:
            gpu.profile_enable(True)
        t0 = time.perf_counter()
        gpu.mapping_step()
        gpu.synchronize()
        dt = time.perf_counter() - t0
        prof = None
        if profile:
            p = gpu.profile()
            prof = {s: p[s]["total_ms"] / max(1, p[s]["launches"]) for s in SLOTS}
            gpu.profile_enable(False)
        return dt, prof

    res = {"workload": wl.describe(True) + f", state saved after {args.warmup} normal steps", "batch": B}
    timed_step(False)                                                     # warm both paths (code objects, allocations)
    timed_step(True)
    times = {"normal": [], "frozen": []}
    for _ in range(args.repeats):                                         # alternated, so that both see the same machine state
        for name, fr in (("normal", False), ("frozen", True)):
            times[name].append(timed_step(fr)[0])
    for name in times:
        res[f"{name}_mapping_step_ms"] = {"median": 1e3 * float(np.median(times[name])), "min": 1e3 * min(times[name]), "max": 1e3 * max(times[name]),
                                          "repeats": args.repeats}
    res["frozen_vs_normal"] = res["frozen_mapping_step_ms"]["median"] / res["normal_mapping_step_ms"]["median"]
    for name, fr in (("normal", False), ("frozen", True)):
        res[f"{name}_profile_ms_per_step"] = timed_step(fr, profile=True)[1]
    gpu.synchronize()
    res["map_state"] = bench.map_state(gpu)
    gpu.set_map_frozen(None)
    gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
