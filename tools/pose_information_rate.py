"""tools/pose_information_rate.py — what aloam_export_pose_information costs beside the solve whose records it re-reads.

    python tools/pose_information_rate.py [--batch 2048] [--repeats 5] [--map-batch 512] [--map-warmup 80] [--no-mapping] [--out FILE.json]

Two legs in one process, each on bench.py's own workload with the inputs resident in HBM:
  odometry  the headline state (synthetic HDL-64 64 x 2048, batch 2048): per pass one aloam_process_device and one
            aloam_export_pose_information(ALOAM_INFO_ODOMETRY, every sequence); milliseconds per launch of the pose_information profiling slot
            beside those of the k_solve slot (two launches per step) of the same pass
  mapping   bench.py configs[2] (travelling sensor, batch 512, after the warm-up that brings the submap to its steady-state depth): the same with
            aloam_mapping_step, ALOAM_INFO_MAPPING and the map_solve slot
The passes alternate step and export, so both slots see the same clocks and the same state; the figures are the median [min - max] of the
passes.  Slot times are hipEvent intervals on the context's stream (they include the launch gap of a single kernel).  Prints one JSON object.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "passes": len(v)}


def leg(gpu, binding, torch, step, which, solve_slot, batch, repeats):
    size = binding.POSE_INFORMATION_DTYPE.itemsize
    dst = torch.zeros(batch * size, dtype=torch.uint8, device="cuda")
    ids = list(range(batch))
    step()
    gpu.export_pose_information_into(which, ids, dst.data_ptr())            # untimed: first-use allocations
    gpu.synchronize()
    info_ms, solve_ms, nbytes = [], [], 0.0
    for _ in range(repeats):
        gpu.profile_enable(True)                                            # (zeroes the slots)
        step()
        gpu.export_pose_information_into(which, ids, dst.data_ptr())
        prof = gpu.profile()                                                # synchronises
        info_ms.append(prof["pose_information"]["total_ms"] / prof["pose_information"]["launches"])
        solve_ms.append(prof[solve_slot]["total_ms"] / prof[solve_slot]["launches"])
        nbytes = prof["pose_information"]["bytes_per_launch"]
    gpu.profile_enable(False)
    rec = dst.cpu().numpy().view(binding.POSE_INFORMATION_DTYPE)
    ok = rec[rec["status"] == binding.INFO_OK]
    out = {"batch": batch, "pose_information_ms_per_call": spread(info_ms), solve_slot + "_ms_per_launch": spread(solve_ms),
           "algorithmic_bytes_per_call": nbytes, "records_ok": int(len(ok)), "mean_factors": float(np.mean(ok["n_line"] + ok["n_plane"])) if len(ok) else 0.0}
    out["algorithmic_GBps"] = nbytes / (1e6 * out["pose_information_ms_per_call"]["median"]) if nbytes else 0.0
    if len(ok):
        ratio = ok["trans_eigenvalues"][:, 0] / ok["trans_eigenvalues"][:, 1]
        out["translation_lambda0_over_lambda1"] = {"min": float(ratio.min()), "median": float(np.median(ratio)), "max": float(ratio.max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5, help="passes of each leg (one step + one export each)")
    ap.add_argument("--map-batch", type=int, default=512)
    ap.add_argument("--map-frames", type=int, default=100)
    ap.add_argument("--map-warmup", type=int, default=80)
    ap.add_argument("--map-pool", type=int, default=262144)
    ap.add_argument("--no-mapping", action="store_true", help="the odometry leg only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    res = {}

    wl = bench.Workload(syn, torch, "HDL-64", args.batch, args.frames, 0, "cuda")
    gpu = wl.ctx(binding, wl.B, 0)
    order = iter(bench.frame_order(wl.T, 4 + 2 * args.repeats))
    nin = {k: wl.nin(k) for k in range(wl.T)}
    base = wl.data.data_ptr()

    def step():
        k = next(order)
        gpu.process_device(base + k * wl.NP * 16, wl.seq_stride, nin[k])

    for _ in range(3):
        step()
    res["odometry"] = dict(leg(gpu, binding, torch, step, binding.INFO_ODOMETRY, "k_solve", wl.B, args.repeats), workload=wl.describe(False))
    gpu.close()
    del wl

    if not args.no_mapping:
        wl = bench.TravelWorkload(syn, torch, args.map_batch, args.map_frames, 0, "cuda")
        gpu = wl.ctx(binding, wl.B, 0)
        gpu.mapping_enable(0.4, 0.8, args.map_pool)
        order = iter(bench.frame_order(wl.T, args.map_warmup + 2 + 2 * args.repeats))
        nin = {k: wl.nin(k) for k in range(wl.T)}
        base = wl.data.data_ptr()

        def map_step():
            k = next(order)
            gpu.process_device(base + k * wl.NP * 16, wl.seq_stride, nin[k])
            gpu.mapping_step()

        for _ in range(args.map_warmup):
            map_step()
        res["mapping"] = dict(leg(gpu, binding, torch, map_step, binding.INFO_MAPPING, "map_solve", wl.B, args.repeats), workload=wl.describe(True),
                              map_state=bench.map_state(gpu))
        gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
