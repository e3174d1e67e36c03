"""tools/export_rate.py — what reading the results of a batch costs: the per-sequence getters against the batched export
(aloam_export_poses / aloam_export_clouds), on bench.py's headline workload (synthetic HDL-64 64 x 2048, inputs resident in HBM).

    python tools/export_rate.py [--batch 2048] [--steps 20] [--out export_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/export_rate.py --kernels-only     (k_export_* kernel times)

Prints one JSON object.  Wall times are host clocks around work that ends in a stream synchronise.  Algorithmic bytes of an export:
16 B read + 16 B written per point, 16 B per segment (its count and offset); kernel times come from the separate rocprofv3 run.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FEATURE_AND_LAST = list(range(1, 7))     # sharp, less sharp, flat, less flat, corner last, surf last
FEATURES = list(range(1, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20, help="steps of each end-to-end leg")
    ap.add_argument("--repeats", type=int, default=5, help="timed repetitions of each export")
    ap.add_argument("--kernels-only", action="store_true", help="only the exports (for a rocprofv3 run): no getter loop, no end-to-end legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    wl = bench.Workload(syn, torch, "HDL-64", args.batch, args.frames, 0, "cuda")
    B = wl.B
    gpu = wl.ctx(binding, B, 0)
    order = bench.frame_order(wl.T, 3 + 3 * args.steps)
    nin = {k: wl.nin(k) for k in range(wl.T)}
    base = wl.data.data_ptr()
    it = iter(order)

    def step():
        k = next(it)
        gpu.process_device(base + k * wl.NP * 16, wl.seq_stride, nin[k])

    for _ in range(3):
        step()
    gpu.synchronize()
    res = {"workload": wl.describe(False), "batch": B}

    # sizes of the six feature and last clouds, and buffers for them
    off_dev = torch.zeros(len(FEATURE_AND_LAST) * B + 1, dtype=torch.int64, device="cuda")
    gpu.export_clouds(FEATURE_AND_LAST, 0, 0, off_dev.data_ptr())
    gpu.synchronize()
    total = int(off_dev[-1])
    segs = len(FEATURE_AND_LAST) * B
    alg_bytes = 32.0 * total + 16.0 * segs
    res["six_clouds"] = {"points": total, "segments": segs, "algorithmic_bytes": alg_bytes}
    pts_dev = torch.empty((total, 4), dtype=torch.float32, device="cuda")
    pts_pin = torch.empty((total, 4), dtype=torch.float32, pin_memory=True)
    off_pin = torch.zeros(segs + 1, dtype=torch.int64, pin_memory=True)
    rec_dev = torch.empty(B * ctypes.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, device="cuda")
    rec_pin = torch.empty(B * ctypes.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)

    def timed(fn, repeats=args.repeats):
        fn()
        gpu.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            gpu.synchronize()
            ts.append(time.perf_counter() - t0)
        return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "repeats": repeats}

    def export_dev():
        gpu.export_poses(rec_dev.data_ptr())
        gpu.export_clouds(FEATURE_AND_LAST, pts_dev.data_ptr(), total, off_dev.data_ptr())

    def export_pin():
        gpu.export_poses(rec_pin.data_ptr())
        gpu.export_clouds(FEATURE_AND_LAST, pts_pin.data_ptr(), total, off_pin.data_ptr())

    res["export_poses_and_six_clouds_device"] = timed(export_dev)
    res["export_poses_and_six_clouds_pinned_host"] = timed(export_pin)

    def memcpy_d2h():                                     # the same byte count as the pinned export: one hipMemcpyAsync device-to-host (torch's stream)
        pts_pin.copy_(pts_dev, non_blocking=True)
        torch.cuda.synchronize()

    res["memcpy_d2h_same_bytes"] = timed(memcpy_d2h)
    res["pinned_export_vs_memcpy"] = res["memcpy_d2h_same_bytes"]["median_ms"] / res["export_poses_and_six_clouds_pinned_host"]["median_ms"]
    if args.kernels_only:
        print(json.dumps(res))
        return

    # the per-sequence getter loop every consumer ran before: one pose and six clouds per sequence, each a blocking round trip
    t0 = time.perf_counter()
    for b in range(B):
        gpu.pose(b)
    res["getter_loop_poses_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    got = 0
    for b in range(B):
        for w in FEATURE_AND_LAST:
            got += len(gpu.cloud(w, b))
    res["getter_loop_six_clouds_ms"] = 1e3 * (time.perf_counter() - t0)
    assert got == total, (got, total)

    # end to end: process_device alone, and process_device + export_poses + the four feature clouds every step (pinned host memory, device memory)
    off4 = torch.zeros(len(FEATURES) * B + 1, dtype=torch.int64, pin_memory=True)

    def leg(with_export, pinned=True):
        pts, rec = (pts_pin, rec_pin) if pinned else (pts_dev, rec_dev)
        gpu.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
            if with_export:
                gpu.export_poses(rec.data_ptr())
                gpu.export_clouds(FEATURES, pts.data_ptr(), total, off4.data_ptr())
        gpu.synchronize()
        dt = time.perf_counter() - t0
        return {"steps": args.steps, "ms_per_step": 1e3 * dt / args.steps, "sweeps_per_s": args.steps * B / dt}

    res["process_device_alone"] = leg(False)
    res["process_device_plus_export_pinned_host"] = leg(True)
    res["process_device_plus_export_device"] = leg(True, pinned=False)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    del pts_dev, pts_pin, rec_dev, rec_pin, off_dev, off_pin, off4
    gpu.close()


if __name__ == "__main__":
    main()
