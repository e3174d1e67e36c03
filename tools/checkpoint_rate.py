"""tools/checkpoint_rate.py — what saving and loading whole sequences costs (aloam_save_sequences / aloam_load_sequences): every slot of a batch
saved into and loaded from device memory and pinned host memory, against a hipMemcpyAsync of the same bytes, and the latency of one sequence's
save-and-load round trip.  Two legs: odometry only (bench.py's headline workload, synthetic HDL-64, inputs resident) and with mapping (the
travelling configs[2] drive after a warm-up, so the maps have depth).

    python tools/checkpoint_rate.py [--batch 2048] [--map-batch 512] [--map-warmup 40] [--out checkpoint_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/checkpoint_rate.py --repeats 3     (k_ckpt_* kernel times)

Prints one JSON object.  Wall times are host clocks around work that ends in a stream synchronise (median of --repeats).  Algorithmic bytes
of a save or load: every record byte read once and written once.
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


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "repeats": repeats}


def leg(torch, binding, gpu, B, repeats):
    """Save / load of all B slots, device and pinned, against copies of the same bytes; one sequence's round trip; the load's host wait."""
    ids = list(range(B))
    off_dev = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    off_pin = torch.zeros(B + 1, dtype=torch.int64, pin_memory=True)
    gpu.save_sequences_into(ids, 0, 0, off_pin.data_ptr())
    gpu.synchronize()
    total = int(off_pin[-1])
    off_host = off_pin.numpy().copy()
    dev = torch.empty(total, dtype=torch.uint8, device="cuda")
    dev2 = torch.empty(total, dtype=torch.uint8, device="cuda")
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    res = {"batch": B, "record_bytes": total, "bytes_per_sequence": total / B, "algorithmic_bytes": 2.0 * total}

    def save_dev():
        gpu.save_sequences_into(ids, dev.data_ptr(), total, off_dev.data_ptr())
        gpu.synchronize()

    def save_pin():
        gpu.save_sequences_into(ids, pin.data_ptr(), total, off_pin.data_ptr())
        gpu.synchronize()

    def load_dev():
        gpu.load_sequences(ids, dev, off_host)
        gpu.synchronize()

    def load_pin():
        gpu.load_sequences(ids, pin.numpy(), off_host)
        gpu.synchronize()

    def copy_d2d():                                       # the same byte count: one hipMemcpyAsync each (torch's stream)
        dev2.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()

    def copy_d2h():
        pin.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()

    def copy_h2d():
        dev2.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()

    res["save_device"] = timed(save_dev, repeats)
    res["load_device"] = timed(load_dev, repeats)
    res["memcpy_d2d_same_bytes"] = timed(copy_d2d, repeats)
    res["save_pinned_host"] = timed(save_pin, repeats)
    res["load_pinned_host"] = timed(load_pin, repeats)
    res["memcpy_d2h_same_bytes"] = timed(copy_d2h, repeats)
    res["memcpy_h2d_same_bytes"] = timed(copy_h2d, repeats)
    med = {k: res[k]["median_ms"] for k in res if isinstance(res[k], dict)}
    res["save_device_vs_memcpy"] = med["memcpy_d2d_same_bytes"] / med["save_device"]
    res["load_device_vs_memcpy"] = med["memcpy_d2d_same_bytes"] / med["load_device"]
    res["save_pinned_vs_memcpy"] = med["memcpy_d2h_same_bytes"] / med["save_pinned_host"]
    res["load_pinned_vs_memcpy"] = med["memcpy_h2d_same_bytes"] / med["load_pinned_host"]
    res["save_device_tb_s"] = 2.0 * total / (med["save_device"] * 1e-3) / 1e12
    res["load_device_tb_s"] = 2.0 * total / (med["load_device"] * 1e-3) / 1e12

    # one sequence: save into pinned memory, synchronise, load it back into its slot, synchronise
    one = torch.empty(int(off_host[1] - off_host[0]) + 256, dtype=torch.uint8, pin_memory=True)
    off1 = torch.zeros(2, dtype=torch.int64, pin_memory=True)

    def round_trip():
        gpu.save_sequences_into([0], one.data_ptr(), one.numel(), off1.data_ptr())
        gpu.synchronize()
        gpu.load_sequences([0], one.numpy(), off1.numpy())
        gpu.synchronize()

    res["one_sequence_round_trip"] = timed(round_trip, max(repeats, 10))

    def load_call_only():                                 # the host part of a load: one stream synchronise, the header reads and checks, the queueing
        t0 = time.perf_counter()
        gpu.load_sequences(ids, pin.numpy(), off_host)
        dt = time.perf_counter() - t0
        gpu.synchronize()
        return dt

    gpu.synchronize()
    res["load_call_host_ms_all_slots"] = 1e3 * float(np.median([load_call_only() for _ in range(repeats)]))
    del dev, dev2, pin
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048, help="sequences of the odometry-only leg")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--map-batch", type=int, default=512, help="sequences of the mapping leg (0: skip it)")
    ap.add_argument("--map-frames", type=int, default=12)
    ap.add_argument("--map-warmup", type=int, default=40, help="mapping steps before the measurement (map depth)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    out = {}

    wl = bench.Workload(syn, torch, "HDL-64", args.batch, args.frames, 0, "cuda")
    gpu = wl.ctx(binding, wl.B, 0)
    for k in range(4):
        gpu.process_device(wl.data.data_ptr() + (k % wl.T) * wl.NP * 16, wl.seq_stride, wl.nin(k % wl.T))
    gpu.synchronize()
    out["odometry"] = {"workload": wl.describe(False), **leg(torch, binding, gpu, wl.B, args.repeats)}
    gpu.close()
    del wl

    if args.map_batch > 0:
        wl = bench.TravelWorkload(syn, torch, args.map_batch, args.map_frames, 0, "cuda")
        gpu = wl.ctx(binding, wl.B, 0)
        gpu.mapping_enable(0.4, 0.8, 262144)
        for k in range(args.map_warmup):
            gpu.process_device(wl.data.data_ptr() + (k % wl.T) * wl.NP * 16, wl.seq_stride, wl.nin(k % wl.T))
            gpu.mapping_step()
        gpu.synchronize()
        out["mapping"] = {"workload": wl.describe(True) + f", {args.map_warmup} steps of warm-up", **leg(torch, binding, gpu, wl.B, args.repeats)}
        gpu.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
