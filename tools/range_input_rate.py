"""tools/range_input_rate.py — what handing sweeps over as 16-bit range images buys, on bench.py's headline workload (synthetic HDL-64
64 x 2048 on the 30 m circle), encoded once.

    python tools/range_input_rate.py [--batch 2048] [--frames 6] [--steps 24] [--repeats 5] [--out range_input_rate.json]

Legs, each repeated --repeats times in ALTERNATING order (one pass runs every leg once, then the next pass; nothing is compared across
processes or boxes), every timing a host clock around work that ends in a stream synchronise, after a warm-up:
  (a) host-fed sweeps/s: aloam_process_host with 16-byte and 12-byte records against aloam_process_range_host (pinned memory, two contexts
      as in bench.py's host-fed leg);
  (b) a plain pinned hipMemcpyAsync of the same range bytes per step;
  (c) resident: aloam_process_device (16-byte records in HBM) against aloam_process_range_device, ms per step;
  (d) the K_FIND_ENDS / K_FRONT profiling slots for both kinds of input (a profiled pass of their own).
Prints one JSON object: medians, min and max of the repeats, and which of the two conditions of DESIGN §7i binds for the range host path
(85 % of the plain copy, or 90 % of the resident range rate).
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


def encode_on_device(torch, wl, dec, model):
    """Every stored sweep of the workload as a range image, on the device: nearest ray (row by elevation, column by azimuth), nearest range
    code - a-loam_amd/range_input.py encode_sweep in torch.  -> int16 tensor [B, T, blob_len]."""
    ri = importlib.import_module("a-loam_amd.range_input")
    rows, cols = model.n_scans, model.columns
    g = model.dirs.reshape(rows, cols, 3).double()
    el_rows = torch.atan2(g[:, 0, 2], torch.hypot(g[:, 0, 0], g[:, 0, 1]))         # decreasing with the row
    mids = -(el_rows[:-1] + el_rows[1:]) / 2                                       # ascending boundaries of -elevation
    az0 = float(torch.atan2(g[0, 0, 1], g[0, 0, 0]))
    step = -2 * np.pi / cols
    hdr = ri.header_len(cols)
    blobs = torch.zeros((wl.B, wl.T, hdr + rows * cols), dtype=torch.int16, device=wl.data.device)
    blobs[:, :, :cols] = torch.arange(cols, dtype=torch.int16, device=wl.data.device)
    scale = float(np.float32(dec.range_scale))
    for b in range(wl.B):
        for k in range(wl.T):
            p = wl.data[b, k, :int(wl.counts[b, k]), :3].double()
            row = torch.bucketize(-torch.atan2(p[:, 2], torch.hypot(p[:, 0], p[:, 1])), mids)
            col = torch.round((torch.atan2(p[:, 1], p[:, 0]) - az0) / step).long() % cols
            code = torch.clamp(torch.round(p.norm(dim=1) / scale), 0, 65535).to(torch.int32)
            blobs[b, k, hdr + row * cols + col] = code.to(torch.int16)             # (the bit pattern of the uint16 code)
    return blobs


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    ri = importlib.import_module("a-loam_amd.range_input")
    wl = bench.Workload(syn, torch, "HDL-64", args.batch, args.frames, 0, "cuda")
    B, T, NP = wl.B, wl.T, wl.NP
    model = wl.model
    cpu_model = syn.sensor_model("HDL-64")
    dec = ri.decoder_from_model(cpu_model)
    t0 = time.perf_counter()
    blobs = encode_on_device(torch, wl, dec, model)
    torch.cuda.synchronize()
    encode_s = time.perf_counter() - t0
    BL = blobs.shape[2] * 2                                                        # bytes of one range image
    order = bench.frame_order(T, args.warmup + args.steps)
    NC = 2 if B % 2 == 0 else 1
    BC = B // NC
    ncols = (ctypes.c_int * BC)(*([model.columns] * BC))
    ncols_all = (ctypes.c_int * B)(*([model.columns] * B))
    nin = {(k, c): wl.nin(k, c * BC, (c + 1) * BC) for k in range(T) for c in range(NC)}
    nin_all = {k: wl.nin(k) for k in range(T)}

    def range_ctx(batch):
        cx = wl.ctx(binding, batch, 0)
        cx.set_range_decoder(dec)
        return cx

    def run(ctxs, step):
        for k in order[:args.warmup]:
            step(k)
        for cx in ctxs:
            cx.synchronize()
        t0 = time.perf_counter()
        for k in order[args.warmup:]:
            step(k)
        for cx in ctxs:
            cx.synchronize()
        return (time.perf_counter() - t0) / args.steps

    host16 = wl.data.cpu().pin_memory()
    host12 = wl.data[..., :3].contiguous().cpu().pin_memory()
    hostr = blobs.cpu().pin_memory()
    hostr_steps = blobs.permute(1, 0, 2).contiguous().cpu().pin_memory()           # [T, B, blob]: the bytes of one step back to back, for leg (b)
    stage = torch.empty((B, blobs.shape[2]), dtype=torch.int16, device="cuda")

    def leg_host_float(stride):
        host = host16 if stride == 16 else host12
        ctxs = [wl.ctx(binding, BC, 0) for _ in range(NC)]
        hp, ss = host.data_ptr(), T * NP * stride
        dt = run(ctxs, lambda k: [cx.process_host(hp + c * BC * ss + k * NP * stride, ss, nin[(k, c)], stride) for c, cx in enumerate(ctxs)])
        for cx in ctxs:
            cx.close()
        return B / dt

    def leg_host_range():
        ctxs = [range_ctx(BC) for _ in range(NC)]
        hp, ss = hostr.data_ptr(), T * BL
        dt = run(ctxs, lambda k: [cx.process_range_host(hp + c * BC * ss + k * BL, ss, ncols) for c, cx in enumerate(ctxs)])
        for cx in ctxs:
            cx.close()
        return B / dt

    def leg_copy():                                                                # the same range bytes per step as ONE contiguous pinned hipMemcpyAsync, nothing else
        def step(k):
            stage.copy_(hostr_steps[k], non_blocking=True)
        for k in order[:args.warmup]:
            step(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in order[args.warmup:]:
            step(k)
        torch.cuda.synchronize()
        return B / ((time.perf_counter() - t0) / args.steps)

    def leg_resident(ranges, profile=False):
        cx = range_ctx(B) if ranges else wl.ctx(binding, B, 0)
        if profile:
            cx.profile_enable(True)
        if ranges:
            base, ss = blobs.data_ptr(), T * BL
            dt = run([cx], lambda k: cx.process_range_device(base + k * BL, ss, ncols_all))
        else:
            base = wl.data.data_ptr()
            dt = run([cx], lambda k: cx.process_device(base + k * NP * 16, wl.seq_stride, nin_all[k]))
        prof = None
        if profile:
            p = cx.profile()
            prof = {k: {"ms_per_launch": p[k]["total_ms"] / max(1, p[k]["launches"]), "algorithmic_bytes": p[k]["bytes_per_launch"]} for k in ("k_find_ends", "k_front")}
        cx.close()
        return dt * 1e3, prof

    legs = {"host_fed_16B_sweeps_per_s": lambda: leg_host_float(16), "host_fed_12B_sweeps_per_s": lambda: leg_host_float(12),
            "host_fed_range_sweeps_per_s": leg_host_range, "pinned_copy_of_the_range_bytes_sweeps_per_s": leg_copy,
            "resident_float_ms_per_step": lambda: leg_resident(False)[0], "resident_range_ms_per_step": lambda: leg_resident(True)[0]}
    got = {k: [] for k in legs}
    slots = {"float": {"k_find_ends": [], "k_front": []}, "range": {"k_find_ends": [], "k_front": []}}
    bytes_of = {}
    for _ in range(args.repeats):                                                  # alternated: every pass runs every leg once
        for name, fn in legs.items():
            got[name].append(fn())
        for kind, ranges in (("float", False), ("range", True)):
            _, prof = leg_resident(ranges, profile=True)
            for k in prof:
                slots[kind][k].append(prof[k]["ms_per_launch"])
                bytes_of[(kind, k)] = prof[k]["algorithmic_bytes"]
    res = {"workload": wl.describe(False), "batch": B, "frames": T, "steps": args.steps, "range_image_bytes": BL, "record_bytes_16": NP * 16,
           "encode_s": round(encode_s, 2), "device": torch.cuda.get_device_name(0)}
    res.update({k: stats(v) for k, v in got.items()})
    res["slots_ms_per_launch"] = {kind: {k: dict(stats(v), algorithmic_bytes=bytes_of[(kind, k)]) for k, v in d.items()} for kind, d in slots.items()}
    rate = res["host_fed_range_sweeps_per_s"]["median"]
    copy_cap = 0.85 * res["pinned_copy_of_the_range_bytes_sweeps_per_s"]["median"]
    resident_cap = 0.9 * B / (res["resident_range_ms_per_step"]["median"] * 1e-3)
    res["condition"] = {"85_percent_of_plain_copy": copy_cap, "90_percent_of_resident_range": resident_cap,
                        "binds": "copy" if copy_cap < resident_cap else "resident", "met": bool(rate >= min(copy_cap, resident_cap))}
    res["gain_over_12B"] = rate / res["host_fed_12B_sweeps_per_s"]["median"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
