"""tools/place_rate.py — what place recognition costs on the device: k_place_descriptor for a batch of HDL-64 sweeps
beside a device-to-device copy of the bytes it reads, and aloam_places_match at three shapes - one query against a large store, many
queries against one shared range, many queries each against a range of its own.  Median of --repeats, events on aloam_stream.

    python tools/place_rate.py [--batch 2048] [--repeats 5] [--out place_rate.json]

Every sequence registers the same synthetic sweep (what a descriptor or a match costs does not depend on what is in it); the store is
filled with random records through aloam_places_load.  The descriptor is timed as the difference between an aloam_places_add that has to
make the descriptors and one that finds them made (the add kernel itself copies 10 KB per entry).  Prints one JSON object."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_F32_MATRIX_TF = 157.3
FLOP_PER_PAIR = 2 * 64 * 1200          # the 64 x 1200 product row block one (query, entry) pair costs on the matrix cores (60 of the 64 rows are shifts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--columns", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    B = args.batch
    scans, R, t, model = syn.make_sequence("HDL-64", 1, seed=31, columns=args.columns)
    sweep = scans[0].contiguous()
    n_pts = sweep.shape[0]
    gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=B, max_points=n_pts + 64)
    data = sweep.cuda()[None].expand(B, n_pts, 4).contiguous()
    nin = [n_pts] * B
    own = 256
    gpu.places_enable(max(B * own, 16384))
    stream = torch.cuda.ExternalStream(gpu.stream())

    def timed(fn, prepare=None):
        ms = []
        for _ in range(args.repeats):
            if prepare:
                prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            gpu.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "repeats": args.repeats}

    def register():
        gpu.places_clear()
        gpu.scan_register_device(data.data_ptr(), n_pts * 16, nin)
        gpu.odometry_step()

    seqs = list(range(B))
    register(); gpu.places_add(seqs); gpu.synchronize()                   # warm: code objects
    kept = int(gpu.places_export(0, 1)["n_points"][0])
    with_desc = timed(lambda: gpu.places_add(seqs), prepare=register)
    add_only = timed(lambda: gpu.places_add(seqs), prepare=gpu.places_clear)
    src = torch.empty(B * kept * 16, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src)
    copy(); gpu.synchronize()
    cp = timed(copy)
    desc_ms = with_desc["median_ms"] - add_only["median_ms"]
    gb = B * kept * 16 / 1e9
    res = {"batch": B, "sweep_points_kept": kept,
           "descriptor": {"add_with_descriptors": with_desc, "add_alone": add_only, "k_place_descriptor_ms": desc_ms, "bytes_read_gb": gb,
                          "tb_per_s": gb / desc_ms, "d2d_copy_same_bytes": cp, "d2d_copy_tb_per_s_read_plus_write": 2 * gb / cp["median_ms"]}}

    # the store: random non-negative cells with a few empty columns, 16384 records uploaded once and loaded until every query has a range of its own
    rng = np.random.default_rng(7)
    rec = np.zeros(16384, binding.PLACE_DTYPE)
    rec["cells"] = rng.random((16384, 60, 20), dtype=np.float32) * (rng.random((16384, 60, 1)) > 0.1)
    rec["q"][:, 3] = 1.0
    dev = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    gpu.places_clear()
    while gpu.places_info()["count"] + len(rec) <= gpu.places_info()["capacity"]:
        gpu.places_load(dev)
    gpu.synchronize()
    count = gpu.places_info()["count"]
    out = torch.zeros(B * 16, dtype=torch.uint8, device="cuda")
    shapes = [("one query, 16384 entries", [0], [(0, 16384)]),
              (f"{B} queries, one range of 1024", seqs, [(0, 1024)] * B),
              (f"{B} queries, 256 entries each of its own", seqs, [((own * i) % (count - own + 1), (own * i) % (count - own + 1) + own) for i in range(B)])]
    res["match"] = []
    for name, ids, ranges in shapes:
        call = lambda: gpu.places_match_into(ids, ranges, 1, out.data_ptr())
        call(); gpu.synchronize()                                          # warm: scratch
        tm = timed(call)
        pairs = sum(hi - lo for lo, hi in ranges)
        ns = 1e6 * tm["median_ms"] / pairs
        tf = FLOP_PER_PAIR / ns / 1e3
        res["match"].append({"shape": name, "n": len(ids), "pairs": pairs, "call": tm, "ns_per_pair": ns, "tf_f32": tf,
                             "share_of_157_tf_matrix_peak": tf / PEAK_F32_MATRIX_TF, "untuned_lds_tiled_gemm_tf_for_scale": 122.0})
    gpu.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
