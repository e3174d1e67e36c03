"""tools/atlas_rate.py — what keeping the cubes that leave the window costs (aloam_map_spill_enable, aloam_export_map_spill): bench.py's
configs[2] workload (512 travelling sequences, synthetic HDL-64) is brought to steady-state map depth with normal mapping steps and saved;
two contexts, one with the spill enabled and one without (which launches what a library without the spill launches), load that state and
are timed against each other, alternated.

    python tools/atlas_rate.py [--batch 512] [--frames 84] [--warmup 80] [--repeats 5] [--out atlas_rate.json]
    rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/atlas_rate.py --repeats 1        (per-kernel times; never with counters)

  no_shift      a normal mapping step in which no window moves (almost every step): host clock around the step and a synchronise
  spilling      a step in which every window is moved so far that every cube from the sensor's column on falls off (aloam_set_map_frame):
                the map_begin profiling scope of both contexts (its difference is k_map_spill), tiles, points and bytes spilled
  --atlas       aloam_atlas_load of sequence 0's window (host clock; it synchronises), its device bytes against one copy per slot, and the
                map_begin scope of a frozen step of unattached sequences, of attached ones whose windows are all cut anew, and of attached
                ones with nothing to do
  export        aloam_export_map_spill of all slots, empty (the every-step drain of a recording run) and after the spilling step, into
                device and pinned memory: host clock around the call and a synchronise
Prints one JSON object.
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

MAX_TILES, MAX_POINTS = 512, 1 << 17


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512, help="sequences (configs[2]: 512)")
    ap.add_argument("--frames", type=int, default=84, help="distinct sweeps per sequence")
    ap.add_argument("--warmup", type=int, default=80, help="normal mapping steps before the state is saved (steady-state map depth)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--atlas", action="store_true", help="time the atlas instead of the spill: aloam_atlas_load of sequence 0's window, and a frozen step in which "
                                                         "all windows are cut from it, against a frozen step of unattached sequences")
    args = ap.parse_args()
    assert args.warmup + 2 <= args.frames

    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("a-loam_amd.binding")
    syn = importlib.import_module("a-loam_amd.synthetic")
    wl = bench.TravelWorkload(syn, torch, args.batch, args.frames, 0, "cuda")
    B, k0 = wl.B, args.warmup
    ctxs = {}
    for name in ("off", "on"):
        g = wl.ctx(binding, B, 0)
        g.mapping_enable(0.4, 0.8, 262144)
        ctxs[name] = g
    ctxs["on"].map_spill_enable(MAX_TILES, MAX_POINTS)

    def sweep(g, k):
        g.process_device(wl.data.data_ptr() + k * wl.NP * 16, wl.seq_stride, wl.nin(k))

    g = ctxs["off"]
    for k in range(k0):
        sweep(g, k)
        g.mapping_step()
    g.synchronize()
    blob, off = g.save_sequences(range(B), pinned=False)

    def prepared(name, edge):
        """The saved state in context `name`, frame k0 run untimed, frame k0 + 1 registered; edge: every window then moved so that the
        cubes from the sensor's column on fall off in the next step."""
        g = ctxs[name]
        g.load_sequences(range(B), blob, off)
        sweep(g, k0)
        g.mapping_step()
        sweep(g, k0 + 1)
        g.synchronize()
        if edge:
            for b in range(B):
                info, p = g.map_info(b), g.map_pose(b)
                # the centre cube goes from index cx to cx - 18: the loop shifts s = 21 - cx times and every cube from column cx on falls off
                cen = (info["cenW"] - 18, info["cenH"], info["cenD"])
                g.set_map_frame(cen, p["q_wmap_wodom"], p["t_wmap_wodom"], info["frame_count"], seq=b)
            g.synchronize()
        return g

    def timed_step(name, edge=False, profile=False):
        g = prepared(name, edge)
        if profile:
            g.profile_enable(True)
        t0 = time.perf_counter()
        g.mapping_step()
        g.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        begin = None
        if profile:
            p = g.profile()["map_begin"]
            begin = p["total_ms"] / max(1, p["launches"])
            g.profile_enable(False)
        return dt, begin

    def buffers(pinned, n_tiles, n_points):
        where = {"pin_memory": True} if pinned else {"device": "cuda"}
        return (torch.zeros(max(1, n_tiles) * 32, dtype=torch.uint8, **where), torch.zeros((max(1, n_points), 4), dtype=torch.float32, **where),
                torch.zeros(2 * (B + 1), dtype=torch.int64, pin_memory=True))

    def timed_export(bufs, clear):
        g = ctxs["on"]
        tl, pt, of = bufs
        g.synchronize()
        t0 = time.perf_counter()
        g.export_map_spill_into(range(B), tl.data_ptr(), len(tl) // 32, pt.data_ptr(), len(pt), of.data_ptr(), clear=clear)
        g.synchronize()
        return 1e3 * (time.perf_counter() - t0), int(of[B]), int(of[2 * B + 1])

    res = {"workload": wl.describe(True) + f", state saved after {k0} normal steps", "batch": B, "max_tiles": MAX_TILES, "max_points": MAX_POINTS}
    if args.atlas:
        atlas = importlib.import_module("a-loam_amd.atlas")
        g = ctxs["on"]
        prepared("on", False)
        tiles, points = atlas.window_tiles(g, 0)
        loads = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            g.atlas_load(tiles, points)
            loads.append(1e3 * (time.perf_counter() - t0))
        info = g.atlas_info()
        res["atlas"] = {"tiles": len(tiles), "points": len(points), "load_ms": stats(loads), "device_bytes": info["device_bytes"],
                        "per_slot_copies_bytes": B * len(points) * 16, "largest_window": info["largest_window"]}
        scopes = {"frozen": [], "attached_recut": [], "attached_no_shift": []}
        for _ in range(args.repeats):                                       # alternated; every variant starts from the loaded state
            for name in scopes:
                g.atlas_attach([name != "frozen"] * B)
                g.set_map_frozen([True] * B)
                prepared("on", False)                                       # (its untimed step has cut the attached windows: the next one finds nothing to do)
                if name == "attached_recut":                                # attaching anew marks every window stale: the timed step cuts all of them
                    g.atlas_attach(None)
                    g.atlas_attach([True] * B)
                g.profile_enable(True)
                g.mapping_step()
                g.synchronize()
                p = g.profile()["map_begin"]
                scopes[name].append(p["total_ms"] / max(1, p["launches"]))
                g.profile_enable(False)
        res["atlas"]["map_begin_scope_ms"] = {name: stats(v) for name, v in scopes.items()}
        res["atlas"]["recut_bytes"] = B * sum(info["points"]) * 16
        g.atlas_attach(None)
        for g in ctxs.values():
            g.close()
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    for name in ctxs:                                                       # warm both contexts (code objects, allocations)
        timed_step(name)
    times = {"off": [], "on": []}
    for _ in range(args.repeats):                                           # alternated, so that both see the same machine state
        for name in times:
            times[name].append(timed_step(name)[0])
    res["no_shift_mapping_step_ms"] = {name: stats(v) for name, v in times.items()}
    res["no_shift_map_begin_scope_ms"] = {name: timed_step(name, profile=True)[1] for name in ctxs}
    res["export_empty_ms"] = {}
    for pinned in (False, True):
        bufs = buffers(pinned, 1024, 1024)
        timed_export(bufs, True)
        res["export_empty_ms"]["pinned" if pinned else "device"] = stats([timed_export(bufs, True)[0] for _ in range(args.repeats)])
    begin = {name: [] for name in ctxs}
    for _ in range(max(1, args.repeats // 2)):
        for name in ctxs:
            if name == "on":                                                # start from empty rows: a size query, then a drain that holds it
                _, nt, npts = timed_export(buffers(False, 1, 1), False)
                timed_export(buffers(False, nt, npts), True)
            begin[name].append(timed_step(name, edge=True, profile=True)[1])
    res["spilling_map_begin_scope_ms"] = {name: stats(v) for name, v in begin.items()}
    _, n_tiles, n_points = timed_export(buffers(False, 1, 1), False)        # the size query
    res["spilled"] = {"tiles": n_tiles, "points": n_points, "bytes": n_tiles * 32 + n_points * 16}
    res["export_spilled_ms"] = {}
    for pinned in (False, True):                                            # clear = 0: the same spill is drained by every repeat
        bufs = buffers(pinned, n_tiles, n_points)
        runs = [timed_export(bufs, False) for _ in range(args.repeats + 1)][1:]
        res["export_spilled_ms"]["pinned" if pinned else "device"] = stats([r[0] for r in runs])
    dropped = sum(ctxs["on"].map_spill_info(b)["dropped_tiles"] for b in range(B))
    res["dropped_tiles"] = dropped
    for g in ctxs.values():
        try:
            g.synchronize()
        except binding.AloamError as e:                                     # (a full spill is reported here, and in dropped_tiles)
            res["synchronize"] = str(e)
        g.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
