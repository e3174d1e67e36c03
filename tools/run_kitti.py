#!/usr/bin/env python
"""Run the MI355X path on a KITTI-odometry-style folder (the input side of reference src/kittiHelper.cpp, without ROS).

Layout read (reference src/kittiHelper.cpp:68-72,95-134, relative to --dataset):
    sequences/<seq>/times.txt                       one stamp per line
    velodyne/sequences/<seq>/velodyne/%06d.bin      float32 x, y, z, reflectance per point (16 B = the record the C ABI takes)
    results/<seq>.txt                               optional ground truth: 3x4 row-major camera-frame poses, one per line
Ground truth is moved into the lidar / "/camera_init" convention exactly like kittiHelper (R_transform = [0 0 1; -1 0 0; 0 -1 0],
:78-80,104-107).  Output: <out>/<seq>_odometry.txt and (with --mapping) <out>/<seq>_mapped.txt, one line `stamp tx ty tz qx qy qz qw`
per sweep, plus the ATE (RMSE of translation, same start, no alignment) against the ground truth when it is present.

KITTI is not part of this repository or image; `--selftest` writes a tiny synthetic sequence in this layout and runs on it.

Localization against a prior map (one --seq): `--mapping --save-map m.npz` writes the map of the run (both classes' cubes, window centre and
frame count) at its end; a later `--prior-map m.npz` run injects it into a fresh context (aloam_set_map / aloam_set_map_frame, identity
correction or --initial-pose; `--relocalize RADIUS_M YAW_DEG` searches a grid of corrections around that guess after the first frozen step
and installs the best, aloam_score_map_corrections / aloam_apply_map_corrections), freezes the sequence (aloam_set_map_frozen) and writes <out>/<seq>_localized.txt: every sweep localized in
that map, which it leaves unchanged.  The file is a map, not a sequence record: the second run starts its odometry fresh.
`--save-map` holds the final 21 x 21 x 11 window only; `--mapping --save-atlas a.npz` also keeps every cube that left the window on the way
(aloam_map_spill_enable, drained with aloam_export_map_spill after every step) and writes the whole map as tiles (a-loam_amd/atlas.py);
`--prior-atlas a.npz` localizes in such a map of any extent (aloam_atlas_load, aloam_atlas_attach), with --initial-pose / --relocalize as above.
`--save-atlas` also stores a place - the scan-context descriptor of the sweep with its mapped pose, aloam_places_add - every --place-spacing
metres of travel, in the same file; `--prior-atlas a.npz --global-relocalize` then needs no --initial-pose: the first sweep is matched
against the stored places (aloam_places_match), the pose and yaw of the best one become the first guess (a-loam_amd/places.py
guess_from_match), one frozen step is taken from it, relocalize() searches its default grid around it, and the run continues.

`--range-input` hands every sweep over as a 16-bit range image instead of float records (aloam_set_range_decoder, aloam_scan_register_range_host): the
.bin sweep is put back on the grid of an HDL-64 with --range-columns columns (a-loam_amd/range_input.py encode_sweep: nearest ray, range quantised
to 2 mm) - what a driver would hand over had it kept the sensor's own numbers.  Meant for the --selftest drive, whose sensor is known; recorded KITTI
sweeps are motion-compensated and no longer sit on a grid.

`--seqs 00 05 07 ... --batch N` runs several sequences at once by continuous batching (schedule() below): every one of the N slots of one
context runs one sequence; when it ends, the slot is reset in place (aloam_reset_sequences) and takes the next one, and slots with nothing
left sit the step out (aloam_set_active).  `--slice K` time-slices more sequences than slots (schedule_sliced()): after K frames a sequence
is saved (aloam_save_sequences) and the longest-waiting one loaded (aloam_load_sequences).  Each sequence's output files are byte-identical
to running it alone.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R_TRANSFORM = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], float)


def read_times(path):
    """times.txt, one stamp per line, parsed like `stof(line)` (reference src/kittiHelper.cpp:88): single precision."""
    return [float(np.float32(l)) for l in open(path) if l.strip()]


def read_lidar(path):
    """One velodyne/%06d.bin: float32 x, y, z, reflectance per point (reference src/kittiHelper.cpp:25-35 read_lidar_data)."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def read_gt(path):
    """-> (N,3,3) rotations and (N,3) translations in the /camera_init convention of kittiHelper.cpp: every entry goes through
    `stof` (:95-102, single precision), then q = q_transform * q_w_i and t = q_transform * t (:104-107) with
    R_transform = [0 0 1; -1 0 0; 0 -1 0] (:78-80)."""
    P = np.loadtxt(path, dtype=np.float32, ndmin=2).astype(np.float64).reshape(-1, 3, 4)
    return np.einsum("ij,njk->nik", R_TRANSFORM, P[:, :, :3]), P[:, :, 3] @ R_TRANSFORM.T


def schedule(lengths, batch):
    """Continuous batching of sequences with `lengths` sweeps over `batch` slots, without a device: a list of steps
    (active, resets, frames) - active[slot] whether the slot takes part, resets = the slots to reset before the step (a new sequence
    enters them), frames = {slot: (sequence index, frame)} of the active slots.  Sequences enter the slots in order."""
    assert batch >= 1 and all(n >= 0 for n in lengths)
    pending = [i for i, n in enumerate(lengths) if n > 0]
    pending.reverse()
    slot_seq, slot_next = [None] * batch, [0] * batch
    steps = []
    while True:
        resets, frames = [], {}
        for s in range(batch):
            if slot_seq[s] is None or slot_next[s] >= lengths[slot_seq[s]]:
                slot_seq[s] = pending.pop() if pending else None
                slot_next[s] = 0
                if slot_seq[s] is not None:
                    resets.append(s)
            if slot_seq[s] is not None:
                frames[s] = (slot_seq[s], slot_next[s])
                slot_next[s] += 1
        if not frames:
            return steps
        steps.append(([s in frames for s in range(batch)], resets, frames))


def schedule_sliced(lengths, batch, k):
    """Time-sliced continuous batching, without a device: like schedule(), but a resident sequence that has run `k` frames since it entered
    its slot leaves it for the longest-waiting sequence, if one waits.  A list of steps (active, resets, frames, saves, loads): saves = the
    (slot, sequence) pairs to save before the step (the sequence leaves with frames left), then resets = the slots a new sequence enters,
    loads = the (slot, sequence) pairs whose saved record is loaded (the sequence resumes).  Waiting sequences enter in first-in first-out
    order, new ones in order.  With k >= the longest sequence no sequence is preempted and (active, resets, frames) are schedule()'s."""
    assert batch >= 1 and k >= 1 and all(n >= 0 for n in lengths)
    waiting = [i for i, n in enumerate(lengths) if n > 0]
    started = set()
    slot_seq, slot_run, nxt = [None] * batch, [0] * batch, [0] * len(lengths)
    steps = []
    while True:
        saves, resets, loads, frames = [], [], [], {}
        room = len(waiting)                                  # preempt no more sequences than wait
        for s in range(batch):
            i = slot_seq[s]
            if i is not None and nxt[i] >= lengths[i]:
                slot_seq[s] = None                           # finished
            elif i is not None and slot_run[s] >= k and room > 0:
                saves.append((s, i)); waiting.append(i); slot_seq[s] = None; room -= 1
        for s in range(batch):
            if slot_seq[s] is None and waiting:
                i = slot_seq[s] = waiting.pop(0)
                slot_run[s] = 0
                (loads.append((s, i)) if i in started else resets.append(s))
                started.add(i)
            if slot_seq[s] is not None:
                i = slot_seq[s]
                frames[s] = (i, nxt[i])
                nxt[i] += 1; slot_run[s] += 1
        if not frames:
            return steps
        steps.append(([s in frames for s in range(batch)], resets, frames, saves, loads))


def write_selftest(folder, seq="00", frames=6, seed=77):
    syn = importlib.import_module("a-loam_amd.synthetic")
    scans, R, t, model = syn.make_sequence("HDL-64", frames, seed=seed, columns=1024)
    os.makedirs(os.path.join(folder, "sequences", seq), exist_ok=True)
    os.makedirs(os.path.join(folder, "velodyne", "sequences", seq, "velodyne"), exist_ok=True)
    os.makedirs(os.path.join(folder, "results"), exist_ok=True)
    with open(os.path.join(folder, "sequences", seq, "times.txt"), "w") as f:
        f.writelines(f"{0.1 * k:e}\n" for k in range(frames))
    Rn, tn = R.numpy(), t.numpy()
    with open(os.path.join(folder, "results", seq + ".txt"), "w") as f:
        for k in range(frames):                       # camera-frame pose whose kittiHelper image is the lidar pose relative to frame 0
            Rl, tl = Rn[0].T @ Rn[k], Rn[0].T @ (tn[k] - tn[0])
            P = np.concatenate([R_TRANSFORM.T @ Rl, (R_TRANSFORM.T @ tl)[:, None]], 1)
            f.write(" ".join(f"{v:.9e}" for v in P.reshape(-1)) + "\n")
    for k, s in enumerate(scans):
        s.numpy().astype(np.float32).tofile(os.path.join(folder, "velodyne", "sequences", seq, "velodyne", f"{k:06d}.bin"))


PLACE_CAPACITY = 16384                                # --save-atlas: places of one run (about 10 KB of device memory each; 49 km at the default spacing)
SPILL_TILES, SPILL_POINTS = 2048, 1 << 20              # --save-atlas: room per class for what one step's shift empties (it is drained after every step)


def save_map(gpu, path):
    """The map of sequence 0 (aloam_map_cube_counts / aloam_get_map_cube of both classes) with its window centre and frame count."""
    info = gpu.map_info(0)
    out = {"cen": np.array([info["cenW"], info["cenH"], info["cenD"]], np.int32), "frames": np.int32(info["frame_count"])}
    for cls in (0, 1):
        cubes = gpu.map_cubes(cls, 0)
        ids = np.array(sorted(cubes), np.int32)
        out[f"ids{cls}"] = ids
        out[f"counts{cls}"] = np.array([len(cubes[int(i)]) for i in ids], np.int32)
        out[f"points{cls}"] = np.concatenate([cubes[int(i)] for i in ids]) if len(ids) else np.zeros((0, 4), np.float32)
    with open(path, "wb") as f:
        np.savez(f, **out)


def load_prior_map(gpu, path, initial_pose=None):
    """Inject a save_map() file into sequence 0 of a fresh context: its cubes, its window centre, the correction map <- odometry (identity,
    or initial_pose = (tx, ty, tz, yaw)), frame count 0; then freeze the sequence."""
    m = np.load(path)
    for cls in (0, 1):
        ids, cnt, pts = m[f"ids{cls}"], m[f"counts{cls}"], m[f"points{cls}"]
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        gpu.set_map({int(i): pts[off[j]:off[j + 1]] for j, i in enumerate(ids)}, cls, seq=0)
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    if initial_pose is not None:
        tx, ty, tz, yaw = initial_pose
        q, t = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.array([tx, ty, tz])
    gpu.set_map_frame(m["cen"], q, t, 0, seq=0)
    gpu.set_map_frozen([1])
    return q, t


def load_prior_atlas(gpu, path, initial_pose=None):
    """Load a --save-atlas file into the context's atlas and attach sequence 0 to it: its window is cut from the atlas wherever it goes.
    Correction and frame count as load_prior_map; the first step cuts the window around the guess."""
    atlas = importlib.import_module("a-loam_amd.atlas")
    tiles, points = atlas.load_atlas(path)
    gpu.atlas_load(tiles, points)
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    if initial_pose is not None:
        tx, ty, tz, yaw = initial_pose
        q, t = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.array([tx, ty, tz])
    gpu.set_map_frozen([1])
    gpu.atlas_attach([1])
    gpu.set_map_frame((10, 10, 5), q, t, 0, seq=0)
    return q, t


def global_guess(gpu, stored):
    """The first guess of --global-relocalize, with no prior: sequence 0's sweep (registered, odometry step taken) matched against the
    stored places; the best one's pose and yaw as the map <- odometry correction, installed for the first frozen step."""
    places = importlib.import_module("a-loam_amd.places")
    m = gpu.places_match([0])[0, 0]
    if m["entry"] < 0:
        sys.exit("--global-relocalize: no stored place matches the first sweep (an empty sweep, or an atlas without places)")
    odom = gpu.pose(0)
    q, t = places.guess_from_match(stored["q"][m["entry"]], stored["t"][m["entry"]], int(m["shift"]), odom["q_w"], odom["t_w"])
    gpu.set_map_frame((10, 10, 5), q, t, 0, seq=0)
    print(f"matched place {int(m['entry'])} of {len(stored)} (frame {int(stored['frame'][m['entry']])}), shift {int(m['shift'])} "
          f"({int(m['shift']) * places.SECTOR_DEG:.0f} deg), distance {float(m['distance']):.3f}")
    return q, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", help="dataset_folder of kitti_helper.launch")
    ap.add_argument("--seq", default="00")
    ap.add_argument("--seqs", nargs="+", help="several sequences, run together by continuous batching over --batch slots")
    ap.add_argument("--batch", type=int, default=1, help="slots of the context with --seqs")
    ap.add_argument("--slice", type=int, default=0, help="with --seqs: time slices of this many frames; a preempted sequence is saved into pinned host "
                                                        "memory (aloam_save_sequences) and later loaded into whichever slot is free (schedule_sliced)")
    ap.add_argument("--out", default="kitti_out")
    ap.add_argument("--mapping", action="store_true")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--selftest", action="store_true")
    ap.add_argument("--reference-order", action="store_true", help="sum voxel members in pcl::VoxelGrid's own order (the reference's bits; ~4x slower for one sensor): for runs that are compared pose by pose with A-LOAM's")
    ap.add_argument("--distortion", action="store_true", help="per-point interpolation ratio (the reference's DISTORTION 1; real KITTI sweeps are already de-skewed, so the reference ships 0)")
    ap.add_argument("--save-map", metavar="FILE.npz", help="with --mapping, one --seq: write the map of the run (cubes of both classes, cen, frame count) at its end")
    ap.add_argument("--save-atlas", metavar="FILE.npz", help="with --mapping, one --seq: write the whole map of the run as tiles (a-loam_amd/atlas.py): every cube "
                                                             "that left the 21 x 21 x 11 window on the way (the map spill, drained after every step) and the final window")
    ap.add_argument("--prior-map", metavar="FILE.npz", help="one --seq: localize every sweep against this --save-map file, frozen (the map is not "
                                                            "changed); writes <seq>_localized.txt")
    ap.add_argument("--prior-atlas", metavar="FILE.npz", help="one --seq: like --prior-map, against a --save-atlas file of any extent (aloam_atlas_load / "
                                                              "aloam_atlas_attach: the window is cut from the atlas wherever the sensor goes)")
    ap.add_argument("--initial-pose", nargs=4, type=float, metavar=("TX", "TY", "TZ", "YAW"), help="with --prior-map: the first guess of the map <- odometry "
                                                                                                  "correction (metres, radians); default identity")
    ap.add_argument("--relocalize", nargs=2, type=float, metavar=("RADIUS_M", "YAW_DEG"), help="with --prior-map: after the first frozen step, score a grid of "
                    "corrections of this half-width (0.5 m, 2.5 deg cells) around the first guess on the device, install the best, continue")
    ap.add_argument("--place-spacing", type=float, default=3.0, metavar="METRES", help="with --save-atlas: also store a place (scan-context descriptor + mapped "
                    "pose) every this many metres of travel, in the same file; 0 stores none")
    ap.add_argument("--global-relocalize", action="store_true", help="with --prior-atlas, instead of --initial-pose: match the first sweep against the places "
                    "stored in the atlas file, start from the best one's pose and yaw, then search relocalize()'s default grid around it")
    ap.add_argument("--range-input", action="store_true", help="hand the sweeps over as 16-bit range images (encoded from the .bin points on the grid of an "
                    "HDL-64 with --range-columns columns) through the range entry points")
    ap.add_argument("--range-columns", type=int, default=1024, help="with --range-input: columns of the sensor grid (the --selftest drive has 1024)")
    ap.add_argument("--pose-information", action="store_true", help="after every step, also export the information matrix of each slot's odometry solve (and, "
                    "with --mapping, of its mapping solve): <seq>_info_odom.npy / <seq>_info_map.npy beside the poses, one record of "
                    "binding.POSE_INFORMATION_DTYPE per sweep (a-loam_amd/information.py: covariance(), degeneracy())")
    args = ap.parse_args()
    if args.global_relocalize and not args.prior_atlas:
        ap.error("--global-relocalize needs --prior-atlas")
    if args.global_relocalize and (args.initial_pose or args.relocalize):
        ap.error("--global-relocalize replaces --initial-pose and --relocalize")
    if args.prior_atlas and args.prior_map:
        ap.error("--prior-atlas and --prior-map exclude each other")
    prior_atlas = args.prior_atlas
    if prior_atlas:                                    # everything else treats it as a prior map
        args.prior_map = prior_atlas
    if args.relocalize and not args.prior_map:
        ap.error("--relocalize needs --prior-map")
    if (args.save_map or args.prior_map) and args.seqs:
        ap.error("--save-map / --prior-map / --prior-atlas take one --seq, not --seqs")
    if args.save_map and not args.mapping:
        ap.error("--save-map needs --mapping")
    if args.save_atlas and not args.mapping:
        ap.error("--save-atlas needs --mapping")
    if args.save_atlas and (args.seqs or args.prior_map):
        ap.error("--save-atlas takes one --seq that maps (no --seqs, no --prior-map)")
    if args.initial_pose and not args.prior_map:
        ap.error("--initial-pose needs --prior-map")
    if args.prior_map:
        args.mapping = True
    seqs = args.seqs or [args.seq]
    if args.selftest:
        args.dataset = os.path.join(args.out, "selftest_dataset")
        for i, seq in enumerate(seqs):                 # sequences of unequal length, so that slots finish at different steps
            write_selftest(args.dataset, seq, frames=6 + 2 * (i % 3), seed=77 + i)
    binding = importlib.import_module("a-loam_amd.binding")
    times = []
    for seq in seqs:
        ts = read_times(os.path.join(args.dataset, "sequences", seq, "times.txt"))
        times.append(ts[: args.max_frames] if args.max_frames else ts)
    batch = args.batch if args.seqs else 1
    # launch/aloam_velodyne_HDL_64.launch: scan_line 64, minimum_range 5, mapping resolutions 0.4 / 0.8
    gpu = binding.Aloam(n_scans=64, min_range=5.0, batch=batch, max_points=140000, distortion=args.distortion)
    if args.reference_order:
        gpu.set_voxel_sum_order(True)
    rin = None
    if args.range_input:                               # the sensor of the drive, and its decoder
        rin = importlib.import_module("a-loam_amd.range_input")
        range_model = importlib.import_module("a-loam_amd.synthetic").sensor_model("HDL-64", columns=args.range_columns)
        range_dec = rin.decoder_from_model(range_model)
        gpu.set_range_decoder(range_dec)
    if args.mapping:
        gpu.mapping_enable(0.4, 0.8, pool_points=1 << 17)          # where the map starts: the pools double as it grows (src/laserMapping.cpp:737-783 push_back)
    os.makedirs(args.out, exist_ok=True)
    import torch                                       # (after the binding: it loads torch's HIP runtime first)
    rec_buf = torch.empty(batch * ctypes.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)   # the poses of a step, written by the device
    recs = (binding.AloamPoseRecord * batch).from_address(rec_buf.data_ptr())
    odo, mapped = [[] for _ in seqs], [[] for _ in seqs]
    info_kinds = ([("odom", binding.INFO_ODOMETRY)] + ([("map", binding.INFO_MAPPING)] if args.mapping else [])) if args.pose_information else []
    info_buf = {name: torch.zeros(batch * binding.POSE_INFORMATION_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True) for name, _ in info_kinds}
    info_rows = {name: [[] for _ in seqs] for name, _ in info_kinds}
    spill = None                                       # --save-atlas: the pinned destinations of the drain that follows every mapping step
    if args.save_atlas:
        atlas = importlib.import_module("a-loam_amd.atlas")
        gpu.map_spill_enable(SPILL_TILES, SPILL_POINTS)
        spill = {"tiles": torch.zeros(2 * SPILL_TILES * 32, dtype=torch.uint8, pin_memory=True), "points": torch.zeros((2 * SPILL_POINTS, 4), dtype=torch.float32, pin_memory=True),
                 "off": torch.zeros(4, dtype=torch.int64, pin_memory=True), "log": atlas.TileLog()}
        if args.place_spacing > 0:
            gpu.places_enable(PLACE_CAPACITY)
    last_place = None                                  # --save-atlas: mapped position of the last stored place
    stored = None                                      # --global-relocalize: the places of the atlas file
    if args.global_relocalize:
        stored = importlib.import_module("a-loam_amd.atlas").load_atlas_places(prior_atlas)
        if not len(stored):
            sys.exit(f"--global-relocalize: {prior_atlas} holds no places (written without --place-spacing?)")
        gpu.places_enable(len(stored))
        gpu.places_load(stored)
    factors = []                                       # --prior-map: last-iteration factors of every sweep (aloam_get_map_info), the fit to the map
    idle = np.zeros((0, 4), np.float32)
    lengths = [len(ts) for ts in times]
    plan = schedule_sliced(lengths, batch, args.slice) if args.slice > 0 else [(*st, [], []) for st in schedule(lengths, batch)]
    parked = {}                                        # sequence -> (record bytes in pinned host memory, offsets)
    guess = None                                       # --prior-map: the first guess, until --relocalize has searched around it
    for active, resets, frames, saves, loads in plan:
        if saves:
            blob, off = gpu.save_sequences([s for s, _ in saves])
            for j, (_, i) in enumerate(saves):
                parked[i] = (blob[off[j]:off[j + 1]], np.array([0, off[j + 1] - off[j]], np.int64))
        for s, i in loads:
            gpu.load_sequences([s], *parked.pop(i))
        if resets:
            gpu.reset_sequences(resets)                # a new sequence enters these slots: a fresh context's state, in place
            if args.prior_map:                         # (one --seq: only slot 0, at the first step) the map goes in after that reset
                guess = (load_prior_atlas if prior_atlas else load_prior_map)(gpu, args.prior_map, args.initial_pose)
        gpu.set_active(None if all(active) else active)
        scans = [idle] * batch
        for slot, (i, k) in frames.items():
            scans[slot] = read_lidar(os.path.join(args.dataset, "velodyne", "sequences", seqs[i], "velodyne", f"{k:06d}.bin"))
        if rin:
            blobs = [rin.encode_sweep(x, range_model, range_dec)[0] if len(x) else np.zeros(0, np.uint16) for x in scans]
            gpu.scan_register_range(blobs, [args.range_columns if len(x) else 0 for x in scans])
        else:
            gpu.scan_register(scans)
        gpu.odometry_step()
        if stored is not None and guess is not None:   # the first sweep: its best stored place is the first guess
            guess = global_guess(gpu, stored)
        if args.mapping:
            gpu.mapping_step()
        if spill:                                      # stream-ordered, no synchronise of its own: read after the step's synchronize() below
            gpu.export_map_spill_into([0], spill["tiles"].data_ptr(), 2 * SPILL_TILES, spill["points"].data_ptr(), 2 * SPILL_POINTS, spill["off"].data_ptr(), clear=True)
        if (args.relocalize or stored is not None) and guess is not None:   # the first frozen step has left its stacks and submap grid: search around the first guess
            relocalize = importlib.import_module("a-loam_amd.relocalize")
            grid = dict(radius_m=args.relocalize[0], step_m=0.5, yaw_deg=args.relocalize[1], yaw_step_deg=2.5) if args.relocalize else {}
            found = relocalize.relocalize(gpu, [0], guesses={0: guess}, **grid)[0]
            b, node = found["scores"][found["best"]], found["nodes"][found["best"]]
            print(f"{seqs[0]} relocalized: {len(found['nodes'])} corrections scored, best node ({node[0]:+.1f} m, {node[1]:+.1f} m, {node[2]:+.1f} deg) "
                  f"with {int(b['corner_factors']) + int(b['surf_factors'])} factors")
            guess = None
        gpu.export_poses(rec_buf.data_ptr())           # odometry and mapped poses of every slot in one call
        for name, which in info_kinds:                 # --pose-information: one more stream-ordered call per kind, every slot listed
            gpu.export_pose_information_into(which, range(batch), info_buf[name].data_ptr())
        try:
            gpu.synchronize()
        except binding.AloamError as e:
            if spill and "map spill full" in str(e):
                sys.exit(f"--save-atlas: one step's window shift emptied more than {SPILL_TILES} cubes or {SPILL_POINTS} points of one class; the atlas would be "
                         f"incomplete.  Raise SPILL_TILES / SPILL_POINTS in tools/run_kitti.py.  ({e})")
            raise
        for slot, (i, k) in frames.items():
            r = recs[slot]
            odo[i].append([times[i][k], *r.t_w, *r.q_w])
            if args.mapping:
                mapped[i].append([times[i][k], *r.map_t_w, *r.map_q_w])
            for name, _ in info_kinds:
                info_rows[name][i].append(info_buf[name].numpy().view(binding.POSE_INFORMATION_DTYPE)[slot].copy())
        if spill and int(spill["off"][1]):             # (the rows hold at most what the destinations hold: a drain is always written)
            nt, npts = int(spill["off"][1]), int(spill["off"][3])
            spill["log"].add(spill["tiles"].numpy()[:nt * 32].view(atlas.TILE_DTYPE), spill["points"].numpy()[:npts])
        if spill and args.place_spacing > 0 and gpu.places_info()["count"] < PLACE_CAPACITY:
            here = np.array(recs[0].map_t_w)
            if last_place is None or np.linalg.norm(here - last_place) >= args.place_spacing:
                gpu.places_add([0])                    # the sweep just mapped, with the pose the step has given it
                last_place = here
        if args.prior_map:
            info = gpu.map_info(0)
            factors.append(info["corner_num1"] + info["surf_num1"])
    if args.save_map:
        save_map(gpu, args.save_map)
    if args.save_atlas:
        tiles, points = spill["log"].result(atlas.window_tiles(gpu, 0))
        stored_now = gpu.places_export() if args.place_spacing > 0 else None
        atlas.save_atlas(args.save_atlas, tiles, points, places=stored_now)
        print(f"{seqs[0]} atlas: {len(tiles)} tiles, {len(points)} points, {0 if stored_now is None else len(stored_now)} places ({sum(len(t) for t, _ in spill['log'].parts)} tiles left the window on the way)")
    gpu.close()
    mapped_name = "localized" if args.prior_map else "mapped"
    if factors:
        print(f"{seqs[0]} localized: factors per sweep (last iteration) min {min(factors)}, mean {np.mean(factors):.0f}")
    for i, seq in enumerate(seqs):
        np.savetxt(os.path.join(args.out, f"{seq}_odometry.txt"), np.array(odo[i]), fmt="%.9e")
        if mapped[i]:
            np.savetxt(os.path.join(args.out, f"{seq}_{mapped_name}.txt"), np.array(mapped[i]), fmt="%.9e")
        for name, _ in info_kinds:
            rows = np.array(info_rows[name][i], dtype=binding.POSE_INFORMATION_DTYPE)
            np.save(os.path.join(args.out, f"{seq}_info_{name}.npy"), rows)
            ok = rows[rows["status"] == binding.INFO_OK]
            if args.selftest and len(ok):
                ratio = ok["trans_eigenvalues"][:, 0] / ok["trans_eigenvalues"][:, 1]
                print(f"{seq} pose information ({name}): {len(ok)} of {len(rows)} sweeps with a matrix, translation lambda0 / lambda1 in [{ratio.min():.3f}, {ratio.max():.3f}]")
        gt_path = os.path.join(args.dataset, "results", seq + ".txt")
        if os.path.exists(gt_path):
            Rg, tg = read_gt(gt_path)
            tg = (tg[: len(odo[i])] - tg[0]) @ Rg[0]   # same start as the estimate (identity at the first sweep)
            for name, tr in (("odometry", odo[i]), (mapped_name, mapped[i])):
                if tr:
                    e = np.array(tr)[:, 1:4] - tg
                    print(f"{seq} {name}: {len(tr)} sweeps, ATE (RMSE, no alignment) = {np.sqrt((e ** 2).sum(1).mean()):.4f} m, final error = {np.linalg.norm(e[-1]):.4f} m")


if __name__ == "__main__":
    main()
