"""Scoring and applying batches of map-pose hypotheses on the MI355X (aloam_score_map_corrections / aloam_apply_map_corrections): the factor
counts are exactly those of a frozen mapping step started from the candidate, every field agrees with the numpy model built from the
oracle's primitives, scoring writes nothing and is deterministic, any batch shape equals single-candidate calls, sequences without a frozen
step's state are refused before anything is queued, an applied candidate continues bit for bit like aloam_set_map_frame's, and a grid search
brings every guess of the +-3 m / +-10 deg spread into the basin the frozen steps converge from."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import relocalize_model as M
from test_gpu_checkpoint import make
from test_gpu_localization import GUESSES, _quat_of, frame, pose_part
from test_gpu_sequence_lifecycle import diff, snap

pytestmark = pytest.mark.gpu
F, G = 12, 5                                                              # frames mapped into the record, frozen frames after it
EXTRA_GUESSES = [(2.8, -1.3, 7.0), (-3.0, 3.0, -10.0), (0.7, 2.2, -4.0)]  # displaced guesses that are no grid multiples
GRID = dict(radius_m=3.5, step_m=0.5, yaw_deg=12.5, yaw_step_deg=2.5)     # 15 x 15 x 11 = 2475 nodes, one within 0.36 m / 1.25 deg of any guess


@pytest.fixture(scope="module")
def reloc():
    return importlib.import_module("a-loam_amd.relocalize")


@pytest.fixture(scope="module")
def rec(binding, sequence):
    """One saved record: HDL-64, 12 frames mapped, seed 44 (the drive of test_multi_hypothesis_best_score_is_the_truth)."""
    scans, R, t, model = sequence("HDL-64", F + G, seed=44, columns=512)
    mp = max(len(s) for s in scans) + 64
    A = make(binding, model, 1, mp, True)
    for k in range(F):
        frame(A, [scans[k]])
    blob, off = A.save_sequences([0])
    truth, info = A.map_pose(0), A.map_info(0)
    A.close()
    return dict(scans=scans, R=R, t=t, model=model, mp=mp, blob=blob.copy(), off=off, truth=truth, cen=(info["cenW"], info["cenH"], info["cenD"]),
                frame_count=info["frame_count"])


def loaded(binding, rec, B, sweeps=None, fresh=()):
    """A context whose B slots hold the record (the slots in `fresh` are reset again: no map, first frame) and have taken frame F through
    registration and odometry (sweeps: per-slot sweep)."""
    g = make(binding, rec["model"], B, rec["mp"], True)
    n = rec["off"][1] - rec["off"][0]
    g.load_sequences(list(range(B)), np.concatenate([rec["blob"]] * B), (np.arange(B + 1) * n).astype(np.int64))
    g.reset_sequences(list(fresh))
    g.set_active([True] * B)
    g.scan_register(sweeps if sweeps is not None else [rec["scans"][F]] * B)
    g.odometry_step()
    return g


def displaced(reloc, rec, dx, dy, dyaw):
    """The true correction turned by dyaw degrees about the sensor and moved by (dx, dy): the construction of the multi-hypothesis test."""
    tr = rec["truth"]
    if dx == 0 and dy == 0 and dyaw == 0:
        return tr["q_wmap_wodom"].copy(), tr["t_wmap_wodom"].copy()         # the truth itself, bit for bit
    h = math.radians(dyaw) / 2
    dq = np.array([0.0, 0.0, math.sin(h), math.cos(h)])
    c = tr["t_w"]
    return reloc._qmul(dq, tr["q_wmap_wodom"]), reloc._qrot(dq, tr["t_wmap_wodom"] - c) + c + np.array([dx, dy, 0.0])


def spread(reloc, rec, K, seed=5):
    """K corrections over +-3 m / +-10 deg around the truth; the first is the truth itself."""
    rng = np.random.default_rng(seed)
    d = [(0.0, 0.0, 0.0)] + [(float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), float(rng.uniform(-10, 10))) for _ in range(K - 1)]
    qt = [displaced(reloc, rec, *x) for x in d]
    return np.array([q for q, _ in qt]), np.array([t for _, t in qt]), d


def model_inputs(binding, gpu, b):
    """What the model needs, read back with the getters: stacks, the window's cubes in window order, the odometry pose of the frame."""
    info, p, od = gpu.map_info(b), gpu.map_pose(b), gpu.pose(b)
    cen = (info["cenW"], info["cenH"], info["cenD"])
    cubes = [gpu.map_cubes(cls, b) for cls in (0, 1)]
    return dict(stack_c=gpu.map_cloud(binding.MAP_CORNER_STACK, b), stack_s=gpu.map_cloud(binding.MAP_SURF_STACK, b), cubes=cubes, cen=cen,
                q_wodom=od["q_w"], t_wodom=od["t_w"], info=info, pose=p)


def model_scores(inp, center, q, t):
    return M.score_model(inp["stack_c"], inp["stack_s"], M.submap(inp["cubes"][0], center), M.submap(inp["cubes"][1], center), inp["q_wodom"], inp["t_wodom"],
                         list(zip(q, t)))


def state(binding, gpu, b):
    s = snap(binding, gpu, b, True)
    s["stacks"] = [gpu.map_cloud(w, b).tobytes() for w in (binding.MAP_CORNER_STACK, binding.MAP_SURF_STACK)]
    return s


@pytest.fixture(scope="module")
def scored(binding, rec, reloc):
    """Slot 0 keeps the record's correction; slot 1 + c starts its frozen step of the same frame from candidate c (aloam_set_map_frame)."""
    K = 32
    q, t, d = spread(reloc, rec, K)
    g = loaded(binding, rec, K + 2)                                        # the last slot is never listed
    for c in range(K):
        g.set_map_frame(rec["cen"], q[c], t[c], rec["frame_count"], seq=1 + c)
    g.set_map_frozen([True] * (K + 2))
    g.mapping_step()
    g.synchronize()
    yield dict(gpu=g, q=q, t=t, d=d, K=K, cand=binding.map_corrections(q, t))
    g.close()


def test_factor_counts_equal_a_frozen_step_from_the_candidate(binding, rec, scored):
    g, K = scored["gpu"], scored["K"]
    sc, best = g.score_map_corrections([0], scored["cand"])
    inp = model_inputs(binding, g, 0)
    center0 = M.center_cube(M.start_pose(inp["q_wodom"], inp["t_wodom"], rec["truth"]["q_wmap_wodom"], rec["truth"]["t_wmap_wodom"]), rec["cen"])
    kept = 0
    for c in range(K):
        i = g.map_info(1 + c)
        center = M.center_cube(M.start_pose(inp["q_wodom"], inp["t_wodom"], scored["q"][c], scored["t"][c]), rec["cen"])
        print(f"candidate {c:2d} {scored['d'][c]}: scored {sc[0, c]['corner_factors']} / {sc[0, c]['surf_factors']}, step {i['corner_num0']} / {i['surf_num0']}")
        if (i["cenW"], i["cenH"], i["cenD"]) != inp["cen"] or center != center0:
            continue
        kept += 1
        assert (int(sc[0, c]["corner_factors"]), int(sc[0, c]["surf_factors"])) == (i["corner_num0"], i["surf_num0"]), (c, scored["d"][c], sc[0, c], i)
    assert kept >= 28, kept
    i0 = g.map_info(0)                                                    # candidate 0 is the correction slot 0 itself started from
    assert (int(sc[0, 0]["corner_factors"]), int(sc[0, 0]["surf_factors"])) == (i0["corner_num0"], i0["surf_num0"])
    assert len({(int(s["corner_factors"]), int(s["surf_factors"])) for s in sc[0]}) > K // 2     # the candidates are told apart


def test_scores_equal_the_model(binding, rec, scored):
    g, K = scored["gpu"], scored["K"]
    sc, best = g.score_map_corrections([0], scored["cand"])
    inp = model_inputs(binding, g, 0)
    center = M.center_cube(M.start_pose(inp["q_wodom"], inp["t_wodom"], rec["truth"]["q_wmap_wodom"], rec["truth"]["t_wmap_wodom"]), rec["cen"])
    want = model_scores(inp, center, scored["q"], scored["t"])
    for c in range(K):
        for k in ("corner_factors", "surf_factors", "corner_found", "surf_found"):
            assert int(sc[0, c][k]) == want[c][k], (c, k, sc[0, c], want[c])
        rel = abs(float(sc[0, c]["cost"]) - want[c]["cost"]) / max(want[c]["cost"], 1e-300)
        print(f"candidate {c:2d}: cost {float(sc[0, c]['cost']):.12g} model {want[c]['cost']:.12g} rel {rel:.2e}")
        assert rel <= 1e-9, (c, sc[0, c], want[c])
    assert int(best[0]) == M.best_of(want)


def test_scoring_writes_nothing_and_is_deterministic(binding, rec, scored):
    g, K = scored["gpu"], scored["K"]
    listed, unlisted = [5, 0, 17], K + 1
    before = {b: state(binding, g, b) for b in listed + [unlisted]}
    a, best_a = g.score_map_corrections(listed, scored["cand"])
    b, best_b = g.score_map_corrections(listed, scored["cand"], pinned=False)
    assert a.tobytes() == b.tobytes() and best_a.tobytes() == best_b.tobytes()
    for s in listed + [unlisted]:
        assert not diff(state(binding, g, s), before[s]), s
    # every slot took the same sweep against the same map: a score does not depend on the correction the slot itself holds
    assert a[0].tobytes() == a[1].tobytes() == a[2].tobytes()
    # a constructed tie: the best candidate twice, the copy first - the lower index wins
    w = int(best_a[0])
    tie = np.concatenate([scored["cand"][w:w + 1], scored["cand"]])
    t, best_t = g.score_map_corrections([0], tie)
    assert t[0, 0].tobytes() == t[0, 1 + w].tobytes() == a[1, w].tobytes() and int(best_t[0]) == 0
    last = np.concatenate([scored["cand"], scored["cand"][w:w + 1]])
    assert int(g.score_map_corrections([0], last)[1][0]) == w


def _single_calls(torch, g, seqs, cand):
    """scores[i][c] from one K = 1 call per (sequence, candidate), queued back to back."""
    out = torch.zeros(len(seqs) * len(cand) * 32, dtype=torch.uint8).pin_memory()
    for i, s in enumerate(seqs):
        for c in range(len(cand)):
            g.score_map_corrections_into([s], cand[c:c + 1].ctypes.data, 1, out.data_ptr() + 32 * (i * len(cand) + c))
    g.synchronize()
    return out.numpy().view(importlib.import_module("a-loam_amd.binding").MAP_SCORE_DTYPE).reshape(len(seqs), len(cand))


def test_batch_shapes_equal_single_candidate_calls(binding, rec, reloc):
    import torch
    B = 16
    sweeps = [rec["scans"][F][(s % 4) * 50:] for s in range(B)]           # four different sweeps: four different stacks
    g = loaded(binding, rec, B, sweeps, fresh=[B - 1])                    # an empty map: its step fails the gate (:554)
    g.set_map_frozen([True] * B)
    g.mapping_step()
    g.synchronize()
    assert g.map_info(B - 1)["from_map_corner"] == 0
    q, t, _ = spread(reloc, rec, 2048, seed=9)
    cand = binding.map_corrections(q, t)
    big, best = g.score_map_corrections([1], cand)                        # n = 1, K = 2048
    assert big.tobytes() == _single_calls(torch, g, [1], cand).tobytes()
    assert int(best[0]) == min(range(2048), key=lambda c: (-(int(big[0, c]["corner_factors"]) + int(big[0, c]["surf_factors"])), float(big[0, c]["cost"]), c))
    assert len({int(s["surf_factors"]) for s in big[0]}) > 100
    every, best = g.score_map_corrections(list(range(B)), cand[:3])       # n = batch = 16, K = 3
    single = _single_calls(torch, g, list(range(B)), cand[:3])
    assert every.tobytes() == single.tobytes()
    assert every[0].tobytes() == every[4].tobytes() and every[0].tobytes() != every[1].tobytes()
    assert not every[B - 1].tobytes().strip(b"\0") and int(best[B - 1]) == 0   # gated out: zeros, and the lowest index wins the tie
    sub = [9, 2, 15, 4]                                                    # a listed subset, not ascending, the gated-out sequence among it
    part, best_p = g.score_map_corrections(sub, cand[:3])
    assert part.tobytes() == every[sub].tobytes() and list(best_p) == [int(best[s]) for s in sub]
    none, _ = g.score_map_corrections([], cand[:3])
    assert none.shape == (0, 3)
    # the largest call the library takes: 2^18 pairs (2^21 workgroups); one pair more is refused before anything is queued
    most = np.tile(cand, 128)
    huge, best_h = g.score_map_corrections([1], most)
    assert huge.reshape(128, 2048).tobytes() == big.tobytes() * 128 and int(best_h[0]) == int(g.score_map_corrections([1], cand)[1][0])
    with pytest.raises(binding.AloamError) as e:
        g.score_map_corrections([1], np.concatenate([most, cand[:1]]))
    assert e.value.code == binding.E_ARG
    g.close()


def test_sequences_without_a_frozen_steps_state_and_bad_arguments_are_refused(binding, rec, reloc):
    import torch
    g = loaded(binding, rec, 4)
    q, t, _ = spread(reloc, rec, 4)
    cand = binding.map_corrections(q, t)
    sc = torch.zeros(4 * 4 * 32, dtype=torch.uint8).pin_memory()
    best = torch.zeros(4, dtype=torch.int32).pin_memory()

    def score(seqs, K=4, scores_ptr=None, c=cand):
        return binding.lib().aloam_score_map_corrections(g.h, (C.c_int * max(1, len(seqs)))(*seqs), len(seqs), C.c_void_p(c.ctypes.data), K,
                                                         C.c_void_p(sc.data_ptr() if scores_ptr is None else scores_ptr), C.c_void_p(best.data_ptr()))

    def hashes():
        g.synchronize()
        return [pose_part(binding, g, b) for b in range(4)], sc.numpy().tobytes(), best.numpy().tobytes()

    assert score([0]) == binding.E_STATE                                  # no mapping step since the load
    g.set_map_frozen([True, False, True, True])
    g.mapping_step()
    g.synchronize()
    h0 = hashes()
    assert score([0]) == 0 and score([2, 3]) == 0
    g.synchronize()
    h0 = (h0[0], sc.numpy().tobytes(), best.numpy().tobytes())
    assert score([1]) == binding.E_STATE and score([0, 1]) == binding.E_STATE   # its last step grew its map
    assert "sequence 1" in binding.lib().aloam_last_error(g.h).decode()
    # argument errors: nothing is queued
    pageable = np.zeros(4 * 32, np.uint8)
    assert score([0], scores_ptr=pageable.ctypes.data) == binding.E_ARG
    assert score([0, 0]) == binding.E_ARG and score([4]) == binding.E_ARG and score([0], K=0) == binding.E_ARG
    assert binding.lib().aloam_score_map_corrections(g.h, (C.c_int * 1)(0), 1, None, 4, C.c_void_p(sc.data_ptr()), None) == binding.E_ARG
    assert hashes() == h0
    # the events that invalidate the grid
    def buffers():
        g.synchronize()
        return sc.numpy().tobytes(), best.numpy().tobytes()

    g.reset_sequences([2])
    assert score([0, 3]) == 0
    kept = buffers()
    assert score([2]) == binding.E_STATE and score([0, 2]) == binding.E_STATE and buffers() == kept
    n = rec["off"][1] - rec["off"][0]
    g.load_sequences([3], rec["blob"], np.array([0, n], np.int64))
    assert score([3]) == binding.E_STATE and score([0, 3]) == binding.E_STATE and buffers() == kept
    p, i = g.map_pose(0), g.map_info(0)
    g.set_map_frame((i["cenW"], i["cenH"], i["cenD"]), p["q_wmap_wodom"], p["t_wmap_wodom"], i["frame_count"], seq=0)
    assert score([0]) == binding.E_STATE and buffers() == kept
    # apply: a choice outside 0 .. K-1 leaves its sequence untouched and is reported once
    before = [pose_part(binding, g, b) for b in range(4)]
    g.apply_map_corrections([1, 0], cand, [2, 7])
    with pytest.raises(binding.AloamError) as e:
        g.synchronize()
    assert e.value.code == binding.E_ARG and "1 choice" in str(e.value)
    g.synchronize()                                                       # reported once
    after = [pose_part(binding, g, b) for b in range(4)]
    assert after[0] == before[0] and after[2:] == before[2:] and after[1] != before[1]
    m = g.map_pose(1)
    assert m["q_wmap_wodom"].tobytes() == q[2].tobytes() and m["t_wmap_wodom"].tobytes() == t[2].tobytes()
    g.close()


def test_applied_candidate_continues_like_set_map_frame_and_keeps_the_grid(binding, rec, reloc):
    import torch
    q, t, _ = spread(reloc, rec, 32, seed=11)
    cand = binding.map_corrections(q[1:], t[1:])                           # (without the truth: the best one still has something to refine)
    guess = displaced(reloc, rec, 1.5, -1.0, 4.0)
    out = {}
    for how in ("apply", "set_map_frame"):
        g = loaded(binding, rec, 1)
        g.set_map_frame(rec["cen"], guess[0], guess[1], rec["frame_count"])
        g.set_map_frozen([True])
        g.mapping_step()
        sc = torch.zeros(len(cand) * 32, dtype=torch.uint8).pin_memory()
        best = torch.zeros(1, dtype=torch.int32).pin_memory()
        g.score_map_corrections_into([0], cand.ctypes.data, len(cand), sc.data_ptr(), best.data_ptr())
        again = lambda: binding.lib().aloam_score_map_corrections(g.h, (C.c_int * 1)(0), 1, C.c_void_p(cand.ctypes.data), 1, C.c_void_p(one.data_ptr()), None)
        one = torch.zeros(32, dtype=torch.uint8).pin_memory()
        if how == "apply":                                                # score -> apply(best) -> next frame: the host reads nothing back in between
            g.apply_map_corrections_from([0], cand.ctypes.data, len(cand), best.data_ptr())
            assert again() == 0                                           # the grid is still the one the stacks were searched in
        else:
            g.synchronize()
            i = g.map_info(0)
            w = int(best[0])
            g.set_map_frame((i["cenW"], i["cenH"], i["cenD"]), cand[w]["q_wmap_wodom"], cand[w]["t_wmap_wodom"], i["frame_count"])
            assert again() == binding.E_STATE                             # invalidated: the next step builds it anew
        g.scan_register([rec["scans"][F + 1]], check=False)
        g.odometry_step()
        g.profile_enable(True)
        g.mapping_step()
        g.synchronize()
        out[how] = dict(part=pose_part(binding, g, 0), snap=snap(binding, g, 0, True), best=int(best[0]), grid_ms=g.profile()["map_grid"]["total_ms"],
                        scores=sc.numpy().tobytes())
        g.profile_enable(False)
        g.close()
    a, b = out["apply"], out["set_map_frame"]
    assert a["best"] == b["best"] and a["scores"] == b["scores"]
    assert not diff(a["part"], b["part"]) and not diff(a["snap"], b["snap"]), (diff(a["part"], b["part"]), diff(a["snap"], b["snap"]))
    print(f"map_grid of the step after: applied (grid kept) {a['grid_ms']:.4f} ms, set_map_frame (grid rebuilt) {b['grid_ms']:.4f} ms")
    assert a["grid_ms"] < b["grid_ms"], (a["grid_ms"], b["grid_ms"])


def test_grid_search_brings_every_guess_into_the_basin(binding, rec, reloc):
    guesses = [tuple(float(v) for v in x) for x in GUESSES] + EXTRA_GUESSES
    K = len(guesses)
    g = loaded(binding, rec, K)
    start = {}
    for s, d in enumerate(guesses):
        start[s] = displaced(reloc, rec, *d)
        g.set_map_frame(rec["cen"], start[s][0], start[s][1], rec["frame_count"], seq=s)
    g.set_map_frozen([True] * K)
    g.mapping_step()
    found = reloc.relocalize(g, list(range(K)), guesses=start, **GRID)
    for k in range(F + 1, F + G):
        g.scan_register([rec["scans"][k]] * K, check=False)
        g.odometry_step()
        g.mapping_step()
    g.synchronize()
    k = F + G - 1
    gt_t, gt_q = rec["R"][0].T @ (rec["t"][k] - rec["t"][0]), _quat_of(rec["R"][0].T @ rec["R"][k])
    bad = []
    for s, d in enumerate(guesses):
        r = found[s]
        node = r["nodes"][r["best"]]
        left = (d[0] + node[0], d[1] + node[1], d[2] + node[2])          # what the chosen node leaves of the displacement
        p = g.map_pose(s)
        e_t = float(np.linalg.norm(p["t_w"] - gt_t))
        e_a = 2 * math.degrees(math.acos(min(1.0, abs(float(np.dot(p["q_w"], gt_q))))))
        b = r["scores"][r["best"]]
        print(f"guess {d}: node {tuple(node)} leaves ({left[0]:+.2f} m, {left[1]:+.2f} m, {left[2]:+.2f} deg), factors {int(b['corner_factors'])} + {int(b['surf_factors'])}, "
              f"cost {float(b['cost']):.4f}; after {G - 1} more frames |t - gt| = {e_t:.4f} m, angle {e_a:.3f} deg")
        if not (e_t < 0.05 and e_a < 0.5):
            bad.append((d, tuple(node), e_t, e_a))
    assert not bad, bad
    g.close()


def test_kitti_runner_relocalizes_from_a_coarse_initial_pose(tmp_path):
    """The guess (2.8 m, -1.3 m, 7 deg) is outside the basin of the frozen steps: the run ends on the mapping run's poses with --relocalize
    and does not without it."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = tmp_path / "m.npz"

    def run(out, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "run_kitti.py"), "--selftest", "--out", str(tmp_path / out), *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    run("map", "--mapping", "--save-map", str(m))
    mapped = np.loadtxt(tmp_path / "map" / "00_mapped.txt")
    pose = ["--prior-map", str(m), "--initial-pose", "2.8", "-1.3", "0", "0.122"]
    stdout = run("reloc", *pose, "--relocalize", "3.5", "12.5")
    assert "00 relocalized: 2475 corrections scored" in stdout, stdout
    run("plain", *pose)
    err = {out: np.linalg.norm(np.loadtxt(tmp_path / out / "00_localized.txt")[:, 1:4] - mapped[:, 1:4], axis=1) for out in ("reloc", "plain")}
    print("error against the mapping run per sweep: with --relocalize", np.round(err["reloc"], 3), "without", np.round(err["plain"], 3))
    assert err["reloc"][-1] < 0.1, err["reloc"]
    assert not err["plain"][-1] < 0.1, err["plain"]
