"""Scan-to-map problems built to drive the map solve (k_map_solve: map_evaluate, lm_solve_block, the information record behind it) off the
happy path, on its two public routes: the mapping step (aloam_mapping_step against Oracle.mapping_step) and the loop registration
(aloam_graph_register_loops against loopreg_model.register).  The counterpart of lm_scenarios.py for the odometry solve.  Used by the CPU test
that pins WHICH branches the oracle takes and how stable its decisions are (tests/test_map_lm_scenarios.py) and by the GPU test that demands
the same of the HIP path (tests/test_gpu_map_lm_branches.py).

The scene is loopreg_model.fixture(seed=7), the noise-free room at the VLP-16 leaf sizes.  A scenario is a test frame - the filtered clouds of
node 9, whole or cut to a few points - the world pose it starts from, lm_max_iterations (4 or 8) and the loop route's outer_iterations
(1, 2 or 3).  The frames it is solved against are the same for all:
  mapping step   three map frames, the raw clouds of nodes 3, 4, 5 at their true poses (frames two and three are themselves refined);
  loop route     the target of nodes 0 .. 8 in the frame of node 4, the guess Z = X_4^-1 o (start pose).
Families: the whole source at the truth, at the entered drift, 1 m / 10 deg, 2 m / 20 deg and 30 m off; sources cut to (corner, surf) =
(0,1) .. (3,6) points, from the drift and from the truth; a ground-only surf source with 0 and 2 corner points; seeded random draws (offset
0.2 - 2.5 m, 2 - 35 deg, cut sources, lm 8), which supply the rejected steps.  RANDOM_DRAWS names the draws that passed the stability and
admission rules of tests/test_map_lm_scenarios.py when the list was made; a draw that fails them is taken out here, never tolerated there.

Every scenario is evaluated on the CPU three times per route - the oracle's dual-number Jacobians, its closed-form Jacobians, and the factor
records handed to the solver last to first - and spread_k is the largest pose difference among them: the yardstick the device's deviation is
held to."""
import functools
import importlib
import math

import numpy as np

import loopreg_model as M
import oracle_py

MAP_NODES = (3, 4, 5)
TARGET = (4, 0, 9)                               # node i, first, count of the loop route's target
SOURCE = 9
N_SCANS, MIN_RANGE = 16, 0.3
CUTS = ((0, 1), (0, 3), (1, 1), (1, 2), (2, 0), (2, 2), (3, 3), (0, 5), (0, 12), (3, 6))
DRAW_CORNER, DRAW_SURF = (0, 1, 2, 3, 10, 169), (0, 2, 3, 6, 12, 50, 1081)
N_DRAWS = 118
RANDOM_DRAWS = (2, 4, 5, 10, 17, 18, 26, 33, 34, 35, 36, 40, 47, 49, 51, 53, 58, 66, 73, 77, 78, 84, 86, 96, 101, 102, 108, 109, 111, 113)
FULL_SPREAD, DEFICIENT_SPREAD = 1e-10, 1e-7      # admission: the largest spread_k of a full-rank / a rank-deficient scenario
STEP_BOUND, LOOP_BOUND = 1e-9, 1e-8              # full-rank pose bounds: tests/test_gpu_mapping.py, Z_BOUND of tests/test_gpu_loop_register.py
# (name, route) whose pose is not compared, three at most; every other assertion about them stands.  draw36-c0-p1 is ONE plane factor that the
# mapping step's first solve follows for five accepted steps of 15 .. 34 (tangent units) while the radius grows: the damped, scaled system has a
# condition number of 1e10 .. 5e11 at every iteration (lm_trace), so Cholesky on it and QR on the Jacobian may part by eps x condition x |step|
# ~ 1e-4; the device was measured 1.0003e-8 from the oracle, bound 1e-8 (spread_k 2e-12).  tests/test_map_lm_scenarios.py prints the trace.
POSE_NOT_COMPARED = (("draw36-c0-p1", "step"),)


def _P():
    return importlib.import_module("a-loam_amd.posegraph")


def _L():
    return importlib.import_module("a-loam_amd.loopreg")


def _info():
    return importlib.import_module("a-loam_amd.information")


@functools.lru_cache(maxsize=None)
def scene():
    fx = M.fixture(seed=7)
    kf = M.keyframe_clouds(fx)
    # the target nodes' poses as a solver-off mapping step leaves them: q_wmap_wodom o (the pose handed in), the increment re-derived after every
    # frame, so a node's pose is the entered one only up to rounding - the oracle does the same arithmetic as the device
    orc = oracle_py.Oracle(n_scans=N_SCANS, min_range=MIN_RANGE, lm_max_iterations=0)
    orc.map_config(*M.LEAF)
    poses = [orc.mapping_step(fx["q"][k], fx["t"][k], fx["raw"][k][0], fx["raw"][k][1], fx["raw"][k][1][:4]) for k in range(TARGET[1] + TARGET[2])]
    nq, nt = np.array([p["q_w"] for p in poses]), np.array([p["t_w"] for p in poses])
    tc, ts = _L().target_cloud(nq, nt, kf, TARGET[0], TARGET[1], TARGET[2], M.LEAF, M.voxel_filter)
    return {"fx": fx, "kf": kf, "target": (tc, ts), "node_q": nq, "node_t": nt}


def moved(q, t, metres, degrees, direction=(0.8, -0.55, 0.23)):
    d = np.asarray(direction, np.float64)
    return M.drifted(q, t, dt=tuple(metres * d / np.linalg.norm(d)), dyaw=math.radians(degrees))


def _cut(cloud, n, seed):
    if n >= len(cloud):
        return cloud
    keep = np.sort(np.random.default_rng(seed).permutation(len(cloud))[:n])
    return np.ascontiguousarray(cloud[keep])


@functools.lru_cache(maxsize=None)
def candidates():
    """Every candidate scenario, admitted or not: a list of dicts (name, corner, surf, q, t, lm, outer)."""
    sc = scene()
    fx, (corner, surf) = sc["fx"], sc["kf"][SOURCE]
    qt, tt = fx["q_true"][SOURCE], fx["t_true"][SOURCE]
    starts = {"truth": (qt, tt), "drift": M.drifted(qt, tt), "1m10deg": moved(qt, tt, 1.0, 10.0), "2m20deg": moved(qt, tt, 2.0, 20.0), "30m": (qt, tt + np.array([30.0, 0.0, 0.0]))}
    out = []

    def add(name, c, s, start, lm, outer):
        out.append({"name": name, "corner": np.ascontiguousarray(c, np.float32).reshape(-1, 4), "surf": np.ascontiguousarray(s, np.float32).reshape(-1, 4),
                    "q": np.asarray(start[0], np.float64), "t": np.asarray(start[1], np.float64), "lm": lm, "outer": outer})

    for k, (name, lm, outer) in enumerate((("truth", 4, 2), ("drift", 4, 2), ("drift", 8, 3), ("1m10deg", 4, 2), ("1m10deg", 8, 1), ("2m20deg", 8, 3),
                                           ("30m", 4, 2), ("30m", 8, 1))):
        add(f"full-{name}-lm{lm}-o{outer}", corner, surf, starts[name], lm, outer)
    for k, (nc, ns) in enumerate(CUTS):
        for w, name in enumerate(("drift", "truth")):
            add(f"cut-c{nc}-p{ns}-{name}", _cut(corner, nc, 100 + k), _cut(surf, ns, 200 + k), starts[name], (4, 8)[(k + w) % 2], (2, 1, 3)[(k + w) % 3])
    world = M.associate_to_map(surf, np.concatenate([qt, tt]))
    ground = surf[np.abs(world[:, 2]) < 0.05]
    for k, (nc, ng, name) in enumerate(((0, len(ground), "drift"), (2, len(ground), "drift"), (0, 12, "truth"), (2, 12, "drift"), (0, 40, "truth"), (2, 40, "1m10deg"))):
        add(f"ground-c{nc}-p{ng}-{name}", _cut(corner, nc, 300 + k), _cut(ground, ng, 400 + k), starts[name], (4, 8)[k % 2], (2, 3, 1)[k % 3])
    rng = np.random.default_rng(1)
    for k in range(N_DRAWS):
        metres, degrees = rng.uniform(0.2, 2.5), rng.uniform(2.0, 35.0)
        direction = rng.normal(size=3) * np.array([1.0, 1.0, 0.3])
        nc, ns = DRAW_CORNER[rng.integers(len(DRAW_CORNER))], DRAW_SURF[rng.integers(len(DRAW_SURF))]
        seed = int(rng.integers(1 << 30))
        if nc + ns == 0:
            ns = 1
        if k in RANDOM_DRAWS:
            add(f"draw{k}-c{nc}-p{ns}", _cut(corner, nc, seed), _cut(surf, ns, seed + 1), moved(qt, tt, metres, degrees, direction), 8, (2, 1, 3)[k % 3])
    return out


def scenarios():
    return candidates()


# ---- the CPU side --------------------------------------------------------------------------------------------------------------------------
def _rank(lines, planes, par):
    if len(lines) + len(planes) == 0:
        return 0
    _, jl, _, jp = _info().factor_rows(lines, planes, par[:4], par[4:])
    return int(np.linalg.matrix_rank(np.concatenate([jl.reshape(-1, 6), jp.reshape(-1, 6)])))


def _map_oracle(lm, analytic):
    fx = scene()["fx"]
    orc = oracle_py.Oracle(n_scans=N_SCANS, min_range=MIN_RANGE, lm_max_iterations=lm, analytic_jacobian=analytic)
    orc.map_config(*M.LEAF)
    for k in MAP_NODES:
        orc.mapping_step(fx["q"][k], fx["t"][k], fx["raw"][k][0], fx["raw"][k][1], fx["raw"][k][1][:4])
    return orc


@functools.lru_cache(maxsize=None)
def _submap(lm, analytic):
    """(corner, surf, q_wmap_wodom, t_wmap_wodom) the test frame meets: the cubes of the window in the order the mapping step gathers them."""
    orc = _map_oracle(lm, analytic)
    clouds = []
    for cls in (0, 1):
        cubes = orc.map_cubes(cls)
        order = sorted(cubes, key=lambda i: (i % 21, (i // 21) % 21, i // 441))
        clouds.append(np.concatenate([cubes[i] for i in order]))
    p = orc.map_pose()
    return clouds[0], clouds[1], p["q_wmap_wodom"], p["t_wmap_wodom"]


def model_step(sc, analytic=False, reverse=False):
    """The mapping step's two solves composed from the oracle's pieces (loopreg_model.factors, oracle_py.lm_solve) on the oracle's own submap:
    the view that has `successful` and takes the records in either order."""
    P = _P()
    mc, ms, qm, tm = _submap(sc["lm"], analytic)
    q, t = P.qmul(qm, sc["q"]), P.qrot(qm, sc["t"]) + tm
    rounds = []
    step = -1 if reverse else 1
    if len(mc) > 10 and len(ms) > 50:
        for _ in range(2):
            entry = np.concatenate([q, t])
            lines, planes = M.factors(sc["corner"], sc["surf"], mc, ms, entry)
            qn, tn, sm = oracle_py.lm_solve(lines[::step], M.planes_as_point_factors(planes)[::step], q, t, max_iterations=sc["lm"], analytic=analytic)
            rounds.append({"n_line": len(lines), "n_plane": len(planes), "summary": sm, "factors": (lines, planes), "entry": entry})
            if sm["termination"] != 5:
                q, t = qn, tn
    return {"q": q, "t": t, "rounds": rounds}


def _full(sc):
    """The full-resolution cloud of a test frame: four points, it plays no part in the solve."""
    return np.concatenate([sc["surf"], sc["corner"]])[:4]


def run_oracle_step(sc, analytic=False):
    """Oracle.mapping_step of the test frame behind the three map frames: pose, map_info, both stacks."""
    orc = _map_oracle(sc["lm"], analytic)
    pose = orc.mapping_step(sc["q"], sc["t"], sc["corner"], sc["surf"], _full(sc))
    return {"pose": pose, "info": orc.map_info(), "stacks": (orc.map_cloud(oracle_py.MAP_CORNER_STACK), orc.map_cloud(oracle_py.MAP_SURF_STACK))}


def raw_guess(sc):
    """Z of the loop route as the request carries it: X_4^-1 o (start pose)."""
    fx = scene()["fx"]
    return _P().relative_pose(fx["q"][TARGET[0]], fx["t"][TARGET[0]], sc["q"], sc["t"])


def guess(sc):
    """The guess as aloam_graph_register_loops stores it: the request's quaternion divided by its norm, the squares summed in index order."""
    qz, tz = raw_guess(sc)
    q = [float(v) for v in qz]
    nn = 0.0
    for v in q:
        nn += v * v
    nn = math.sqrt(nn)
    return np.array([v / nn for v in q]), tz


def run_oracle_loop(sc, analytic=False, reverse=False):
    tc, ts = scene()["target"]
    qz, tz = guess(sc)
    return M.register(tc, ts, sc["corner"], sc["surf"], qz, tz, outer_iterations=sc["outer"], lm_max_iterations=sc["lm"], analytic=analytic, reverse=reverse)


def decisions(rounds):
    return tuple((r["n_line"], r["n_plane"], r["summary"]["iterations"], r["summary"]["successful"], r["summary"]["termination"]) for r in rounds)


def _classify(rounds, q, t):
    """(full_rank, model status) from a route's rounds: every solve has six independent rows and decompose of the last records' information at
    the final pose is INFO_OK."""
    I = _info()
    if not rounds or rounds[-1]["n_line"] + rounds[-1]["n_plane"] == 0:
        return False, I.INFO_NO_FACTORS
    lines, planes = rounds[-1]["factors"]
    status = I.decompose(I.information_from_factors(lines, planes, q, t)["info"])["status"]
    ranks = [_rank(r["factors"][0], r["factors"][1], r["entry"]) for r in rounds]
    return min(ranks) >= 6 and status == I.INFO_OK, status


@functools.lru_cache(maxsize=None)
def evaluate(name):
    """Everything the tests need of one scenario, from the oracle alone: per route the decisions of the three variants, the poses, spread_k,
    the class; `stable`: the variants agree on every decision."""
    sc = next(s for s in candidates() if s["name"] == name)
    out = {"name": name}
    # mapping step: Oracle.mapping_step (dual numbers, closed form), the composed model (same order: it must tell the oracle's story; reversed)
    step = [run_oracle_step(sc, analytic=a) for a in (False, True)]
    models = [model_step(sc), model_step(sc, reverse=True)]
    keys = ("corner_num0", "surf_num0", "lm_iterations0", "termination0", "corner_num1", "surf_num1", "lm_iterations1", "termination1")
    told = [tuple(s["info"][k] for k in keys) for s in step]
    told += [tuple(v for r in m["rounds"] for v in (r["n_line"], r["n_plane"], r["summary"]["iterations"], r["summary"]["termination"])) for m in models]
    poses = [np.concatenate([s["pose"]["q_w"], s["pose"]["t_w"]]) for s in step] + [np.concatenate([m["q"], m["t"]]) for m in models]
    full, status = _classify(models[0]["rounds"], step[0]["pose"]["q_w"], step[0]["pose"]["t_w"])
    out["step"] = {"oracle": step[0], "rounds": models[0]["rounds"], "decisions": decisions(models[0]["rounds"]), "stable": len(set(told)) == 1 and decisions(models[0]["rounds"]) == decisions(models[1]["rounds"]),
                   "told": told, "spread": max(float(np.abs(p - poses[0]).max()) for p in poses), "full_rank": full, "status": status}
    # loop route
    regs = [run_oracle_loop(sc), run_oracle_loop(sc, analytic=True), run_oracle_loop(sc, reverse=True)]
    told = [(decisions(r["rounds"]), r["status"]) for r in regs]
    poses = [np.concatenate([r["q"], r["t"]]) for r in regs]
    full, status = _classify(regs[0]["rounds"], regs[0]["q"], regs[0]["t"]) if regs[0]["rounds"] else (False, _info().INFO_NONE)
    out["loop"] = {"oracle": regs[0], "rounds": regs[0]["rounds"], "decisions": decisions(regs[0]["rounds"]), "stable": len(set(told)) == 1, "told": told,
                   "spread": max(float(np.abs(p - poses[0]).max()) for p in poses), "full_rank": full, "status": status}
    out["class"] = "full-rank" if out["step"]["full_rank"] and out["loop"]["full_rank"] else "rank-deficient"
    return out


def lm_trace(lines, planes, entry, max_iterations):
    """The Levenberg-Marquardt loop of lm_device.hpp / oracle_solver.cpp restated in numpy on one round's records, for what neither exposes:
    per iteration the condition number of the damped, Jacobi-scaled 6 x 6 system (H + D / radius) that the device factorises by Cholesky and
    the oracle solves by QR on the Jacobian, with the length of the step it yields.  Returns (summary, [(condition number, |step|, accepted)]);
    the summary must equal the oracle's for the trace to speak for it."""
    I = _info()
    S2 = np.array([2.0, 2.0, 2.0, 1.0, 1.0, 1.0])                 # information.py's tangent is theta = 2 delta

    def sums(q, t):
        rec = I.information_from_factors(lines, planes, q, t)
        return rec["info"] * np.outer(S2, S2), rec["gradient"] * S2, rec["cost"]

    q, t = np.array(entry[:4], np.float64), np.array(entry[4:], np.float64)
    H, g, cost = sums(q, t)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))

    def gmax_of(q, t, g):
        return max(np.abs(q - oracle_py.quat_plus(q, -g[:3])).max(), np.abs(t - (t + (-g[3:]))).max())

    gmax = gmax_of(q, t, g)
    Hs, gs = H * np.outer(scale, scale), g * scale
    radius, decrease, reuse, invalid, it, ok_steps, term = 1e4, 2.0, False, 0, 0, 0, 0
    x_norm = math.sqrt(float(q @ q + t @ t))
    diag = np.zeros(6)
    trace = []
    while True:
        if it >= max_iterations:
            term = 0
            break
        if gmax <= 1e-10:
            term = 3
            break
        it += 1
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(Hs), 1e-6), 1e32)
        A = Hs + np.diag(diag / radius)
        step = -np.linalg.solve(A, gs)
        reuse = True
        change = -float(step @ gs) - 0.5 * float(step @ Hs @ step)
        if not (np.isfinite(step).all() and change > 0.0):
            invalid += 1
            trace.append((float(np.linalg.cond(A)), float("nan"), False))
            if invalid >= 5:
                term = 5
                break
            radius, decrease = radius / decrease, decrease * 2.0
            continue
        invalid = 0
        delta = step * scale
        qc, tc = oracle_py.quat_plus(q, delta[:3]), t + delta[3:]
        Hc, gc, cost_c = sums(qc, tc)
        sn = math.sqrt(float((q - qc) @ (q - qc) + (t - tc) @ (t - tc)))
        if sn <= 1e-8 * (x_norm + 1e-8):
            term = 1
            trace.append((float(np.linalg.cond(A)), float(np.linalg.norm(delta)), False))
            break
        if abs(cost - cost_c) <= 1e-6 * cost:
            term = 2
            trace.append((float(np.linalg.cond(A)), float(np.linalg.norm(delta)), False))
            break
        rel = (cost - cost_c) / change
        trace.append((float(np.linalg.cond(A)), float(np.linalg.norm(delta)), rel > 1e-3))
        if rel > 1e-3:
            q, t, cost, ok_steps = qc, tc, cost_c, ok_steps + 1
            x_norm = math.sqrt(float(q @ q + t @ t))
            gmax = gmax_of(q, t, gc)
            Hs, gs = Hc * np.outer(scale, scale), gc * scale
            c3 = 2.0 * rel - 1.0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - c3 * c3 * c3))
            decrease, reuse = 2.0, False
        else:
            radius, decrease = radius / decrease, decrease * 2.0
    return {"iterations": it, "successful": ok_steps, "termination": term}, trace


def pose_bound(ev, route):
    """What the device's pose may deviate from the oracle's: the full-rank bound of the route, or max(1e-8, 10 spread_k) for a rank-deficient
    solve - spread_k samples the roundings of ONE algorithm, the device also changes the algorithm (Cholesky on the normal equations against QR)."""
    if ev[route]["full_rank"]:
        return STEP_BOUND if route == "step" else LOOP_BOUND
    return max(1e-8, 10.0 * ev[route]["spread"])


def branches(rounds):
    """What a route's solves provably went through.  rounds: dicts with `iterations`, `termination` and, where the view has it, `successful`
    (the oracle's lm_solve summary).  The device's records carry no `successful`: the GPU test hands in the device's own iterations and
    termination with the oracle's `successful` only after it has found the first two and the pose equal to the oracle's - a device that accepted
    the step the oracle rejected would have moved to another pose."""
    seen = set()
    for r in rounds:
        it, term, ok = r["iterations"], r["termination"], r.get("successful")
        seen.add(f"termination{term}")
        if ok is not None and it - ok - (1 if term in (1, 2) else 0) > 0:
            seen.add("rejected")
    return seen


def visible(route, rounds):
    """The rounds whose termination the device's records show: the mapping step exposes termination0 (the first solve's), a loop result the
    last round's."""
    return list(rounds[:1]) if route == "step" else list(rounds[-1:])


def rejected_rounds(rounds):
    return sum(1 for r in rounds if "rejected" in branches([r]))


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------------
def run_gpu_step(binding, scs, lm):
    """One context of batch len(scs): the three map frames for every sequence, then each scenario's test frame in ONE aloam_mapping_step.
    Returns per scenario dict(pose, info, stacks, factors, information: the aloam_pose_information record of the step)."""
    fx = scene()["fx"]
    gpu = binding.Aloam(n_scans=N_SCANS, min_range=MIN_RANGE, batch=len(scs), max_points=4096, lm_max_iterations=lm)
    gpu.mapping_enable(*M.LEAF, pool_points=1 << 16)

    def frame(inputs):
        for b, (corner, surf, q, t) in enumerate(inputs):
            gpu.set_last(corner, surf, b)
            gpu.set_full_cloud(np.concatenate([surf, corner])[:4], b)
            gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(q, np.float64), np.array(t, np.float64), b)
        gpu.mapping_step()
        gpu.synchronize()

    try:
        for k in MAP_NODES:
            frame([(fx["raw"][k][0], fx["raw"][k][1], fx["q"][k], fx["t"][k])] * len(scs))
        frame([(sc["corner"], sc["surf"], sc["q"], sc["t"]) for sc in scs])
        recs = gpu.export_pose_information(binding.INFO_MAPPING, list(range(len(scs))))
        out = []
        for b in range(len(scs)):
            out.append({"pose": gpu.map_pose(b), "info": gpu.map_info(b), "factors": gpu.map_factors(b), "information": recs[b].copy(),
                        "stacks": (gpu.map_cloud(binding.MAP_CORNER_STACK, b), gpu.map_cloud(binding.MAP_SURF_STACK, b))})
    finally:
        gpu.close()
    return out


def loop_context(binding, scs):
    """One sequence, solver off: nodes 0 .. 8 are the target's keyframes, node 9 + k holds the source clouds of scs[k]."""
    fx = scene()["fx"]
    gpu = binding.Aloam(n_scans=N_SCANS, min_range=MIN_RANGE, batch=1, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(*M.LEAF, pool_points=1 << 16)
    gpu.graph_enable(len(scs) + 16, 2 * len(scs) + 32)
    gpu.graph_keyframes_enable(1 << 15, 1 << 17)
    gpu.graph_loops_enable(max(len(scs), 1), 4096, 16384)
    frames = [(fx["raw"][k][0], fx["raw"][k][1], fx["q"][k], fx["t"][k]) for k in range(TARGET[2])]
    frames += [(sc["corner"], sc["surf"], fx["q_true"][SOURCE], fx["t_true"][SOURCE]) for sc in scs]
    stacks = []
    for corner, surf, q, t in frames:
        gpu.set_last(corner, surf, 0)
        gpu.set_full_cloud(np.concatenate([surf, corner])[:4], 0)
        gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(q, np.float64), np.array(t, np.float64), 0)
        gpu.mapping_step()
        gpu.graph_add_nodes([0], np.eye(6) * 100.0)
        gpu.synchronize()
        stacks.append((gpu.map_cloud(binding.MAP_CORNER_STACK, 0), gpu.map_cloud(binding.MAP_SURF_STACK, 0)))
    return gpu, stacks


def loop_request(sc, k):
    qz, tz = raw_guess(sc)
    return (0, TARGET[0], TARGET[2] + k, TARGET[1], TARGET[2], 0, qz, tz)


def run_gpu_loop(gpu, scs, index, outer, lm):
    """One aloam_graph_register_loops call for the scenarios scs (index[name] = the scenario's place among the context's source nodes)."""
    return gpu.graph_register_loops([loop_request(sc, index[sc["name"]]) for sc in scs], outer_iterations=outer, lm_max_iterations=lm)
