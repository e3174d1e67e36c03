"""The map solve on the MI355X off the happy path (k_map_solve: map_evaluate, lm_solve_block, the information record and k_loop_result behind
it), on its two public routes against the oracle, over the scenarios of tests/map_lm_scenarios.py: rejected steps, terminations 0 .. 4, fewer
residual rows than parameters, ground-only problems, frames 2 m / 20 degrees and 30 m off.  tests/test_map_lm_scenarios.py shows from the
oracle alone what the list reaches and how far the oracle's own variants lie apart (spread_k).

Decisions and counts are exact.  Poses: a full-rank scenario within 1e-9 (mapping step) / 1e-8 (loop route), a rank-deficient one within
max(1e-8, 10 spread_k) - map_lm_scenarios.pose_bound.  The deviation and spread_k of every scenario are printed; DESIGN.md section 7o holds
the table."""
import importlib

import numpy as np
import pytest

import map_lm_scenarios as S

pytestmark = pytest.mark.gpu
info = importlib.import_module("a-loam_amd.information")
L = importlib.import_module("a-loam_amd.loopreg")
P = importlib.import_module("a-loam_amd.posegraph")

POSE_KEYS = ("q_w", "t_w", "q_wmap_wodom", "t_wmap_wodom")
INDEPENDENT = ("full-2m20deg-lm8-o3", "draw40-c10-p50", "full-drift-lm8-o3")        # diverging (termination 0 twice), a rejected step, well-posed


def raw(rec):
    return np.ascontiguousarray(rec).view(np.uint8).tobytes()


def step_bytes(d):
    return (tuple(raw(d["pose"][k]) for k in POSE_KEYS), tuple(sorted(d["info"].items())), raw(d["factors"][0]), raw(d["factors"][1]), raw(d["information"]),
            raw(d["stacks"][0]), raw(d["stacks"][1]))


@pytest.fixture(scope="module")
def oracle(O):
    return {sc["name"]: S.evaluate(sc["name"]) for sc in S.scenarios()}


@pytest.fixture(scope="module")
def step_runs(binding):
    """One context per lm_max_iterations, its batch the scenarios of that value: one aloam_mapping_step per frame runs them all."""
    out = {}
    for lm in (4, 8):
        scs = [sc for sc in S.scenarios() if sc["lm"] == lm]
        for sc, d in zip(scs, S.run_gpu_step(binding, scs, lm)):
            out[sc["name"]] = d
    return out


@pytest.fixture(scope="module")
def loop_world(binding):
    scs = S.scenarios()
    gpu, stacks = S.loop_context(binding, scs)
    yield {"gpu": gpu, "stacks": stacks, "index": {sc["name"]: k for k, sc in enumerate(scs)}}
    gpu.close()


@pytest.fixture(scope="module")
def loop_runs(loop_world):
    """One aloam_graph_register_loops call per (outer_iterations, lm_max_iterations): every scenario of the pair at once."""
    out = {}
    for outer in (1, 2, 3):
        for lm in (4, 8):
            scs = [sc for sc in S.scenarios() if (sc["outer"], sc["lm"]) == (outer, lm)]
            if scs:
                res = S.run_gpu_loop(loop_world["gpu"], scs, loop_world["index"], outer, lm)
                for sc, r in zip(scs, res):
                    out[sc["name"]] = r.copy()
    return out


def model_sums(rec, lines, planes, q, t):
    """information_from_factors on the same records and pose, with the scales of tests/test_gpu_pose_information._check_against_model: sqrt(H_ii
    H_jj) for the matrix, sqrt(2 cost H_ii) for the gradient.  Where a diagonal entry of the model is exactly zero every Jacobian entry of that
    column is, so its row and column (and its gradient entry) are compared absolutely against zero, on the scale of the largest diagonal entry."""
    want = info.information_from_factors(lines, planes, q, t)
    dia = np.diag(want["info"])
    zero = dia == 0.0
    assert not want["info"][zero].any() and not want["info"][:, zero].any()
    either = np.outer(zero, np.ones(6, bool)) | np.outer(np.ones(6, bool), zero)
    want["h_scale"] = np.sqrt(np.where(either, dia.max() ** 2, np.outer(dia, dia)))
    want["g_scale"] = np.sqrt(2.0 * want["cost"] * np.where(zero, dia.max(), dia))
    want["zero"] = int(zero.sum())
    return want


def check_information(rec, lines, planes, q, t, label):
    """The matrix of aloam_pose_information against the model (|dH_ij| <= 1e-10 sqrt(H_ii H_jj)), the counts, and the status against decompose
    of the device's matrix and of the model's.  Returns (status, problems)."""
    if len(lines) + len(planes) == 0:
        ok = int(rec["status"]) == info.INFO_NO_FACTORS and not rec["info"].any() and not rec["gradient"].any() and rec["cost"] == 0 and int(rec["rows"]) == 0
        ok = ok and not any(rec[name].any() for name in ("eigenvalues", "eigenvectors", "trans_info", "rot_info", "trans_eigenvalues", "rot_eigenvalues"))
        return info.INFO_NO_FACTORS, [] if ok else [(label, "a record without factors is not all zero")]
    bad = []
    want = model_sums(rec, lines, planes, q, t)
    H, Hm = rec["info"], want["info"]
    dH = (np.abs(H - Hm) / want["h_scale"]).max()
    print(f"{label}: factors {rec['n_line']} + {rec['n_plane']}, zero diagonal entries {want['zero']}, max |dH| / scale {dH:.3g}")
    if (int(rec["n_line"]), int(rec["n_plane"]), int(rec["rows"])) != (want["n_line"], want["n_plane"], want["rows"]):
        bad.append((label, "counts", int(rec["n_line"]), int(rec["n_plane"]), int(rec["rows"])))
    if not (dH <= 1e-10 and np.array_equal(H, H.T)):
        bad.append((label, "matrix", float(dH)))
    d = info.decompose(H)
    if not int(rec["status"]) == d["status"] == info.decompose(Hm)["status"]:
        bad.append((label, "status", int(rec["status"]), d["status"], info.decompose(Hm)["status"]))
    return d["status"], bad


def check_decomposition(rec, label):
    """Eigenpairs against the device's own matrix, marginals against decompose() of it, by the yardsticks of
    tests/test_gpu_pose_information._check_decomposition; a marginal the model zeroes is zero.  Returns the problems."""
    bad = []
    H = rec["info"]
    lam, V = rec["eigenvalues"], rec["eigenvectors"]
    top = lam[5]
    res, dl = np.linalg.norm(H @ V - V * lam, axis=0).max(), np.abs(lam - np.linalg.eigvalsh(H)).max()
    if not (np.all(np.diff(lam) >= 0) and res <= 1e-10 * top and dl <= 1e-10 * top and np.abs(V.T @ V - np.eye(6)).max() <= 1e-12):
        bad.append((label, "eigenpairs", float(res / top), float(dl / top)))
    d = info.decompose(H)
    vecs = [V]
    for name in ("trans", "rot"):
        Mx, lam3, V3 = rec[name + "_info"], rec[name + "_eigenvalues"], rec[name + "_eigenvectors"]
        if not d[name + "_info"].any() and not d[name + "_eigenvalues"].any():              # the model zeroes this marginal
            if Mx.any() or lam3.any() or V3.any():
                bad.append((label, name, "not zeroed"))
            continue
        sc = d[name + "_eigenvalues"][2]
        dm, dl3, r3 = np.abs(Mx - d[name + "_info"]).max(), np.abs(lam3 - d[name + "_eigenvalues"]).max(), np.linalg.norm(Mx @ V3 - V3 * lam3, axis=0).max()
        print(f"{label}: {name} marginal top eigenvalue {sc:.3g} (block diagonal {np.diag(H)[3:].max() if name == 'trans' else np.diag(H)[:3].max():.3g}), |dM| {dm:.3g}, |dlambda| {dl3:.3g}, residual {r3:.3g}")
        if not (dm <= 1e-9 * sc and dl3 <= 1e-9 * sc and r3 <= 1e-10 * sc):
            bad.append((label, name, "marginal", float(sc), float(dm), float(dl3), float(r3)))
        vecs.append(V3)
    for W in vecs:
        for k in range(W.shape[1]):
            if not W[int(np.argmax(np.abs(W[:, k]))), k] > 0:                               # the sign rule
                bad.append((label, "sign rule", k))
    return bad


def test_mapping_step_against_the_oracle(O, binding, oracle, step_runs):
    """Teacher-forced: three map frames, then every scenario's test frame in one step.  Every shared map_info key (lm_iterations0 / 1 and
    termination0 among them), both stacks bit for bit, the pose within the scenario's bound; the information record of the step on the device's
    own factors and pose."""
    shared = [k for k in O.MAP_INFO_KEYS if k in binding.MAP_INFO_KEYS]
    assert {"lm_iterations0", "lm_iterations1", "termination0", "frame_count", "corner_num1", "surf_num1"} <= set(shared)
    statuses, worst, bad = [], [], []
    for sc in S.scenarios():
        ev, got = oracle[sc["name"]], step_runs[sc["name"]]
        want = ev["step"]["oracle"]
        dev = max(float(np.abs(want["pose"][k] - got["pose"][k]).max()) for k in POSE_KEYS)
        bound = S.pose_bound(ev, "step")
        print(f"{sc['name']:24s} {'full-rank' if ev['step']['full_rank'] else 'rank-deficient':14s} device - oracle {dev:.2e}, spread_k {ev['step']['spread']:.2e}, bound {bound:.1e}, "
              f"LM {got['info']['lm_iterations0']} + {got['info']['lm_iterations1']}, termination0 {got['info']['termination0']}")
        for key in shared:
            if want["info"][key] != got["info"][key]:
                bad.append((sc["name"], key, want["info"], got["info"]))
        for cls in (0, 1):
            if not (got["stacks"][cls].shape == want["stacks"][cls].shape and np.array_equal(got["stacks"][cls].view(np.uint32), want["stacks"][cls].view(np.uint32))):
                bad.append((sc["name"], "stack", cls))
        if (sc["name"], "step") not in S.POSE_NOT_COMPARED:
            worst.append((dev / bound, sc["name"]))
        lines, planes = got["factors"]
        if (len(lines), len(planes)) != (got["info"]["corner_num1"], got["info"]["surf_num1"]) or int(got["information"]["frame"]) != got["info"]["frame_count"]:
            bad.append((sc["name"], "the records are not the second solve's"))
        status, problems = check_information(got["information"], lines, planes, got["pose"]["q_w"], got["pose"]["t_w"], sc["name"])
        statuses.append(status)
        bad += problems
    print("largest deviation / bound:", sorted(worst)[-3:])
    bad += [("pose", name, w) for w, name in worst if not w <= 1.0]
    assert not bad, bad
    assert info.INFO_SINGULAR in statuses and info.INFO_NO_FACTORS in statuses and info.INFO_OK in statuses


def test_final_cost_and_gradient_at_the_devices_pose(oracle, step_runs, loop_runs):
    """The cost of the device's record against the model evaluated at the device's pose within 1e-12 relative (both routes), the gradient within
    1e-10 sqrt(2 cost H_ii) (mapping step).  The few-point scenarios of the noise-free room converge onto their planes: final costs down to
    6e-28, residuals n . lp + d of 1e-13 m that are differences of terms of 1 .. 10 m.  Such a cost is decided by the rounding of every
    product and sum, so the model states the residual in the kernel's order, each operation rounded on its own (information.factor_rows; with
    np.einsum, whose order is not defined, the same records differed by up to 2.8e-4 relative).  Measured: cost within 1.9e-16 (mapping step)
    and 3.0e-16 (loop route), gradient within 2.3e-16 of its scale."""
    bad = []
    for sc in S.scenarios():
        got = step_runs[sc["name"]]
        lines, planes = got["factors"]
        if len(lines) + len(planes):
            rec = got["information"]
            want = model_sums(rec, lines, planes, got["pose"]["q_w"], got["pose"]["t_w"])
            dg = np.abs(rec["gradient"] - want["gradient"])
            dc = abs(rec["cost"] - want["cost"]) / want["cost"] if want["cost"] > 0 else abs(rec["cost"])
            print(f"{sc['name']:24s} step: cost {want['cost']:.3g} rel {dc:.3g}, max |dg| / sqrt(2 cost Hii) {(dg / np.where(want['g_scale'] > 0, want['g_scale'], 1.0)).max():.3g}")
            if not (dc <= 1e-12 and np.all(dg <= 1e-10 * want["g_scale"])):
                bad.append((sc["name"], "step", float(want["cost"]), float(dc)))
        res, m = loop_runs[sc["name"]], oracle[sc["name"]]["loop"]["oracle"]
        if int(res["status"]) == L.LOOP_OK == m["status"]:
            want = info.information_from_factors(m["factors"][0], m["factors"][1], res["q"], res["t"])
            dc = abs(res["cost"] - want["cost"]) / want["cost"]
            print(f"{sc['name']:24s} loop: cost {want['cost']:.3g} rel {dc:.3g}")
            if not dc <= 1e-12:
                bad.append((sc["name"], "loop", float(want["cost"]), float(dc)))
    assert not bad, bad


def test_eigenpairs_and_marginals_of_the_mapping_record(step_runs):
    """The decomposition of every scenario's record by the yardsticks of tests/test_gpu_pose_information._check_decomposition, SINGULAR records
    with their zeroed marginals included.  Twelve of the 90 marginals belong to matrices of rank <= 3 whose block to eliminate is still positive
    definite: the Schur complement D - C^T A^-1 C cancels completely (top eigenvalues of 2e-20 .. 1e-12 beside block entries of 1 .. 164), and
    what is left is the rounding of the operations themselves.  information._schur therefore does them one by one as schur3 does; measured:
    all 90 marginals are the model's bit for bit, their eigenvalues within 6.6e-11 of the top one (allowed 1e-9), residuals within 2.9e-13."""
    bad, singular = [], 0
    for sc in S.scenarios():
        rec = step_runs[sc["name"]]["information"]
        if int(rec["status"]) in (info.INFO_OK, info.INFO_SINGULAR):
            bad += check_decomposition(rec, sc["name"])
            singular += int(rec["status"]) == info.INFO_SINGULAR
    assert singular >= 1
    assert not bad, bad


def test_loop_route_against_the_model(binding, oracle, loop_world, loop_runs):
    """The same clouds as keyframes (solver off), every scenario of one (outer_iterations, lm_max_iterations) in one call: status, factor
    counts, lm_iterations and the LAST round's termination exact; Z within the bound when LOOP_OK; the guess bit for bit and zero information
    when LOOP_SOLVE_FAILED, which the rank-deficient scenarios reach with factors, through a pivot that is not positive."""
    gpu, kf = loop_world["gpu"], S.scene()["kf"]
    for k in range(S.TARGET[2]):                                  # the keyframes are what the oracle's target was made of
        for cls in (0, 1):
            assert np.array_equal(loop_world["stacks"][k][cls].view(np.uint32), kf[k][cls].view(np.uint32)), (k, cls)
    first = S.scenarios()[0]
    gpu.graph_register_loops([S.loop_request(first, 0)], outer_iterations=first["outer"], lm_max_iterations=first["lm"])
    for cls in (0, 1):
        assert np.array_equal(gpu.graph_loop_target(0, cls).view(np.uint32), S.scene()["target"][cls].view(np.uint32))
    nodes = gpu.graph_export(0)
    assert np.array_equal(nodes["q"][:S.TARGET[2]], S.scene()["node_q"]) and np.array_equal(nodes["t"][:S.TARGET[2]], S.scene()["node_t"])
    failed_with_factors, worst, bad = 0, [], []
    for k, sc in enumerate(S.scenarios()):
        ev, res = oracle[sc["name"]], loop_runs[sc["name"]]
        m = ev["loop"]["oracle"]
        for cls in (0, 1):
            src = (sc["corner"], sc["surf"])[cls]
            assert np.array_equal(loop_world["stacks"][S.TARGET[2] + k][cls].view(np.uint32), src.view(np.uint32)) and int(res["source_points"][cls]) == len(src)
        dq, dt = float(np.abs(res["q"] - m["q"]).max()), float(np.abs(res["t"] - m["t"]).max())
        bound = S.pose_bound(ev, "loop")
        print(f"{sc['name']:24s} {'full-rank' if ev['loop']['full_rank'] else 'rank-deficient':14s} status {res['status']} / {m['status']}, factors {res['n_line']} + {res['n_plane']}, "
              f"LM {res['lm_iterations']} / {m['lm_iterations']}, termination {res['lm_termination']} / {m['lm_termination']}, device - model {max(dq, dt):.2e}, "
              f"spread_k {ev['loop']['spread']:.2e}, bound {bound:.1e}")
        told = (int(res["status"]), int(res["n_line"]), int(res["n_plane"]), int(res["lm_iterations"]), int(res["lm_termination"]))
        if told != (m["status"], m["n_line"], m["n_plane"], m["lm_iterations"], m["lm_termination"]):
            bad.append((sc["name"], "decisions", told, (m["status"], m["n_line"], m["n_plane"], m["lm_iterations"], m["lm_termination"])))
            continue
        qz, tz = S.guess(sc)
        if m["status"] == L.LOOP_SOLVE_FAILED:
            if not (np.array_equal(res["q"], qz) and np.array_equal(res["t"], tz) and not res["info"].any() and not res["info_left"].any()):
                bad.append((sc["name"], "a failed solve does not return the guess and zero information"))
            failed_with_factors += m["n_line"] + m["n_plane"] > 0
        else:
            assert m["status"] == L.LOOP_OK
            if (sc["name"], "loop") not in S.POSE_NOT_COMPARED:
                worst.append((max(dq, dt) / bound, sc["name"]))
            # the information: the model evaluated on its records at the device's Z
            want = info.information_from_factors(m["factors"][0], m["factors"][1], res["q"], res["t"])
            H, Hm = P.info_full(res["info_left"]), want["info"]
            dia = np.sqrt(np.diag(Hm))
            dH = (np.abs(H - Hm) / np.outer(dia, dia)).max()
            E, Em = P.info_full(res["info"]), L.edge_information(Hm, res["q"])
            de = (np.abs(E - Em) / np.outer(np.sqrt(np.diag(Em)), np.sqrt(np.diag(Em)))).max()
            print(f"    max |d info_left| / sqrt(HiiHjj) {dH:.3g}, max |d info| / sqrt(EiiEjj) {de:.3g}")
            if not (dH <= 1e-10 and de <= 1e-10):
                bad.append((sc["name"], "information", float(dH), float(de)))
    print("largest deviation / bound:", sorted(worst)[-3:])
    bad += [("pose", name, w) for w, name in worst if not w <= 1.0]
    assert not bad, bad
    assert failed_with_factors >= 5


def test_a_scenario_does_not_depend_on_its_batch(binding, step_runs, loop_world, loop_runs):
    """A diverging scenario, one with a rejected step and a well-posed one: each one's records in the batch are byte for byte its records alone
    and in a batch of reversed order, on both routes."""
    picks = [next(sc for sc in S.scenarios() if sc["name"] == n) for n in INDEPENDENT]
    assert {sc["lm"] for sc in picks} == {8}
    group = [sc for sc in S.scenarios() if sc["lm"] == 8]
    rev = dict(zip([sc["name"] for sc in group[::-1]], S.run_gpu_step(binding, group[::-1], 8)))
    for sc in picks:
        alone = S.run_gpu_step(binding, [sc], 8)[0]
        assert step_bytes(alone) == step_bytes(step_runs[sc["name"]]) == step_bytes(rev[sc["name"]]), sc["name"]
    gpu, index = loop_world["gpu"], loop_world["index"]
    for sc in picks:
        same = [s for s in S.scenarios() if (s["outer"], s["lm"]) == (sc["outer"], sc["lm"])]
        alone = S.run_gpu_loop(gpu, [sc], index, sc["outer"], sc["lm"])[0]
        back = S.run_gpu_loop(gpu, same[::-1], index, sc["outer"], sc["lm"])[len(same) - 1 - same.index(sc)]
        assert len(same) > 1 and raw(alone) == raw(loop_runs[sc["name"]]) == raw(back), sc["name"]


def test_the_device_reaches_every_branch(oracle, step_runs, loop_runs):
    """branches() over the device's own summaries - termination0 and lm_iterations0 of the mapping step, the last round's pair of a loop
    result - with the oracle's `successful` of the same round, which the two tests above have tied to the device's by equal iterations,
    terminations and poses."""
    for route in ("step", "loop"):
        seen, rejected = set(), 0
        for sc in S.scenarios():
            (r,) = S.visible(route, [x["summary"] for x in oracle[sc["name"]][route]["rounds"]])
            if route == "step":
                own = {"iterations": step_runs[sc["name"]]["info"]["lm_iterations0"], "termination": step_runs[sc["name"]]["info"]["termination0"]}
            else:
                own = {"iterations": int(loop_runs[sc["name"]]["lm_iterations"]), "termination": int(loop_runs[sc["name"]]["lm_termination"])}
            if (own["iterations"], own["termination"]) == (r["iterations"], r["termination"]):
                own["successful"] = r["successful"]
            seen |= S.branches([own])
            rejected += S.rejected_rounds([own])
        print(f"{route}: {sorted(seen)}, {rejected} rounds with a rejected step")
        assert {f"termination{k}" for k in range(5)} <= seen and "termination5" not in seen and rejected >= 3, (route, seen, rejected)
