"""The scenario list of tests/map_lm_scenarios.py against the oracle alone (no GPU): what the list reaches, how stable the oracle's decisions
are on it, and which scenarios are admitted to which class.  tests/test_gpu_map_lm_branches.py demands the same of the device; this file keeps
it from passing by emptiness."""
import importlib

import numpy as np
import pytest

import loopreg_model as M
import map_lm_scenarios as S

info = importlib.import_module("a-loam_amd.information")
L = importlib.import_module("a-loam_amd.loopreg")


@pytest.fixture(scope="module")
def evaluated(O):
    return [(sc, S.evaluate(sc["name"])) for sc in S.scenarios()]


def test_the_list_holds_every_family(O):
    scs = S.scenarios()
    names = [sc["name"] for sc in scs]
    assert len(set(names)) == len(names) >= 40
    for family in ("full-truth", "full-drift", "full-1m10deg", "full-2m20deg", "full-30m", "ground-c0", "ground-c2", "draw"):
        assert any(n.startswith(family) for n in names), family
    for nc, ns in S.CUTS:
        for start in ("drift", "truth"):
            sc = next(s for s in scs if s["name"] == f"cut-c{nc}-p{ns}-{start}")
            assert (len(sc["corner"]), len(sc["surf"])) == (nc, ns)
    assert {sc["lm"] for sc in scs} == {4, 8} and {sc["outer"] for sc in scs} == {1, 2, 3}
    assert len(S.POSE_NOT_COMPARED) <= 3 and all(n in names and r in ("step", "loop") for n, r in S.POSE_NOT_COMPARED)
    for sc in scs:                                    # a filtered point is alone in its voxel: both routes' filters hand the cut clouds on as they are
        assert np.isfinite(sc["corner"]).all() and np.isfinite(sc["surf"]).all()
        for cloud, leaf in ((sc["corner"], M.LEAF[0]), (sc["surf"], M.LEAF[1])):
            if len(cloud):
                assert np.array_equal(M.voxel_filter(cloud, leaf).view(np.uint32), cloud.view(np.uint32)), sc["name"]


def test_decisions_are_stable_and_every_scenario_is_admitted(evaluated):
    """Factor counts, iterations, successful steps and terminations of every round (and the loop route's status) are the same under the oracle's
    dual-number and closed-form Jacobians and with the records in reversed order; on the mapping step the composed model tells
    Oracle.mapping_step's story.  spread_k, the largest pose difference among the variants, is within the class's admission bound."""
    deficient = 0
    for sc, ev in evaluated:
        print(f"{sc['name']:24s} {ev['class']:14s} lm {sc['lm']} outer {sc['outer']}  step: spread_k {ev['step']['spread']:.2e} {ev['step']['decisions']}  "
              f"loop: spread_k {ev['loop']['spread']:.2e} status {ev['loop']['oracle']['status']} {ev['loop']['decisions']}")
        for route in ("step", "loop"):
            e = ev[route]
            assert e["stable"], (sc["name"], route, e["told"])
            assert e["spread"] <= (S.FULL_SPREAD if e["full_rank"] else S.DEFICIENT_SPREAD), (sc["name"], route, e["spread"])
        step = ev["step"]["oracle"]
        assert step["info"]["frame_count"] == len(S.MAP_NODES) + 1 and step["info"]["from_map_corner"] > 10 and step["info"]["from_map_surf"] > 50
        assert (len(step["stacks"][0]), len(step["stacks"][1])) == (len(sc["corner"]), len(sc["surf"]))
        deficient += ev["class"] == "rank-deficient"
    print(f"{len(evaluated)} scenarios, {deficient} rank-deficient")
    assert len(evaluated) >= 40 and deficient >= 12


def test_both_routes_reach_every_branch_but_failure(evaluated):
    """Terminations 0 .. 4 and at least three rounds with a rejected step on each route; an INFO_SINGULAR and a NO_FACTORS record behind the
    mapping step; LOOP_SOLVE_FAILED both without a factor and, with factors, through a pivot that is not positive.  Termination 5 needs a
    non-finite sum, which finite f32 clouds cannot give (lm_device.hpp): not demanded, not provoked."""
    for route in ("step", "loop"):
        seen, rejected = set(), 0
        for sc, ev in evaluated:
            rounds = [r["summary"] for r in ev[route]["rounds"]]
            seen |= S.branches(rounds)
            rejected += S.rejected_rounds(rounds)
        print(f"{route}: {sorted(seen)}, {rejected} rounds with a rejected step")
        assert {f"termination{k}" for k in range(5)} <= seen and "termination5" not in seen and rejected >= 3, (route, seen, rejected)
        # what the device's records can show: termination0 of the mapping step, the last round's termination of a loop result
        shown, shown_rejected = set(), 0
        for sc, ev in evaluated:
            rounds = S.visible(route, [r["summary"] for r in ev[route]["rounds"]])
            shown |= S.branches(rounds)
            shown_rejected += S.rejected_rounds(rounds)
        print(f"{route}, the rounds the device shows: {sorted(shown)}, {shown_rejected} with a rejected step")
        assert {f"termination{k}" for k in range(5)} <= shown and shown_rejected >= 3, (route, shown, shown_rejected)
    statuses = [ev["step"]["status"] for _, ev in evaluated]
    assert info.INFO_SINGULAR in statuses and info.INFO_NO_FACTORS in statuses and info.INFO_OK in statuses
    gate = next(ev for sc, ev in evaluated if sc["name"].startswith("full-30m"))["step"]["oracle"]["info"]
    assert gate["from_map_corner"] > 10 and gate["from_map_surf"] > 50 and gate["corner_num1"] + gate["surf_num1"] == 0      # the gate is true, no factor
    failed = [ev["loop"]["oracle"] for _, ev in evaluated if ev["loop"]["oracle"]["status"] == L.LOOP_SOLVE_FAILED]
    assert any(r["n_line"] + r["n_plane"] == 0 for r in failed) and sum(1 for r in failed if r["n_line"] + r["n_plane"] > 0) >= 5
    assert sum(1 for _, ev in evaluated if ev["loop"]["oracle"]["status"] == L.LOOP_OK and not ev["loop"]["full_rank"]) >= 1
    assert all(ev["loop"]["oracle"]["status"] in (L.LOOP_OK, L.LOOP_SOLVE_FAILED) for _, ev in evaluated)


def test_the_trace_tells_the_oracles_story_and_explains_the_poses_not_compared(evaluated):
    """lm_trace, the numpy restatement of the loop, ends every round of a sample of scenarios with the oracle's iterations, successful steps
    and termination.  For a (scenario, route) on POSE_NOT_COMPARED it must show what the issue asks before a pose may be left out: the
    condition number of the damped, scaled system at every iteration, and eps x condition x |step| far above the bound."""
    listed = {n for n, _ in S.POSE_NOT_COMPARED}
    sample = [(sc, ev) for sc, ev in evaluated if sc["name"] in listed or sc["name"].startswith(("full-drift", "cut-c2-p0", "draw40", "draw66", "ground-c2-p12"))]
    assert len(sample) >= 6
    for sc, ev in sample:
        for route in ("step", "loop"):
            worst = 0.0
            for k, r in enumerate(ev[route]["rounds"]):
                if r["n_line"] + r["n_plane"] == 0:
                    continue
                summary, trace = S.lm_trace(r["factors"][0], r["factors"][1], r["entry"], sc["lm"])
                assert summary == {key: r["summary"][key] for key in ("iterations", "successful", "termination")}, (sc["name"], route, k)
                worst = max([worst] + [np.finfo(float).eps * c * d for c, d, _ in trace if np.isfinite(d)])
                if (sc["name"], route) in S.POSE_NOT_COMPARED:
                    print(f"{sc['name']} {route} round {k}: (condition number, |step|, accepted) " + " ".join(f"({c:.1e}, {d:.1e}, {int(a)})" for c, d, a in trace))
            if (sc["name"], route) in S.POSE_NOT_COMPARED:
                print(f"{sc['name']} {route}: eps x condition x |step| up to {worst:.1e}, bound {S.pose_bound(ev, route):.1e}")
                assert worst > 100.0 * S.pose_bound(ev, route)


def test_branches_names_what_a_summary_proves():
    assert S.branches([{"iterations": 8, "successful": 5, "termination": 0}]) == {"termination0", "rejected"}
    assert S.branches([{"iterations": 3, "successful": 2, "termination": 2}]) == {"termination2"}        # a tolerance exit spends an iteration
    assert S.branches([{"iterations": 4, "successful": 2, "termination": 1}]) == {"termination1", "rejected"}
    assert S.branches([{"iterations": 3, "successful": 3, "termination": 3}, {"iterations": 0, "successful": 0, "termination": 4}]) == {"termination3", "termination4"}
    assert S.branches([{"iterations": 8, "termination": 0}]) == {"termination0"}                          # no `successful`, no claim


def test_the_pivot_rule_of_the_model_is_the_devices():
    """np.linalg.cholesky accepts a pivot that rounding left at +1e-17; the device and information.decompose do not."""
    J = np.array([[1.0, 0.5, 0, 0, 0, 0.25], [0, 1.0, 0.5, 0, 0, 0], [0, 0, 1.0, 0.5, 0, 0], [0, 0, 0, 1.0, 0.5, 0], [0, 0, 0, 0, 1.0, 0.5]])
    H = J.T @ J                                                                   # rank 5
    assert not M.positive_definite(H) and M.positive_definite(H + 1e-6 * np.eye(6)) and M.positive_definite(np.eye(6))
    assert not M.positive_definite(np.zeros((6, 6)))
