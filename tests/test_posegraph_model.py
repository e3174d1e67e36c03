"""The numpy model of the pose graphs (a-loam_amd/posegraph.py) against itself, against central differences and against scipy: no GPU."""
import numpy as np
import pytest

import posegraph_cases as pc
from posegraph_cases import OPTIONS, eps_ref, pg


@pytest.fixture(scope="module")
def small():
    d = pg.drifted_laps(1, 120, 2)
    return d, np.concatenate([d["odom"], d["loop"]])


def test_the_residual_is_zero_on_a_consistent_graph():
    d = pg.drifted_laps(4, 60, 3, noise=0.0)
    edges = np.concatenate([d["odom"], d["loop"], pg.anchor_from_localization(31, d["q_true"][31], d["t_true"][31], d["info"]),
                            pg.loop_from_localization(5, d["q_true"][5], d["t_true"][5], 50, d["q_true"][50], d["t_true"][50], d["info"])])
    r = pg.residual(d["q_true"], d["t_true"], edges)
    print(f"largest residual on the ground truth: {np.abs(r).max():.3e}")
    assert np.abs(r).max() <= 1e-13                     # a handful of f64 roundings on translations of ten metres
    assert pg.cost(d["q_true"], d["t_true"], edges) <= 1e-18
    # and the chain built from the odometry edges alone reproduces them
    assert np.abs(pg.residual(d["q"], d["t"], d["odom"])).max() <= 1e-12


@pytest.mark.parametrize("robust", [False, True, pytest.param(0.3, id="dense-0.3"), pytest.param(3.0, id="dense-3.0")])
def test_gradient_against_central_differences(robust):
    """The two isotropic cases, and the dense one: step_case(1e4) - every edge with a dense information of its own at condition 1e4 (1e6 with
    the radian / metre scaling), anchors on nodes 0, 1 and 17, flagged edges on both sides of delta^2 at either delta."""
    d = pg.drifted_laps(2, 14, 2)
    edges = np.concatenate([d["odom"], d["loop"], pg.anchor_from_localization(9, d["q_true"][9], d["t_true"][9], d["info"])])
    delta = 1.0
    if robust not in (False, True):
        d, delta = pc.step_case(1e4), robust
        edges = d["edges"]
    elif robust:
        edges["flags"][-3:] = pg.EDGE_ROBUST
        delta = 0.5
        s = np.einsum("ea,eab,eb->e", *(lambda r: (r, pg.info_full(edges["info"]), r))(pg.residual(d["q"], d["t"], edges)))
        assert (s[-3:] > delta ** 2).any()              # the Huber branch is exercised
    g = pg.gradient(d["q"], d["t"], edges, delta)
    num, h = np.zeros_like(g), 1e-6
    for k in range(1, len(g)):
        for c in range(6):
            dd = np.zeros((len(g), 6)); dd[k, c] = h
            num[k, c] = (pg.cost(*pg.retract(d["q"], d["t"], dd), edges, delta) - pg.cost(*pg.retract(d["q"], d["t"], -dd), edges, delta)) / (2 * h)
    err = np.abs(g - num).max() / np.abs(g).max()
    print(f"gradient against central differences: relative {err:.3e}")
    assert (g[0] == 0).all() and err <= 1e-7            # h^2 truncation plus eps / h of the cost's rounding


@pytest.mark.parametrize("delta", [0.3, 3.0])
def test_normal_equations_against_central_differences_of_the_residual(delta):
    """H of normal_equations without linearize: J by central differences of residual() per edge and node, rho' from s, and
    H_num = sum rho' J^T Omega J assembled here.  The bound: an entry of J is good to dJ = h^2 / 6 D3 + 4 eps |t| / h, with the residual's
    third derivative D3 and |t| at most 20 (a rotation acting on t_j - t_i, at most the circle's diameter): 3e-10 + 2e-9 at h = 1e-5.  An
    entry of H collects 36 products dJ Omega J twice, so against max |H| >= max |Omega| the error is at most 72 dJ max |J| =
    72 * 2.3e-9 * 20 = 3.3e-6 if every term aligned.  A dropped block or a transposed one is an error of order one."""
    c = pc.step_case(1e4)
    q, t, edges = c["q"], c["t"], c["edges"]
    N, E, h = len(q), len(edges), 1e-5
    H, _, _ = pg.normal_equations(q, t, edges, delta)
    Om = pg.info_full(edges["info"])
    s = pc.edge_s(q, t, edges)
    big = (edges["flags"] != 0) & (s > delta ** 2)
    w = np.where(big, delta / np.sqrt(s), 1.0)
    J = np.zeros((E, 6, N, 6))
    for k in range(1, N):
        touched = (edges["i"] == k) | (edges["j"] == k)
        for a in range(6):
            dd = np.zeros((N, 6)); dd[k, a] = h
            J[touched, :, k, a] = (pg.residual(*pg.retract(q, t, dd), edges[touched]) - pg.residual(*pg.retract(q, t, -dd), edges[touched])) / (2 * h)
    Jm = J[:, :, 1:, :].reshape(E, 6, 6 * (N - 1))
    Hn = np.einsum("e,eax,eab,eby->xy", w, Jm, Om, Jm, optimize=True)
    err = np.abs(H - Hn).max() / np.abs(H).max()
    print(f"H against sum rho' J^T Omega J with J by central differences, delta {delta}: relative {err:.3e} (bound 3.3e-6); {int(big.sum())} edges on Huber's linear part")
    assert big.any() and ((edges["flags"] != 0) & ~big).any()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    assert err <= 3.3e-6


def truncated_cases():
    """Every truncated solve of test_gpu_posegraph_steps.py / test_posegraph_emulation.py at its largest k: (name, case, options)."""
    out = [(f"steps cond {c:g} delta {d}", pc.step_case(c), dict(pc.STEP_OPTIONS, huber_delta=d, max_iterations=max(pc.STEPS))) for c in pc.CONDS for d in pc.DELTAS]
    out.append(("rejected", pc.rejected_case(), dict(pc.STEP_OPTIONS, max_iterations=max(pc.REJECTED_STEPS))))
    out.append(("one PCG iteration", pc.step_case(pc.CONDS[0]), dict(pc.STEP_OPTIONS, max_iterations=2, pcg_max_iterations=1)))
    out.append(("hub 515", pc.hub_case(), dict(pc.STEP_OPTIONS, max_iterations=2)))
    return out


@pytest.mark.parametrize("index", range(9))
def test_the_truncated_cases_decide_far_from_the_thresholds(index):
    """What the truncated comparisons rest on: both of the model's solvers take the same decisions, every rel is at least 0.05 away from the
    acceptance threshold 1e-3 (so that a layer with another rounding decides alike), and no iteration ends on the function tolerance.  A
    solve stopped after k iterations is the first k of these."""
    cases = truncated_cases()
    assert len(cases) == 9
    name, case, options = cases[index]
    pair = pc.model_pair(case["q"], case["t"], case["edges"], **options)
    first, chain = pair["first"][3], pair["chain"][3]
    print(f"{name}: " + ", ".join(f"{a['decision']} rel {a['rel']:.3f} | {b['rel']:.3f} radius {a['radius']:.3g}" for a, b in zip(first, chain)) + f"; eps {pair['eps']:.3e}")
    assert len(first) == len(chain) == options["max_iterations"] == pair["first"][2]["lm_iterations"]
    assert pc.decisions(first) == pc.decisions(chain) and set(pc.decisions(first)) <= {"accepted", "rejected"}
    assert all(abs(s["rel"] - 1e-3) >= 0.05 for s in first + chain)
    assert all(abs(a["radius"] - b["radius"]) <= 1e-6 * a["radius"] for a, b in zip(first, chain))
    assert pair["first"][2]["termination"] == pair["chain"][2]["termination"] == 0
    if name == "rejected":
        assert np.cumsum([d == "accepted" for d in pc.decisions(first)]).tolist() == pc.REJECTED_ACCEPTED


def test_the_trace_changes_nothing():
    d = pg.drifted_laps(2, 30, 2)
    edges = np.concatenate([d["odom"], d["loop"]])
    trace = []
    a, b = pg.optimize(d["q"], d["t"], edges, **OPTIONS), pg.optimize(d["q"], d["t"], edges, trace=trace, **OPTIONS)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert len(trace) == a[2]["lm_iterations"] and sum(s["decision"] == "accepted" for s in trace) == a[2]["accepted_steps"]


def test_the_step_cases_carry_what_they_claim():
    for cond in pc.CONDS + (1e4,):
        c = pc.step_case(cond)
        e, s = c["extra"], pc.edge_s(c["q"], c["t"], c["extra"])
        flagged = e["flags"] != 0
        for delta in (0.3, 3.0):
            assert (s[flagged] > delta ** 2).any() and (s[flagged] <= delta ** 2).any()
        loops = e[e["i"] >= 0]
        assert (loops["i"] < loops["j"]).any() and (loops["i"] > loops["j"]).any() and (loops["i"] == loops["j"] + 1).any()
        assert sorted(e["j"][e["i"] < 0]) == [0, 1, 17]
        ev = np.linalg.eigvalsh(pg.info_full(c["edges"]["info"]) * np.outer(pc.SIGMA, pc.SIGMA))
        assert np.allclose(ev[:, -1] / ev[:, 0], cond, rtol=1e-6)                # the condition asked for, with both ends present
        assert np.abs(pg.info_full(c["edges"]["info"])[:, :3, 3:]).min() > 0      # rotation and translation are coupled on every edge
        assert np.abs(pg.residual(c["q"], c["t"], c["odom"])).max() <= 1e-12      # the chain is the odometry's
    h = pc.hub_case()
    assert len(h["q"]) == 515 and (np.r_[h["edges"]["i"], h["edges"]["j"]] == 7).sum() == 302


def test_optimize_against_scipy(small):
    d, edges = small
    q, t, res = pg.optimize(d["q"], d["t"], edges, **OPTIONS)
    qs, ts, sol = pc.scipy_optimize(d["q"], d["t"], edges)
    eps = pg.pose_difference(q, t, qs, ts)
    print(f"eps_ref on drifted_laps(1, 120, 2): {eps:.3e} (300 nodes: {eps_ref():.4e}); model {res}; scipy cost {sol.cost:.12g} optimality {sol.optimality:.3e}")
    assert res["status"] == 0 and res["termination"] == 3
    assert abs(res["final_cost"] - sol.cost) <= 1e-9 * sol.cost
    assert eps <= eps_ref()                              # the smaller graph's two answers are no further apart than the larger's


def test_eps_ref_is_measured_on_the_graph_of_the_gpu_tests():
    """eps_ref: the model, run here, against scipy's recorded answer on drifted_laps(1, 300, 2).  The record is scipy's minimum of the same
    problem: its cost is the model's to 1e-9, and the model's gradient there is what scipy reported as its optimality (within a factor of
    two: scipy's figure is of the whitened problem in its own scaling)."""
    d = pg.drifted_laps(*pc.REF_GRAPH)
    edges = np.concatenate([d["odom"], d["loop"]])
    ref = pc.scipy_reference()
    eps = eps_ref()
    _, _, m = pg.optimize(d["q"], d["t"], edges, **OPTIONS)
    g = float(np.abs(pg.gradient(ref["q"], ref["t"], edges)).max())
    print(f"eps_ref on drifted_laps{pc.REF_GRAPH}: {eps:.4e}; scipy cost {float(ref['cost']):.12g} optimality {float(ref['optimality']):.3e}; "
          f"model cost {m['final_cost']:.12g}; model gradient at scipy's answer {g:.3e}")
    assert abs(pg.cost(ref["q"], ref["t"], edges) - float(ref["cost"])) <= 1e-9 * float(ref["cost"])
    assert abs(m["final_cost"] - float(ref["cost"])) <= 1e-9 * float(ref["cost"])
    assert g <= 2 * float(ref["optimality"])
    assert 0.0 < eps < 1e-6                              # two minima of one problem, not two problems


def test_chain_preconditioner_against_block_jacobi():
    d = pg.drifted_laps(1, 300, 2)
    edges = np.concatenate([d["odom"], d["loop"]])
    H, g, _ = pg.normal_equations(d["q"], d["t"], edges)
    D = np.clip(np.diag(H), 1e-6, 1e32) / 1e4
    xc, kc = pg.chain_solver(1e-8, 5000)(H, D, g)
    xj, kj = pg.jacobi_solver(1e-8, 20000)(H, D, g)
    print(f"PCG iterations on the first linearisation (300 nodes, 2 loops): chain {kc}, block-Jacobi {kj}")
    exact = np.linalg.solve(H + np.diag(D), g)
    assert np.abs(xc - exact).max() <= 1e-6 * np.abs(exact).max()
    assert kc <= 60 and kj >= 10 * kc


def test_ate_improves(small):
    d, edges = small
    q, t, res = pg.chain_pcg(d["q"], d["t"], edges, **OPTIONS)
    before, after = pg.ate(d["t"], d["t_true"]), pg.ate(t, d["t_true"])
    print(f"ATE before {before:.4f} m, after {after:.4f} m; chain_pcg {res}")
    assert res["final_cost"] < res["initial_cost"] and after < before
    qd, td, _ = pg.optimize(d["q"], d["t"], edges, **OPTIONS)
    assert pg.pose_difference(q, t, qd, td) <= eps_ref()      # both linear solvers lead to the same minimum


def test_edges_from_a_localization():
    d = pg.drifted_laps(3, 30, 0)
    a = pg.anchor_from_localization(12, d["q_true"][12], d["t_true"][12], d["info"], seq=2, robust=True)[0]
    assert (a["seq"], a["i"], a["j"], a["flags"]) == (2, -1, 12, pg.EDGE_ROBUST) and np.array_equal(pg.info_full(a["info"]), d["info"])
    e = pg.loop_from_localization(4, d["q_true"][4], d["t_true"][4], 25, d["q_true"][25], d["t_true"][25], d["info"])
    assert np.abs(pg.residual(d["q_true"], d["t_true"], np.concatenate([a[None], e]))).max() <= 1e-13
