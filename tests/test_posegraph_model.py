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


@pytest.mark.parametrize("robust", [False, True])
def test_gradient_against_central_differences(robust):
    d = pg.drifted_laps(2, 14, 2)
    edges = np.concatenate([d["odom"], d["loop"], pg.anchor_from_localization(9, d["q_true"][9], d["t_true"][9], d["info"])])
    delta = 1.0
    if robust:
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
