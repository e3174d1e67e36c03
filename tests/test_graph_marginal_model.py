"""posegraph.marginals, the numpy model of aloam_graph_marginals, without a GPU: against brute force (Jacobians by central
differences of the residual under the retraction, the inverse of the full H), its identities, its two routes against each other, and the
chi-square gate on the seven candidates the device is tested with."""
import numpy as np
import pytest

import graph_marginal_cases as mc
import posegraph_cases as pc
from posegraph_cases import pg

H_STEP = 1e-5                          # central differences: truncation ~ h^2 = 1e-10, rounding ~ 1e-16 x 10 m / h = 1e-10


def numeric_jacobian(q, t, edges):
    """d residual / d (left perturbation of every node) [E, 6, N, 6] by central differences."""
    N = len(q)
    J = np.zeros((len(edges), 6, N, 6))
    for k in range(N):
        for a in range(6):
            d = np.zeros((N, 6))
            d[k, a] = H_STEP
            rp = pg.residual(*pg.retract(q, t, d), edges)
            rm = pg.residual(*pg.retract(q, t, -d), edges)
            J[:, :, k, a] = (rp - rm) / (2 * H_STEP)
    return J


def brute_force(q, t, edges, cand, huber_delta=1.0):
    N = len(q)
    w = pg.linearize(q, t, edges, huber_delta)[1]
    Je = numeric_jacobian(q, t, edges)[:, :, 1:, :].reshape(len(edges), 6, 6 * (N - 1))
    H = np.einsum("e,eak,eab,ebl->kl", w, Je, pg.info_full(edges["info"]), Je)
    Hinv = np.linalg.inv(H)
    Jc = numeric_jacobian(q, t, cand)[:, :, 1:, :].reshape(len(cand), 6, 6 * (N - 1))
    cov = np.einsum("cak,kl,cbl->cab", Jc, Hinv, Jc)
    r = pg.residual(q, t, cand)
    Om = pg.info_full(cand["info"])
    s_edge = np.einsum("ca,cab,cb->c", r, Om, r)
    chi2 = np.array([r[c] @ np.linalg.solve(cov[c] + np.linalg.inv(Om[c]), r[c]) for c in range(len(cand))])
    return dict(cov=cov, s_edge=s_edge, chi2=chi2)


@pytest.mark.parametrize("cond", pc.CONDS)
def test_against_brute_force(cond):
    """The difference is what central differences with h = 1e-5 leave (1e-10 of a Jacobian entry, carried through H^-1); an error of
    structure - a dropped or transposed block, a sign, a missing rho' - changes Sigma_r by a part of itself.  1e-5 lies between the two
    with four decades to either side.  Measured: 3.1e-10 at condition 1e2, 5.1e-10 at 1e6."""
    case, q, t = mc.solved(cond)
    cand = mc.candidates(case)
    m = pg.marginals(q, t, case["edges"], cand)
    b = brute_force(q, t, case["edges"], cand)
    dev = mc.deviation(m, b)
    print(f"cond {cond:g}: the model against brute force {dev:.3e}")
    assert (m["status"] == pg.MARGINAL_OK).all() and dev <= 1e-5
    at = pg.marginals(q, t, case["edges"], cand, pg.MARGINAL_AT_ESTIMATE)
    assert not at["chi2"].any() and not at["s_edge"].any() and np.abs(at["r"]).max() <= 1e-14
    zq, zt = at["q"], at["t"]
    for c in range(len(cand)):
        i, j = int(cand["i"][c]), int(cand["j"][c])
        want = pg.relative_pose(pc.IDENT_Q if i < 0 else q[i], pc.ZERO_T if i < 0 else t[i], q[j], t[j])
        assert np.array_equal(zq[c], want[0]) and np.array_equal(zt[c], want[1])
    moved = cand.copy()
    moved["q"], moved["t"] = zq, zt
    assert mc.deviation(dict(at, chi2=b["chi2"] * 0, s_edge=b["s_edge"] * 0), dict(brute_force(q, t, case["edges"], moved), chi2=b["chi2"] * 0, s_edge=b["s_edge"] * 0)) <= 1e-5


@pytest.mark.parametrize("name", [1e2, 1e6, "hub"])
def test_identities_and_the_gate(name):
    """chi2 <= s_edge for every candidate; the six consistent candidates below the 6-dof 0.999 quantile (2.6 - 14.9 over the three graphs), the
    one displaced by 1.5 m above it (255 - 3357); the two routes of the model agree (eps_marg); (-1, 0) has Sigma_r = 0 and chi2 == s_edge."""
    case, q, t = mc.solved(name)
    cand = mc.candidates(case)
    pair = mc.model_pair(q, t, case["edges"], cand)
    m, chain = pair["dense"], pair["chain"]
    print(f"{name}: chi2 {m['chi2'].round(2).tolist()} against {mc.GATE:.2f}; s_edge {m['s_edge'].round(1).tolist()}; eps_marg {pair['eps']:.3e}; PCG {chain['pcg_iterations'].tolist()}")
    assert len(cand) == 7 and (m["status"] == 0).all() and (chain["status"] == 0).all()
    assert (m["chi2"] <= m["s_edge"]).all() and (m["chi2"] > 0).all()
    assert (m["chi2"][:6] < mc.GATE).all() and m["chi2"][6] > mc.GATE
    assert 2.5 < m["chi2"][:6].min() and m["chi2"][:6].max() < 15.0 and 250 < m["chi2"][6] < 3400
    assert pair["eps"] <= (1e-9 if name == 1e6 else 1e-12)          # the conditioning of H times the PCG tolerance of 1e-13, with room
    assert (chain["pcg_iterations"] > 0).all() and (chain["pcg_iterations"] <= 6 * 200).all()
    zero = pg.marginals(q, t, case["edges"], pg.make_edges(0, [-1], [0], pc.IDENT_Q[None], np.array([[0.1, -0.2, 0.3]]), np.diag([4.0, 5, 6, 7, 8, 9])[None]),
                        solve=pg.marginal_solver(mc.TOL, 200))
    assert zero["status"][0] == 0 and not zero["cov"].any() and zero["pcg_iterations"][0] == 0 and zero["chi2"][0] == zero["s_edge"][0] > 0


@pytest.mark.parametrize("cond", pc.CONDS)
def test_woodbury(cond):
    """A plain candidate appended to the edges, at the same estimates: Sigma_r' = Sigma_r - Sigma_r S^-1 Sigma_r with S = Sigma_r + Omega^-1."""
    case, q, t = mc.solved(cond)
    cand = mc.candidates(case)
    for c in (0, 1, 2, 4):
        one = cand[c:c + 1]
        before = pg.marginals(q, t, case["edges"], one)["cov"][0]
        after = pg.marginals(q, t, np.concatenate([case["edges"], one]), one)["cov"][0]
        S = before + np.linalg.inv(pg.info_full(one["info"][0]))
        want = before - before @ np.linalg.solve(S, before)
        d = np.sqrt(np.diag(want))
        dev = float(np.max(np.abs(after - want) / (d[:, None] * d[None, :])))
        print(f"cond {cond:g} candidate {c}: Woodbury {dev:.3e}")
        assert dev <= (1e-6 if cond == 1e6 else 1e-10)              # f64 through H^-1 twice; an edge entered with a wrong weight or tangent misses by a part of Sigma_r


def test_statuses_and_the_capped_route():
    case, q, t = mc.solved(1e2)
    cand = mc.candidates(case)[:2]
    none = pg.marginals(q[:1], t[:1], case["edges"][:0], pg.make_edges(0, [-1], [0], pc.IDENT_Q[None], pc.ZERO_T[None], np.eye(6)[None]))
    assert none["status"][0] == pg.MARGINAL_NO_EDGES and not none["cov"].any() and none["nodes"][0] == 1
    one = pg.marginals(q, t, case["edges"], cand, solve=pg.marginal_solver(1e-10, 1))
    assert (one["status"] == pg.MARGINAL_NOT_CONVERGED).all() and (one["pcg_iterations"] == 6).all()
    a, b = (pg.marginals(q, t, case["edges"], cand, solve=s(mc.TOL, 1)) for s in (pg.chain_solver, pc.chain_solver_dense))
    assert mc.deviation(one, a) <= 1e-12 and mc.deviation(a, b) <= 1e-12        # marginal_solver is chain_solver with its factor kept
    robust = case["edges"].copy()
    robust["flags"] = pg.EDGE_ROBUST
    tight, loose = (pg.marginals(q, t, robust, cand, huber_delta=d)["cov"] for d in (0.3, 1e6))
    plain = pg.marginals(q, t, case["edges"], cand)["cov"]                  # every s is far below 1e12: flagged edges weigh as plain ones
    assert np.array_equal(loose, plain) and (np.einsum("kii->ki", tight) > np.einsum("kii->ki", loose)).all()      # down-weighted edges: a wider marginal
