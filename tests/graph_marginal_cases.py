"""What the tests of the pose-graph marginals share (aloam_graph_marginals, posegraph.marginals): the seven candidate edges of
the gate, the yardstick eps_marg measured between the model's two routes, and the comparison every layer's result is held to."""
import functools

import numpy as np

import posegraph_cases as pc
from posegraph_cases import pg

TOL = 1e-13                           # pcg_tolerance of every device-against-model comparison
GATE = pg.chi2_gate()                 # the 6-dof 0.999 quantile, 22.46
RESULT_DTYPE = np.dtype([("status", np.int32), ("mode", np.int32), ("seq", np.int32), ("i", np.int32), ("j", np.int32), ("pcg_iterations", np.int32),
                         ("nodes", np.int32), ("edges", np.int32), ("chi2", np.float64), ("s_edge", np.float64), ("r", np.float64, 6), ("q", np.float64, 4),
                         ("t", np.float64, 3), ("cov", np.float64, (6, 6))])


def candidates(case, seq=0):
    """Six candidate edges measured on the case's ground truth with the noise of their own information (far apart, near, anchors, to the fixed
    node, in both orientations, neighbours), and a copy of the first displaced by 1.5 m along x: the seven requests of the gate."""
    N = len(case["q"])
    good = pc.dense_edges(np.random.default_rng(5), case["q_true"], case["t_true"], [2, 30, -1, 0, N - 1, 5], [N - 2, 9, N - 1, N - 1, 1, 6], 1e2, seq=seq)
    bad = good[:1].copy()
    bad["t"][0, 0] += 1.5
    return np.concatenate([good, bad])


def requests(cand, mode=pg.MARGINAL_MEASURED):
    r = np.zeros(len(cand), pg.MARGINAL_REQUEST_DTYPE)
    r["edge"], r["mode"] = cand, mode
    return r


def deviation(a, ref):
    """The largest of: |cov_a - cov_ref| entrywise relative to sqrt(cov_ref[i, i] cov_ref[j, j]); the relative deviations of chi2 and s_edge
    (absolute where the reference is 0).  a and ref are dicts or structured arrays with cov, chi2, s_edge."""
    ca, cr = np.asarray(a["cov"], np.float64).reshape(-1, 6, 6), np.asarray(ref["cov"], np.float64).reshape(-1, 6, 6)
    d = np.sqrt(np.einsum("kii->ki", cr))
    scale = d[:, :, None] * d[:, None, :]
    worst = float(np.max(np.abs(ca - cr) / np.where(scale > 0, scale, 1.0)))
    for f in ("chi2", "s_edge"):
        x, y = np.asarray(a[f], np.float64).ravel(), np.asarray(ref[f], np.float64).ravel()
        worst = max(worst, float(np.max(np.abs(x - y) / np.where(y != 0, np.abs(y), 1.0))))
    return worst


_PAIR = {}


def model_pair(q, t, edges, cand, mode=pg.MARGINAL_MEASURED, huber_delta=1.0, tol=TOL, max_iterations=200):
    """The model's two routes on one problem: dense (np.linalg.solve) and chain-PCG (marginal_solver) at `tol`; eps = their deviation."""
    key = (np.asarray(q).tobytes(), np.asarray(t).tobytes(), edges.tobytes(), cand.tobytes(), np.asarray(mode).tobytes(), huber_delta, tol, max_iterations)
    if key not in _PAIR:
        dense = pg.marginals(q, t, edges, cand, mode, huber_delta)
        chain = pg.marginals(q, t, edges, cand, mode, huber_delta, solve=pg.marginal_solver(tol, max_iterations))
        _PAIR[key] = dict(dense=dense, chain=chain, eps=deviation(chain, dense))
    return _PAIR[key]


def check_against_model(what, res, q, t, edges, cand, eps, mode=pg.MARGINAL_MEASURED, huber_delta=1.0):
    """A layer's results `res` (RESULT_DTYPE, run with pcg_tolerance TOL) for the candidates at the estimates (q, t): within 8 eps of the model's
    dense route (eps = eps_marg of the family), its iterations at most twice the model's."""
    pair = model_pair(q, t, edges, cand, mode, huber_delta)
    dev = deviation(res, pair["dense"])
    its, model_its = res["pcg_iterations"].astype(int), pair["chain"]["pcg_iterations"].astype(int)
    print(f"{what}: against the model's dense route {dev:.3e} (the model's two routes {pair['eps']:.3e}, eps_marg {eps:.3e}, tolerance {8 * eps:.3e}); "
          f"chi2 {np.array2string(res['chi2'], precision=2)} s_edge {np.array2string(res['s_edge'], precision=1)}; PCG {its.tolist()} (model {model_its.tolist()})")
    assert (res["status"] == pg.MARGINAL_OK).all() and (res["nodes"] == len(q)).all() and (res["edges"] == len(edges)).all()
    assert (res["i"] == cand["i"]).all() and (res["j"] == cand["j"]).all()
    assert dev <= 8 * eps
    assert (its <= 2 * model_its).all() and its.sum() <= 2 * model_its.sum()
    return dev


@functools.lru_cache(maxsize=None)
def solved(name):
    """The model's solve of a case (pc.OPTIONS): (case, q, t).  name: 1e2, 1e6 (step_case) or "hub" (solved with the chain-PCG route: the dense
    solve of 515 nodes takes a quarter of a minute)."""
    case = pc.hub_case() if name == "hub" else pc.step_case(name)
    q, t, m = pg.optimize(case["q"], case["t"], case["edges"], solve=pg.marginal_solver(1e-10, 200) if name == "hub" else None, **pc.OPTIONS)
    assert m["status"] == 0 and m["final_cost"] < m["initial_cost"], m
    return case, q, t
