"""What the pose-graph tests share: the solver options they run with, eps_ref, and the helpers that enter a graph into a context through
aloam_set_state and read it back."""
import functools
import importlib
import os

import numpy as np

pg = importlib.import_module("a-loam_amd.posegraph")

GOLDEN_SCIPY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_scipy_300.npy")
REF_GRAPH = (1, 300, 2)              # drifted_laps arguments: the graph the GPU tests solve


@functools.lru_cache(maxsize=None)
def eps_ref():
    """What two CPU solvers differ by on the graph the GPU tests solve, measured where it is used: the largest difference in any pose
    component (radians, metres) between posegraph.optimize, run here, and scipy.optimize.least_squares (trf, ftol = xtol = gtol = 1e-15) on
    the whitened residuals of drifted_laps(*REF_GRAPH).  scipy's answer is recorded (tests/golden/posegraph_scipy_300.npy, written by
    `python tests/posegraph_cases.py`: its solve takes twenty seconds, and the GPU tests need the figure too);
    test_posegraph_model.py checks the record against the model and runs scipy itself on a smaller graph.  About 1.0e-8: scipy stops on
    xtol at optimality 8.5e-10."""
    d = pg.drifted_laps(*REF_GRAPH)
    q, t, _ = pg.optimize(d["q"], d["t"], np.concatenate([d["odom"], d["loop"]]), **OPTIONS)
    ref = scipy_reference()
    return pg.pose_difference(q, t, ref["q"], ref["t"])


def scipy_reference():
    """The record: rows 0 .. N - 1 hold q | t, the last row scipy's cost and optimality."""
    a = np.load(GOLDEN_SCIPY)
    return dict(q=a[:-1, :4], t=a[:-1, 4:], cost=float(a[-1, 0]), optimality=float(a[-1, 1]))


# function_tolerance 0: a solve ends on its gradient, so that two solvers are compared at the minimum and not where each one gave up.
OPTIONS = dict(max_iterations=50, function_tolerance=0.0, gradient_tolerance=1e-10, pcg_tolerance=1e-8, pcg_max_iterations=200, huber_delta=1.0)
IDENT_Q, ZERO_T = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)


def enter(gpu, graphs, info):
    """graphs: {seq: (q [n, 4], t [n, 3])}.  Node k of every sequence is entered with one aloam_graph_add_nodes after its pose was
    injected as the odometry's q_w / t_w."""
    longest = max(len(q) for q, _ in graphs.values())
    for k in range(longest):
        listed = [b for b, (q, _) in graphs.items() if k < len(q)]
        for b in listed:
            gpu.set_state(IDENT_Q, ZERO_T, graphs[b][0][k], graphs[b][1][k], seq=b)
        gpu.graph_add_nodes(listed, info)


def with_seq(edges, seq):
    e = edges.copy()
    e["seq"] = seq
    return e


def scipy_optimize(q0, t0, edges):
    """least_squares on the whitened residuals L^T r (Omega = L L^T), parameters = a left perturbation of the start; returns q, t."""
    from scipy.optimize import least_squares
    N = len(q0)
    Lw = np.linalg.cholesky(pg.info_full(edges["info"])).transpose(0, 2, 1)

    def left_jacobian(th):
        n = np.linalg.norm(th, axis=-1)[:, None, None]
        K = pg._skew(th)
        m = np.where(n > 1e-8, n, 1.0)
        a = np.where(n > 1e-8, (1 - np.cos(m)) / m ** 2, 0.5)
        b = np.where(n > 1e-8, (m - np.sin(m)) / m ** 3, 1 / 6.0)
        return np.eye(3) + a * K + b * K @ K

    def unpack(x):
        d = np.zeros((N, 6))
        d[1:] = x.reshape(N - 1, 6)
        return pg.retract(q0, t0, d), d

    def fun(x):
        (q, t), _ = unpack(x)
        return np.einsum("eab,eb->ea", Lw, pg.residual(q, t, edges)).ravel()

    def jac(x):
        (q, t), d = unpack(x)
        _, _, Ji, Jj, _ = pg.linearize(q, t, edges)
        JL = left_jacobian(d[:, :3])
        J = np.zeros((len(edges), 6, N, 6))
        for e in range(len(edges)):
            i, j = int(edges["i"][e]), int(edges["j"][e])
            A = Jj[e].copy(); A[:, :3] = A[:, :3] @ JL[j]
            J[e, :, j, :] = Lw[e] @ A
            if i >= 0:
                A = Ji[e].copy(); A[:, :3] = A[:, :3] @ JL[i]
                J[e, :, i, :] = Lw[e] @ A
        return J[:, :, 1:, :].reshape(len(edges) * 6, (N - 1) * 6)

    sol = least_squares(fun, np.zeros(6 * (N - 1)), jac=jac, method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
    (q, t), _ = unpack(sol.x)
    return q, t, sol


if __name__ == "__main__":          # records scipy's solution of the GPU tests' graph
    d = pg.drifted_laps(*REF_GRAPH)
    q, t, sol = scipy_optimize(d["q"], d["t"], np.concatenate([d["odom"], d["loop"]]))
    np.save(GOLDEN_SCIPY, np.vstack([np.hstack([q, t]), [sol.cost, sol.optimality, 0, 0, 0, 0, 0]]))
    print(f"{GOLDEN_SCIPY}: cost {sol.cost:.12g}, optimality {sol.optimality:.3e}, status {sol.status}, eps_ref {eps_ref():.4e}")
