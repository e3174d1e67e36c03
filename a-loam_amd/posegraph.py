"""Pose graphs over keyframes: the numpy model of aloam_graph_* (include/aloam_mi355x.h, "pose graphs").

A pose X = (q, t) maps a point of the node's frame into the frame the graph lives in: x' = q x q* + t, q = (x, y, z, w).

    compose(Xa, Xb)      = (q_a q_b, q_a t_b + t_a)
    relative_pose(Xi, Xj) = X_i^-1 o X_j
    edge (i, j, Z, Omega): E = Z^-1 o X_i^-1 o X_j  (X_i = identity for an anchor, i = -1); q_E negated when its w < 0;
                           r = (2 q_E.xyz, t_E),  s = r^T Omega r
    cost = 1/2 sum rho(s);  rho(s) = s, or for robust edges Ceres' HuberLoss(delta): s <= delta^2 ? s : 2 delta sqrt(s) - delta^2
    node 0 is fixed; the tangent of node k is a LEFT perturbation q' = exp(theta / 2) q, t' = t + dt, order (theta, t).

Everything here is float64 numpy on the host: the definition the device is tested against, a dense Levenberg-Marquardt reference
(optimize), the chain-preconditioned conjugate gradients of the device restated (chain_pcg), the robust solve over the flagged edges
(optimize_robust: GNC-TLS), the two lines of algebra that turn a relocalized pose into an edge, the loop proposal by pose proximity
(propose_loops), the sliding window (trim: aloam_graph_trim restated), the joined graphs of several sequences (join, align_member, split,
optimize_joint: aloam_graph_optimize_joint restated), and the fixture generators of the tests (drifted_laps, false_loops, cut_drive).
"""
from __future__ import annotations

import numpy as np

from .records import GRAPH_EDGE_DTYPE as EDGE_DTYPE, GRAPH_MARGINAL_REQUEST_DTYPE as MARGINAL_REQUEST_DTYPE, GRAPH_NODE_DTYPE as NODE_DTYPE
from .joint_records import GRAPH_LINK_DTYPE as LINK_DTYPE
from .link_records import GRAPH_LINK_REQUEST_DTYPE as LINK_REQUEST_DTYPE
from .records import GRAPH_LOOP_REQUEST_DTYPE as LOOP_REQUEST_DTYPE, GRAPH_POSE_ENTERED as POSE_ENTERED, GRAPH_POSE_OPTIMIZED as POSE_OPTIMIZED

EDGE_ROBUST = 1
_IU = np.triu_indices(6)


# ---- quaternions and poses (batched over leading axes) -----------------------------------------------------------------------------
def qmul(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(q):
    q = np.asarray(q, np.float64)
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def qrot(q, v):
    """q v q* as Eigen evaluates it: uv = 2 u x v; v + w uv + u x uv."""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    u = q[..., :3]
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[..., 3:4] * uv + np.cross(u, uv)


def rotmat(q):
    return np.stack([qrot(q, e) for e in np.eye(3)], -1)


def qexp(theta):
    """exp(theta / 2): the unit quaternion of the rotation vector theta."""
    theta = np.asarray(theta, np.float64)
    n = np.linalg.norm(theta, axis=-1, keepdims=True)
    h = 0.5 * n
    k = np.where(n > 0, np.sin(h) / np.where(n > 0, n, 1.0), 0.5)
    return np.concatenate([k * theta, np.cos(h)], -1)


def compose(qa, ta, qb, tb):
    return qmul(qa, qb), qrot(qa, tb) + np.asarray(ta, np.float64)


def inverse(q, t):
    qi = qconj(q)
    return qi, -qrot(qi, t)


def relative_pose(qi, ti, qj, tj):
    """X_i^-1 o X_j: node j in the frame of node i, operation by operation as the device forms an odometry edge."""
    qc = qconj(qi)
    return qmul(qc, qj), qrot(qc, np.asarray(tj, np.float64) - np.asarray(ti, np.float64))


def info_full(info21):
    a = np.asarray(info21, np.float64)
    m = np.zeros(a.shape[:-1] + (6, 6))
    m[..., _IU[0], _IU[1]] = a
    m[..., _IU[1], _IU[0]] = a
    return m


def info_upper(m):
    return np.asarray(m, np.float64)[..., _IU[0], _IU[1]]


def make_edges(seq, i, j, q, t, info, robust=False):
    """A structured array of EDGE_DTYPE; info is [n, 6, 6] / [6, 6] (full) or [n, 21] / [21] (upper triangle)."""
    i = np.atleast_1d(np.asarray(i, np.int32))
    e = np.zeros(len(i), EDGE_DTYPE)
    info = np.asarray(info, np.float64)
    if info.shape[-1] == 6:
        info = info_upper(info)
    e["seq"], e["i"], e["j"], e["q"], e["t"], e["info"] = seq, i, j, q, t, info
    e["flags"] = np.where(np.broadcast_to(robust, i.shape), EDGE_ROBUST, 0)
    return e


# ---- the problem ---------------------------------------------------------------------------------------------------------------------
def _edge_frames(q, t, edges):
    i, j = edges["i"], edges["j"]
    anchor = i < 0
    qi = np.where(anchor[:, None], np.array([0.0, 0.0, 0.0, 1.0]), q[np.maximum(i, 0)])
    ti = np.where(anchor[:, None], 0.0, t[np.maximum(i, 0)])
    return qi, ti, q[j], t[j], anchor


def residual(q, t, edges):
    """r [E, 6] = (2 q_E.xyz, t_E) with E = Z^-1 o X_i^-1 o X_j."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    qi, ti, qj, tj, _ = _edge_frames(q, t, edges)
    qd, td = relative_pose(qi, ti, qj, tj)
    qz = qconj(edges["q"])
    qe, te = qmul(qz, qd), qrot(qz, td - edges["t"])
    qe = np.where(qe[:, 3:4] < 0, -qe, qe)
    return np.concatenate([2.0 * qe[:, :3], te], 1)


def _rho(s, robust, delta):
    big = robust & (s > delta * delta)
    rs = np.sqrt(np.where(big, s, 1.0))
    rho0 = np.where(big, 2.0 * delta * rs - delta * delta, s)
    rho1 = np.where(big, np.maximum(2.2250738585072014e-308, delta / rs), 1.0)
    return rho0, rho1


def cost(q, t, edges, huber_delta=1.0):
    r = residual(q, t, edges)
    s = np.einsum("ea,eab,eb->e", r, info_full(edges["info"]), r)
    return 0.5 * float(np.sum(_rho(s, (edges["flags"] & EDGE_ROBUST) != 0, huber_delta)[0]))


def _skew(v):
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1), np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def linearize(q, t, edges, huber_delta=1.0):
    """r [E, 6], w [E] (rho'), J_i and J_j [E, 6, 6] in the left tangent of the two nodes (J_i of an anchor is zero), rho [E]."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    qi, ti, qj, tj, anchor = _edge_frames(q, t, edges)
    qa = qmul(qconj(edges["q"]), qconj(qi))            # A = Z^-1 o X_i^-1 (rotation part)
    RA = rotmat(qa)
    qe = qmul(qa, qj)
    r0 = residual(q, t, edges)
    qe = np.where(qe[:, 3:4] < 0, -qe, qe)
    B = (qe[:, 3, None, None] * np.eye(3) - _skew(qe[:, :3])) @ RA        # d(2 q_E.xyz) / d theta_j
    E = len(edges)
    Jj = np.zeros((E, 6, 6)); Ji = np.zeros((E, 6, 6))
    Jj[:, :3, :3] = B; Jj[:, 3:, 3:] = RA
    Ji[:, :3, :3] = -B; Ji[:, 3:, 3:] = -RA; Ji[:, 3:, :3] = RA @ _skew(tj - ti)
    Ji[anchor] = 0.0
    s = np.einsum("ea,eab,eb->e", r0, info_full(edges["info"]), r0)
    rho0, rho1 = _rho(s, (edges["flags"] & EDGE_ROBUST) != 0, huber_delta)
    return r0, rho1, Ji, Jj, rho0


def gradient(q, t, edges, huber_delta=1.0):
    """d cost / d (theta_k, t_k) [N, 6]; the row of the fixed node 0 is zero."""
    r, w, Ji, Jj, _ = linearize(q, t, edges, huber_delta)
    Om = info_full(edges["info"])
    wr = w[:, None] * np.einsum("eab,eb->ea", Om, r)
    g = np.zeros((len(q), 6))
    np.add.at(g, edges["j"], np.einsum("eab,ea->eb", Jj, wr))
    m = edges["i"] >= 0
    np.add.at(g, edges["i"][m], np.einsum("eab,ea->eb", Ji[m], wr[m]))
    g[0] = 0.0
    return g


def normal_equations(q, t, edges, huber_delta=1.0):
    """Dense Gauss-Newton H [6 (N - 1), 6 (N - 1)] and g over the nodes 1 .. N - 1, and the cost."""
    r, w, Ji, Jj, rho0 = linearize(q, t, edges, huber_delta)
    N = len(q)
    Om = info_full(edges["info"]) * w[:, None, None]
    H = np.zeros((N, 6, N, 6)); g = np.zeros((N, 6))
    for e in range(len(edges)):
        i, j = int(edges["i"][e]), int(edges["j"][e])
        Tj = Om[e] @ Jj[e]
        H[j, :, j, :] += Jj[e].T @ Tj
        g[j] += Tj.T @ r[e]
        if i >= 0:
            Ti = Om[e] @ Ji[e]
            H[i, :, i, :] += Ji[e].T @ Ti
            g[i] += Ti.T @ r[e]
            Hij = Ji[e].T @ Tj
            H[i, :, j, :] += Hij
            H[j, :, i, :] += Hij.T
    n = 6 * (N - 1)
    return H[1:, :, 1:, :].reshape(n, n), g[1:].reshape(n), 0.5 * float(rho0.sum())


def retract(q, t, delta):
    """The left perturbation delta [N, 6] applied to every node."""
    return qmul(qexp(delta[:, :3]), q), t + delta[:, 3:]


DEFAULT_OPTIONS = dict(max_iterations=20, function_tolerance=1e-10, gradient_tolerance=1e-10, pcg_tolerance=1e-8, pcg_max_iterations=200,
                       huber_delta=1.0)
TERMINATION = {0: "max_iterations", 2: "function_tolerance", 3: "gradient_tolerance", 5: "failure", 6: "min_radius"}


def optimize(q, t, edges, max_iterations=20, function_tolerance=1e-10, gradient_tolerance=1e-10, huber_delta=1.0, solve=None, trace=None, **_):
    """Levenberg-Marquardt with the trust-region rules of the device (lm_device.hpp's, without Jacobi scaling and without the parameter
    tolerance) and a dense solve of every step.  `solve(H, D, g)` replaces the dense solve (chain_pcg's hook).
    `trace`, a list, receives one dict per iteration: rel, model_change, the radius the step was solved with, the cost before and of the
    candidate, and the decision ("accepted", "rejected", "invalid", "function_tolerance").  Returns q, t and a dict with the fields of
    aloam_graph_result."""
    q, t = np.array(q, np.float64), np.array(t, np.float64)
    N = len(q)
    res = dict(status=1, termination=0, lm_iterations=0, accepted_steps=0, pcg_iterations=0, nodes=N, edges=len(edges), initial_cost=0.0,
               final_cost=0.0, gradient_max=0.0)
    if N < 2 or len(edges) == 0:
        return q, t, res
    H, g, c = normal_equations(q, t, edges, huber_delta)
    res.update(status=0, initial_cost=c)
    q0, t0 = q.copy(), t.copy()
    radius, decrease, diag, reuse, invalid, it = 1e4, 2.0, None, False, 0, 0
    gmax = float(np.abs(g).max())
    term = 0
    while True:
        if not (np.isfinite(c) and np.isfinite(gmax)): term = 5; break      # a non-finite cost, gradient or block: failure
        if it >= max_iterations: term = 0; break
        if gmax <= gradient_tolerance: term = 3; break
        if radius <= 1e-32: term = 6; break
        it += 1
        if not reuse:
            diag = np.clip(np.diag(H), 1e-6, 1e32)
        D = diag / radius
        reuse = True
        try:
            if solve is None:
                y = np.linalg.solve(H + np.diag(D), g)
            else:
                y, k = solve(H, D, g)
                res["pcg_iterations"] += k
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            ok = False
        model_change = float(y @ g - 0.5 * y @ (H @ y)) if ok else 0.0
        step = dict(rel=np.nan, model_change=model_change, radius=radius, cost=c, candidate_cost=np.nan, decision="invalid")
        if trace is not None: trace.append(step)
        if not ok or not model_change > 0.0:
            invalid += 1
            if invalid >= 5: term = 5; break
            radius /= decrease; decrease *= 2.0
            continue
        invalid = 0
        d = np.zeros((N, 6)); d[1:] = -y.reshape(N - 1, 6)
        qc, tc = retract(q, t, d)
        cc = cost(qc, tc, edges, huber_delta)
        step.update(candidate_cost=cc, decision="function_tolerance")
        if abs(c - cc) <= function_tolerance * c: term = 2; break
        rel = (c - cc) / model_change
        step.update(rel=rel, decision="accepted" if rel > 1e-3 else "rejected")
        if rel > 1e-3:
            q, t = qc, tc
            H, g, c = normal_equations(q, t, edges, huber_delta)
            res["accepted_steps"] += 1
            gmax = float(np.abs(g).max())
            c3 = 2.0 * rel - 1.0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - c3 ** 3))
            decrease, reuse = 2.0, False
        else:
            radius /= decrease; decrease *= 2.0
    if term == 5 or not c <= res["initial_cost"]:
        q, t, c = q0, t0, res["initial_cost"]
        if term != 5: res["status"] = 2
    if term == 5: res["status"] = 2
    res.update(termination=term, lm_iterations=it, final_cost=c, gradient_max=gmax)
    return q, t, res


# ---- the device's linear solver, restated -------------------------------------------------------------------------------------------
def _chain_mask(n_blocks):
    """Block-tridiagonal pattern over n_blocks 6 x 6 blocks."""
    k = np.arange(n_blocks)
    return np.kron(np.abs(k[:, None] - k[None, :]) <= 1, np.ones((6, 6), bool))


def pcg(A, b, apply_minv, tol=1e-8, max_iterations=200):
    """Preconditioned conjugate gradients from x = 0; stops when sqrt(r^T M^-1 r) <= tol * its first value.  Returns x, iterations."""
    x = np.zeros_like(b); r = b.copy()
    z = apply_minv(r); p = z.copy()
    rz = float(r @ z); rz0 = rz
    k = 0
    if not rz0 > 0.0:
        return x, 0
    while k < max_iterations:
        Ap = A @ p
        alpha = rz / float(p @ Ap)
        x += alpha * p; r -= alpha * Ap
        k += 1
        z = apply_minv(r)
        rz_new = float(r @ z)
        if not rz_new > tol * tol * rz0:
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k


def chain_solver(tol=1e-8, max_iterations=200):
    """solve(H, D, g) for optimize(): PCG on H + diag(D) preconditioned with its block-tridiagonal part (the chain)."""
    def solve(H, D, g):
        from scipy.linalg import cholesky_banded, cho_solve_banded
        A = H + np.diag(D)
        n = len(g)
        band = np.zeros((12, n))                        # upper form: band[11 + i - j, j] = M[i, j]; the chain lies inside bandwidth 11
        M = np.where(_chain_mask(n // 6), A, 0.0)
        for u in range(12):
            band[11 - u, u:] = np.diagonal(M, u)
        cb = cholesky_banded(band)
        return pcg(A, g, lambda r: cho_solve_banded((cb, False), r), tol, max_iterations)
    return solve


def jacobi_solver(tol=1e-8, max_iterations=100000):
    """The same with the 6 x 6 diagonal blocks alone (block-Jacobi): what the chain preconditioner is measured against."""
    def solve(H, D, g):
        A = H + np.diag(D)
        n = len(g) // 6
        inv = np.stack([np.linalg.inv(A[6 * k:6 * k + 6, 6 * k:6 * k + 6]) for k in range(n)])
        return pcg(A, g, lambda r: np.einsum("kab,kb->ka", inv, r.reshape(n, 6)).reshape(-1), tol, max_iterations)
    return solve


def chain_pcg(q, t, edges, **options):
    """optimize() with every step solved by the chain-preconditioned PCG; the result's pcg_iterations is the yardstick of the device's."""
    o = dict(DEFAULT_OPTIONS); o.update(options)
    return optimize(q, t, edges, solve=chain_solver(o["pcg_tolerance"], o["pcg_max_iterations"]), **o)


# ---- the robust solve: graduated non-convexity with a truncated least-squares loss over the flagged edges ----------
ROBUST_DEFAULTS = dict(inlier_chi2=22.46, mu_step=1.4, max_outer_iterations=100)


def edge_chi2(q, t, edges):
    """s [E] = r^T Omega r of every edge with its own information, at the poses (q, t)."""
    r = residual(q, t, edges)
    return np.einsum("ea,eab,eb->e", r, info_full(edges["info"]), r)


def gnc_thresholds(mu, c2):
    """(lo, hi): a flagged edge with s <= lo has weight 1, with s >= hi weight 0."""
    return mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2


def gnc_weights(s, mu, c2):
    """The GNC-TLS weights of flagged edges with the squared Mahalanobis distances s, at mu: 1 up to lo, 0 from hi, between them
    sqrt(c2 mu (mu + 1) / s) - mu, which is 1 at lo and 0 at hi."""
    s = np.asarray(s, np.float64)
    lo, hi = gnc_thresholds(mu, c2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.sqrt(c2 * mu * (mu + 1.0) / s) - mu
    return np.where(s <= lo, 1.0, np.where(s >= hi, 0.0, mid))


def weighted_edges(edges, weights):
    """The weighted problem: every edge's information scaled by its weight, every flag cleared."""
    e = edges.copy()
    e["info"] = edges["info"] * np.asarray(weights, np.float64)[:, None]
    e["flags"] = 0
    return e


def optimize_robust(q, t, edges, inlier_chi2=22.46, mu_step=1.4, max_outer_iterations=100, solve=None, trace=None, **options):
    """aloam_graph_optimize_robust restated: GNC-TLS (Yang, Antonante, Tzoumas, Carlone, RA-L 2020) over the edges flagged EDGE_ROBUST, an
    outer loop of weighted solves by optimize().  R = the flagged edges, s_e = r^T Omega r with the edge's own information, c2 = inlier_chi2.
    The weighted problem for weights w is the plain problem with Omega_e <- w_e Omega_e for e in R and every flag cleared: no Huber here,
    huber_delta is unused.

      1. s at the entry estimates, s_max = max over R.  A non-finite s or pose: FAILED with termination 5, nothing changes.
      2. R empty or 2 s_max - c2 <= 0: GNC is skipped, one solve with w = 1; outer_iterations = 1, mu = 0, every flagged edge an inlier.
      3. mu = c2 / (2 s_max - c2); for it = 1 .. max_outer_iterations: s at the current estimates; gnc_weights(s, mu, c2) on R; optimize()
         on the weighted problem from the current estimates; stop after the solve of the first iteration in which every weight was exactly
         0 or 1, otherwise mu *= mu_step.
      4. An inner solve that ended as a failure: FAILED, the estimates are the entry's.  One that accepts nothing is no failure.

    `solve` is optimize()'s hook (chain_solver); `options` are optimize()'s.  `trace`, a list, receives one dict per outer iteration: mu,
    lo, hi, s (of the flagged edges, before the solve), weights (of the flagged edges) and the inner solve's result.  Returns q, t and a
    dict with the fields of aloam_graph_robust_result (the fields of its `solve` at the top level) and `weights` [E]: 1 for unflagged edges."""
    q, t = np.array(q, np.float64), np.array(t, np.float64)
    N, E, c2 = len(q), len(edges), float(inlier_chi2)
    res = dict(status=1, termination=0, lm_iterations=0, accepted_steps=0, pcg_iterations=0, nodes=N, edges=E, initial_cost=0.0, final_cost=0.0,
               gradient_max=0.0, outer_iterations=0, robust_edges=0, inliers=0, outliers=0, mu=0.0, s_max=0.0, truncated_cost=0.0, weights=np.ones(E))
    if N < 2 or E == 0:
        return q, t, res
    flagged = (edges["flags"] & EDGE_ROBUST) != 0
    options = {k: v for k, v in options.items() if k != "huber_delta"}
    with np.errstate(over="ignore", invalid="ignore"):
        s = edge_chi2(q, t, edges)
    res.update(status=0, robust_edges=int(flagged.sum()), initial_cost=0.5 * float(s.sum()), final_cost=0.5 * float(s.sum()))
    if not (np.all(np.isfinite(s)) and np.all(np.isfinite(q)) and np.all(np.isfinite(t))):
        res.update(status=2, termination=5)
        return q, t, res
    s_max = float(s[flagged].max()) if flagged.any() else 0.0
    res["s_max"] = s_max
    skip = not flagged.any() or 2.0 * s_max - c2 <= 0.0
    mu = 0.0 if skip else c2 / (2.0 * s_max - c2)
    q0, t0, w, failed = q.copy(), t.copy(), np.ones(E), False
    for it in range(1, 2 if skip else max_outer_iterations + 1):
        lo, hi = (0.0, 0.0) if skip else gnc_thresholds(mu, c2)
        if not skip:
            with np.errstate(over="ignore", invalid="ignore"):
                s = edge_chi2(q, t, edges)
            w = np.where(flagged, gnc_weights(s, mu, c2), 1.0)
        q, t, inner = optimize(q, t, weighted_edges(edges, w), solve=solve, **options)
        for k in ("lm_iterations", "accepted_steps", "pcg_iterations"):
            res[k] += inner[k]
        res.update(termination=inner["termination"], gradient_max=inner["gradient_max"], final_cost=inner["final_cost"], outer_iterations=it, mu=mu)
        if trace is not None:
            trace.append(dict(mu=mu, lo=lo, hi=hi, s=s[flagged].copy(), weights=w[flagged].copy(), solve=inner))
        if inner["status"] == 2:
            failed = True
            break
        if skip or np.all((w == 0.0) | (w == 1.0)):
            break
        mu *= mu_step
    if failed:
        q, t = q0, t0
        res.update(status=2, final_cost=res["initial_cost"])
    s = edge_chi2(q, t, edges)
    res.update(weights=w, inliers=int((w[flagged] == 1.0).sum()), outliers=int((w[flagged] == 0.0).sum()),
               truncated_cost=0.5 * float(s[~flagged].sum() + np.minimum(s[flagged], c2).sum()))
    return q, t, res


# ---- marginals: the covariance of an edge's residual under the graph, and the chi-square gate ----------------------
MARGINAL_MEASURED, MARGINAL_AT_ESTIMATE = 0, 1
MARGINAL_OK, MARGINAL_NO_EDGES, MARGINAL_NOT_CONVERGED, MARGINAL_FAILED = 0, 1, 2, 3
MARGINAL_DEFAULTS = dict(pcg_max_iterations=200, pcg_tolerance=1e-10, huber_delta=1.0)
INFO_PIVOT_TOL = 1e-12               # kInfoPivotTol: a Cholesky pivot counts as positive when it exceeds this times its diagonal entry


def marginal_request(seq, i, j, q=None, t=None, info=None, mode=MARGINAL_MEASURED):
    """Requests of aloam_graph_marginals, a structured array of MARGINAL_REQUEST_DTYPE: the candidate edges (i, j, Z = (q, t), info) in
    the mode given (one for all, or one each).  AT_ESTIMATE ignores Z and info: they default to the identity."""
    i = np.atleast_1d(np.asarray(i, np.int32))
    n = len(i)
    q = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if q is None else q
    t = np.zeros((n, 3)) if t is None else t
    info = np.tile(np.eye(6), (n, 1, 1)) if info is None else info
    r = np.zeros(n, MARGINAL_REQUEST_DTYPE)
    r["edge"] = make_edges(seq, i, j, q, t, info)
    r["mode"] = mode
    return r


def chi2_gate(dof=6, p=0.999):
    """The quantile a chi2 is held against: 22.46 for the 6 degrees of freedom of an edge at p = 0.999."""
    from scipy.stats import chi2
    return float(chi2.ppf(p, dof))


def _cholesky6(A, tol=0.0):
    """Lower factor of a 6 x 6 matrix in the order of the device (row by row, each sum in index order); False when a pivot is not above
    tol times its diagonal entry."""
    L = np.zeros((6, 6))
    for a in range(6):
        for b in range(a + 1):
            s = A[a][b]
            for m in range(b):
                s -= L[a][m] * L[b][m]
            if a == b:
                if not s > tol * A[a][a]:
                    return L, False
                L[a][a] = np.sqrt(s)
            else:
                L[a][b] = s / L[b][b]
    return L, True


def innovation(r, cov, info21):
    """s_edge = r^T Omega r and chi2 = r^T (cov + Omega^-1)^-1 r as the device's one thread computes them: Omega^-1 from the Cholesky factor of
    Omega, S = cov + Omega^-1 factored with the INFO_PIVOT_TOL rule, chi2 = |L_S^-1 r|^2.  With cov = 0, chi2 is s_edge.  Returns
    (s_edge, chi2, ok); ok False (chi2 0) when a factorisation fails."""
    Om = info_full(info21)
    s_edge = 0.0
    for a in range(6):
        o = 0.0
        for b in range(6):
            o += Om[a][b] * r[b]
        s_edge += r[a] * o
    if not np.any(cov):
        return s_edge, s_edge, True
    L, ok = _cholesky6(Om, INFO_PIVOT_TOL)
    if not ok:
        return s_edge, 0.0, False
    X = np.zeros((6, 6))                               # L^-1, column by column, by forward substitution
    for c in range(6):
        for a in range(c, 6):
            s = 1.0 if a == c else 0.0
            for m in range(c, a):
                s -= L[a][m] * X[m][c]
            X[a][c] = s / L[a][a]
    S = np.zeros((6, 6))
    for a in range(6):
        for b in range(a + 1):
            s = 0.0
            for m in range(a, 6):                      # (L^-T L^-1)[a][b], a >= b
                s += X[m][a] * X[m][b]
            S[a][b] = S[b][a] = cov[a][b] + s
    Ls, ok = _cholesky6(S, INFO_PIVOT_TOL)
    if not ok:
        return s_edge, 0.0, False
    chi2, y = 0.0, np.zeros(6)
    for a in range(6):
        s = r[a]
        for m in range(a):
            s -= Ls[a][m] * y[m]
        y[a] = s / Ls[a][a]
        chi2 += y[a] * y[a]
    return s_edge, chi2, True


def marginal_solver(tol=1e-10, max_iterations=200):
    """chain_solver for the six right-hand sides of a marginal: the same chain-preconditioned PCG (pcg's stopping rule), with the banded factor
    and a sparse copy of H kept while the same H comes back (every column of every candidate solves with one H).  Carries its cap so that
    marginals() can tell a column that ran into it."""
    kept = {}

    def solve(H, D, g):
        from scipy.linalg import cholesky_banded, cho_solve_banded
        from scipy.sparse import csr_matrix
        if kept.get("H") is not H or not np.array_equal(kept["D"], D):
            A = H + np.diag(D)
            n = len(g)
            band = np.zeros((12, n))
            for u in range(12):
                d = np.diagonal(A, u).copy()
                k = np.arange(n - u)
                d[(k + u) // 6 - k // 6 > 1] = 0.0      # outside the block-tridiagonal chain (never true inside bandwidth 11)
                band[11 - u, u:] = d
            kept.update(H=H, D=np.array(D), A=csr_matrix(A), cb=cholesky_banded(band))
        cb = kept["cb"]
        return pcg(kept["A"], g, lambda r: cho_solve_banded((cb, False), r), tol, max_iterations)
    solve.max_iterations = max_iterations
    return solve


def marginals(q, t, edges, cand, mode=MARGINAL_MEASURED, huber_delta=1.0, solve=None):
    """aloam_graph_marginals restated.  For every candidate edge of `cand` (EDGE_DTYPE; never robustified) at the estimates (q, t) of a graph
    with `edges`: H = sum rho' J^T Omega J over the graph's edges (normal_equations: node 0 fixed, no damping); r, J_i, J_j of the candidate
    (linearize); Sigma_r = J H^-1 J^T from the six solves H y_c = (J^T)_c, symmetrised; s_edge and chi2 (innovation).  mode (one, or one per
    candidate) AT_ESTIMATE replaces Z by X_i^-1 o X_j of the estimates (X_j for i = -1) and reports s_edge = chi2 = 0.
    Dense by default (np.linalg.solve); `solve(H, D, b)` (chain_solver, marginal_solver) takes the chain-PCG route, a column at a time from
    x = 0, a zero column in 0 iterations.  Returns a dict of arrays over the candidates: status, cov [n, 6, 6], chi2, s_edge, r [n, 6],
    q, t (the Z used), pcg_iterations (the total of the six columns), nodes, edges."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    n, N = len(cand), len(q)
    mode = np.broadcast_to(np.asarray(mode, np.int32), (n,))
    out = dict(status=np.full(n, MARGINAL_OK, np.int32), cov=np.zeros((n, 6, 6)), chi2=np.zeros(n), s_edge=np.zeros(n), r=np.zeros((n, 6)),
               q=np.array(cand["q"], np.float64).reshape(n, 4), t=np.array(cand["t"], np.float64).reshape(n, 3), pcg_iterations=np.zeros(n, np.int32),
               nodes=np.full(n, N, np.int32), edges=np.full(n, len(edges), np.int32))
    if N < 2 or len(edges) == 0:
        out["status"][:] = MARGINAL_NO_EDGES
        return out
    H, _, c = normal_equations(q, t, edges, huber_delta)
    D = np.zeros(len(H))
    for k in range(n):
        e = cand[k:k + 1].copy()
        e["flags"] = 0
        i, j = int(e["i"][0]), int(e["j"][0])
        if mode[k] == MARGINAL_AT_ESTIMATE:
            qi, ti = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)) if i < 0 else (q[i], t[i])
            e["q"][0], e["t"][0] = relative_pose(qi, ti, q[j], t[j])
            out["q"][k], out["t"][k] = e["q"][0], e["t"][0]
            e["info"][0] = info_upper(np.eye(6))                                   # the request's is ignored
        r, _, Ji, Jj, _ = linearize(q, t, e)
        out["r"][k] = r[0]
        if not (np.isfinite(c) and np.all(np.isfinite(H))):
            out["status"][k] = MARGINAL_FAILED
            continue
        J = np.zeros((6, 6 * (N - 1)))
        if i >= 1: J[:, 6 * (i - 1):6 * i] = Ji[0]
        if j >= 1: J[:, 6 * (j - 1):6 * j] = Jj[0]
        if solve is None:
            Y = np.linalg.solve(H, J.T)
        else:
            Y, capped = np.zeros((len(H), 6)), False
            for col in range(6):
                if np.any(J[col]):
                    Y[:, col], its = solve(H, D, J[col].copy())
                    out["pcg_iterations"][k] += its
                    capped |= its >= getattr(solve, "max_iterations", np.inf)
            if capped: out["status"][k] = MARGINAL_NOT_CONVERGED
        M = J @ Y
        out["cov"][k] = 0.5 * (M + M.T)
        if mode[k] == MARGINAL_AT_ESTIMATE:
            continue
        out["s_edge"][k], out["chi2"][k], ok = innovation(r[0], out["cov"][k], e["info"][0])
        if not ok:
            out["status"][k], out["cov"][k], out["chi2"][k] = MARGINAL_FAILED, 0.0, 0.0
    return out


# ---- edges from a localization -------------------------------------------------------------------------------------------------------
def anchor_from_localization(j, q_map, t_map, info, seq=0, robust=False):
    """Node j was localized at (q_map, t_map) in the fixed world (atlas) frame with information `info`: the anchor edge (-1, j)."""
    return make_edges(seq, -1, j, np.asarray(q_map, np.float64)[None], np.asarray(t_map, np.float64)[None], np.asarray(info)[None], robust)


def loop_from_localization(i, q_place, t_place, j, q_reloc, t_reloc, info, seq=0, robust=False):
    """The sweep of node j was relocalized at (q_reloc, t_reloc) in the frame in which the stored place of node i has the pose
    (q_place, t_place): the loop edge (i, j) with Z = X_place^-1 o X_reloc.  `info` is passed through unchanged: a localization's
    information is in the LEFT tangent of the relocalized pose, the graph's residual perturbs Z on the right, so this is exact only up to
    the rotation of Z - harmless for near-isotropic information.  aloam_graph_register_loops (loopreg.edge_information) rotates the matrix,
    info = T^T info_left T with T = blockdiag(R_Z, R_Z): that matters in a corridor whose weak direction is not the sensor's x axis."""
    qz, tz = relative_pose(q_place, t_place, q_reloc, t_reloc)
    return make_edges(seq, i, j, qz[None], tz[None], np.asarray(info)[None], robust)


# ---- loop candidates by pose proximity (aloam_graph_propose_loops) -------------------------------------------------------------------
PROPOSE_MAX_K = 16


def propose_loops(q, t, j, radius_m, growth_m_per_node, min_gap, half_window, separation, K, seq=0, pose=POSE_OPTIMIZED):
    """aloam_graph_propose_loops for one query (seq, j), operation by operation: (q, t) are the poses the call reads (the entered ones
    or the estimates, as `pose` says; `pose` itself only goes into the records).  A node i in [0, j - min_gap] is a hit when
    d2 = (dx dx + dy dy) + dz dz of t_i - t_j is <= r r, r = (j - i) growth_m_per_node + radius_m.  At most K rounds: the live hit with
    the least (d2, i) is taken and every hit within `separation` indices of it dies.  Returns (requests [K] of GRAPH_LOOP_REQUEST_DTYPE
    with first = max(0, i - half_window), count = i + half_window - first + 1 and the guess relative_pose(X_i, X_j); count; dist2 [K]);
    rows behind the count are zero."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    j, K = int(j), int(K)
    req, dist2 = np.zeros(K, LOOP_REQUEST_DTYPE), np.zeros(K, np.float64)
    i = np.arange(max(0, j - int(min_gap) + 1))
    d = t[i] - t[j]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = (j - i).astype(np.float64) * np.float64(growth_m_per_node) + np.float64(radius_m)
    with np.errstate(over="ignore"):
        live = d2 <= r * r
    taken = 0
    while taken < K and live.any():
        cand = i[live]
        best = d2[cand].min()
        w = int(cand[d2[cand] == best][0])
        live &= np.abs(i - w) > int(separation)
        first = max(0, w - int(half_window))
        qd, td = relative_pose(q[w], t[w], q[j], t[j])
        rec = req[taken]
        rec["seq"], rec["i"], rec["j"], rec["first"], rec["count"], rec["pose"] = int(seq), w, j, first, w + int(half_window) - first + 1, int(pose)
        rec["q"], rec["t"] = qd, td
        dist2[taken] = d2[w]
        taken += 1
    return req, taken, dist2


def propose_links(q_i, t_i, q_j, t_j, j, frame, radius_m, half_window, separation, K, seq_i=0, seq_j=1, pose=POSE_OPTIMIZED):
    """aloam_graph_propose_links for one query (seq_j, j, seq_i), operation by operation: (q_i, t_i) are the poses of seq_i's nodes the call
    reads and (q_j, t_j) those of seq_j's (the entered ones or the estimates, as `pose` says; `pose` itself only goes into the records).
    X_j' = X_j when `frame` is None (its bits), else compose(A, X_j) with A = frame = (q_A, t_A) or the seven numbers, q_A stored normalised
    (stored_q).  EVERY node i of seq_i is eligible and is a hit when d2 = (dx dx + dy dy) + dz dz of t_i - t_j' is <= radius_m radius_m.  At
    most K rounds of propose_loops' greedy rule.  Returns (requests [K] of LINK_REQUEST_DTYPE with first = max(0, i - half_window),
    count = min(i + half_window, nodes - 1) - first + 1 and the guess relative_pose(X_i, X_j'); count; dist2 [K]); rows behind the count
    are zero."""
    q_i, t_i = np.asarray(q_i, np.float64).reshape(-1, 4), np.asarray(t_i, np.float64).reshape(-1, 3)
    q_j, t_j = np.asarray(q_j, np.float64), np.asarray(t_j, np.float64)
    j, K, nodes = int(j), int(K), len(t_i)
    req, dist2 = np.zeros(K, LINK_REQUEST_DTYPE), np.zeros(K, np.float64)
    qj, tj = q_j[j], t_j[j]
    if frame is not None:
        f = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in frame]) if isinstance(frame, tuple) else np.asarray(frame, np.float64).reshape(7)
        qj, tj = compose(stored_q(f[:4]), f[4:], qj, tj)
    i = np.arange(nodes)
    d = t_i - tj
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(over="ignore"):
        live = d2 <= np.float64(radius_m) * np.float64(radius_m)
    taken = 0
    while taken < K and live.any():
        cand = i[live]
        best = d2[cand].min()
        w = int(cand[d2[cand] == best][0])
        live &= np.abs(i - w) > int(separation)
        first = max(0, w - int(half_window))
        qd, td = relative_pose(q_i[w], t_i[w], qj, tj)
        rec = req[taken]
        rec["seq_i"], rec["i"], rec["first"], rec["count"] = int(seq_i), w, first, min(w + int(half_window), nodes - 1) - first + 1
        rec["seq_j"], rec["j"], rec["pose"] = int(seq_j), j, int(pose)
        rec["q"], rec["t"] = qd, td
        dist2[taken] = d2[w]
        taken += 1
    return req, taken, dist2


def frame_from_link(q_i, t_i, link, q_j, t_j):
    """The pose A of seq_j's frame in seq_i's frame that a link (node j of seq_j measured in the frame of node i of seq_i) stands for:
    A = (X_i o Z) o X_j^-1 with X_i = (q_i, t_i) the estimate of the link's node i and X_j = (q_j, t_j) that of its node j, q_A divided by its
    norm - align_member's transform for the seq_j side, without its side effects.  Returns (q_A, t_A)."""
    qa, ta = compose(*compose(q_i, t_i, np.array(link["q"], np.float64).reshape(4), np.array(link["t"], np.float64).reshape(3)), *inverse(q_j, t_j))
    return stored_q(qa), ta


def unclosed(requests, edges, gap):
    """The proposals (i, j) of `requests` next to which the graph holds no loop edge yet: a proposal is dropped when some edge (a, b) of
    `edges` (EDGE_DTYPE records of the same sequence, or pairs) has |a - i| <= gap and |b - j| <= gap.  The host added the edges, so it is
    the host that knows them."""
    requests = np.asarray(requests)
    if getattr(getattr(edges, "dtype", None), "names", None):
        ab = np.stack([edges["i"], edges["j"]], 1).astype(np.int64)
    else:
        ab = np.asarray(edges, np.int64).reshape(-1, 2)
    keep = np.ones(len(requests), bool)
    for k, rq in enumerate(requests):
        keep[k] = not np.any((np.abs(ab[:, 0] - int(rq["i"])) <= gap) & (np.abs(ab[:, 1] - int(rq["j"])) <= gap))
    return requests[keep]


# ---- the sliding window ----------------------------------------------------------------------------------------------------------------
TRIM_KEPT, TRIM_ANCHORED, TRIM_KEPT_ON_FIRST, TRIM_REVERSE, TRIM_FIXED = 0, 1, 2, 3, 4


def trim_classes(i, j, first):
    """What aloam_graph_trim does with an edge (i, j) when node `first` > 0 becomes node 0, as TRIM_* codes, the rules in the header's order:
    1 j > f and (i >= f or i == -1): kept;  2 j > f and 0 <= i < f: anchored;  3 i > f and j == f: kept;  4 i > f and 0 <= j < f: removed, a
    reverse edge;  5 everything else touches no node above f: removed, a constant."""
    i, j, f = np.asarray(i, np.int64), np.asarray(j, np.int64), int(first)
    code = np.full(i.shape, TRIM_FIXED, np.int32)
    code[(i > f) & (j >= 0) & (j < f)] = TRIM_REVERSE
    code[(i > f) & (j == f)] = TRIM_KEPT_ON_FIRST
    code[(j > f) & (i >= 0) & (i < f)] = TRIM_ANCHORED
    code[(j > f) & ((i >= f) | (i == -1))] = TRIM_KEPT
    return code


def trim(nodes, edges, first):
    """aloam_graph_trim restated (include/aloam_mi355x.h, "trimming a graph in place"): nodes [0, first) are dropped, old node
    n >= first becomes node n - first as a bit copy, and the edges are compacted in their stored order - kept ones with their indices shifted,
    the ones from a dropped node i to a kept node j turned into anchors with Z' = X_opt[i] o Z (compose, operation by operation; stored as
    computed), info and flags copied.  The dropped nodes and node `first` are conditioned on at their estimates, not marginalised.
    first = 0 changes nothing.  Returns (nodes', edges', stats) with stats = [nodes', edges', anchored, removed_fixed, removed_reverse]."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    f = int(first)
    assert 0 <= f < len(nodes), "0 <= first < nodes"
    if f == 0:
        return nodes.copy(), edges.copy(), np.array([len(nodes), len(edges), 0, 0, 0], np.int64)
    code = trim_classes(edges["i"], edges["j"], f)
    keep = code <= TRIM_KEPT_ON_FIRST
    out = edges[keep].copy()
    anchored = code[keep] == TRIM_ANCHORED
    out["i"] = np.where(anchored | (out["i"] < 0), -1, out["i"] - f)
    out["j"] -= f
    src = edges[code == TRIM_ANCHORED]
    if len(src):
        qz, tz = compose(nodes["q_opt"][src["i"]], nodes["t_opt"][src["i"]], src["q"], src["t"])
        q, t = out["q"], out["t"]
        q[anchored], t[anchored] = qz, tz
        out["q"], out["t"] = q, t
    stats = np.array([len(nodes) - f, len(out), int(anchored.sum()), int((code == TRIM_FIXED).sum()), int((code == TRIM_REVERSE).sum())], np.int64)
    return nodes[f:].copy(), out, stats


# ---- joined graphs: links between sequences and a joint solve ---------------------------------------------------------
def make_links(seq_i, i, seq_j, j, q, t, info, robust=False):
    """A structured array of LINK_DTYPE: node j of seq_j measured in the frame of node i of seq_i; info as make_edges takes it."""
    i = np.atleast_1d(np.asarray(i, np.int32))
    l = np.zeros(len(i), LINK_DTYPE)
    info = np.asarray(info, np.float64)
    if info.shape[-1] == 6:
        info = info_upper(info)
    l["seq_i"], l["i"], l["seq_j"], l["j"], l["q"], l["t"], l["info"] = seq_i, i, seq_j, j, q, t, info
    l["flags"] = np.where(np.broadcast_to(robust, i.shape), EDGE_ROBUST, 0)
    return l


def stored_q(q):
    """A measurement's rotation as the C ABI stores it (aloam_graph_add_edges, the links of a joint call): divided by its norm, the
    squares summed in index order."""
    q = np.asarray(q, np.float64)
    nn = np.zeros(q.shape[:-1])
    for a in range(4):
        nn = nn + q[..., a] * q[..., a]
    return q / np.sqrt(nn)[..., None]


def tree_links(seqs, links):
    """Per member of a group (its sequences `seqs` in member order) the index of its tree link in `links`, -1 for the first member: the
    first link, in list order, that joins the member to a member earlier in the list."""
    at = {int(s): m for m, s in enumerate(seqs)}
    tree = np.full(len(seqs), -1, np.int64)
    for k, l in enumerate(links):
        later = max(at[int(l["seq_i"])], at[int(l["seq_j"])])
        if tree[later] < 0:
            tree[later] = k
    assert (tree[1:] >= 0).all(), "every member after the first needs a link to an earlier member"
    return tree


def align_member(nodes, edges, q_g, t_g, link, own, seq_i_side):
    """A member that is still in its own frame, moved into its group's: (q_g, t_g) is the estimate Xg of the tree link's node in the earlier
    member as placed in the joined row, `link` the tree link, `own` the member's node of it, `seq_i_side` true when the member is the link's
    seq_i side.  A = (Xg o Z) o X[own]^-1, with Z inverted first for the seq_i side; compose and inverse operation by operation, then q_A divided
    by its norm (stored_q); nothing else is renormalised.  Every (q_opt, t_opt) becomes A o X_opt and every anchor A o Z; q, t, frame, relative edges, info and flags are untouched.
    Returns (nodes', edges', (q_A, t_A))."""
    nodes, edges = np.array(nodes, NODE_DTYPE), np.array(edges, EDGE_DTYPE)
    qz, tz = np.array(link["q"], np.float64), np.array(link["t"], np.float64)
    if seq_i_side:
        qz, tz = inverse(qz, tz)
    qa, ta = compose(*compose(q_g, t_g, qz, tz), *inverse(nodes["q_opt"][own], nodes["t_opt"][own]))
    qa = stored_q(qa)                                  # a rigid transform whatever the norms of the chained estimates it is built from
    nodes["q_opt"], nodes["t_opt"] = compose(qa, ta, nodes["q_opt"], nodes["t_opt"])
    anchor = edges["i"] < 0
    if anchor.any():
        q, t = edges["q"], edges["t"]
        q[anchor], t[anchor] = compose(qa, ta, q[anchor], t[anchor])
        edges["q"], edges["t"] = q, t
    return nodes, edges, (qa, ta)


def join(members, links, seqs=None, align=None):
    """The joined graph of one group (include/aloam_mi355x.h, "joined graphs").  members: [(nodes, edges), ...] in member order; links:
    LINK_DTYPE records whose seq_i / seq_j name members by `seqs` (the members' sequence indices; their positions by default); align: per
    member, non-zero for one that is still in its own frame (never the first).
      nodes: the members' rows end to end, bit copies; off[m] = the nodes of the members before m.
      edges: every member's edges in member order and stored order, i >= 0 and j shifted by off[m], anchors keep i = -1, seq and the rest
             bit copies; then the links in list order as (off[seq_i] + i, off[seq_j] + j, Z, info, flags) with seq = seq_i, q of Z as
             stored_q makes it (the call checks a link like aloam_graph_add_edges checks an edge and stores q normalised).
    An aligned member goes through align_member with Xg read from the rows joined so far, so chains of new members work.
    Returns (nodes, edges, off) with off of length members + 1."""
    seqs = list(range(len(members))) if seqs is None else [int(s) for s in seqs]
    at = {s: m for m, s in enumerate(seqs)}
    links = np.array(links, LINK_DTYPE)
    links["q"] = stored_q(links["q"]) if len(links) else links["q"]
    align = np.zeros(len(members), np.int32) if align is None else np.asarray(align, np.int32)
    assert len(at) == len(members) and not align[0], "distinct members; the first member defines the frame"
    off = np.concatenate([[0], np.cumsum([len(n) for n, _ in members])]).astype(np.int64)
    tree = tree_links(seqs, links) if len(members) > 1 else np.full(1, -1, np.int64)
    out_n, out_e = np.zeros(off[-1], NODE_DTYPE), []
    for m, (nodes, edges) in enumerate(members):
        nodes, edges = np.ascontiguousarray(nodes, NODE_DTYPE), np.ascontiguousarray(edges, EDGE_DTYPE).copy()
        if align[m]:
            l = links[tree[m]]
            inv = at[int(l["seq_i"])] == m
            other = off[at[int(l["seq_j"])]] + int(l["j"]) if inv else off[at[int(l["seq_i"])]] + int(l["i"])
            nodes, edges, _ = align_member(nodes, edges, out_n["q_opt"][other], out_n["t_opt"][other], l, int(l["i"]) if inv else int(l["j"]), inv)
        out_n[off[m]:off[m + 1]] = nodes
        edges["i"] = np.where(edges["i"] >= 0, edges["i"] + off[m], edges["i"])
        edges["j"] += off[m]
        out_e.append(edges)
    tail = np.zeros(len(links), EDGE_DTYPE)
    for k, l in enumerate(links):
        tail[k] = (l["seq_i"], off[at[int(l["seq_i"])]] + l["i"], off[at[int(l["seq_j"])]] + l["j"], l["flags"], l["q"], l["t"], l["info"])
    return out_n, np.concatenate(out_e + [tail]), off


def split(members, nodes, edges, off, align=None):
    """The write-back of a joint solve: every member's q_opt / t_opt are the joined row's; an aligned member's anchors take the joined
    row's Z'.  Everything else of a member is what it was.  Returns [(nodes, edges), ...]."""
    align = np.zeros(len(members), np.int32) if align is None else np.asarray(align, np.int32)
    out, e0 = [], 0
    for m, (n, e) in enumerate(members):
        n, e = np.array(n, NODE_DTYPE), np.array(e, EDGE_DTYPE)
        n["q_opt"], n["t_opt"] = nodes["q_opt"][off[m]:off[m + 1]], nodes["t_opt"][off[m]:off[m + 1]]
        if align[m]:
            je = edges[e0:e0 + len(e)]
            anchor = e["i"] < 0
            q, t = e["q"], e["t"]
            q[anchor], t[anchor] = je["q"][anchor], je["t"][anchor]
            e["q"], e["t"] = q, t
        e0 += len(e)
        out.append((n, e))
    return out


def optimize_joint(members, links, seqs=None, align=None, robust=None, solve=None, **options):
    """aloam_graph_optimize_joint (robust = None) / aloam_graph_optimize_joint_robust (robust = a dict of optimize_robust's options)
    restated for one group: join, optimize or optimize_robust on the joined graph (its node 0 fixed), split.  With a joined graph of fewer
    than two nodes or no edge nothing is written back.  Returns ([(nodes, edges), ...], the result dict, (joined nodes, joined edges))."""
    nodes, edges, off = join(members, links, seqs, align)
    if robust is None:
        q, t, res = optimize(nodes["q_opt"], nodes["t_opt"], edges, solve=solve, **options)
    else:
        q, t, res = optimize_robust(nodes["q_opt"], nodes["t_opt"], edges, solve=solve, **dict(options, **robust))
    if res["status"] == 1:
        return [(np.array(n, NODE_DTYPE), np.array(e, EDGE_DTYPE)) for n, e in members], res, (nodes, edges)
    nodes["q_opt"], nodes["t_opt"] = q, t
    return split(members, nodes, edges, off, align), res, (nodes, edges)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def drifted_laps(seed, nodes, loops, radius=10.0, per_lap=None, sigma_theta=5e-3, sigma_t=5e-2, yaw_bias=1.5e-3, noise=1.0):
    """Ground-truth laps of a circle (with a slow climb), odometry edges with seeded noise and a yaw bias, `loops` loop edges between
    laps; noise = 0 makes every edge exact.  Returns dict(q_true, t_true, q, t (the drifted chain: node 0 true, then X[k] = X[k - 1] o Z_k), odom (edges (k - 1, k)),
    loop (edges), info (the 6 x 6 information every edge carries))."""
    rng = np.random.default_rng(seed)
    per_lap = per_lap or max(8, nodes // 3)
    k = np.arange(nodes)
    ang = 2.0 * np.pi * k / per_lap
    t_true = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.002 * k], 1)
    yaw = ang + 0.5 * np.pi
    q_true = np.stack([0.02 * np.sin(ang), 0.02 * np.cos(ang), np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    q_true /= np.linalg.norm(q_true, axis=1, keepdims=True)
    info = np.diag([1.0 / sigma_theta ** 2] * 3 + [1.0 / sigma_t ** 2] * 3)

    def noisy(qz, tz, n):
        dth = noise * sigma_theta * rng.standard_normal((n, 3))
        return qmul(qz, qexp(dth)), tz + noise * sigma_t * rng.standard_normal((n, 3))

    qz, tz = relative_pose(q_true[:-1], t_true[:-1], q_true[1:], t_true[1:])
    qz, tz = noisy(qz, tz, nodes - 1)
    qz = qmul(qz, qexp(np.tile([0.0, 0.0, noise * yaw_bias], (nodes - 1, 1))))
    odom = make_edges(0, k[:-1], k[1:], qz, tz, info)
    q, t = [q_true[0]], [t_true[0]]
    for e in range(nodes - 1):
        a, b = compose(q[-1], t[-1], qz[e], tz[e])
        q.append(a); t.append(b)
    q, t = np.array(q), np.array(t)
    # loop edges: node j against the node one or more laps earlier at the same place
    js = np.linspace(per_lap + 1, nodes - 1, loops).astype(int) if loops else np.zeros(0, int)
    is_ = js - per_lap * (js // per_lap)
    is_ = np.where(is_ == js, js - per_lap, is_)
    ql, tl = relative_pose(q_true[is_], t_true[is_], q_true[js], t_true[js])
    if loops:
        ql, tl = noisy(ql, tl, loops)
    loop = make_edges(0, is_, js, ql.reshape(-1, 4), tl.reshape(-1, 3), info)
    return dict(q_true=q_true, t_true=t_true, q=q, t=t, odom=odom, loop=loop, info=info)


def false_loops(g, n, seed):
    """n wrong loop edges for the graph g of drifted_laps, flagged robust: between nodes a quarter to a half of the graph apart, the true
    relative pose displaced by up to 8 m per axis and rotated by up to 0.5 rad per axis, with g's information."""
    rng = np.random.default_rng(seed)
    N = len(g["q"])
    fi = rng.integers(0, N // 2, n)
    fj = fi + rng.integers(N // 4, N // 2, n)
    qz, tz = relative_pose(g["q_true"][fi], g["t_true"][fi], g["q_true"][fj], g["t_true"][fj])
    tz = tz + rng.uniform(-8, 8, (n, 3))
    qz = qmul(qz, qexp(rng.uniform(-0.5, 0.5, (n, 3))))
    return make_edges(0, fi, fj, qz, tz, g["info"], robust=True)


def graph_nodes(q, t, q_opt=None, t_opt=None, frame=-1):
    """NODE_DTYPE records with the entered poses (q, t) and the estimates (the entered poses by default)."""
    n = np.zeros(len(q), NODE_DTYPE)
    n["q"], n["t"], n["q_opt"], n["t_opt"], n["frame"] = q, t, q if q_opt is None else q_opt, t if t_opt is None else t_opt, frame
    return n


def cut_drive(g, c, frame, seqs=(0, 1)):
    """The graph g of drifted_laps cut at node c into two sessions: nodes [0, c) with the edges among them, and nodes [c, N) renumbered
    from 0 and expressed in another rigid frame, X' = F o X with F = frame = (q_F, t_F).  The edges that cross the cut become links, the
    cut odometry edge (c - 1, c) first, then the others in their order.  Returns dict(members = [(nodes, edges)] * 2, links,
    whole = (nodes, edges) of the uncut graph, seqs)."""
    edges = np.concatenate([g["odom"], g["loop"]])
    i, j = edges["i"], edges["j"]
    first, second = edges[(i < c) & (j < c)].copy(), edges[(i >= c) & (j >= c)].copy()
    second["i"] -= c; second["j"] -= c
    first["seq"], second["seq"] = seqs
    cross = np.flatnonzero((i < c) != (j < c))
    cut = [k for k in cross if (i[k], j[k]) == (c - 1, c)]
    x = edges[np.array(cut + [k for k in cross if k not in cut], np.int64)]
    low = x["i"] < c
    links = make_links(np.where(low, seqs[0], seqs[1]), np.where(low, x["i"], x["i"] - c), np.where(x["j"] < c, seqs[0], seqs[1]),
                       np.where(x["j"] < c, x["j"], x["j"] - c), x["q"], x["t"], x["info"], x["flags"] != 0)
    qf, tf = np.asarray(frame[0], np.float64), np.asarray(frame[1], np.float64)
    q2, t2 = compose(qf, tf, g["q"][c:], g["t"][c:])
    return dict(members=[(graph_nodes(g["q"][:c], g["t"][:c]), first), (graph_nodes(q2, t2), second)], links=links,
                whole=(graph_nodes(g["q"], g["t"]), edges), seqs=tuple(seqs))


def apply_correction(q, t, q_opt, t_opt, live):
    """aloam_graph_apply restated: the correction D of a solved graph, the live poses moved by it and the rebase of the nodes.

    q, t, q_opt, t_opt: the K >= 1 nodes as exported before the call; live: [(q, t), ...] poses of the live state (q_wmap_wodom / t_wmap_wodom,
    q_w_curr / t_w_curr).  D comes from the last node: q_D = normalise(q_opt conj(q)), t_D = t_opt - q_D t, every operation a separately
    rounded f64 operation in the order of the device.  Returns ((q_D, t_D), [D o X for X in live], (q, t) after the rebase = bit copies of
    (q_opt, t_opt))."""
    q, t, q_opt, t_opt = (np.asarray(v, np.float64) for v in (q, t, q_opt, t_opt))
    qd = qmul(q_opt[-1], qconj(q[-1]))
    qd = qd / np.sqrt(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3])
    td = t_opt[-1] - qrot(qd, t[-1])
    moved = [(qmul(qd, np.asarray(ql, np.float64)), qrot(qd, np.asarray(tl, np.float64)) + td) for ql, tl in live]
    return (qd, td), moved, (q_opt.copy(), t_opt.copy())


def ate(t, t_true):
    """Absolute trajectory error: the RMS distance of the positions (both trajectories share node 0; no alignment)."""
    return float(np.sqrt(np.mean(np.sum((np.asarray(t) - np.asarray(t_true)) ** 2, 1))))


def pose_difference(qa, ta, qb, tb):
    """The largest of |t_a - t_b| and 2 |q_a -+ q_b| over all nodes and components (radians and metres)."""
    qa, qb = np.asarray(qa), np.asarray(qb)
    sgn = np.where(np.sum(qa * qb, 1, keepdims=True) < 0, -1.0, 1.0)
    return float(max(np.abs(np.asarray(ta) - np.asarray(tb)).max(), 2.0 * np.abs(qa - sgn * qb).max()))
