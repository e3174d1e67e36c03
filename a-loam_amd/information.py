"""Pose information: the numpy model (f64) of aloam_export_pose_information, and what a caller does with a record.

The definition is the one include/aloam_mi355x.h gives operation by operation; this file restates it so that the kernels can be checked
against something that shares no code with them.

  information_from_factors(lines, planes, q, t, s=None)   J^T J, J^T r and the cost of a factor set at a pose, in radians and metres
  decompose(info)                                          eigenpairs with the sign rule, both marginals, the status
  covariance(rec)                                          sigma^2 V diag(1 / lambda) V^T
  degeneracy(rec)                                          (lambda0 / lambda1 of the translation marginal, its weakest direction)

Factor layouts are those of the getters: odometry lines [n, 9] (cp, a, b) and planes [n, 12] (cp, j, l, m) from aloam_get_correspondences,
mapping lines [n, 9] (cp, a, b) and planes [n, 7] (cp, n, d) from aloam_get_map_factors.  q is (x, y, z, w).

The tangent is the solver's: a left perturbation q' = exp(theta / 2) q by the rotation vector theta, expressed in the target frame (the
last sweep's frame for the odometry, the map frame for the mapping), and t' = t + dt.  Ceres' EigenQuaternionParameterization::Plus moves
by delta = theta / 2, so the solver's J^T J is S^-1 info S^-1 with S = diag(1/2, 1/2, 1/2, 1, 1, 1).
"""
from __future__ import annotations

import numpy as np

INFO_ODOMETRY, INFO_MAPPING = 0, 1
INFO_OK, INFO_NONE, INFO_NO_FACTORS, INFO_SINGULAR = 0, 1, 2, 3
HUBER_A = 0.1
PIVOT_TOL = 1e-12          # a Cholesky pivot counts as positive when it exceeds PIVOT_TOL times its diagonal entry (as on the device)

def _rotate(q, v):
    """q v q^-1 for a unit quaternion (x, y, z, w) and points [n, 3]."""
    u = q[:3]
    uv = 2.0 * np.cross(u, v)
    return v + q[3] * uv + np.cross(u, uv)


def _slerp_scales(w, s):
    """Identity.slerp(s, q) = c0 * Identity + c1 * q as Eigen evaluates it (a coefficient blend, not re-normalised), and d c0 / d w, d c1 / d w."""
    one = 1.0 - np.finfo(np.float64).eps
    ad = abs(w)
    if ad >= one:
        c0, c1, d0, d1 = 1.0 - s, s.copy(), np.zeros_like(s), np.zeros_like(s)
    else:
        th = np.arccos(ad)
        st, ct = np.sin(th), np.cos(th)
        s0, s1 = np.sin((1.0 - s) * th), np.sin(s * th)
        c0, c1 = s0 / st, s1 / st
        g = (1.0 if w < 0.0 else -1.0) / st                                   # d theta / d w
        d0 = ((1.0 - s) * np.cos((1.0 - s) * th) * st - s0 * ct) / (st * st) * g
        d1 = (s * np.cos(s * th) * st - s1 * ct) / (st * st) * g
    if w < 0.0:
        c1, d1 = -c1, -d1
    return c0, c1, d0, d1


def _points(cp, q, t, s):
    """lp [n, 3] and d lp / d (theta, t) [n, 3, 6] of the points cp [n, 3]: lp = q cp + t, or with ratios s [n] lp = slerp(identity, q, s) cp + s t."""
    n = len(cp)
    D = np.zeros((n, 3, 6))
    if s is None:
        rcp = _rotate(q, cp)
        lp = rcp + t
        # lp(theta) = exp(theta) (q cp) + t: d lp / d theta = -[q cp]x
        D[:, 0, 1], D[:, 0, 2] = rcp[:, 2], -rcp[:, 1]
        D[:, 1, 0], D[:, 1, 2] = -rcp[:, 2], rcp[:, 0]
        D[:, 2, 0], D[:, 2, 1] = rcp[:, 1], -rcp[:, 0]
        D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
        return lp, D
    s = np.asarray(s, np.float64)
    c0, c1, d0, d1 = _slerp_scales(q[3], s)
    u = c1[:, None] * q[None, :3]                                             # vector part of the blend, [n, 3]
    w = c0 + c1 * q[3]
    uv = 2.0 * np.cross(u, cp)
    lp = cp + w[:, None] * uv + np.cross(u, uv) + s[:, None] * t
    # d lp / d u_k = 2 w (e_k x cp) + e_k x uv + u x (2 e_k x cp);  d lp / d w = uv
    Du = np.zeros((n, 3, 3))
    for k in range(3):
        e = np.zeros(3); e[k] = 1.0
        ev = 2.0 * np.cross(e, cp)
        Du[:, :, k] = w[:, None] * ev + np.cross(e, uv) + np.cross(u, ev)
    M = np.zeros((n, 3, 4))                                                   # d lp / d (qx, qy, qz, qw)
    M[:, :, :3] = c1[:, None, None] * Du
    M[:, :, 3] = d1[:, None] * (Du @ q[:3]) + uv * (d0 + d1 * q[3] + c1)[:, None]
    # q(delta) = (sin|delta| delta / |delta|, cos|delta|) * q: d q / d delta at 0, rows x, y, z, w; theta = 2 delta
    P = np.array([[q[3], q[2], -q[1]], [-q[2], q[3], q[0]], [q[1], -q[0], q[3]], [-q[0], -q[1], -q[2]]])
    D[:, :, :3] = 0.5 * (M @ P)
    D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = s
    return lp, D


def factor_rows(lines, planes, q, t, s=None):
    """Unweighted residuals and Jacobian rows of a factor set at (q, t): (r_line [nl, 3], J_line [nl, 3, 6], r_plane [np], J_plane [np, 6]),
    columns (theta_x, theta_y, theta_z, t_x, t_y, t_z) in radians and metres.  s: None, or (s_line [nl], s_plane [np]) interpolation ratios."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    L = np.asarray(lines, np.float64).reshape(-1, 9)
    P = np.asarray(planes, np.float64)
    P = P.reshape(-1, P.shape[-1] if P.ndim == 2 and P.shape[-1] in (7, 12) else 12)
    sl, sp = (None, None) if s is None else s
    lp, D = _points(L[:, :3], q, t, sl)
    a, b = L[:, 3:6], L[:, 6:9]
    inv = 1.0 / np.linalg.norm(a - b, axis=1)
    r_line = np.cross(lp - a, lp - b) * inv[:, None]
    wv = (b - a) * inv[:, None]                                               # d r / d lp = [wv]x
    A = np.zeros((len(L), 3, 3))
    A[:, 0, 1], A[:, 0, 2] = -wv[:, 2], wv[:, 1]
    A[:, 1, 0], A[:, 1, 2] = wv[:, 2], -wv[:, 0]
    A[:, 2, 0], A[:, 2, 1] = -wv[:, 1], wv[:, 0]
    J_line = A @ D
    lp, D = _points(P[:, :3], q, t, sp)
    if P.shape[1] == 12:                                                      # LidarPlaneFactor: n = normalize((j - l) x (j - m)), r = n . (lp - j)
        j = P[:, 3:6]
        n = np.cross(j - P[:, 6:9], j - P[:, 9:12])
        n = n / np.linalg.norm(n, axis=1)[:, None]
        r_plane = np.einsum("ij,ij->i", lp - j, n)
    else:                                                                     # LidarPlaneNormFactor: r = n . lp + d
        n = P[:, 3:6]
        # every product and sum rounded on its own, in the order of map_evaluate (mapping_solve_device.hpp): at a converged pose r is a difference of terms ten orders above it,
        # and another summation order (einsum's is not defined) moves a cost of 1e-23 by 1e-4 of itself
        r_plane = ((n[:, 0] * lp[:, 0] + n[:, 1] * lp[:, 1]) + n[:, 2] * lp[:, 2]) + P[:, 6]
    J_plane = np.einsum("ij,ijk->ik", n, D)
    return r_line, J_line, r_plane, J_plane


def huber(s2):
    """HuberLoss(0.1): (rho, rho') of the squared norms s2."""
    s2 = np.asarray(s2, np.float64)
    out = s2 > HUBER_A * HUBER_A
    r = np.sqrt(np.where(out, s2, 1.0))
    return np.where(out, 2.0 * HUBER_A * r - HUBER_A * HUBER_A, s2), np.where(out, HUBER_A / r, 1.0)


def information_from_factors(lines, planes, q, t, s=None):
    """The definition: info [6, 6] = sum rho' J^T J, gradient [6] = sum rho' J^T r, cost = 1/2 sum rho over the residual blocks, with the
    counts.  A dict with the names of aloam_pose_information."""
    r_l, J_l, r_p, J_p = factor_rows(lines, planes, q, t, s)
    rho_l, w_l = huber(np.einsum("ij,ij->i", r_l, r_l))
    rho_p, w_p = huber(r_p * r_p)
    info = np.einsum("n,nri,nrj->ij", w_l, J_l, J_l) + np.einsum("n,ni,nj->ij", w_p, J_p, J_p)
    grad = np.einsum("n,nri,nr->i", w_l, J_l, r_l) + np.einsum("n,ni,n->i", w_p, J_p, r_p)
    return {"info": 0.5 * (info + info.T), "gradient": grad, "cost": 0.5 * (float(np.sum(rho_l)) + float(np.sum(rho_p))),
            "n_line": len(r_l), "n_plane": len(r_p), "rows": 3 * len(r_l) + len(r_p)}


def _signed(vec):
    """The sign rule: the component of largest magnitude of every column is positive, the lowest index deciding a tie."""
    vec = vec.copy()
    for k in range(vec.shape[1]):
        if vec[int(np.argmax(np.abs(vec[:, k]))), k] < 0.0:
            vec[:, k] = -vec[:, k]
    return vec


def _eigen(m):
    val, vec = np.linalg.eigh(m)
    return val, _signed(vec)


def _schur(a, c, d):
    """d - c^T a^-1 c through the Cholesky factor of a; None when a pivot does not exceed PIVOT_TOL times its diagonal entry.  Operation by
    operation as schur3 of information_device.hpp does it (a = L L^T with the products subtracted one by one, Y = L^-1 c by forward substitution, M_ij = d_ij -
    ((Y_0i Y_0j + Y_1i Y_1j) + Y_2i Y_2j) on the upper triangle, mirrored): where the complement cancels completely - a matrix of rank <= 3
    whose block `a` is still positive definite - what is left is the rounding of these very operations, and only the same operations give it."""
    L = np.zeros((3, 3))
    for i in range(3):
        for j in range(i + 1):
            v = float(a[i, j])
            for k in range(j):
                v -= L[i, k] * L[j, k]
            if i == j:
                if not v > PIVOT_TOL * a[i, i]:
                    return None
                L[i, i] = np.sqrt(v)
            else:
                L[i, j] = v / L[j, j]
    y = np.zeros((3, 3))
    for col in range(3):
        for i in range(3):
            v = float(c[i, col])
            for k in range(i):
                v -= L[i, k] * y[k, col]
            y[i, col] = v / L[i, i]
    m = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            m[i, j] = m[j, i] = d[i, j] - ((y[0, i] * y[0, j] + y[1, i] * y[1, j]) + y[2, i] * y[2, j])
    return m


def decompose(info):
    """Eigenpairs of a 6 x 6 information matrix (ascending, column k of eigenvectors belongs to eigenvalues[k], sign rule), the translation
    and rotation marginals (Schur complements) with theirs, and the status: INFO_OK, or INFO_SINGULAR when a block that a marginal needs is
    not positive definite (that marginal is zero)."""
    H = np.asarray(info, np.float64).reshape(6, 6)
    out = {"info": H}
    out["eigenvalues"], out["eigenvectors"] = _eigen(H)
    ok = True
    for name, m in (("trans", _schur(H[:3, :3], H[:3, 3:], H[3:, 3:])), ("rot", _schur(H[3:, 3:], H[3:, :3], H[:3, :3]))):
        if m is None:
            ok = False
            out[name + "_info"], out[name + "_eigenvalues"], out[name + "_eigenvectors"] = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
        else:
            out[name + "_info"] = m
            out[name + "_eigenvalues"], out[name + "_eigenvectors"] = _eigen(m)
    out["status"] = INFO_OK if ok else INFO_SINGULAR
    return out


def covariance(rec):
    """6 x 6 covariance of a record (a row of POSE_INFORMATION_DTYPE or a dict with its names), order (theta, t), radians and metres:
    sigma^2 V diag(1 / lambda) V^T with sigma^2 = 2 cost / (rows - 6), the residual variance of the solve.  Directions whose eigenvalue is
    not positive are unconstrained: their variance is infinite.  None for a record without a valid matrix or with rows <= 6."""
    if int(rec["status"]) in (INFO_NONE, INFO_NO_FACTORS) or int(rec["rows"]) <= 6:
        return None
    lam, V = np.asarray(rec["eigenvalues"], np.float64), np.asarray(rec["eigenvectors"], np.float64).reshape(6, 6)
    sigma2 = 2.0 * float(rec["cost"]) / (int(rec["rows"]) - 6)
    with np.errstate(divide="ignore"):
        inv = np.where(lam > 0.0, 1.0 / np.where(lam > 0.0, lam, 1.0), np.inf)
    return sigma2 * (V * inv) @ V.T


ROS_ORDER = (3, 4, 5, 0, 1, 2)      # nav_msgs/Odometry pose.covariance is (x, y, z, rot_x, rot_y, rot_z): cov[np.ix_(ROS_ORDER, ROS_ORDER)]


def degeneracy(rec):
    """(lambda0 / lambda1 of the translation marginal, its weakest direction [3]) - a ratio near 0 says the pose slides along that direction.
    (nan, zeros) for a record without a translation marginal."""
    lam = np.asarray(rec["trans_eigenvalues"], np.float64)
    V = np.asarray(rec["trans_eigenvectors"], np.float64).reshape(3, 3)
    if int(rec["status"]) in (INFO_NONE, INFO_NO_FACTORS) or not lam[1] > 0.0:
        return float("nan"), np.zeros(3)
    return float(lam[0] / lam[1]), V[:, 0].copy()
