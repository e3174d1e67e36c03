"""A numpy model of aloam_score_map_corrections, built from the oracle's exposed primitives (oracle_py.knn_search, sym_eigen3, lstsq_5x3)
with the transform restated in the device's operation order (k_map_begin / associate_to_map: separately rounded f64 operations, the sum
stored to f32).  test_relocalize_model.py checks it against Oracle.mapping_step; the GPU tests check the kernel against it."""
import math

import numpy as np

import oracle_py


def quat_mul(a, b):
    """Hamilton product, (x, y, z, w), evaluated left to right as the device's quat_mul."""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_rotate(q, vx, vy, vz):
    """lm_device.hpp quat_rotate: v + 2 w (q x v) + q x (2 q x v); vx, vy, vz scalars or arrays of f64."""
    ux = q[1] * vz - q[2] * vy; uy = q[2] * vx - q[0] * vz; uz = q[0] * vy - q[1] * vx
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return (vx + q[3] * ux + (q[1] * uz - q[2] * uy), vy + q[3] * uy + (q[2] * ux - q[0] * uz), vz + q[3] * uz + (q[0] * uy - q[1] * ux))


def start_pose(q_wodom, t_wodom, q_corr, t_corr):
    """transformAssociateToMap (src/laserMapping.cpp:142-146) as k_map_begin computes it: par[0:4] = q, par[4:7] = t."""
    q_wodom, t_wodom, q_corr, t_corr = (np.asarray(v, np.float64) for v in (q_wodom, t_wodom, q_corr, t_corr))
    q = quat_mul(q_corr, q_wodom)
    r = quat_rotate(q_corr, t_wodom[0], t_wodom[1], t_wodom[2])
    return np.concatenate([q, [r[0] + t_corr[0], r[1] + t_corr[1], r[2] + t_corr[2]]])


def associate_to_map(pts, par):
    """pointAssociateToMap (:157-166) of float32 points [n, 4]: f64 rotation + translation, stored back to f32."""
    p = np.asarray(pts, np.float32)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    ox, oy, oz = quat_rotate(par[:4], x, y, z)
    out = p.copy()
    out[:, 0], out[:, 1], out[:, 2] = (ox + par[4]).astype(np.float32), (oy + par[5]).astype(np.float32), (oz + par[6]).astype(np.float32)
    return out


def huber_half(s):
    """0.5 * HuberLoss(0.1).rho(s)."""
    return 0.5 * (2.0 * 0.1 * math.sqrt(s) - 0.1 * 0.1 if s > 0.1 * 0.1 else s)


def window_cubes(center):
    """Cube indices of the 5 x 5 x 3 window around the centre cube, in the i, j, k order of src/laserMapping.cpp:512-529."""
    cI, cJ, cK = center
    return [i + 21 * j + 441 * k for i in range(cI - 2, cI + 3) for j in range(cJ - 2, cJ + 3) for k in range(cK - 1, cK + 2)
            if 0 <= i < 21 and 0 <= j < 21 and 0 <= k < 11]


def submap(cubes, center):
    """laserCloudCornerFromMap / SurfFromMap: the window's cubes concatenated in window order ({cube index: (n, 4) points})."""
    parts = [cubes[c] for c in window_cubes(center) if c in cubes and len(cubes[c])]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 4), np.float32)


def center_cube(par, cen):
    """Centre cube of a start pose (:311-321)."""
    out = []
    for v, c in zip(par[4:7], cen):
        k = int((v + 25.0) / 50.0) + c
        out.append(k - 1 if v + 25.0 < 0 else k)
    return tuple(out)


def score_one(stack_corner, stack_surf, submap_corner, submap_surf, par):
    """(corner_factors, surf_factors, corner_found, surf_found, cost) of one start pose."""
    cf = sf = cfound = sfound = 0
    terms = []
    if not (len(submap_corner) > 10 and len(submap_surf) > 50):               # :554
        return 0, 0, 0, 0, 0.0
    q, t = par[:4], par[4:7]
    if len(stack_corner):
        sel = associate_to_map(stack_corner, par)
        idx, d2 = oracle_py.knn_search(submap_corner, sel, 5)
        for i in np.nonzero((idx[:, 4] >= 0) & (d2[:, 4] < np.float32(1.0)))[0]:
            cfound += 1
            near = submap_corner[idx[i], :3].astype(np.float64)
            c = np.zeros(3)
            for j in range(5):
                c = c + near[j]
            c = c / 5.0
            cov = np.zeros((3, 3))
            for j in range(5):
                z = near[j] - c
                cov = cov + np.outer(z, z)
            vals, vecs = oracle_py.sym_eigen3(cov)
            if vals[2] > 3 * vals[1]:
                cf += 1
                d = vecs[:, 2]
                a, b = 0.1 * d + c, -0.1 * d + c
                o = stack_corner[i].astype(np.float64)
                lp = np.array(quat_rotate(q, o[0], o[1], o[2])) + t
                de = a - b
                inv = 1.0 / math.sqrt(de[0] * de[0] + de[1] * de[1] + de[2] * de[2])
                r = np.cross(lp - a, lp - b) * inv
                terms.append(huber_half(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
    if len(stack_surf):
        sel = associate_to_map(stack_surf, par)
        idx, d2 = oracle_py.knn_search(submap_surf, sel, 5)
        for i in np.nonzero((idx[:, 4] >= 0) & (d2[:, 4] < np.float32(1.0)))[0]:
            sfound += 1
            near = submap_surf[idx[i], :3].astype(np.float64)
            x = oracle_py.lstsq_5x3(near, -np.ones(5))
            ln = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
            d = 1 / ln
            n = x / ln
            if all(abs(n[0] * p[0] + n[1] * p[1] + n[2] * p[2] + d) <= 0.2 for p in near):
                sf += 1
                o = stack_surf[i].astype(np.float64)
                rc = quat_rotate(q, o[0], o[1], o[2])
                r = (n[0] * (rc[0] + t[0]) + n[1] * (rc[1] + t[1]) + n[2] * (rc[2] + t[2])) + d
                terms.append(huber_half(r * r))
    return cf, sf, cfound, sfound, math.fsum(terms)


def score_model(stack_corner, stack_surf, submap_corner, submap_surf, q_wodom, t_wodom, cand):
    """cand: iterable of (q_wmap_wodom, t_wmap_wodom).  Returns a list of dicts with the fields of aloam_map_score."""
    sc, ss = np.asarray(stack_corner, np.float32), np.asarray(stack_surf, np.float32)
    mc, msf = np.ascontiguousarray(submap_corner, np.float32), np.ascontiguousarray(submap_surf, np.float32)
    out = []
    for q, t in cand:
        v = score_one(sc, ss, mc, msf, start_pose(q_wodom, t_wodom, q, t))
        out.append(dict(zip(("corner_factors", "surf_factors", "corner_found", "surf_found", "cost"), v)))
    return out


def best_of(scores):
    """The ranking rule of aloam_score_map_corrections: most factors, then the lower cost, then the lower index."""
    cost = lambda c: scores[c]["cost"] if scores[c]["cost"] == scores[c]["cost"] else math.inf          # NaN ranks as +infinity
    return min(range(len(scores)), key=lambda c: (-(scores[c]["corner_factors"] + scores[c]["surf_factors"]), cost(c), c))


def _neighbours(stack, sub, par):
    """The five neighbours [m, 5, 3] (f64) of the stack points whose 5th neighbour is closer than 1 m under the pose par."""
    if not len(stack):
        return np.zeros((0, 5, 3))
    idx, d2 = oracle_py.knn_search(sub, associate_to_map(stack, par), 5)
    keep = (idx[:, 4] >= 0) & (d2[:, 4] < np.float32(1.0))
    return sub[idx[keep], :3].astype(np.float64)


def factor_bounds(stack_corner, stack_surf, submap_corner, submap_surf, par, floor=0, tol=1e-9):
    """(lower, upper, found): bounds of corner_factors + surf_factors of one start pose from numpy's batched eigenvalues / SVD instead of one
    oracle call per point.  numpy and the oracle's fits agree to ~1e-15 relative, so a point whose test quantity is further than `tol`
    (relative; absolute for the 0.2 m plane test) from its threshold is decided the same way by both; the points inside that margin, and
    the rank-deficient plane fits, count in `upper` only.  Used to prune, never to score.  A pose with fewer than `floor` points found is
    not fitted at all: (0, found, found)."""
    near, near_s = _neighbours(stack_corner, submap_corner, par), _neighbours(stack_surf, submap_surf, par)
    found = len(near) + len(near_s)
    if found < floor:
        return 0, found, found
    lo = hi = 0
    if len(near):
        z = near - near.sum(axis=1, keepdims=True) / 5.0
        vals = np.linalg.eigvalsh(np.einsum("mja,mjb->mab", z, z))
        a, b = vals[:, 2], 3 * vals[:, 1]
        unsure = ~(np.abs(a - b) > tol * (np.abs(a) + np.abs(b)))
        sure = (a > b) & ~unsure
        lo += int(sure.sum()); hi += int(sure.sum() + unsure.sum())
    near = near_s
    if len(near):
        U, s, Vt = np.linalg.svd(near, full_matrices=False)
        with np.errstate(all="ignore"):
            x = np.einsum("mka,mk->ma", Vt, np.einsum("mjk,mj->mk", U, -np.ones(near.shape[:2])) / s)
            ln = np.sqrt((x * x).sum(axis=1))
            r = np.abs(np.einsum("mja,ma->mj", near, x / ln[:, None]) + (1 / ln)[:, None]).max(axis=1)
        unsure = ~(np.abs(r - 0.2) > tol) | ~(s[:, 2] > 1e-6 * s[:, 0]) | ~np.isfinite(r)
        sure = (r < 0.2) & ~unsure
        lo += int(sure.sum()); hi += int(sure.sum() + unsure.sum())
    return lo, hi, found


def best_model(stack_corner, stack_surf, submap_corner, submap_surf, q_wodom, t_wodom, cand):
    """best_of(score_model(...)) - the same argmax, decided by the same oracle fits - without fitting every candidate.  A candidate has at
    most as many factors as stack points with five neighbours within 1 m (the search alone), and factor_bounds brackets its count; only the
    candidates whose upper bound reaches the largest lower bound can be the best, and only those go through score_one.  The candidates are
    visited in descending order of the points found for every 8th stack point, so that the largest lower bound is met early (the order
    changes the work, not the result).  Returns (best index, its score, how many candidates were fitted exactly)."""
    sc, ss = np.asarray(stack_corner, np.float32), np.asarray(stack_surf, np.float32)
    mc, msf = np.ascontiguousarray(submap_corner, np.float32), np.ascontiguousarray(submap_surf, np.float32)
    pars = [start_pose(q_wodom, t_wodom, q, t) for q, t in cand]
    rough = [len(_neighbours(sc[::8], mc, p)) + len(_neighbours(ss[::8], msf, p)) for p in pars]
    floor, upper = 0, {}
    for c in sorted(range(len(pars)), key=lambda c: (-rough[c], c)):
        lo, upper[c], _ = factor_bounds(sc, ss, mc, msf, pars[c], floor)
        floor = max(floor, lo)
    alive = sorted(c for c, hi in upper.items() if hi >= floor)
    keys = ("corner_factors", "surf_factors", "corner_found", "surf_found", "cost")
    scores = [dict(zip(keys, score_one(sc, ss, mc, msf, pars[c]))) for c in alive]
    w = best_of(scores)
    return alive[w], scores[w], len(alive)
