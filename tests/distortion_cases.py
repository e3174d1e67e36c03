"""Odometry problems with distortion = 1 built to drive the de-skew, its closed-form Jacobian and the hand-written trigonometry
(a-loam_amd/csrc/odometry_solve_device.hpp: slerp_scales, deskew_point, deskew_jacobian_row; aloam_trig.hpp) through what free-running
sweeps never reach: w < 0, the linear guard and the first w below it, trig arguments below 2^-27 and far above pi / 4, ratios of 9.99,
below zero and exactly zero, rotations near and at 180 degrees.  No GPU in here.  Used by tests/test_distortion_cases.py, which pins from
the oracle alone what the list reaches, and by tests/test_gpu_distortion_edges.py, which demands the same of the HIP path.

Everything derives from sweep 1 of sequence("VLP-16", 2, seed=3, columns=512) as an oracle with distortion registers it.  A scenario is
(name, features, last corner cloud, last surf cloud, para_q, para_t), one per (pose, ratio mode):

  pose   para_t = T0, para_q = (sqrt(1 - w w) AXIS, w) exactly as constructed (never re-normalised) for the w of W_CASES, and the same
         quaternion negated as a whole (its "twin": the same rotation, the other sign of w).  The twin of w = 0 has w = -0.0.
  mode   `rendered` keeps the intensities; `quirk` gives a fifth of the points ring - 0.001f (key ring - 1, s = 9.99; on ring 0 s = -0.01:
         the reference's int(intensity) on a point before the first ray's azimuth) and another fifth ring + 0.0999f; `zero` gives every
         point its ring, s = 0.  Which fifth is a function of the bits of the point's x, so a point has one ratio in all four lists.
  last   the sweep's own less-sharp / less-flat points de-skewed, each with its own ratio, at the build pose - BUILD_ANGLE about
         BUILD_AXIS on the left of para_q, para_t + BUILD_SHIFT - by the f64 model (a-loam_amd/information.py), rounded to f32, intensity =
         ring, stable-sorted by ring: every query has its neighbours centimetres away whatever the rotation.
"""
import functools
import importlib
import math

import numpy as np

import oracle_py

F = np.float32
N_SCANS, COLUMNS, SEED = 16, 512, 3
T0 = np.array([0.9, 0.05, -0.02])
AXIS = np.array([0.36, -0.48, 0.8])                       # a unit vector whose components and squares are short decimals
ONE = 1.0 - 2.0 ** -52                                    # Eigen's slerp: |w| >= 1 - epsilon blends linearly
W_CASES = (("identity", 1.0), ("guard", ONE), ("below-guard", float(np.nextafter(ONE, 0.0))), ("small", math.cos(0.5e-5)),
           ("ordinary", math.cos(0.015)), ("large", math.cos(0.35)), ("near-180", math.cos(1.55)), ("180", 0.0))
MODES = ("rendered", "quirk", "zero")
BUILD_AXIS, BUILD_ANGLE, BUILD_SHIFT = np.array([0.3, -0.5, 0.8]), 5e-3, np.array([0.03, -0.02, 0.01])
TINY = 2.0 ** -27                                         # below it trig_ksin / trig_kcos return early
S2 = np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0])             # Ceres' tangent delta is half the rotation vector theta of the information record


def _info():
    return importlib.import_module("a-loam_amd.information")


def poses():
    """[(name, para_q as constructed, w case name)]: sixteen, a pose and its twin next to each other."""
    out = []
    for name, w in W_CASES:
        q = np.concatenate([math.sqrt(1.0 - w * w) * AXIS, [w]])
        out.append((name, q, name))
        out.append((name + "-twin", -q, name))
    return out


def ratio(intensity):
    """(intensity - int(intensity)) / SCAN_PERIOD: an f32 difference divided by the double 0.1."""
    w = np.asarray(intensity, F)
    return (w - np.trunc(w).astype(F)).astype(np.float64) / 0.1


def with_mode(cloud, mode):
    """The cloud with the fractional part of its intensities rewritten, and the ring of every point."""
    ring = np.trunc(cloud[:, 3]).astype(F)
    out = cloud.copy()
    if mode == "quirk":
        pick = np.ascontiguousarray(cloud[:, 0]).view(np.uint32) % 5
        out[:, 3] = np.where(pick == 0, ring - F(0.001), np.where(pick == 1, ring + F(0.0999), cloud[:, 3])).astype(F)
    elif mode == "zero":
        out[:, 3] = ring
    return out, ring


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def build_pose(q, t):
    n = BUILD_AXIS / np.linalg.norm(BUILD_AXIS)
    dq = np.concatenate([math.sin(0.5 * BUILD_ANGLE) * n, [math.cos(0.5 * BUILD_ANGLE)]])
    return qmul(dq, q), t + BUILD_SHIFT


@functools.lru_cache(maxsize=None)
def sweep():
    """The four feature lists of sweep 1 and the sensor model."""
    syn = importlib.import_module("a-loam_amd.synthetic")
    scans, _, _, model = syn.make_sequence("VLP-16", 2, seed=SEED, columns=COLUMNS)
    orc = oracle_py.Oracle(n_scans=model.n_scans, min_range=model.min_range, distortion=True)
    f = None
    for x in scans:
        f = orc.scan_register(x.numpy())
        orc.odometry_step()
    return {k: f[k] for k in ("sharp", "less_sharp", "flat", "less_flat")}, model


@functools.lru_cache(maxsize=None)
def scenarios():
    """The 48 scenarios, in batch order: pose-major, the modes of a pose next to each other."""
    I = _info()
    f, _ = sweep()
    out = []
    for pname, q, _ in poses():
        qb, tb = build_pose(q, T0)
        for mode in MODES:
            feats, last = {}, {}
            for k in ("sharp", "less_sharp", "flat", "less_flat"):
                feats[k], ring = with_mode(f[k], mode)
                if k.startswith("less"):
                    lp, _ = I._points(feats[k][:, :3].astype(np.float64), qb, tb, ratio(feats[k][:, 3]))
                    c = np.concatenate([lp.astype(F), ring[:, None]], axis=1).astype(F)
                    last[k] = c[np.argsort(ring.astype(int), kind="stable")]
            out.append((f"{pname}/{mode}", feats, last["less_sharp"], last["less_flat"], q.copy(), T0.copy()))
    return out


def pose_of(name):
    return name.split("/")[0]


def mode_of(name):
    return name.split("/")[1]


def twin_pairs():
    """[(index of a scenario, index of its twin's)] in scenarios()."""
    names = [sc[0] for sc in scenarios()]
    return [(i, names.index(pose_of(n) + "-twin/" + mode_of(n))) for i, n in enumerate(names) if not pose_of(n).endswith("-twin")]


def feed(dev, sc, **seq):
    """Hand a scenario to the library's context or to the oracle (same method names); the caller steps."""
    _, f, corner, surf, q, t = sc
    dev.set_features(f, **seq)
    dev.set_last(corner, surf, **seq)
    dev.set_state(q, t, [0, 0, 0, 1.0], [0, 0, 0.0], inited=True, **seq)


def oracle(lm, outer=2):
    _, model = sweep()
    return oracle_py.Oracle(n_scans=model.n_scans, min_range=model.min_range, lm_max_iterations=lm, outer_iterations=outer, distortion=True)


def ratios_of(sc, eq, pq):
    """(s of the edge factors, s of the plane factors) from the intensity of the query each one names."""
    return ratio(sc[1]["sharp"][eq, 3]), ratio(sc[1]["flat"][pq, 3])


@functools.lru_cache(maxsize=None)
def run_oracle(index, lm):
    """One odometry step of the oracle on scenario `index`: (stats, pose, correspondences)."""
    orc = oracle(lm)
    feed(orc, scenarios()[index])
    pose = orc.odometry_step()
    return orc.odom_stats(), pose, orc.correspondences()


def autodiff_rows(e, p, s, q, t):
    """Unweighted residuals and rows of every factor from the oracle's dual numbers through its Eigen slerp stand-in, columns in the
    information record's tangent (theta, t): (r_line [n, 3], J_line [n, 3, 6], r_plane [n], J_plane [n, 6])."""
    e, p = np.asarray(e, np.float64).reshape(-1, 9), np.asarray(p, np.float64).reshape(-1, 12)
    rl, Jl, rp, Jp = np.zeros((len(e), 3)), np.zeros((len(e), 3, 6)), np.zeros(len(p)), np.zeros((len(p), 6))
    for i in range(len(e)):
        rl[i], Jl[i] = oracle_py.factor_eval_s(0, e[i], s[0][i], q, t)
    for i in range(len(p)):
        r, J = oracle_py.factor_eval_s(1, p[i], s[1][i], q, t)
        rp[i], Jp[i] = r[0], J[0]
    return rl, Jl * S2, rp, Jp * S2


def autodiff_sums(e, p, s, q, t):
    """The Huber-weighted sums of autodiff_rows with the names of aloam_pose_information."""
    I = _info()
    rl, Jl, rp, Jp = autodiff_rows(e, p, s, q, t)
    rho_l, w_l = I.huber(np.einsum("ij,ij->i", rl, rl))
    rho_p, w_p = I.huber(rp * rp)
    H = np.einsum("n,nri,nrj->ij", w_l, Jl, Jl) + np.einsum("n,ni,nj->ij", w_p, Jp, Jp)
    g = np.einsum("n,nri,nr->i", w_l, Jl, rl) + np.einsum("n,ni,n->i", w_p, Jp, rp)
    return {"info": 0.5 * (H + H.T), "gradient": g, "cost": 0.5 * (float(np.sum(rho_l)) + float(np.sum(rho_p))),
            "n_line": len(rl), "n_plane": len(rp), "rows": 3 * len(rl) + len(rp)}


def deviation(rec, want):
    """(dH, dg, dcost) normalised as test_gpu_pose_information._check_against_model does."""
    dia = np.sqrt(np.diag(want["info"]))
    dH = np.abs(rec["info"] - want["info"]) / np.outer(dia, dia)
    dg = np.abs(rec["gradient"] - want["gradient"]) / np.sqrt(2.0 * want["cost"] * np.diag(want["info"]))
    return float(dH.max()), float(dg.max()), abs(float(rec["cost"]) - want["cost"]) / want["cost"]


def reach(s, w):
    """What the factors with ratios s reach in slerp_scales at quaternion scalar w, as counts."""
    s = np.asarray(s, np.float64)
    if abs(w) >= ONE:
        return {"linear": len(s)}
    th = math.acos(abs(w))
    a0, a1 = np.abs((1.0 - s) * th), np.abs(s * th)
    return {"trig": len(s), "tiny": int(((a0 < TINY) | (a1 < TINY)).sum()), "above_pio4": int((s * th > math.pi / 4).sum()), "above_15": int((s * th > 15.0).sum())}


# ---- the oracle's second opinion: closed-form Jacobians and Cholesky on the normal equations ---------------------------------------------------------
def lm_closed_form(e, p, s, q, t, max_iterations):
    """The Levenberg-Marquardt loop of oracle_solver.cpp restated in numpy (as map_lm_scenarios.lm_trace does for the map solve), with
    the sums of information_from_factors - the closed form of the de-skew Jacobian - and a solve of the damped normal equations where the
    oracle takes dual numbers and a QR of the stacked Jacobian.  Returns (q, t, summary)."""
    I = _info()
    K = 1.0 / S2

    def sums(q, t):
        rec = I.information_from_factors(e, p, q, t, s)
        return rec["info"] * np.outer(K, K), rec["gradient"] * K, rec["cost"]

    q, t = np.array(q, np.float64), np.array(t, np.float64)
    if len(e) + len(p) == 0:
        return q, t, {"iterations": 0, "successful": 0, "termination": 4}
    H, g, cost = sums(q, t)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))

    def gmax_of(q, t, g):
        return max(np.abs(q - oracle_py.quat_plus(q, -g[:3])).max(), np.abs(t - (t + (-g[3:]))).max())

    gmax = gmax_of(q, t, g)
    Hs, gs = H * np.outer(scale, scale), g * scale
    radius, decrease, reuse, invalid, it, ok_steps, term = 1e4, 2.0, False, 0, 0, 0, 0
    x_norm = math.sqrt(float(q @ q + t @ t))
    diag = np.zeros(6)
    while True:
        if it >= max_iterations:
            term = 0
            break
        if gmax <= 1e-10:
            term = 3
            break
        it += 1
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(Hs), 1e-6), 1e32)
        step = -np.linalg.solve(Hs + np.diag(diag / radius), gs)
        reuse = True
        change = -float(step @ gs) - 0.5 * float(step @ Hs @ step)
        if not (np.isfinite(step).all() and change > 0.0):
            invalid += 1
            if invalid >= 5:
                term = 5
                break
            radius, decrease = radius / decrease, decrease * 2.0
            continue
        invalid = 0
        delta = step * scale
        qc, tc = oracle_py.quat_plus(q, delta[:3]), t + delta[3:]
        Hc, gc, cost_c = sums(qc, tc)
        sn = math.sqrt(float((q - qc) @ (q - qc) + (t - tc) @ (t - tc)))
        if sn <= 1e-8 * (x_norm + 1e-8):
            term = 1
            break
        if abs(cost - cost_c) <= 1e-6 * cost:
            term = 2
            break
        rel = (cost - cost_c) / change
        if rel > 1e-3:
            q, t, cost, ok_steps = qc, tc, cost_c, ok_steps + 1
            x_norm = math.sqrt(float(q @ q + t @ t))
            gmax = gmax_of(q, t, gc)
            Hs, gs = Hc * np.outer(scale, scale), gc * scale
            c3 = 2.0 * rel - 1.0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - c3 * c3 * c3))
            decrease, reuse = 2.0, False
        else:
            radius, decrease = radius / decrease, decrease * 2.0
    return q, t, {"iterations": it, "successful": ok_steps, "termination": term}


@functools.lru_cache(maxsize=None)
def spread(index, lm):
    """(largest difference of (para_q, para_t) between the oracle's step and the same step solved by lm_closed_form on the oracle's own
    association at each outer iteration, whether the two took the same decisions)."""
    sc = scenarios()[index]
    so, po, _ = run_oracle(index, lm)
    q, t = sc[4].copy(), sc[5].copy()
    same = True
    for k in range(2):
        orc = oracle(0, outer=1)
        feed(orc, (sc[0], sc[1], sc[2], sc[3], q, t))
        orc.odometry_step()
        e, p, eq, pq = orc.correspondences()
        q, t, sm = lm_closed_form(e, p, ratios_of(sc, eq, pq), q, t, lm)
        same = same and (len(e), len(p), sm["iterations"], sm["successful"], sm["termination"]) == \
            (so["corner_corr"][k], so["plane_corr"][k], so["lm_iterations"][k], so["lm_successful"][k], so["termination"][k])
    return max(float(np.abs(q - po["q_lc"]).max()), float(np.abs(t - po["t_lc"]).max())), same


POSE_TOL = 1e-4                                           # test_gpu_parity._assert_pose_close: metres and radians


def pose_bound(index, lm):
    """What the device's pose may deviate from the oracle's: the bound of _assert_pose_close, or ten times the spread of the oracle's
    own two variants where that spread exceeds a tenth of it."""
    sp, _ = spread(index, lm)
    return POSE_TOL if sp <= 0.1 * POSE_TOL else max(POSE_TOL, 10.0 * sp)


# ---- 50 digits -----------------------------------------------------------------------------------------------------------------------------------------
def mp_point_and_derivative(cp, s, q, t, dps=50):
    """lp = Identity.slerp(s, q) cp + s t and d lp / d (theta, t) [3, 6] at 50 digits, the rotation columns by differentiating
    lp(Plus(q, delta)) numerically in delta (theta = 2 delta).  The branch of the slerp (linear blend or trigonometric, the sign of w) is
    the one the unperturbed q takes, continued analytically: at w = 0 that is the one-sided derivative dual numbers give."""
    import mpmath as mp
    with mp.workdps(dps + 10):
        qm = [mp.mpf(float(v)) for v in q]
        tm = [mp.mpf(float(v)) for v in t]
        v = [mp.mpf(float(x)) for x in cp]
        sm = mp.mpf(float(s))
        linear, sign = abs(float(q[3])) >= ONE, (-1 if float(q[3]) < 0.0 else 1)

        def lp_of(qq):
            d = sign * qq[3]
            if linear:
                c0, c1 = 1 - sm, sm
            else:
                th = mp.acos(d)
                c0, c1 = mp.sin((1 - sm) * th) / mp.sin(th), mp.sin(sm * th) / mp.sin(th)
            c1 = sign * c1
            u, w = [c1 * qq[0], c1 * qq[1], c1 * qq[2]], c0 + c1 * qq[3]
            cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            uv = [2 * x for x in cr(u, v)]
            uuv = cr(u, uv)
            return [v[k] + w * uv[k] + uuv[k] + sm * tm[k] for k in range(3)]

        def plus(delta):
            nd = mp.sqrt(sum(x * x for x in delta))
            if nd == 0:
                return qm
            k = mp.sin(nd) / nd
            a = [k * delta[0], k * delta[1], k * delta[2], mp.cos(nd)]
            return [a[3] * qm[0] + a[0] * qm[3] + a[1] * qm[2] - a[2] * qm[1], a[3] * qm[1] - a[0] * qm[2] + a[1] * qm[3] + a[2] * qm[0],
                    a[3] * qm[2] + a[0] * qm[1] - a[1] * qm[0] + a[2] * qm[3], a[3] * qm[3] - a[0] * qm[0] - a[1] * qm[1] - a[2] * qm[2]]

        lp = lp_of(qm)
        D = np.zeros((3, 6))
        for c in range(3):
            for r in range(3):
                f = lambda h, c=c, r=r: lp_of(plus([h if k == c else mp.mpf(0) for k in range(3)]))[r]
                D[r, c] = float(mp.diff(f, 0) / 2)
            D[c, 3 + c] = float(sm)
        return np.array([float(x) for x in lp]), D
