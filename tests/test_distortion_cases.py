"""What tests/distortion_cases.py reaches, from the oracle and numpy alone (no GPU): the GPU test over the same list
(tests/test_gpu_distortion_edges.py) must not be able to pass on an empty case, on a branch nobody took or against a reference that is
itself off.  Prints the reach and accuracy figures DESIGN.md section 7w tables."""
import importlib
import math

import numpy as np
import pytest

import distortion_cases as D

info = importlib.import_module("a-loam_amd.information")

N = 48
NONZERO = [i for i in range(N) if i % 3 != 2]             # the rendered and quirk scenarios


@pytest.fixture(scope="module")
def scs(O):
    return D.scenarios()


def test_the_list(scs):
    """Sixteen poses handed in as constructed, a twin being the exact negation; three modes; a point has one ratio in all four lists."""
    f, model = D.sweep()
    assert model.n_scans == D.N_SCANS and [len(f[k]) for k in ("sharp", "less_sharp", "flat", "less_flat")] == [172, 1363, 349, 5738]
    assert len(scs) == N and [D.mode_of(sc[0]) for sc in scs[:3]] == list(D.MODES)
    ws = sorted({float(sc[4][3]) for sc in scs})
    assert len(D.poses()) == 16 and D.ONE in ws and np.nextafter(D.ONE, 0.0) in ws and 1.0 in ws and -1.0 in ws
    assert D.ONE == 1.0 - np.finfo(np.float64).eps and D.ONE == 1.0 - 2.220446049250313e-16      # the constant of slerp_scales
    for i, j in D.twin_pairs():
        assert np.array_equal(scs[i][4], -scs[j][4]) and np.array_equal(np.signbit(scs[i][4]), ~np.signbit(scs[j][4])), scs[i][0]
        for k in ("sharp", "less_sharp", "flat", "less_flat"):
            assert scs[i][1][k].tobytes() == scs[j][1][k].tobytes()
    zero_twin = next(sc for sc in scs if sc[0] == "180-twin/zero")
    assert zero_twin[4][3] == 0.0 and np.signbit(zero_twin[4][3])
    for sc in scs:
        ft = sc[1]
        have = {p[:3].tobytes(): p[3] for p in ft["less_sharp"]}
        assert all(have[p[:3].tobytes()] == p[3] for p in ft["sharp"])                  # every sharp point is a less-sharp point
        seen = {}
        for k in ("sharp", "less_sharp", "flat", "less_flat"):                         # (the less-flat list is voxel-filtered: points of its own)
            for p in ft[k]:
                assert seen.setdefault(p[:3].tobytes(), p[3]) == p[3]
        for last in (sc[2], sc[3]):
            key = last[:, 3].astype(int)
            assert np.array_equal(last[:, 3], key.astype(np.float32)) and (np.diff(key) >= 0).all() and key.min() >= 0 and key.max() < D.N_SCANS
    s = D.ratio(scs[1][1]["less_flat"][:, 3])              # a quirk scenario
    ring = np.trunc(f["less_flat"][:, 3])
    print(f"quirk ratios: {int((s > 9.9).sum())} of {len(s)} at 9.99, {int((s < 0).sum())} below zero, {int((np.abs(s - 0.999) < 1e-3).sum())} at 0.999")
    assert (s > 9.9).sum() > 800 and np.allclose(s[s > 9.9], 9.99, atol=1e-4) and (s[s > 9.9] < 10.0).all()
    assert (s < 0).sum() > 30 and np.allclose(s[s < 0], -0.01, atol=1e-6) and (ring[s < 0] == 0).all() and (ring[s > 9.9] >= 1).all()
    assert not D.ratio(scs[2][1]["less_flat"][:, 3]).any() and not D.ratio(scs[2][1]["sharp"][:, 3]).any()


def test_correspondence_counts_and_branch_reach(scs):
    """At the named pose every rendered and quirk scenario has factors, and over the set they reach every branch of slerp_scales and of
    the trigonometry port that free-running sweeps leave alone."""
    total = {}
    least = (10 ** 9, 10 ** 9, None)
    for i in range(N):
        st, pose, (e, p, eq, pq) = D.run_oracle(i, 0)
        assert st["lm_iterations"] == [0, 0] and np.array_equal(pose["q_lc"], scs[i][4]) and np.array_equal(pose["t_lc"], scs[i][5])
        assert (len(e), len(p)) == (st["corner_corr"][1], st["plane_corr"][1])
        if i in NONZERO:
            assert len(e) >= 30 and len(p) >= 100, (scs[i][0], len(e), len(p))
            if len(e) + len(p) < least[0] + least[1]:
                least = (len(e), len(p), scs[i][0])
        s = np.concatenate(D.ratios_of(scs[i], eq, pq))
        r = D.reach(s, float(scs[i][4][3]))
        r["s<0"], r["s>9.9"], r["s=0"], r["w<0"] = int((s < 0).sum()), int((s > 9.9).sum()), int((s == 0).sum()), len(s) * bool(scs[i][4][3] < 0)
        for k, v in r.items():
            total[k] = total.get(k, 0) + v
        print(f"{scs[i][0]:26s} factors {len(e):3d} + {len(p):3d}  {r}")
    print(f"fewest factors: {least}; factors per branch over the set: {total}")
    for k in ("linear", "trig", "tiny", "above_pio4", "above_15", "s<0", "s>9.9", "s=0", "w<0"):
        assert total[k] >= 50, (k, total)


def test_zero_mode_rows_are_zero(scs):
    """s = 0: lp = cp whatever the pose, so every row of every Jacobian is exactly zero while the cost is not."""
    for i in range(2, N, 3):
        _, _, (e, p, eq, pq) = D.run_oracle(i, 0)
        s = D.ratios_of(scs[i], eq, pq)
        assert len(p) >= 100 and not s[0].any() and not s[1].any()
        rl, Jl, rp, Jp = D.autodiff_rows(e, p, s, scs[i][4], scs[i][5])
        assert not Jl.any() and not Jp.any() and not np.isnan(Jl).any() and not np.isnan(Jp).any(), scs[i][0]
        want = D.autodiff_sums(e, p, s, scs[i][4], scs[i][5])
        assert want["cost"] > 1e-4 and not want["info"].any() and not want["gradient"].any()
        assert info.decompose(want["info"])["status"] == info.INFO_SINGULAR


# The oracle's termination codes (oracle_solver.cpp): 0 the iteration limit, 1 parameter tolerance, 2 function tolerance, 3 gradient tolerance.
def test_solver_branches(scs):
    """lm_max_iterations = 4: accepted steps, rejected steps, at w = 0 four iterations none of which succeeds, in the zero mode an exit
    on the gradient tolerance before the first iteration; the last two leave the pose as it was, bit for bit."""
    accepted = rejected = 0
    terms = set()
    for i in range(N):
        st, pose, _ = D.run_oracle(i, 4)
        name = scs[i][0]
        print(f"{name:26s} iterations {st['lm_iterations']} successful {st['lm_successful']} termination {st['termination']} cost {st['initial_cost'][0]:.4g} -> {st['final_cost'][1]:.4g}")
        untouched = np.array_equal(pose["q_lc"], scs[i][4]) and np.array_equal(pose["t_lc"], scs[i][5])
        if D.mode_of(name) == "zero":
            assert st["lm_iterations"] == [0, 0] and st["lm_successful"] == [0, 0] and st["termination"] == [3, 3] and untouched, (name, st)
            assert st["initial_cost"][0] > 0 and st["final_cost"] == st["initial_cost"]
        elif D.pose_of(name) == "180":                    # (its twin, w = -0.0 about -AXIS, turns the way the last clouds were built and solves)
            assert st["lm_iterations"] == [4, 4] and st["lm_successful"] == [0, 0] and st["termination"] == [0, 0] and untouched, (name, st)
        else:
            assert not untouched and st["lm_successful"][0] >= 1 and st["final_cost"][1] < st["initial_cost"][0], (name, st)
        for k in range(2):
            terms.add(st["termination"][k])
            accepted += st["lm_successful"][k]
            rejected += st["lm_iterations"][k] - st["lm_successful"][k] - (1 if st["termination"][k] in (1, 2) else 0)
    print(f"accepted steps {accepted}, rejected steps {rejected}, termination codes {sorted(terms)}")
    assert accepted >= 28 and rejected >= 16 and {0, 3} <= terms


def test_the_autodiff_sums_agree_with_the_closed_form_model(scs):
    """The reference of the GPU test (sums of factor_eval_s rows) against information_from_factors, which restates the device's closed
    form: two derivations of one matrix, two and one order below the bounds the device is held to."""
    worst = [0.0, 0.0, 0.0]
    for i in NONZERO:
        _, _, (e, p, eq, pq) = D.run_oracle(i, 0)
        s = D.ratios_of(scs[i], eq, pq)
        want = D.autodiff_sums(e, p, s, scs[i][4], scs[i][5])
        model = info.information_from_factors(e, p, scs[i][4], scs[i][5], s)
        dev = D.deviation(model, want)
        assert dev[0] <= 1e-12 and dev[1] <= 1e-12 and dev[2] <= 1e-13, (scs[i][0], dev)
        worst = [max(a, b) for a, b in zip(worst, dev)]
    print(f"information_from_factors against the autodiff sums over {len(NONZERO)} scenarios: dH {worst[0]:.2e}, dg {worst[1]:.2e}, cost {worst[2]:.2e}")


def test_rows_against_fifty_digits(scs):
    """Rows of both derivations against a 50-digit evaluation of lp and its manifold derivative: every pose, ratios 0, -0.01, 0.999,
    9.99 and rendered ones, edge and plane factors."""
    rng = np.random.default_rng(5)
    worst = {"autodiff": 0.0, "closed form": 0.0, "residual": 0.0}
    rows = 0
    seen_s = set()
    for i in range(N):
        _, _, (e, p, eq, pq) = D.run_oracle(i, 0)
        s = D.ratios_of(scs[i], eq, pq)
        q, t = scs[i][4], scs[i][5]
        pe, pp = rng.permutation(len(e))[:1], rng.permutation(len(p))[:(5 if i % 3 == 1 else 3)]
        if i % 3 == 1:                                                      # quirk: one plane factor of each special ratio where there is one
            pp = np.unique(np.concatenate([pp] + [np.flatnonzero(m)[:1] for m in (s[1] > 9.9, s[1] < 0, np.abs(s[1] - 0.999) < 1e-3)]))
        ee, sp_e, pl, sp_p = e[pe], s[0][pe], p[pp], s[1][pp]
        rl, Jl, rp, Jp = D.autodiff_rows(ee, pl, (sp_e, sp_p), q, t)
        ml, MJl, mp_, MJp = info.factor_rows(ee, pl, q, t, (sp_e, sp_p))
        for k in range(len(pl)):
            lp, Dm = D.mp_point_and_derivative(pl[k, :3], sp_p[k], q, t)
            n = np.cross(pl[k, 3:6] - pl[k, 6:9], pl[k, 3:6] - pl[k, 9:12])
            n /= np.linalg.norm(n)
            row, top = n @ Dm, np.abs(n @ Dm).max()
            rows += 1
            seen_s.add(round(float(sp_p[k]), 3))
            if top > 0:
                worst["autodiff"] = max(worst["autodiff"], np.abs(Jp[k] - row).max() / top)
                worst["closed form"] = max(worst["closed form"], np.abs(MJp[k] - row).max() / top)
            else:
                assert not Jp[k].any() and not MJp[k].any()
            worst["residual"] = max(worst["residual"], abs(rp[k] - n @ (lp - pl[k, 3:6])), abs(mp_[k] - n @ (lp - pl[k, 3:6])))
        for k in range(len(ee)):
            lp, Dm = D.mp_point_and_derivative(ee[k, :3], sp_e[k], q, t)
            wv = (ee[k, 6:9] - ee[k, 3:6]) / np.linalg.norm(ee[k, 3:6] - ee[k, 6:9])
            A = np.array([[0, -wv[2], wv[1]], [wv[2], 0, -wv[0]], [-wv[1], wv[0], 0]])
            blk = A @ Dm
            top = np.abs(blk).max(axis=1, keepdims=True)
            rows += 3
            if top.min() > 0:
                worst["autodiff"] = max(worst["autodiff"], (np.abs(Jl[k] - blk) / top).max())
                worst["closed form"] = max(worst["closed form"], (np.abs(MJl[k] - blk) / top).max())
    print(f"{rows} rows against 50 digits, ratios {sorted(seen_s)[:4]} .. {sorted(seen_s)[-2:]}: largest deviation / largest entry of the row {worst}")
    assert rows >= 200 and {0.0, -0.01, 0.999, 9.99} <= seen_s
    assert worst["autodiff"] <= 1e-12 and worst["closed form"] <= 1e-12 and worst["residual"] <= 1e-12


def test_the_spread_of_the_oracles_two_variants(scs):
    """The solve leg's yardstick: the oracle's step (dual numbers, QR) and lm_closed_form (closed form, normal equations) on the same
    associations.  Printed for every scenario; where the two part by more than a tenth of the pose bound the bound widens with them."""
    wide = []
    for lm in (4, 8):
        for i in range(N):
            sp, same = D.spread(i, lm)
            b = D.pose_bound(i, lm)
            if b > D.POSE_TOL or not same:
                wide.append((scs[i][0], lm, sp, same))
            print(f"lm {lm} {scs[i][0]:26s} spread {sp:.2e} same decisions {same} bound {b:.1e}")
            if D.mode_of(scs[i][0]) == "zero" or D.pose_of(scs[i][0]) == "180":
                assert sp == 0.0 and same, scs[i][0]
    print("scenarios with a widened bound or differing decisions:", wide)
    assert len(wide) <= 4


def test_the_oracle_treats_a_quaternion_and_its_negation_alike(scs):
    """q and -q: the same statistics, costs and correspondences bit for bit at the fixed pose, except where w = 0 turns the two signs
    opposite ways (Eigen's slerp takes the short way round by the sign of w, and +0 and -0 both count as not negative)."""
    differ = []
    for i, j in D.twin_pairs():
        (si, _, ci), (sj, _, cj) = D.run_oracle(i, 0), D.run_oracle(j, 0)
        same = all(np.array_equal(a, b) for a, b in zip(ci, cj)) and all(np.array(si[k]).tobytes() == np.array(sj[k]).tobytes() for k in si)
        if not same:
            differ.append(scs[i][0])
    assert differ == ["180/rendered", "180/quirk"], differ
