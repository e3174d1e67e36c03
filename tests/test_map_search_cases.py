"""What the constructed map frame of tests/map_search_cases.py proves about itself, on the CPU: that its inputs force the paths of k_mapgrid_build /
k_map_search / k_map_fit they are there for (from the kernels' own cell and bucket arithmetic, restated), that every edge is visible in a factor
record (the plain definition evaluated once more with the plausible mistake), how far the oracle's Eigen stand-ins sit from an independent f64
evaluation on these very neighbour sets (the tolerance the device is held to is 100 times that), and that every decision but the deliberately
exact ones is far from its threshold.  tests/test_gpu_map_search_geometry.py counts only as far as these hold."""
import numpy as np
import pytest

import loopreg_model as M
import map_search_cases as mc
from assoc_cases import dist2

F = np.float32


@pytest.fixture(scope="module")
def ev(O):
    return mc.evaluated()


def _tagged(s, cls, tag):
    return [i for i, t in enumerate(s.tags[cls]) if t == tag]


def test_the_filters_hand_map_and_stack_on_unchanged(O, ev):
    s = ev.scene
    for cls in (0, 1):
        st = s.stack[cls]
        assert np.array_equal(O.voxel_filter(st, mc.LEAF, canonical=True).view(np.uint32), st.view(np.uint32))      # each stack point alone in its voxel
        a = s.map_frames[0][cls]
        assert len(O.voxel_filter(a, mc.LEAF, canonical=True)) == len(a)
        total = sum(len(f[cls]) for f in s.map_frames)
        assert len(ev.tgt[cls]) == total == ev.info[("from_map_corner", "from_map_surf")[cls]]                      # the duplicates survived
        assert set(ev.cubes[cls]) == {10 + 21 * 10 + 441 * 5}                                                        # one cube: its order is the submap's
        assert {tuple(p) for p in ev.tgt[cls][:, :3].tolist()} == {tuple(p) for f in s.map_frames for p in (f[cls][:, :3].astype(np.float64) + f[2]).astype(F).tolist()}
    assert ev.info["frame_count"] == len(s.map_frames) + 1 and ev.info["from_map_corner"] > 10 and ev.info["from_map_surf"] > 50
    assert mc.table_size(mc.POOL_POINTS) == 4096 and mc.table_size(1 << 20) == 32768 and mc.table_size(4096) == 4096


def test_the_model_is_the_loop_registration_models_and_tells_the_oracles_counts(O, ev):
    """factors_by_query with the oracle's knn_search == with the plain definition of the five; its records are loopreg_model.factors' in stack order;
    its counts are Oracle.mapping_step's."""
    s = ev.scene
    lines, planes = M.factors(s.stack[0], s.stack[1], ev.tgt[0], ev.tgt[1], np.array([0, 0, 0, 1.0, 0, 0, 0]))
    for cls, recs in enumerate((lines, planes)):
        by_def = mc.factors_by_query(cls, s.stack[cls], ev.tgt[cls])
        assert sorted(by_def) == sorted(ev.model[cls])
        for i in by_def:
            assert by_def[i][0] == ev.model[cls][i][0] and np.array_equal(by_def[i][1], ev.model[cls][i][1]), (cls, i)
        assert len(recs) == len(ev.model[cls]) == ev.info[("corner_num1", "surf_num1")[cls]] == ev.info[("corner_num0", "surf_num0")[cls]]
        for r, i in zip(recs, sorted(ev.model[cls])):
            assert np.array_equal(r[:3], s.stack[cls][i, :3].astype(np.float64)) and np.array_equal(r[3:], ev.model[cls][i][1])
        print(f"class {cls}: {len(s.stack[cls])} stack points, {len(recs)} records")


def test_caps_and_expectations(ev):
    s = ev.scene
    for cls in (0, 1):
        n, with_record = len(s.stack[cls]), len(ev.model[cls])
        assert with_record >= 20 and n - with_record >= 5, (cls, n, with_record)
        assert all(s.tags[cls]) and len(s.tags[cls]) == n
        for i, want in enumerate(s.expect[cls]):
            assert (i in ev.model[cls]) == want, (cls, i, s.tags[cls][i])


def test_tolerance_is_measured(ev):
    spread = mc.measured_spread()
    print(f"oracle stand-ins against numpy eigh / lstsq over the frame's neighbour sets: largest difference {spread:.3e}; the device gets {mc.device_tolerance():.3e}")
    assert 0.0 < spread < 1e-12                                                # two f64 algorithms on well-separated decisions


@pytest.mark.parametrize("mistake", sorted(mc.MISTAKES))
def test_sensitivity_to_the_plausible_mistakes(ev, mistake):
    """Each mistake, made in the DEFINITION, changes the record of at least the stated number of queries per class: a record appears or disappears, or
    moves by more than 1000 times the tolerance."""
    s, tol = ev.scene, mc.device_tolerance()
    for cls in (0, 1):
        wrong = mc.factors_by_query(cls, s.stack[cls], ev.tgt[cls], **mc.MISTAKES[mistake])
        right = ev.model[cls]
        moved = [i for i in set(wrong) | set(right) if (i in wrong) != (i in right) or mc.record_difference(cls, wrong[i][1], right[i][1]) > 1000.0 * tol]
        print(f"class {cls} mistake {mistake}: {len(moved)} records change (stated: at least {mc.SENSITIVITY[mistake]}): {sorted({s.tags[cls][i] for i in moved})}")
        assert len(moved) >= mc.SENSITIVITY[mistake], (cls, mistake, len(moved))


def test_m1_the_gate(ev):
    s = ev.scene
    for cls in (0, 1):
        for tag, check in (("five-in-range", lambda d: (d < F(1.0)).sum() == 5), ("four-in-range", lambda d: (d < F(1.0)).sum() == 4),
                           ("fifth-at-exactly-1", lambda d: (d < F(1.0)).sum() == 4 and (d == F(1.0)).sum() == 1),
                           ("fifth-one-ulp-inside", lambda d: (d < F(1.0)).sum() == 5 and F(1.0) - np.sort(d)[4] < 1e-5)):
            idx = _tagged(s, cls, tag)
            assert len(idx) == 2
            for i in idx:
                assert check(dist2(ev.tgt[cls], s.stack[cls][i, :3])), (cls, tag, i)


def test_m2_block_choice(ev):
    s = ev.scene
    for cls in (0, 1):
        axes_seen = {}
        for tag in ("frac-0", "frac-0.5", "frac-just-below-0.5", "frac-just-above-0.5"):
            for i in _tagged(s, cls, tag):
                q = s.stack[cls][i, :3]
                g = q * F(0.5)
                frac = g - np.floor(g)
                want = {"frac-0": lambda f: f == 0, "frac-0.5": lambda f: f == F(0.5), "frac-just-below-0.5": lambda f: 0 < F(0.5) - f < 1e-6,
                        "frac-just-above-0.5": lambda f: 0 < f - F(0.5) < 1e-6}[tag]
                axis = [a for a in range(3) if want(frac[a])]
                assert len(axis) == 1, (cls, tag, frac)
                axes_seen.setdefault(tag, set()).add(axis[0])
                c = mc.cell_of(q)
                nb = set(mc.block_of(q)) - {tuple(c)}
                side = {n[axis[0]] - c[axis[0]] for n in nb} - {0}
                assert side == ({-1} if tag in ("frac-0", "frac-just-below-0.5") else {1}), (cls, tag, side)
        assert all(v == {0, 1, 2} for v in axes_seen.values()) and len(axes_seen) == 4
        octants = set()
        for i in _tagged(s, cls, "octant-diagonal-cell"):
            q = s.stack[cls][i, :3]
            five = ev.model[cls][i][0]
            cells = {tuple(c) for c in mc.cell_of(ev.tgt[cls][five])}
            assert len(cells) == 1
            d = np.array(next(iter(cells))) - mc.cell_of(q)
            assert set(np.abs(d).tolist()) == {1}                              # the diagonal neighbour cell only
            octants.add(tuple(d.tolist()))
        assert len(octants) == 8
        allq = s.stack[cls][:, :3]
        assert (allq < 0).any(axis=0).all() and (allq > 0).any(axis=0).all()      # negative and positive coordinates on every axis
        # at fraction 0 the five lie in the cell below: the wrong side sees none of them
        for i in _tagged(s, cls, "frac-0"):
            assert mc.define5(ev.tgt[cls], s.stack[cls][i, :3], wrong_side=True) is None


def test_m3_ties(ev):
    s = ev.scene
    for cls in (0, 1):
        tgt = ev.tgt[cls]
        for i in _tagged(s, cls, "eight-tied-for-fifth"):
            d = dist2(tgt, s.stack[cls][i, :3])
            o = np.lexsort((np.arange(len(d)), d))
            assert d[o[3]] < d[o[4]] and len(set(d[o[4:12]].tolist())) == 1 and d[o[12]] > d[o[11]]      # eight equidistant points for the fifth place
            assert ev.model[cls][i][0] == [int(x) for x in o[:5]] and o[4] == min(o[4:12])               # the lowest submap index wins
        for i in _tagged(s, cls, "a-point-twice-makes-five"):
            five = ev.model[cls][i][0]
            pts = tgt[five, :3]
            assert len(np.unique(pts, axis=0)) == 4 and (dist2(tgt, s.stack[cls][i, :3]) < F(1.0)).sum() == 5
        for i in _tagged(s, cls, "tie-across-two-buckets"):
            d = dist2(tgt, s.stack[cls][i, :3])
            o = np.lexsort((np.arange(len(d)), d))
            assert d[o[4]] == d[o[5]] < d[o[6]]
            ca, cb = mc.cell_of(tgt[o[4]]), mc.cell_of(tgt[o[5]])
            assert mc.map_bucket(*ca, s.H) != mc.map_bucket(*cb, s.H) and {tuple(ca), tuple(cb)} <= set(mc.block_of(s.stack[cls][i, :3]))


def _bucket_counts(tgt, H):
    cells = mc.cell_of(tgt)
    h = np.array([mc.map_bucket(*c, H) for c in cells])
    return h, np.bincount(h, minlength=H)


def test_m4_long_buckets_and_tails(ev):
    s = ev.scene
    for cls in (0, 1):
        tgt = ev.tgt[cls]
        h, cnt = _bucket_counts(tgt, s.H)
        big = int(cnt.max())
        assert big >= (1944, 1875)[cls]                                         # the largest bucket: the one 2 m cell (and whatever far cell shares it)
        for i in _tagged(s, cls, "inside-the-long-bucket"):
            q = s.stack[cls][i, :3]
            assert cnt[mc.map_bucket(*mc.cell_of(q), s.H)] == big and (dist2(tgt, q) < F(1.0)).sum() > 100      # hundreds of candidates pass d < 1
        tails = set()
        for k in range(1, 6):
            (i,) = _tagged(s, cls, f"needs-every-entry-of-a-{k}-bucket")
            five = ev.model[cls][i][0]
            own = np.bincount(h[five], minlength=s.H)                          # entries of the five per bucket: k and 5 - k
            counts = sorted(int(cnt[b]) for b in set(h[five].tolist()))
            assert sorted(own[own > 0].tolist()) == sorted(x for x in (k, 5 - k) if x), (cls, k, own[own > 0])
            assert all(cnt[b] >= own[b] for b in set(h[five].tolist()))      # (a far cell hashed into the bucket only adds entries)
            tails |= {c % 4 for c in counts}
            print(f"class {cls}: the {k}-entry cell's five sit in buckets of {counts} entries")
        (i,) = _tagged(s, cls, "four-in-range-3-and-1")
        d = dist2(tgt, s.stack[cls][i, :3])
        near = np.nonzero(d < F(1.0))[0]
        assert len(near) == 4 and sorted(np.bincount(h[near])[np.bincount(h[near]) > 0].tolist()) == [1, 3]
        assert tails == {0, 1, 2, 3}
        print(f"class {cls}: largest bucket {big}, {int((cnt > 0).sum())} buckets in use of {s.H}")


def test_m5_far_cells_share_the_blocks_buckets(ev):
    s = ev.scene
    for cls in (0, 1):
        tgt = ev.tgt[cls]
        h, cnt = _bucket_counts(tgt, s.H)
        cells = mc.cell_of(tgt)
        idx = _tagged(s, cls, "block-shares-buckets-with-far-cells")
        assert len(idx) == 3
        for i in idx:
            q = s.stack[cls][i, :3]
            foreign = 0
            for c in mc.block_of(q):
                b = mc.map_bucket(*c, s.H)
                other = (h == b) & ~np.all(cells == c, axis=1)
                if other.any():
                    assert np.abs(cells[other] - np.array(c)).max(axis=1).min() >= 4      # far apart
                    assert dist2(tgt[other], q).min() > F(9.0)
                    foreign += int(other.sum())
            assert foreign >= 58, (cls, i, foreign)                              # at least two far cells of 29 entries are walked with this query's block


def test_m6_fits(O, ev):
    s = ev.scene
    (i,) = _tagged(s, 0, "five-collinear")
    near = ev.tgt[0][ev.model[0][i][0], :3].astype(np.float64)
    c = near.mean(axis=0)
    vals, _ = O.sym_eigen3(sum(np.outer(p - c, p - c) for p in near))
    assert vals[1] == 0.0 and vals[2] > 0.1                                   # the line is valid and the middle eigenvalue is 0
    (i,) = _tagged(s, 0, "five-identical")
    five = mc.define5(ev.tgt[0], s.stack[0][i, :3])
    assert five is not None and len(np.unique(ev.tgt[0][five, :3], axis=0)) == 1 and i not in ev.model[0]      # covariance 0: 0 > 3 * 0 is false
    (i,) = _tagged(s, 1, "five-in-an-exact-plane")
    near = ev.tgt[1][ev.model[1][i][0], :3].astype(np.float64)
    rec = ev.model[1][i][1]
    assert np.abs(near @ rec[:3] + rec[3]).max() < 1e-12 and len(set(near[:, 2].tolist())) == 1
    (i,) = _tagged(s, 1, "five-identical")
    five, rec = ev.model[1][i]
    near = ev.tgt[1][five, :3].astype(np.float64)
    assert len(np.unique(near, axis=0)) == 1 and np.linalg.matrix_rank(near) == 1 and sorted(np.abs(rec[:3]).tolist()) == [0.0, 0.0, 1.0]
    (i,) = _tagged(s, 1, "plane-fails-0.2")
    five = mc.define5(ev.tgt[1], s.stack[1][i, :3])
    near = ev.tgt[1][five, :3].astype(np.float64)
    x = O.lstsq_5x3(near, -np.ones(5))
    assert np.abs(near @ x / np.linalg.norm(x) + 1.0 / np.linalg.norm(x)).max() > 0.3      # fails the 0.2 test by a wide margin


def test_decisions_are_far_from_their_thresholds_except_the_exact_ones(O, ev):
    """The oracle's decision log of the test frame (two passes over the stack): kinds 5 (fifth neighbour d2 < 1), 6 (eigenvalue ratio), 7 (plane
    residual > 0.2).  The deliberately exact decisions - the fifth neighbour at d2 = 1.0 and one ulp inside, the zero covariance - are counted; every
    other margin is above 1e-3."""
    kinds, values, thresholds = ev.decisions
    exact = {5: 2 * 2 * 4, 6: 2 * 1, 7: 0}                                     # (passes) x (per frame): 2 classes x (2 at exactly 1 + 2 one ulp inside); the identical corner points
    for kind in (5, 6, 7):
        sel = kinds == kind
        rel = np.abs(values[sel] - thresholds[sel]) / np.maximum(np.abs(thresholds[sel]), 1e-300)
        close = int((rel < 1e-3).sum())
        print(f"{O.DECISION_KINDS[kind]:28s} n = {int(sel.sum()):5d}  within 1e-3 of the threshold: {close} (deliberately: {exact[kind]}), closest other margin {np.sort(rel)[close]:.3g}")
        assert sel.sum() > 50 and close == exact[kind], (kind, close)
        assert (rel[rel < 1e-3] < 1e-5).all()


def test_five_neighbours_at_the_origin_the_model_says_what_the_oracle_says(O):
    """x = 0, len = 0: the oracle (and k_map_fit) go on with NaN and the record stays, because fabs(NaN) > 0.2 is false; loopreg_model.factors says the same."""
    ev0 = mc.evaluated(origin_case=True)
    s = ev0.scene
    (i,) = _tagged(s, 1, "five-at-the-origin")
    five = mc.define5(ev0.tgt[1], s.stack[1][i, :3])
    assert five is not None and not ev0.tgt[1][five, :3].any()
    assert np.array_equal(O.lstsq_5x3(np.zeros((5, 3)), -np.ones(5)), np.zeros(3))
    lines, planes = M.factors(s.stack[0], s.stack[1], ev0.tgt[0], ev0.tgt[1], np.array([0, 0, 0, 1.0, 0, 0, 0]))
    assert len(planes) == ev0.info["surf_num1"] and len(lines) == ev0.info["corner_num1"]
    rec = planes[sorted(ev0.model[1]).index(i)]
    assert i in ev0.model[1] and np.array_equal(rec[:3], s.stack[1][i, :3].astype(np.float64)) and np.isnan(rec[3:6]).all() and np.isinf(rec[6])
