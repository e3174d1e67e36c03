"""What every scene of tests/assoc_cases.py proves about itself, on the CPU: that its inputs force the path of the association kernels it is there
for (path facts, from the kernels' own f32 cell arithmetic restated), that the edge it sits on is visible in the records (sensitivity facts: the plain
definition evaluated once more with the plausible mistake), and that it keeps enough records of both kinds (caps).  The GPU comparison
(tests/test_gpu_assoc_geometry.py) counts only as far as these hold."""
import numpy as np
import pytest

import assoc_cases as ac

F = np.float32
ALL = ac.SMALL + ac.BUILD_LIMITS + ("empty",)
ORDERS = {"S1": (0, 0), "S2a": (0, 0), "S2b": (0, 0), "S3": (0, 0), "S4": (0, 0), "S5": (0, 0), "S8": (0, 0), "empty": (0, 0), "S6-65535": (0, 0), "S6-65536": (0, 0),
          "S1-lowered1": (1, 1), "S5-lowered1": (1, 1), "S1-lowered3": (2, 2), "S5-lowered3": (2, 2)}
_ORACLE = {}


def oracle_records(O, name, pose_name):
    """The oracle's per-query records of a scene at lm_max_iterations = 0, computed once and shared."""
    if (name, pose_name) not in _ORACLE:
        s = ac.scene(name)
        orc = O.Oracle(n_scans=s.n_scans, min_range=0.1, lm_max_iterations=0)
        ac.feed(orc, s, ac.POSES[pose_name])
        orc.odometry_step()
        _ORACLE[name, pose_name] = ac.per_query(s, orc.correspondences())
    return _ORACLE[name, pose_name]


@pytest.mark.parametrize("name", ALL)
def test_plain_definition_gives_the_oracles_records(O, name):
    """At the identity pose sel == raw, so assoc_cases.define() on the scene's own arrays must reproduce the oracle bit for bit: the definition the
    sensitivity facts perturb is the one the GPU test compares against."""
    s = ac.scene(name)
    got = oracle_records(O, name, "identity")
    for cls in (0, 1):
        want = ac.records(s, cls)
        assert np.array_equal(want[0], got[cls][0]) and not ac.changed(want, got[cls]).any(), (name, cls)


@pytest.mark.parametrize("name", ALL)
def test_which_kernel_owns_each_last_cloud(name):
    s = ac.scene(name)
    assert s.order == ORDERS[name], (name, s.order)
    for cls, cloud in enumerate((s.less_sharp, s.less_flat)):
        k = ac.keys_of(cloud)
        if s.order[cls] == 0:
            assert not (np.diff(k) < 0).any()
        else:
            assert (np.maximum.accumulate(k) - k).max() == (1 if s.order[cls] == 1 else 3)      # lowered by 1: nearly sorted; by 3: the literal walks
    fused = [len(c) <= ac.FUSED_MAX_N and ac.grid_H(cls, s.n_scans, s.max_points) <= ac.FUSED_MAX_H for cls, c in enumerate((s.less_sharp, s.less_flat))]
    assert fused == [True, name != "S6-65536"]


@pytest.mark.parametrize("pose_name", sorted(ac.POSES))
@pytest.mark.parametrize("name", ALL)
def test_caps_and_expectations(O, name, pose_name):
    """At least 20 valid and 5 invalid records per class (classes of 0 or 1 queries and the empty scene aside), every query tagged with its purpose, and
    every expectation a scene states about a query met by the oracle - at the rotated pose too, the deliberately exact queries aside."""
    s = ac.scene(name)
    got = oracle_records(O, name, pose_name)
    for cls, (tags, expect, exact) in enumerate(((s.tags_sharp, s.expect_sharp, s.exact_sharp), (s.tags_flat, s.expect_flat, s.exact_flat))):
        valid = got[cls][0]
        assert len(tags) == len(valid) and all(tags)
        if len(valid) > 1:
            assert valid.sum() >= 20 and (~valid).sum() >= 5, (name, pose_name, cls, int(valid.sum()), int((~valid).sum()))
        for i, want in enumerate(expect):
            if want is not None and not (pose_name == "rotated" and exact[i]):
                assert bool(valid[i]) == want, (name, pose_name, cls, i, tags[i])


SENSITIVE = ("S1", "S3", "S4", "S5", "S8")


@pytest.mark.parametrize("name", SENSITIVE)
def test_sensitivity_to_the_plausible_mistakes(name):
    """Each mistake a scene names, made in the DEFINITION, changes at least the stated number of records per class; together the scenes name all four."""
    s = ac.scene(name)
    assert s.sensitivity and {m for n in SENSITIVE for m in ac.scene(n).sensitivity} == set(ac.MISTAKES)
    for mistake, least in s.sensitivity.items():
        for cls in (0, 1):
            n = int(ac.changed(ac.records(s, cls), ac.records(s, cls, **ac.MISTAKES[mistake])).sum())
            print(f"{name} class {cls} mistake {mistake}: {n} records change (stated: at least {least[cls]})")
            assert n >= least[cls], (name, mistake, cls, n)


# ---- path facts -----------------------------------------------------------------------------------------------------------------------------------------
def _tagged(s, cls, tag):
    tags = (s.tags_sharp, s.tags_flat)[cls]
    return [i for i, t in enumerate(tags) if t == tag]


@pytest.mark.parametrize("name,tag", [("S1", "dense"), ("S8", "dense"), ("S2a", "dense-half"), ("S2b", "dense-half"), ("S1-lowered1", "dense"), ("S1-lowered3", "dense")])
def test_dense_block_needs_more_than_three_rounds(name, tag):
    """kept.ok == false, base > 0 and carries across rounds: the query's 3x3x3 fine block holds more than 3 x kRows x 32 candidates, its buckets (hash
    collisions included: there are none) are exactly block_pattern's - empty cells, cells of one entry, runs that end on row and on round borders."""
    s = ac.scene(name)
    for cls in (0, 1):
        rows = ac.pair_rows(cls, s.n_scans)
        last, qs = (s.less_sharp, s.less_flat)[cls], (s.sharp, s.flat)[cls]
        H = ac.grid_H(cls, s.n_scans, s.max_points)
        idx = _tagged(s, cls, tag)
        assert idx or name.startswith("S2")
        for i in idx:
            assert ac.fine_block_members(qs[i], last, cls) > 3 * rows * 32
            cnt = ac.fine_block_counts(qs[i], last, cls, H)
            assert cnt == ac.block_pattern(rows), (name, cls, i)
            cum = np.cumsum(cnt)
            assert {rows * 32, 2 * rows * 32, 3 * rows * 32} <= set(cum.tolist()) and cum[-1] > 3 * rows * 32
            assert 0 in cnt and 1 in cnt and any(c % 32 == 0 and c % (rows * 32) for c in cum.tolist())
        if idx:
            # the ring grid behind it: the second / third neighbours come from buckets longer than one round of the tails (kRows1 x 32 per half)
            i, r = next((i, r) for i in idx for r in [ac.define(qs[i, :3], last, bool(cls))] if r is not None)
            cand = ac.class_candidates(qs[i, :3], last, r[0], bool(cls))
            print(f"{name} class {cls}: {ac.fine_block_members(qs[i], last, cls)} candidates in the fine block = {ac.fine_block_members(qs[i], last, cls) / (rows * 32):.2f} rounds of {rows * 32}; "
                  f"ring-window candidates {len(cand[2])} / {len(cand[3])}; largest buckets (fine, coarse, ring) {ac.largest_bucket(last, cls, H)}")
            assert len(cand[2]) > ((rows + 1) // 2) * 32


@pytest.mark.parametrize("variant", ["a", "b"])
def test_s2_pairs_are_unequal(variant):
    s = ac.scene("S2" + variant)
    mix = 0 if variant == "a" else 1
    tags, qs, last = (s.tags_sharp, s.tags_flat)[mix], (s.sharp, s.flat)[mix], (s.less_sharp, s.less_flat)[mix]
    pairs = {(tags[i], tags[i + 1]) for i in range(0, len(tags) - 1, 2)}
    assert {("dense-half", "alone-half"), ("alone-half", "dense-half"), ("dense-half", "has1-false"), ("has1-false", "dense-half"), ("alone-half", "has1-false"),
            ("has1-false", "alone-half")} <= pairs
    assert len(tags) % 2 == 1 and tags[-1] == "dense-half"                    # the last wave: a dense first half, an inactive second
    assert len((s.sharp, s.flat)[1 - mix]) == (1 if variant == "a" else 0)
    for i, t in enumerate(tags):
        d = ac.dist2(last, qs[i])
        if t == "has1-false":
            assert d.min() > 50.0 ** 2
        if t == "alone-half":
            assert ac.fine_block_members(qs[i], last, mix) == (3 if mix else 2) and d.min() < ac.fine_bound2(qs[i], mix)


def test_s3_nearest_point_lies_outside_the_fine_block():
    s = ac.scene("S3")
    for cls in (0, 1):
        tags, qs, last = (s.tags_sharp, s.tags_flat)[cls], (s.sharp, s.flat)[cls], (s.less_sharp, s.less_flat)[cls]
        need = []
        for i, t in enumerate(tags):
            d = ac.dist2(last, qs[i])
            need.append(bool(d.min() > ac.fine_bound2(qs[i], cls)))
            if t in ("shells-both", "shells-one"):
                assert need[-1] and d.min() < F(25.0), (cls, i)
            elif t == "near-beside-shells":
                assert not need[-1]
            elif t == "beyond-5m":
                assert d.min() > F(27.0)
            elif t == "d2-exactly-25":
                assert np.all(qs[i, :3] == np.round(qs[i, :3])) and (d == F(25.0)).sum() == 3 and d.min() == F(25.0)
            elif t == "d2-one-ulp-below-25":
                assert (d == np.nextafter(F(25.0), F(0.0))).sum() == 3 and d.min() == np.nextafter(F(25.0), F(0.0))
        kinds = [(need[i], need[i + 1]) for i in range(0, len(need) - 1, 2)]
        assert kinds.count((True, True)) >= 4 and kinds.count((True, False)) >= 3 and kinds.count((False, True)) >= 3      # paired and single coarse-shell tails
        far = sorted(float(np.sqrt(ac.dist2(last, qs[i]).min())) for i, t in enumerate(tags) if t.startswith("shells"))
        assert far[0] < 1.21 and any(2.9 < x < 3.1 for x in far) and far[-1] > 4.98


def test_s4_ring_window_stages():
    s = ac.scene("S4")
    for cls in (0, 1):
        tags, qs, last = (s.tags_sharp, s.tags_flat)[cls], (s.sharp, s.flat)[cls], (s.less_sharp, s.less_flat)[cls]
        k = ac.keys_of(last)
        seen = set()
        for i, t in enumerate(tags):
            sel = qs[i, :3]
            closest = int(np.argmin(ac.dist2(last, sel)))
            cand = ac.class_candidates(sel, last, closest, bool(cls))
            classes = (2, 3) if cls else (2,)
            if t == "ring-5x5-decides":                   # no candidate of either class inside the 3x3 ring cells, one inside the 5x5
                for c in classes:
                    off = ac.ring_cell_offsets(sel, last[cand[c]])
                    assert len(off) and off.min() == 2 and off.max() == 2, (cls, i, c, off)
                    lim = np.abs(last[cand[c], :2] - sel[:2]).max(axis=1)
                    assert np.all((lim > 2.625) & (lim < 5.0))
            elif t == "second-beyond-5m":
                assert any(len(cand[c]) == 0 for c in classes)
                assert ((np.abs(k - k[closest]) <= 2) & (ac.dist2(last, sel) < F(40.0))).sum() > 1      # it exists, beyond 5 m
            elif t == "ring+-2-taken":
                dk = k - k[closest]
                c23 = cand[3] if cls else cand[2]
                assert set(np.abs(dk[c23]).tolist()) == {2}
                d = ac.dist2(last, sel)
                assert d[np.abs(dk) == 3].min() < d[c23].min()                                          # the refused ring is the nearer one
                seen.add(int(dk[c23][0]))
            elif t == "ring+-3-refused":
                assert len(cand[3] if cls else cand[2]) == 0 and (np.abs(k - k[closest]) == 3).any()
            elif t == "same-ring-only":
                assert len(cand[2]) == 1 and len(cand[3]) == 0
            elif t == "other-ring-only":
                assert len(cand[2]) == 0 and len(cand[3]) == 1
            elif t in ("ring-0", "ring-15"):
                assert k[closest] == (0 if t == "ring-0" else 15)
        assert seen == {-2, 2}


def test_s5_ties_and_borders():
    s = ac.scene("S5")
    for cls in (0, 1):
        qs, last = (s.sharp, s.flat)[cls], (s.less_sharp, s.less_flat)[cls]
        ties1 = ties2 = 0
        for q in qs:
            d = ac.dist2(last, q)
            ties1 += int((d == d.min()).sum() > 1)
            r = ac.define(q[:3], last, bool(cls))
            if r is not None:
                ties2 += int((d == d[r[1]]).sum() > 2)
        assert ties1 >= 60 and ties2 >= 40, (cls, ties1, ties2)                 # exact 1-NN ties / ties at the second neighbour's distance
        both = np.concatenate([last[:, :3], qs[:, :3]]).astype(np.float64)
        for border in (0.5, 0.75, 2.0, 3.0, 2.625):
            on = (both != 0) & (np.mod(both, border) == 0)
            assert (on & (both > 0)).any() and (on & (both < 0)).any(), border
        xyz = last[:, :3]
        uniq = np.unique(xyz, axis=0)
        assert len(uniq) < len(xyz) - 20                                        # duplicate points under different indices
        assert (last[:, 0] == F(4095.5)).sum() == 8 and np.abs(last[:, :3]).max() < 4096.0


@pytest.mark.parametrize("n", [65535, 65536])
def test_s6_build_limits(n):
    s = ac.scene(f"S6-{n}")
    assert len(s.less_flat) == n and s.max_points <= 160000
    H = ac.grid_H(1, 16, s.max_points)
    big = ac.largest_bucket(s.less_flat, 1, H)
    print(f"S6-{n}: largest buckets (fine, coarse, ring) {big}")
    assert big[0] > 30000 and big[1] > 60000                                    # tens of thousands of entries on the 16-bit counters
    cell = ac.cells(s.less_flat[:, :3], 0.5)
    in_two = np.all(cell == (8, 8, 1), axis=1) | np.all(cell == (9, 8, 1), axis=1)
    assert 200 < (~in_two).sum() < 400
    assert len(s.flat) <= 48
