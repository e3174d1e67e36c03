"""CPU proof of the rings in selection_cases.py: what each forces in pick_sector and the second pass of k_ring_features, and which
mistake it would catch.  For every scene
  (i)   the oracle's labels equal the reference's literal walk (selection_model.literal) over the oracle's own curvature and gaps, and the
        instrumented scheme (selection_cases.run) and the model of test_selection_model.py give the same picks;
  (ii)  facts() shows the forced path with exact counts (FACTS, and the scene-specific tests below);
  (iii) every mutant aimed at the scene changes an exact number of labels (MUTANT_EFFECT; for p: of curvature values);
  (iv)  every squared step is at least 0.01 away from 0.05, and except in C9 every curvature is an exact multiple of 2^-8 below 2^16, the
        same summed forwards and backwards, and none lies in [0.05, 0.2].
The figures in FACTS and MUTANT_EFFECT were computed once from the rings and are asserted with ==: a changed builder, model or oracle shows.
test_census_of_the_sensor_shaped_sweeps prints how often the same paths occur in the sweeps test_gpu_parity.py runs (recorded in
DESIGN.md, not asserted)."""
import numpy as np
import pytest

import selection_cases as sc
from selection_model import THR, literal, model, pick_sector_regs

# redone sectors, redone only because the sector in front was redone, sectors with incoming marks, sectors that pass marks on (shorter than 5),
# corners, flats, kills into register kr - 1, into kr + 1, corner / flat picks tied over lanes, corner / flat picks tied over registers of a lane
FACTS = {
    "C1_redo": (5, 0, 5, 0, 6, 7, 0, 0, 0, 7, 0, 0),
    "C2_chain": (5, 2, 5, 0, 3, 4, 0, 0, 0, 3, 0, 0),
    "C2_stop": (3, 0, 4, 0, 1, 7, 0, 0, 0, 6, 0, 0),
    "C3_flat_17": (5, 0, 5, 4, 0, 1, 0, 0, 0, 0, 0, 0),
    "C3_flat_18": (5, 0, 5, 4, 0, 2, 0, 0, 0, 0, 0, 0),
    "C3_flat_22": (5, 0, 5, 4, 0, 2, 0, 0, 0, 0, 0, 0),
    "C3_flat_23": (4, 0, 4, 2, 0, 2, 0, 0, 0, 2, 0, 0),
    "C3_flat_28": (5, 0, 5, 3, 0, 3, 0, 0, 0, 3, 0, 0),
    "C3_flat_35": (4, 0, 4, 0, 0, 4, 0, 0, 0, 4, 0, 0),
    "C3_flat_40": (4, 0, 4, 0, 0, 5, 0, 0, 0, 4, 0, 0),
    "C3_gaps_17": (4, 0, 4, 4, 2, 0, 0, 0, 0, 0, 0, 0),
    "C3_gaps_18": (4, 0, 5, 4, 2, 0, 0, 0, 0, 0, 0, 0),
    "C3_gaps_22": (4, 0, 5, 2, 3, 0, 0, 0, 0, 0, 0, 0),
    "C3_gaps_23": (5, 0, 5, 3, 3, 0, 0, 0, 0, 0, 0, 0),
    "C3_gaps_28": (4, 0, 4, 2, 3, 2, 0, 0, 1, 0, 0, 0),
    "C3_gaps_35": (5, 0, 5, 2, 3, 2, 0, 0, 0, 1, 0, 0),
    "C3_gaps_40": (4, 0, 4, 0, 2, 4, 0, 0, 0, 2, 0, 0),
    "C3_none_16": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "C4_corner_lanes": (0, 0, 0, 0, 18, 24, 0, 0, 12, 24, 0, 6),
    "C4_corner_regs": (0, 0, 5, 0, 18, 24, 6, 0, 12, 24, 6, 0),
    "C4_corner_both": (0, 0, 5, 0, 24, 24, 6, 0, 18, 24, 6, 0),
    "C4_corner_border": (0, 0, 0, 0, 12, 24, 6, 0, 12, 24, 0, 0),
    "C4_flat_lanes": (0, 0, 5, 0, 6, 24, 6, 0, 0, 24, 0, 0),
    "C4_flat_both": (0, 0, 0, 0, 6, 24, 0, 0, 0, 24, 0, 6),
    "C4_flat_border": (5, 0, 5, 0, 31, 17, 0, 6, 25, 11, 0, 4),
    "C4_flat_regs": (5, 0, 5, 0, 73, 24, 6, 0, 44, 12, 2, 6),
    "C5_borders": (0, 0, 4, 0, 30, 24, 10, 10, 20, 24, 20, 24),
    "C5_victims": (0, 0, 0, 0, 6, 24, 3, 3, 1, 24, 0, 24),
    "C5_gaps": (1, 0, 1, 0, 87, 24, 4, 5, 54, 24, 2, 24),
    "C6_end": (3, 0, 3, 0, 44, 2, 0, 0, 11, 1, 0, 0),
    "C6_isolated": (0, 0, 0, 0, 120, 0, 0, 0, 120, 0, 0, 0),
    "C6_twenty": (1, 0, 1, 0, 110, 6, 0, 0, 22, 0, 0, 0),
    "C6_fourth": (0, 0, 0, 0, 0, 24, 0, 0, 0, 18, 0, 0),
    "C6_one": (2, 1, 2, 0, 1, 20, 0, 0, 0, 17, 0, 0),
    "C7_window_0": (2, 0, 2, 0, 29, 24, 0, 0, 11, 24, 0, 0),
    "C7_window_1": (0, 0, 0, 0, 29, 24, 0, 0, 3, 24, 0, 0),
    "C7_window_2": (2, 0, 2, 0, 28, 24, 0, 0, 4, 23, 0, 0),
    "C7_window_3": (4, 0, 4, 0, 32, 21, 0, 0, 4, 21, 0, 0),
    "C8_17": (5, 0, 5, 4, 0, 1, 0, 0, 0, 0, 0, 0),
    "C8_18": (5, 0, 5, 4, 0, 2, 0, 0, 0, 0, 0, 0),
    "C8_22": (5, 0, 5, 4, 0, 2, 0, 0, 0, 0, 0, 0),
    "C8_256": (0, 0, 0, 0, 3, 24, 0, 0, 1, 24, 0, 0),
    "C8_261": (0, 0, 1, 0, 5, 24, 0, 0, 0, 24, 0, 0),
    "C8_262": (0, 0, 0, 0, 2, 24, 0, 0, 0, 24, 0, 0),
    "C8_266": (0, 0, 1, 0, 9, 24, 0, 0, 3, 22, 0, 0),
    "C8_267": (0, 0, 1, 0, 7, 24, 0, 0, 0, 23, 0, 0),
    "C8_272": (0, 0, 0, 0, 8, 24, 0, 0, 2, 24, 0, 0),
    "C8_512": (0, 0, 0, 0, 10, 24, 1, 0, 5, 24, 0, 19),
    "C8_517": (1, 0, 2, 0, 10, 24, 1, 0, 2, 24, 0, 17),
    "C8_523": (0, 0, 2, 0, 10, 24, 1, 0, 3, 24, 0, 18),
    "C8_1029": (0, 0, 1, 0, 33, 24, 3, 1, 19, 24, 0, 24),
    "C8_2059": (0, 0, 1, 0, 61, 24, 1, 6, 46, 24, 4, 24),
    "C9_threshold": (5, 0, 5, 0, 8, 12, 0, 0, 0, 7, 0, 0),
    "C10_long_4107": (0, 0, 0, 0, 99, 24, 26, 26, 42, 24, 75, 24),
    "C10_2060": (0, 0, 0, 0, 118, 24, 2, 9, 73, 24, 1, 24),
}
AIMED = {"C1": "a", "C2": "ab", "C3": "abcdl", "C4": "efgh", "C5": "eghi", "C6": "aejkl", "C7": "lm", "C8": "p", "C9": "o", "C10": "eghimn"}
MUTANT_EFFECT = {
    "C1_redo": {'a': 10},
    "C2_chain": {'a': 10, 'b': 6},
    "C2_stop": {'a': 9, 'b': 4},
    "C3_flat_17": {'a': 5, 'b': 0, 'c': 2, 'd': 0, 'l': 0},
    "C3_flat_18": {'a': 6, 'b': 1, 'c': 3, 'd': 0, 'l': 0},
    "C3_flat_22": {'a': 6, 'b': 1, 'c': 3, 'd': 0, 'l': 0},
    "C3_flat_23": {'a': 4, 'b': 1, 'c': 3, 'd': 0, 'l': 0},
    "C3_flat_28": {'a': 7, 'b': 2, 'c': 4, 'd': 0, 'l': 0},
    "C3_flat_35": {'a': 6, 'b': 4, 'c': 0, 'd': 0, 'l': 0},
    "C3_flat_40": {'a': 7, 'b': 7, 'c': 0, 'd': 0, 'l': 0},
    "C3_gaps_17": {'a': 4, 'b': 0, 'c': 2, 'd': 0, 'l': 1},
    "C3_gaps_18": {'a': 4, 'b': 1, 'c': 3, 'd': 0, 'l': 0},
    "C3_gaps_22": {'a': 4, 'b': 1, 'c': 3, 'd': 0, 'l': 3},
    "C3_gaps_23": {'a': 6, 'b': 1, 'c': 3, 'd': 0, 'l': 3},
    "C3_gaps_28": {'a': 6, 'b': 2, 'c': 4, 'd': 0, 'l': 6},
    "C3_gaps_35": {'a': 8, 'b': 5, 'c': 4, 'd': 0, 'l': 7},
    "C3_gaps_40": {'a': 7, 'b': 5, 'c': 0, 'd': 0, 'l': 9},
    "C3_none_16": {'a': 0, 'b': 0, 'c': 0, 'd': 0, 'l': 0},
    "C4_corner_lanes": {'e': 12, 'f': 48, 'g': 12, 'h': 0},
    "C4_corner_regs": {'e': 12, 'f': 48, 'g': 12, 'h': 0},
    "C4_corner_both": {'e': 24, 'f': 48, 'g': 12, 'h': 0},
    "C4_corner_border": {'e': 24, 'f': 48, 'g': 0, 'h': 12},
    "C4_flat_lanes": {'e': 0, 'f': 48, 'g': 0, 'h': 0},
    "C4_flat_both": {'e': 0, 'f': 48, 'g': 12, 'h': 0},
    "C4_flat_border": {'e': 24, 'f': 25, 'g': 8, 'h': 22},
    "C4_flat_regs": {'e': 4, 'f': 12, 'g': 16, 'h': 12},
    "C5_borders": {'e': 20, 'g': 54, 'h': 0, 'i': 0},
    "C5_victims": {'e': 0, 'g': 26, 'h': 6, 'i': 6},
    "C5_gaps": {'e': 8, 'g': 36, 'h': 9, 'i': 2},
    "C6_end": {'a': 4, 'e': 6, 'j': 0, 'k': 0, 'l': 13},
    "C6_isolated": {'a': 0, 'e': 120, 'j': 0, 'k': 0, 'l': 0},
    "C6_twenty": {'a': 1, 'e': 10, 'j': 0, 'k': 1, 'l': 19},
    "C6_fourth": {'a': 0, 'e': 0, 'j': 35, 'k': 0, 'l': 0},
    "C6_one": {'a': 14, 'e': 0, 'j': 8, 'k': 0, 'l': 0},
    "C7_window_0": {'l': 10, 'm': 34},
    "C7_window_1": {'l': 11, 'm': 33},
    "C7_window_2": {'l': 6, 'm': 44},
    "C7_window_3": {'l': 8, 'm': 52},
    "C8_17": {'p': 0},
    "C8_18": {'p': 0},
    "C8_22": {'p': 0},
    "C8_256": {'p': 0},
    "C8_261": {'p': 0},
    "C8_262": {'p': 1},
    "C8_266": {'p': 1},
    "C8_267": {'p': 1},
    "C8_272": {'p': 1},
    "C8_512": {'p': 1},
    "C8_517": {'p': 1},
    "C8_523": {'p': 2},
    "C8_1029": {'p': 3},
    "C8_2059": {'p': 8},
    "C9_threshold": {'o': 1},
    "C10_long_4107": {'e': 16, 'g': 64, 'h': 2, 'i': 2, 'm': 8, 'n': 2},
    "C10_2060": {'e': 22, 'g': 46, 'h': 10, 'i': 0, 'm': 88, 'n': 0},
}
NAMES = list(sc.scenes())


def _interior(f):
    n = len(f["curv"])
    return f["curv"][5:n - 5]


def test_every_scene_is_listed():
    assert set(NAMES) == set(FACTS) == set(MUTANT_EFFECT)
    assert all(set(MUTANT_EFFECT[k]) == set(AIMED[k.split("_")[0]]) for k in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_labels_equal_the_literal_walk(O, name):
    f = sc.scene_facts(O, name)
    n = len(f["curv"])
    assert sc.curvature_f32(f["xyz"]).view(np.uint32).tolist() == f["curv"].view(np.uint32).tolist()          # the oracle's stencil, re-done in numpy f32
    if n - 11 < 6:
        assert not f["labels"].any()
        return
    la, pa = literal(f["curv"], f["gap"], n)
    assert np.array_equal(la, f["labels"]), name
    assert np.array_equal(la, f["model_labels"]) and pa == f["picks"], name
    K = sc.K6_4096 if n > 2059 else sc.K6_2048
    lb, pb = model(f["curv"], f["gap"], n, lambda j, m, L, c, r: pick_sector_regs(j, m, L, c, r, spare=K - ((L * (j + 1)) // 6 - (L * j) // 6 + 63) // 64))
    assert np.array_equal(la, lb) and pa == pb, name


@pytest.mark.parametrize("name", NAMES)
def test_scene_forces_its_path(O, name):
    t = sc.scene_facts(O, name)["total"]
    got = (t["redone"], t["redo_after_redo"], t["hit_sectors"], t["carried"], t["corners"], t["flats"], t["prev_kills"], t["next_kills"],
           t["lane_ties"]["corner"], t["lane_ties"]["flat"], t["reg_ties"]["corner"], t["reg_ties"]["flat"])
    print(name, got)
    assert got == FACTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_mutants_change_an_exact_number_of_labels(O, name):
    f = sc.scene_facts(O, name)
    got = {m: sc.mutant_effect(f, m) for m in AIMED[name.split("_")[0]]}
    print(name, got)
    assert got == MUTANT_EFFECT[name]


def test_every_mutant_is_caught_by_a_scene_built_for_it():
    caught = {m: [k for k in NAMES if MUTANT_EFFECT[k].get(m)] for m in sc.MUTANTS}
    assert caught.pop("d") == []                                  # equivalent: the hit test and the initial marks only look at positions < len
    assert all(caught.values()), caught
    for fam, muts in AIMED.items():                               # ... and every family catches what is aimed at it
        for m in muts:
            assert m == "d" or any(MUTANT_EFFECT[k][m] for k in NAMES if k.split("_")[0] == fam), (fam, m)


@pytest.mark.parametrize("name", NAMES)
def test_margins(O, name):
    f = sc.scene_facts(O, name)
    s2 = sc.steps2(f["xyz"]).astype(np.float64)
    assert np.abs(s2 - 0.05).min() >= 0.01
    c = _interior(f).astype(np.float64)
    if name.startswith("C9"):
        assert sorted(c[(c >= 0.05) & (c <= 0.2)].astype(np.float32).view(np.uint32).tolist()) == list(sc.C9_BITS)
        return
    assert np.array_equal(c * 256, np.rint(c * 256)) and c.max() < 65536                                        # exact in f32, with room
    rev = sc.curvature_f32(f["xyz"][::-1])[::-1]                                                               # the sums in reverse order
    assert np.array_equal(rev.view(np.uint32), f["curv"].view(np.uint32))
    x = f["xyz"].astype(np.float64)
    c64 = np.array([((x[i - 5:i + 6].sum(0) - 11 * x[i]) ** 2).sum() for i in range(5, len(x) - 5)])           # f64 curvature
    assert np.array_equal(c64, c)
    assert not ((c >= 0.05) & (c <= 0.2)).any()


# ---- scene-specific paths
def test_c1_every_sector_behind_the_first_is_redone(O):
    s = sc.scene_facts(O, "C1_redo")["sectors"]
    assert [x["redone"] for x in s] == [False] + [True] * 5 and [x["marks"] for x in s] == [0] + [15] * 5
    assert all(len(x["first"][0]) == 2 and len(x["final"][0]) == 1 for x in s[1:])             # the marked second corner is gone


def test_c2_redo_chains(O):
    f = sc.scene_facts(O, "C2_chain")
    _, _, wrong = sc.run(f["curv"], f["gap"], 59, mut="b")
    assert [x["redone"] for x in f["sectors"]] == [False, True, True, True, True, True]
    assert [x["redone"] for x in wrong] == [False, True, True, False, False, True]             # sectors 3 and 4 hang on the post-redo spill of 2 and 3
    f = sc.scene_facts(O, "C2_stop")
    _, _, wrong = sc.run(f["curv"], f["gap"], 59, mut="b")
    assert [x["redone"] for x in f["sectors"]] == [False, True, True, False, False, True]
    assert [x["redone"] for x in wrong][3] and f["sectors"][2]["first_spill"] != f["sectors"][2]["spill"]   # sector 3 must NOT be redone


def test_c3_marks_cross_whole_sectors(O):
    carried = {n: [x["carried"] for x in sc.scene_facts(O, "C3_flat_%d" % n)["sectors"]] for n in sc.C3_LENGTHS}
    assert carried[17] == [0, 15, 7, 3, 1, 0] and carried[18] == [0, 15, 7, 3, 1, 0]           # one-point sectors: the pick of sector 0 reaches sector 5
    assert carried[22] == [0, 7, 1, 0, 7, 1] and carried[23] == [0, 3, 0, 0, 3, 0]             # across three and two sectors
    assert carried[28] == [0, 1, 0, 1, 0, 1] and carried[35] == carried[40] == [0] * 6
    assert [x["len"] for x in sc.scene_facts(O, "C3_flat_17")["sectors"]] == [1] * 6
    f = sc.scene_facts(O, "C3_none_16")
    assert f["sectors"] == [] and not f["labels"].any() and _interior(f).max() > 1             # a corner candidate, but L = 5: not looked at


def test_c4_fourth_flat_decided_between_registers_of_one_lane(O):
    for s in sc.scene_facts(O, "C4_flat_regs")["sectors"]:
        flats = [e for e in s["picks"] if e["kind"] == "flat"]
        assert [e["pos"] for e in flats] == [20, 30, 40, 3] and (flats[3]["tie_lanes"], flats[3]["tie_regs"]) == (1, 2)
    only_regs = {k: sum(1 for s in sc.scene_facts(O, k)["sectors"] for e in s["picks"] if e["kind"] == "corner" and e["tie_lanes"] == 1 and e["tie_regs"] > 1)
                 for k in ("C5_borders", "C10_long_4107")}
    assert only_regs == {"C5_borders": 4, "C10_long_4107": 38}                                 # corners: the same, without any other lane tied


def test_c5_c10_picks_by_register_and_lane_class(O):
    b = sc.scene_facts(O, "C5_borders")["total"]
    assert {k: v for k, v in b["by_reg_lane"].items() if k[1] != "mid"} == {(0, "lo"): 6, (0, "hi"): 5, (1, "lo"): 5, (1, "hi"): 5, (2, "lo"): 5, (2, "hi"): 5}
    assert b["reach"] == {(5, 5): 48}
    g = sc.scene_facts(O, "C5_gaps")
    cut = [e for s in g["sectors"] for e in s["picks"] if (e["prev"] or e["next"]) and (e["fw"], e["bk"]) != (5, 5)]
    assert len(cut) == 8                                                                        # kills that leave lanes 0 .. 63 with a reach cut by a gap
    t = sc.scene_facts(O, "C10_long_4107")["total"]
    want = {(kr, c): 5 for kr in (0, 3, 4, 7, 8) for c in ("lo", "hi")}
    want.update({(0, "lo"): 6, (10, "lo"): 5, (9, "lo"): 1, (9, "hi"): 1})
    assert {k: v for k, v in t["by_reg_lane"].items() if k[1] != "mid"} == want
    assert {k: v for k, v in t["by_reg_lane"].items() if k[1] == "mid"} == {(0, "mid"): 29, (3, "mid"): 6, (4, "mid"): 8, (6, "mid"): 4, (7, "mid"): 6, (8, "mid"): 6, (10, "mid"): 6}
    assert sc.scene_facts(O, "C10_2060")["sectors"][0]["len"] == 341                            # 6 registers would hold 384; n = 2060 is the first length of the <4096> instance


def test_c6_sector_ends_and_counts(O):
    f = sc.scene_facts(O, "C6_end")
    assert sorted(set(e["fw"] for s in f["sectors"] for e in s["picks"] if e["fw"] is not None and e["pos"] + 5 >= s["len"])) == [0, 1, 2, 3, 4, 5]
    f = sc.scene_facts(O, "C6_isolated")
    assert [len(s["final"][0]) for s in f["sectors"]] == [20] * 6 and [s["len"] for s in f["sectors"]] == [30] * 6 and f["total"]["reach"] == {(0, 0): 120}
    assert (_interior(f)[:180] > 0.1).all() and (f["labels"] == 0).sum() == 191 - 120          # the ten behind the 20th: unmarked, and no flats
    f = sc.scene_facts(O, "C6_twenty")
    assert [len(s["final"][0]) for s in f["sectors"]] == [19, 20, 18, 20, 18, 15]
    f = sc.scene_facts(O, "C6_fourth")
    assert all([p - 5 - 19 * j for p in s["final"][1]] == [0, 6, 12, 18] and not s["spill"] for j, s in enumerate(f["sectors"]))
    f = sc.scene_facts(O, "C6_one")
    assert [len(s["final"][0]) for s in f["sectors"]] == [0, 0, 1, 0, 0, 0]


def test_c7_every_reach_is_picked_where_the_window_leaves_its_word(O):
    seen = set()
    for q in range(4):
        f = sc.scene_facts(O, "C7_window_%d" % q)
        got = {5 + (319 * e["sector"]) // 6 + e["pos"]: (e["kind"], e["fw"], e["bk"]) for s in f["sectors"] for e in s["picks"]}
        for P, fw, bk in sc.c7_points(q):
            assert (P + 59) & 31 > 22 and got[P] == ("corner", fw, bk), (q, P)
            seen.add((fw, bk, (P + 59) & 63 > 54))
        assert got[5] == ("flat", 5, 5) and got[323] == ("corner", 5, 5)                        # first and last point a ring can pick
    assert {(fw, bk) for fw, bk, _ in seen} == {(fw, bk) for fw in range(6) for bk in range(6)}
    assert sum(1 for s in seen if s[2]) == 16                                                   # of them across a 64-bit border of the gap words


def test_c9_three_curvatures_around_the_threshold(O):
    f = sc.scene_facts(O, "C9_threshold")
    assert [int(f["curv"][i].view(np.uint32)) for i in sc.C9_INDEX] == [THR - 1, THR, THR + 1] == [0x3DCCCCCC, 0x3DCCCCCD, 0x3DCCCCCE]
    assert [int(f["labels"][i]) for i in sc.C9_INDEX] == [-1, 1, 1]
    picks = {5 + 15 * e["sector"] + e["pos"]: (e["fw"], e["bk"]) for s in f["sectors"] for e in s["picks"]}
    assert all(picks[i] in ((0, 0), (None, None)) for i in sc.C9_INDEX)


def test_sweeps_hold_every_scene(O):
    short, long_ = sc.sweeps(False), sc.sweeps(True)
    assert sorted(k for _, names in short for k in names) == sorted(k for k in NAMES if k not in sc.LONG)
    assert {k for _, names in long_ for k in names if k} == {k for k in NAMES if k in sc.LONG or k.startswith(sc.AGAIN_4096)} | {"C3_none_16", "C3_flat_17", "C3_gaps_22", "C3_flat_18"}
    assert max(len(x) for x, _ in short) <= 8 * 2059 and long_[-1][1][2] is None and long_[-1][1][5] is None


def test_instrumented_scheme_equals_the_model_on_random_rings():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.choice([17, 23, 41, 90, 150, 400, 900]))
        curv = np.round(rng.exponential(0.3, n), 1).astype(np.float32) if trial % 2 else rng.exponential(0.2, n).astype(np.float32)
        gap = rng.random(n) < rng.choice([0.0, 0.05, 0.3, 0.8])
        la, pa = literal(curv, gap, n)
        lb, pb, _ = sc.run(curv, gap, n)
        assert np.array_equal(la, lb) and pa == pb, (trial, n)


CENSUS = [("VLP-16", {}), ("HDL-64", {}), ("HDL-64", {"rough": True})]


def test_census_of_the_sensor_shaped_sweeps(O, sequence):
    """the same facts over the first sweep of three of test_free_running_sequence_matches_oracle's sequences: printed (pytest -s), recorded in
    DESIGN.md, and only the agreement of the scheme with the oracle's labels is asserted"""
    keys = ("rings", "redone", "redo_after_redo", "carried", "prev_kills", "next_kills", "corner lane ties", "corner reg ties", "flat lane ties", "flat reg ties", "picks kr>=8", "short sectors")
    for name, kw in CENSUS:
        scans, _, _, m = sequence(name, 4, seed=1, **kw)
        orc = O.Oracle(n_scans=m.n_scans, min_range=m.min_range, ring_from_field=m.ring_from_field)
        fo = orc.scan_register(scans[0])
        curv, lab, _ = orc.per_point()
        tot = dict.fromkeys(keys, 0)
        reach = set()
        for s0, c0 in zip(*orc.ring_ranges()):
            if c0 - 11 < 6: continue
            f = sc.facts_of(fo["cloud"][s0:s0 + c0, :3], curv[s0:s0 + c0], lab[s0:s0 + c0])
            sel = slice(5, c0 - 6)
            assert np.array_equal(f["model_labels"][sel], lab[s0:s0 + c0][sel]), (name, s0)
            t = f["total"]
            tot["rings"] += 1
            for k in ("redone", "redo_after_redo", "carried", "prev_kills", "next_kills"): tot[k] += t[k]
            for k in ("corner", "flat"): tot[k + " lane ties"] += t["lane_ties"][k]; tot[k + " reg ties"] += t["reg_ties"][k]
            tot["picks kr>=8"] += sum(v for (kr, _), v in t["by_reg_lane"].items() if kr >= 8)
            tot["short sectors"] += sum(1 for s in f["sectors"] if s["len"] < 5)
            reach |= set(t["reach"])
        print("census", name, kw, tot, "reach pairs", len(reach))
