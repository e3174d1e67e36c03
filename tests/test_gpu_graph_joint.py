"""Joined pose graphs on the MI355X (aloam_graph_optimize_joint, aloam_graph_optimize_joint_robust, aloam_graph_joint_export)
against posegraph.join / align_member / split / optimize_joint fed what the device exports: the bytes of gather, alignment and write-back,
the one-member group against the per-sequence solves, the joint solve of a cut drive against the model and against the uncut drive, the
independence of a group from its call, the robust solve with false links, every refusal, and the existing calls on a joined member.

Graphs are entered through posegraph_cases.enter (aloam_set_state + aloam_graph_add_nodes) and aloam_graph_add_edges.  Tolerance for poses
and cost: 8 eps_ref, as test_gpu_posegraph.py.  Every comparison prints the device's figures.  The refusal test's last part enters two
graphs of 2^19 nodes and 2^21 edges with aloam_graph_load to reach the 2^20-node and 2^22-edge limits of a group."""
import ctypes as C

import numpy as np
import pytest

import graph_joint_cases as jc
import graph_robust_cases as rc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, eps_ref, pg
from test_gpu_posegraph import ctx

pytestmark = pytest.mark.gpu
NO_LINKS = np.zeros(0, pg.LINK_DTYPE)


def tol():
    return 8 * eps_ref()


def state(gpu, b):
    info = gpu.graph_info(b)
    return dict(info=info, counts=(info["nodes"], info["edges"]), nodes=gpu.graph_export(b), edges=gpu.graph_export(b, edges=True))


def same(a, b):
    return a["info"] == b["info"] and a["counts"] == b["counts"] and a["nodes"].tobytes() == b["nodes"].tobytes() and a["edges"].tobytes() == b["edges"].tobytes()


def pair(s):
    return s["nodes"], s["edges"]


def loops_of(edges, seq):
    """The edges of a member that aloam_graph_add_nodes does not make itself."""
    return pc.with_seq(edges[edges["j"] - edges["i"] != 1], seq)


def enter_cut(gpu, d, slots, whole=None):
    """The two sessions of a cut drive in slots[0], slots[1], and the uncut drive in `whole`."""
    graphs = {slots[k]: (d["members"][k][0]["q"], d["members"][k][0]["t"]) for k in (0, 1)}
    if whole is not None:
        graphs[whole] = (d["whole"][0]["q"], d["whole"][0]["t"])
    pc.enter(gpu, graphs, d["info"])
    for k in (0, 1):
        gpu.graph_add_edges(loops_of(d["members"][k][1], slots[k]))
    if whole is not None:
        gpu.graph_add_edges(loops_of(d["whole"][1], whole))


def cut(laps, at, seqs):
    g = pg.drifted_laps(*laps)
    return dict(pg.cut_drive(g, at, jc.FRAME, seqs), info=g["info"], g=g)


# ---- the bytes of gather, align and scatter ---------------------------------------------------------------------------------------------
def test_the_bytes_of_gather_align_and_scatter(binding):
    """max_iterations = 0: the solve changes nothing, so the joined rows and the members' rows are what gather, alignment and write-back
    made.  Three groups in one call, members of 1, 255 / 256 / 257 and 2 nodes, the middle one with 255 / 256 / 260 edges; links in both
    directions; member 1 is the seq_i side of its tree link, member 2 hangs on member 1 (a chain of aligned members) by the third link
    listed; member 0 (unaligned) and members 1, 2 (aligned) hold anchors."""
    middles = (255, 256, 257)
    gpu = ctx(binding, 10, max_nodes=260, max_edges=264)
    try:
        groups, extras = [], {}
        for g, middle in enumerate(middles):
            seqs = (3 * g + 1, 3 * g, 3 * g + 2)                       # the member order is not the slot order
            raw, links, info = jc.byte_group(middle, seqs)
            pc.enter(gpu, {seqs[m]: raw[m][:2] for m in range(3)}, info)
            for m in range(3):
                gpu.graph_add_edges(raw[m][2])
            groups.append((list(seqs), links, [0, 1, 1]))
        pc.enter(gpu, {9: jc.byte_group(255)[0][2][:2]}, np.eye(6))
        before = {b: state(gpu, b) for b in range(10)}
        assert [before[g[0][1]]["counts"] for g in groups] == [(255, 255), (256, 256), (257, 260)]
        res = gpu.graph_optimize_joint(groups, **dict(OPTIONS, max_iterations=0))
        after = {b: state(gpu, b) for b in range(10)}
        for g, (seqs, links, align) in enumerate(groups):
            members = [pair(before[b]) for b in seqs]
            jn, je, off = pg.join(members, links, seqs, align)
            want = pg.split(members, jn, je, off, align)
            nodes, edges, counts = gpu.graph_joint_export(g)
            print("group", g, "counts", counts.tolist(), "result", res[g]["status"], res[g]["nodes"], res[g]["edges"], float(res[g]["initial_cost"]))
            assert counts.tolist() == [len(jn), len(je), len(je) - len(links), len(links)]
            assert (res[g]["status"], res[g]["nodes"], res[g]["edges"], res[g]["lm_iterations"]) == (0, len(jn), len(je), 0)
            assert nodes.tobytes() == jn.tobytes() and edges.tobytes() == je.tobytes()
            assert np.isclose(res[g]["initial_cost"], pg.cost(jn["q_opt"], jn["t_opt"], je), rtol=1e-12, atol=0)
            for m, b in enumerate(seqs):
                assert after[b]["counts"] == before[b]["counts"]
                assert after[b]["nodes"].tobytes() == want[m][0].tobytes() and after[b]["edges"].tobytes() == want[m][1].tobytes(), (g, m)
                assert all(after[b]["nodes"][f].tobytes() == before[b]["nodes"][f].tobytes() for f in ("q", "t", "frame"))
                if align[m]:
                    anchor = before[b]["edges"]["i"] < 0
                    assert anchor.any() and not np.array_equal(after[b]["edges"]["q"][anchor], before[b]["edges"]["q"][anchor])
                    assert not np.array_equal(after[b]["nodes"]["q_opt"], before[b]["nodes"]["q_opt"])
                else:
                    assert (before[b]["edges"]["i"] < 0).any() and same(after[b], before[b])      # the unaligned member's anchors are untouched
        assert same(after[9], before[9])
    finally:
        gpu.close()


# ---- one member, no links ---------------------------------------------------------------------------------------------------------------
def test_a_group_of_one_member_is_the_per_sequence_solve(binding):
    """2, 256 and 257 nodes, each in four twin slots: aloam_graph_optimize against the joint call, aloam_graph_optimize_robust against the
    robust joint call; result records, nodes and weights byte for byte."""
    sizes = (2, 256, 257)
    gpu = ctx(binding, 12, max_nodes=257, max_edges=270)
    try:
        graphs, extra = {}, {}
        for k, n in enumerate(sizes):
            g = pg.drifted_laps(20 + k, n, 3 if n > 2 else 0)
            more = g["loop"].copy() if n > 2 else pg.anchor_from_localization(1, g["q_true"][1], g["t_true"][1] + 0.2, g["info"])
            more["flags"] = pg.EDGE_ROBUST
            for b in range(4 * k, 4 * k + 4):
                graphs[b], extra[b] = (g["q"], g["t"]), pc.with_seq(more, b)
            info = g["info"]
        pc.enter(gpu, graphs, info)
        for b in graphs:
            gpu.graph_add_edges(extra[b])
        robust = dict(inlier_chi2=rc.C2, mu_step=rc.MU_STEP)
        for k, n in enumerate(sizes):
            a, b, c, d = range(4 * k, 4 * k + 4)
            r0 = gpu.graph_optimize([a], **OPTIONS)
            r1 = gpu.graph_optimize_joint([([b], NO_LINKS)], **OPTIONS)
            print(n, "nodes: plain", r0[0]["lm_iterations"], float(r0[0]["final_cost"]), "joint", r1[0]["lm_iterations"], float(r1[0]["final_cost"]))
            assert r0[0]["status"] == 0 and r0[0]["accepted_steps"] > 0
            assert r0.tobytes() == r1.tobytes() and gpu.graph_export(a).tobytes() == gpu.graph_export(b).tobytes()
            assert gpu.graph_joint_export(0)[0].tobytes() == gpu.graph_export(b).tobytes()
            (s0, w0), (s1, w1) = gpu.graph_optimize_robust([c], robust, **OPTIONS), gpu.graph_optimize_joint_robust([([d], NO_LINKS)], robust, **OPTIONS)
            print(n, "nodes: robust", s0[0]["outer_iterations"], float(s0[0]["solve"]["final_cost"]), "joint", s1[0]["outer_iterations"], float(s1[0]["solve"]["final_cost"]))
            assert s0[0]["solve"]["status"] == 0
            assert s0.tobytes() == s1.tobytes() and w0.tobytes() == w1.tobytes() and gpu.graph_export(c).tobytes() == gpu.graph_export(d).tobytes()
    finally:
        gpu.close()


# ---- the solve --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("laps,at", [((3, 120, 4), 70), (pc.REF_GRAPH, 140)], ids=["120", "300"])
def test_the_joint_solve_of_a_cut_drive(binding, laps, at):
    d = cut(laps, at, (0, 1))
    N = len(d["whole"][0])
    gpu = ctx(binding, 3, max_nodes=N, max_edges=N + 8)
    try:
        enter_cut(gpu, d, (0, 1), whole=2)
        before = [state(gpu, b) for b in (0, 1, 2)]
        assert abs(before[1]["nodes"]["t"] - before[2]["nodes"]["t"][at:]).max() > 50.0            # the second session is in another frame
        res = gpu.graph_optimize_joint([([0, 1], d["links"], [0, 1])], **OPTIONS)[0]
        ref = gpu.graph_optimize([2], **OPTIONS)[0]
        out = [state(gpu, b) for b in (0, 1, 2)]
        want, m, (jn, je) = pg.optimize_joint([pair(before[0]), pair(before[1])], d["links"], align=[0, 1], **OPTIONS)
        q, t = np.concatenate([out[0]["nodes"]["q_opt"], out[1]["nodes"]["q_opt"]]), np.concatenate([out[0]["nodes"]["t_opt"], out[1]["nodes"]["t_opt"]])
        qm, tm = np.concatenate([w[0]["q_opt"] for w in want]), np.concatenate([w[0]["t_opt"] for w in want])
        dev_model = pg.pose_difference(q, t, qm, tm)
        dev_whole = pg.pose_difference(q, t, out[2]["nodes"]["q_opt"], out[2]["nodes"]["t_opt"])
        print(f"{laps} cut at {at}: {len(d['links'])} links; device joint vs model {dev_model:.3e}, vs the uncut drive on the device {dev_whole:.3e} (tolerance {tol():.2e}); "
              f"cost {float(res['final_cost']):.12g} model {m['final_cost']:.12g} uncut {float(ref['final_cost']):.12g}; LM {res['lm_iterations']} / {ref['lm_iterations']} "
              f"PCG {res['pcg_iterations']} / {ref['pcg_iterations']} termination {res['termination']} / {ref['termination']}")
        assert (res["status"], res["nodes"], res["edges"]) == (0, N, len(je)) == (m["status"], m["nodes"], m["edges"]) and ref["status"] == 0
        assert len(je) == before[2]["counts"][1]
        assert np.isclose(res["initial_cost"], m["initial_cost"], rtol=1e-12, atol=0)
        assert dev_model <= tol() and abs(res["final_cost"] - m["final_cost"]) <= tol()
        assert dev_whole <= tol() and abs(res["final_cost"] - ref["final_cost"]) <= tol()
        for k in (0, 1):
            assert all(out[k]["nodes"][f].tobytes() == before[k]["nodes"][f].tobytes() for f in ("q", "t", "frame")) and out[k]["edges"].tobytes() == before[k]["edges"].tobytes()
    finally:
        gpu.close()


# ---- independence -----------------------------------------------------------------------------------------------------------------------
def test_a_group_does_not_depend_on_its_call(binding):
    """The same group (a cut drive, aligned) alone, between two other groups and listed last, in three sets of twin slots: the same bytes in
    dst and in the members' rows.  The unlisted slot is untouched."""
    laps, at = (5, 90, 3), 31
    gpu = ctx(binding, 9, max_nodes=90, max_edges=100)
    try:
        copies = [cut(laps, at, (2 * k, 2 * k + 1)) for k in range(3)]
        for k in range(3):
            enter_cut(gpu, copies[k], (2 * k, 2 * k + 1))
        other = pg.drifted_laps(9, 40, 2)
        pc.enter(gpu, {6: (other["q"], other["t"]), 7: (other["q"][:20], other["t"][:20]), 8: (other["q"][:7], other["t"][:7])}, other["info"])
        gpu.graph_add_edges(pc.with_seq(other["loop"], 6))
        unlisted = state(gpu, 8)
        group = [([2 * k, 2 * k + 1], copies[k]["links"], [0, 1]) for k in range(3)]
        others = [([6], NO_LINKS), ([7], NO_LINKS)]
        alone = gpu.graph_optimize_joint([group[0]], **OPTIONS)
        between = gpu.graph_optimize_joint([others[0], group[1], others[1]], **OPTIONS)
        last = gpu.graph_optimize_joint([others[1], others[0], group[2]], **OPTIONS)
        print("alone", alone[0]["lm_iterations"], float(alone[0]["final_cost"]), "between", float(between[1]["final_cost"]), "last", float(last[2]["final_cost"]))
        assert alone[0]["status"] == 0 and alone[0]["accepted_steps"] > 0 and between[0]["status"] == 0
        assert alone[0].tobytes() == between[1].tobytes() == last[2].tobytes()
        for m in (0, 1):
            a, b, c = (state(gpu, 2 * k + m) for k in range(3))
            for s in (a, b, c):
                s["edges"]["seq"] = 0
            assert same(a, b) and same(a, c), m
        assert same(state(gpu, 8), unlisted)
    finally:
        gpu.close()


# ---- robust -----------------------------------------------------------------------------------------------------------------------------
def test_false_links_are_rejected(binding):
    """Two false links across the cut, built as false_loops builds them and flagged robust.  The case counts only because the model's own
    trace keeps the margin of test_graph_robust_emulation.py; then the weights end 0 for the false links and 1 for the rest, and the poses
    end within 8 eps_ref of the joint solve without them."""
    laps, at = (3, 120, 4), 70
    d = cut(laps, at, (0, 1))
    f = pg.false_loops(d["g"], 12, 100)
    f = f[(f["i"] < at) & (f["j"] >= at)][:2]
    assert len(f) == 2
    false_links = pg.make_links(0, f["i"], 1, f["j"] - at, f["q"], f["t"], f["info"], True)
    links = np.concatenate([d["links"], false_links])
    robust = dict(inlier_chi2=rc.C2, mu_step=rc.MU_STEP)
    gpu = ctx(binding, 2, max_nodes=120, max_edges=130)
    try:
        enter_cut(gpu, d, (0, 1))
        before = [state(gpu, b) for b in (0, 1)]
        members = [pair(before[0]), pair(before[1])]
        trace = []
        _, m, _ = pg.optimize_joint(members, links, align=[0, 1], robust=robust, trace=trace, **OPTIONS)
        margin = rc.margin(trace)
        assert m["mu"] > 0 and margin >= rc.MARGIN, margin
        clean, _, _ = pg.optimize_joint(members, d["links"], align=[0, 1], **OPTIONS)
        res, w = gpu.graph_optimize_joint_robust([([0, 1], links, [0, 1])], robust, **OPTIONS)
        E = before[0]["counts"][1] + before[1]["counts"][1] + len(links)
        out = [state(gpu, b) for b in (0, 1)]
        q, t = np.concatenate([o["nodes"]["q_opt"] for o in out]), np.concatenate([o["nodes"]["t_opt"] for o in out])
        dev = pg.pose_difference(q, t, np.concatenate([c[0]["q_opt"] for c in clean]), np.concatenate([c[0]["t_opt"] for c in clean]))
        print(f"model margin {margin:.3e}, outer {m['outer_iterations']}; device outer {res[0]['outer_iterations']} inliers {res[0]['inliers']} outliers {res[0]['outliers']} "
              f"weights of the links {w[0][E - len(links):E].tolist()}; against the joint solve without the false links {dev:.3e} (tolerance {tol():.2e})")
        assert res[0]["solve"]["status"] == 0 and res[0]["solve"]["edges"] == E and w.shape[1] == E
        assert (res[0]["robust_edges"], res[0]["inliers"], res[0]["outliers"]) == (2, 0, 2) and res[0]["outer_iterations"] == m["outer_iterations"]
        assert w[0][:E - 2].tolist() == [1.0] * (E - 2) and w[0][E - 2:].tolist() == [0.0, 0.0]
        assert dev <= tol()
    finally:
        gpu.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(binding):
    import torch
    L = binding.lib()
    gpu = ctx(binding, 6, max_nodes=8, max_edges=16)
    try:
        g = pg.drifted_laps(2, 4, 0)
        pc.enter(gpu, {b: (g["q"], g["t"]) for b in (0, 1, 2, 4, 5)}, g["info"])               # slot 3 stays empty
        gpu.graph_add_edges(pg.anchor_from_localization(2, g["q"][2], g["t"][2], g["info"], seq=1))
        before = {b: state(gpu, b) for b in range(6)}
        good = np.concatenate([jc.random_links(1, 0, 1, 1, 2), jc.random_links(2, 2, 0, 1, 3), jc.random_links(3, 4, 1, 5, 1)])
        dst = torch.zeros(4 * 128, dtype=torch.uint8).pin_memory()
        wts = torch.zeros(64, dtype=torch.float64).pin_memory()
        pageable = np.zeros(1024, np.uint8)
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None

        def call(members=(0, 1, 2, 4, 5), align=None, links=good, groups=((0, 3, 0, 2), (3, 2, 2, 1)), opt=None, dst_ptr=dst.data_ptr(), robust=None, w_ptr=None,
                 stride=0, n=None, robust_call=False):
            m, a = arr(members, np.int32), None if align is None else arr(align, np.int32)
            l, gr = arr(links, binding.GRAPH_LINK_DTYPE), arr([tuple(x) for x in groups], binding.GRAPH_JOINT_GROUP_DTYPE)
            nm, nl, ng = n if n is not None else (len(m), len(l), len(gr))
            o = C.byref(gpu.graph_options(**opt)) if opt else None
            lists = (gpu.h, ptr(m), ptr(a), nm, ptr(l), nl, ptr(gr), ng, o)
            if robust_call or robust is not None or w_ptr is not None:
                r = C.byref(gpu.graph_robust_options(**robust)) if robust else None
                return L.aloam_graph_optimize_joint_robust(*lists, r, C.c_void_p(dst_ptr) if dst_ptr else None, C.c_void_p(w_ptr) if w_ptr else None, stride)
            return L.aloam_graph_optimize_joint(*lists, C.c_void_p(dst_ptr) if dst_ptr else None)

        def link(k=0, **fields):
            l = good.copy()
            for f, v in fields.items():
                l[f][k] = v
            return l

        bad_info = np.zeros(21); bad_info[0] = -1.0
        refusals = dict(
            member_below=dict(members=(0, 1, -1, 4, 5)), member_above=dict(members=(0, 1, 6, 4, 5)), member_repeated=dict(members=(0, 1, 2, 4, 0)),
            member_first=dict(groups=((1, 3, 0, 2), (3, 2, 2, 1))), member_gap=dict(groups=((0, 2, 0, 2), (3, 2, 2, 1))), member_count_large=dict(groups=((0, 9, 0, 2), (3, 2, 2, 1))),
            members_left_over=dict(groups=((0, 3, 0, 3),)), link_first=dict(groups=((0, 3, 1, 1), (3, 2, 2, 1))), links_left_over=dict(groups=((0, 3, 0, 1), (3, 2, 1, 1))),
            link_count_negative=dict(groups=((0, 3, 0, -1), (3, 2, 0, 3))), member_count_zero=dict(groups=((0, 0, 0, 0), (0, 3, 0, 2), (3, 2, 2, 1))),
            empty_member=dict(members=(0, 1, 3, 4, 5)), first_member_aligned=dict(align=(1, 0, 0, 0, 0)), second_group_first_aligned=dict(align=(0, 1, 1, 1, 0)),
            seq_i_other_group=dict(links=link(0, seq_i=4)), seq_j_other_group=dict(links=link(2, seq_j=0)), seq_i_no_member=dict(links=link(0, seq_i=3)),
            seq_out_of_range=dict(links=link(0, seq_j=17)), seq_equal=dict(links=link(0, seq_j=0)), i_outside=dict(links=link(0, i=4)), j_negative=dict(links=link(1, j=-1)),
            q_not_unit=dict(links=link(0, q=(0.0, 0.0, 0.0, 1.1))), t_nan=dict(links=link(1, t=(np.nan, 0.0, 0.0))), info_not_pd=dict(links=link(2, info=bad_info)),
            flags=dict(links=link(0, flags=2)), no_link_to_earlier=dict(links=np.concatenate([good[:1], good[:1], good[2:]])),
            middle_member_unlinked=dict(members=(0, 2, 1, 4, 5)),
            max_iterations=dict(opt=dict(max_iterations=-1)), huber=dict(opt=dict(huber_delta=0.0)), mu_step=dict(robust=dict(mu_step=1.0)),
            dst_null=dict(dst_ptr=0), dst_pageable=dict(dst_ptr=pageable.ctypes.data), weights_pageable=dict(w_ptr=pageable.ctypes.data, stride=64),
            negative_members=dict(n=(-1, 3, 2)), negative_links=dict(n=(5, -1, 2)), negative_groups=dict(n=(5, 3, -1)),
            no_groups_with_members=dict(n=(5, 3, 0)))
        for name, kw in refusals.items():
            rc_ = call(**kw)
            said = L.aloam_last_error(gpu.h).decode()
            print(name, rc_, said)
            assert rc_ == binding.E_ARG and said, name
            for b in range(6):
                assert same(state(gpu, b), before[b]), (name, b)
        def unchanged(what):
            for b in range(6):
                assert same(state(gpu, b), before[b]), (what, b)
        # the joined edges of the first group: 3 + 4 + 3 member edges and two links = 12, so a stride of 11 is too small
        assert call(w_ptr=wts.data_ptr(), stride=11) == binding.E_ARG
        unchanged("weights_stride")
        m, l, gr = arr((0, 1, 2, 4, 5), np.int32), good, arr([(0, 3, 0, 2), (3, 2, 2, 1)], binding.GRAPH_JOINT_GROUP_DTYPE)
        for nulls in ((None, ptr(l), ptr(gr)), (ptr(m), None, ptr(gr)), (ptr(m), ptr(l), None)):
            assert L.aloam_graph_optimize_joint(gpu.h, nulls[0], None, 5, nulls[1], 3, nulls[2], 2, None, C.c_void_p(dst.data_ptr())) == binding.E_ARG
            unchanged("a NULL list")
        assert L.aloam_graph_optimize_joint(None, None, None, 0, None, 0, None, 0, None, None) == binding.E_ARG
        counts = np.zeros(4, np.int32)
        assert L.aloam_graph_joint_export(gpu.h, 0, None, 0, None, 0, ptr(counts)) == binding.E_STATE      # no joint call has run
        unchanged("the export before a joint call")
        assert L.aloam_graph_optimize_joint(gpu.h, None, None, 0, None, 0, None, 0, None, None) == 0        # n_groups = 0 is ALOAM_OK
        # and the lists as they stand are accepted
        assert call(opt=dict(max_iterations=0)) == 0
        assert call(opt=dict(max_iterations=0), w_ptr=wts.data_ptr(), stride=12) == 0
        gpu.synchronize()
        assert L.aloam_graph_joint_export(gpu.h, 2, None, 0, None, 0, ptr(counts)) == binding.E_ARG
        assert L.aloam_graph_joint_export(gpu.h, 1, None, 0, None, 0, ptr(counts)) == 0 and counts.tolist() == [8, 7, 6, 1]
    finally:
        gpu.close()
    # ---- the limits of a group: 2^20 summed nodes, 2^22 summed edges and links.  Slots 0 and 1 hold 2^19 nodes and 2^21 edges each,
    # slot 2 holds 2^19 nodes and their chain, entered with one aloam_graph_load; slot 3 holds one node.  Members (0, 1) with one link:
    # 2^20 nodes pass, 2^22 + 1 edges do not.  Members (0, 2, 3) with two links: the edges pass, 2^20 + 1 nodes do not.  Nothing is queued, so a refusal returns at once; what is compared afterwards is aloam_graph_info,
    # the whole node rows and the first and last 4096 edges of each row (the whole edge rows are a gigabyte).
    gr_ = __import__("importlib").import_module("a-loam_amd.graph_records")
    N, E, K = 1 << 19, 1 << 21, 4096
    gpu = ctx(binding, 4, max_nodes=N, max_edges=E)
    try:
        nodes = pg.graph_nodes(np.tile(pc.IDENT_Q, (N, 1)), np.zeros((N, 3)))
        k = np.arange(E) % (N - 1)
        edges = np.zeros(E, pg.EDGE_DTYPE)
        edges["i"], edges["j"], edges["q"], edges["info"] = k, k + 1, pc.IDENT_Q, pg.info_upper(np.eye(6))
        big, chain = gr_.pack(nodes, edges), gr_.pack(nodes, edges[:N - 1])
        gpu.graph_load([0, 1, 2], np.concatenate([big, big, chain]), np.array([0, len(big), 2 * len(big), 2 * len(big) + len(chain)], np.int64))
        pc.enter(gpu, {3: (pc.IDENT_Q[None], pc.ZERO_T[None])}, np.eye(6))
        gpu.synchronize()

        def big_state():
            out = []
            for b in (0, 1, 2, 3):
                info = gpu.graph_info(b)
                e = [gpu.graph_export(b, f, min(K, info["edges"]), edges=True).tobytes() for f in (0, max(0, info["edges"] - K))]
                out.append((info, gpu.graph_export(b).tobytes(), e))
            return out
        held = big_state()
        assert [h[0]["nodes"] for h in held] == [N, N, N, 1] and [h[0]["edges"] for h in held] == [E, E, N - 1, 0]
        cases = (("edges", (0, 1), jc.random_links(5, 0, 7, 1, 9), "2^22"),
                 ("nodes", (0, 2, 3), np.concatenate([jc.random_links(6, 0, 3, 2, 0), jc.random_links(7, 3, 0, 0, 11)]), "2^20"))
        dst = torch.zeros(256, dtype=torch.uint8).pin_memory()
        for what, members, l, word in cases:
            n_links = len(l)
            m, g = arr(members, np.int32), arr([(0, len(members), 0, n_links)], binding.GRAPH_JOINT_GROUP_DTYPE)
            for robust_call in (False, True):
                args = (gpu.h, ptr(m), None, len(m), ptr(l), n_links, ptr(g), 1, None)
                rc_ = (L.aloam_graph_optimize_joint_robust(*args, None, C.c_void_p(dst.data_ptr()), None, 0) if robust_call else
                       L.aloam_graph_optimize_joint(*args, C.c_void_p(dst.data_ptr())))
                said = L.aloam_last_error(gpu.h).decode()
                print("limit of", what, rc_, said)
                assert rc_ == binding.E_ARG and word in said, what
                assert big_state() == held, what
    finally:
        gpu.close()


def test_state_error_before_graph_enable(binding):
    gpu = ctx(binding, 2, graph=False)
    try:
        with pytest.raises(binding.AloamError) as e:
            gpu.graph_optimize_joint([([0], NO_LINKS)])
        assert e.value.code == binding.E_STATE
        with pytest.raises(binding.AloamError) as e:
            gpu.graph_optimize_joint_robust([([0], NO_LINKS)])
        assert e.value.code == binding.E_STATE
    finally:
        gpu.close()


# ---- downstream: the existing calls on a joined member ----------------------------------------------------------------------------------
def test_existing_calls_run_on_a_joined_member(binding):
    """The second session holds two anchors and is aligned by a joint call with max_iterations = 0.  A solo aloam_graph_optimize of it then
    starts at the cost its own edges had before the join (1e-12 relative).  After a joint solve the next aloam_graph_add_nodes of the second
    session enters X_opt[k - 1] o Z of the group-frame estimate, bit for bit."""
    laps, at = (3, 120, 4), 70
    d = cut(laps, at, (0, 1))
    g = d["g"]
    gpu = ctx(binding, 2, max_nodes=72, max_edges=80)
    try:
        enter_cut(gpu, d, (0, 1))
        for j, dt in ((20, 0.05), (40, -0.03)):
            gpu.graph_add_edges(pg.anchor_from_localization(j, *pg.compose(*jc.FRAME, g["q_true"][at + j], g["t_true"][at + j] + dt), 4 * g["info"], seq=1))
        before = state(gpu, 1)
        own = pg.cost(before["nodes"]["q_opt"], before["nodes"]["t_opt"], before["edges"], OPTIONS["huber_delta"])
        group = [([0, 1], d["links"], [0, 1])]
        solo_before = gpu.graph_optimize([1], **dict(OPTIONS, max_iterations=0))[0]
        assert same(state(gpu, 1), before)
        placed = gpu.graph_optimize_joint(group, **dict(OPTIONS, max_iterations=0))[0]
        moved = state(gpu, 1)
        solo = gpu.graph_optimize([1], **dict(OPTIONS, max_iterations=0))[0]
        own_moved = pg.cost(moved["nodes"]["q_opt"], moved["nodes"]["t_opt"], moved["edges"], OPTIONS["huber_delta"])
        print(f"own edges before the join {own:.15g} (the device's solo solve there {float(solo_before['initial_cost']):.15g}), solo initial cost after it "
              f"{float(solo['initial_cost']):.15g} (the model there {own_moved:.15g}), relative {abs(solo['initial_cost'] - own) / own:.3e}; "
              f"joined initial cost {float(placed['initial_cost']):.6g}")
        assert placed["status"] == 0 and solo["status"] == 0 and np.abs(moved["nodes"]["t_opt"] - before["nodes"]["t_opt"]).max() > 50.0
        assert np.isclose(solo["initial_cost"], own, rtol=1e-12, atol=0)
        res = gpu.graph_optimize_joint([([0, 1], d["links"])], **OPTIONS)[0]                       # joined already: no second alignment
        assert res["status"] == 0 and res["accepted_steps"] > 0
        last = state(gpu, 1)["nodes"][-1]
        q_new, t_new = pg.compose(last["q"], last["t"], pg.qexp(np.array([0.01, -0.02, 0.05])), np.array([0.4, 0.1, -0.02]))
        gpu.set_state(pc.IDENT_Q, pc.ZERO_T, q_new, t_new, seq=1)
        gpu.graph_add_nodes([1], g["info"])
        node = state(gpu, 1)["nodes"][-1]
        want = pg.compose(last["q_opt"], last["t_opt"], *pg.relative_pose(last["q"], last["t"], node["q"], node["t"]))
        assert node["q"].tobytes() == q_new.tobytes() and node["t"].tobytes() == t_new.tobytes()
        assert node["q_opt"].tobytes() == want[0].tobytes() and node["t_opt"].tobytes() == want[1].tobytes()
        assert np.abs(node["t_opt"] - node["t"]).max() > 50.0                                       # the estimate lives in the group's frame
    finally:
        gpu.close()
