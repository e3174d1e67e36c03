"""The numpy definition of the joined pose graphs (posegraph.join, align_member, split, optimize_joint, cut_drive): the index
arithmetic and the bit copies of join and split for both link directions, what an alignment leaves of a member's own residuals, and the
cut-drive identity: a drive cut into two sessions, the second in another frame, solved jointly ends where the uncut drive ends."""
import numpy as np
import pytest

import graph_joint_cases as jc
import graph_trim_cases as tc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg


def members_of(middle, seqs=(0, 1, 2)):
    raw, links, _ = jc.byte_group(middle, seqs)
    out = []
    for m, (q, t, extra) in enumerate(raw):
        n = len(q)
        k = np.arange(n)
        odom = tc.random_edges(30 + m, k[:-1], k[1:], np.zeros(n - 1, bool), seq=seqs[m]) if n > 1 else np.zeros(0, pg.EDGE_DTYPE)
        nodes = tc.random_nodes(40 + m, n)
        out.append((nodes, np.concatenate([odom, extra])))
    return out, links


@pytest.mark.parametrize("seqs", [(0, 1, 2), (7, 2, 5)])
def test_join_and_split_are_bit_copies_with_the_stated_indices(seqs):
    members, links = members_of(256, seqs)
    nodes, edges, off = pg.join(members, links, seqs)
    assert off.tolist() == [0, 1, 257, 259] and len(nodes) == 259 and len(edges) == sum(len(e) for _, e in members) + len(links)
    e0 = 0
    for m, (n, e) in enumerate(members):
        assert nodes[off[m]:off[m + 1]].tobytes() == n.tobytes()
        je = edges[e0:e0 + len(e)]
        assert (je["i"] == np.where(e["i"] < 0, -1, e["i"] + off[m])).all() and (je["j"] == e["j"] + off[m]).all()
        assert all(je[f].tobytes() == e[f].tobytes() for f in ("seq", "flags", "q", "t", "info"))
        e0 += len(e)
    at = {s: m for m, s in enumerate(seqs)}
    tail = edges[e0:]
    assert len(tail) == len(links) == 5
    for l, e in zip(links, tail):                                      # both directions: (b -> a), (a -> b), (b -> c), (c -> a), (a -> c)
        assert (e["seq"], e["i"], e["j"], e["flags"]) == (l["seq_i"], off[at[int(l["seq_i"])]] + l["i"], off[at[int(l["seq_j"])]] + l["j"], l["flags"])
        assert all(e[f].tobytes() == l[f].tobytes() for f in ("t", "info")) and e["q"].tobytes() == pg.stored_q(l["q"]).tobytes()
        assert np.abs(e["q"] - l["q"]).max() <= 2 * np.finfo(np.float64).eps
    assert {(at[int(l["seq_i"])] < at[int(l["seq_j"])]) for l in links} == {True, False}
    assert pg.tree_links(seqs, links).tolist() == [-1, 0, 2]
    # the write-back without an alignment: the estimates are the joined row's, everything else is the member's
    moved = nodes.copy()
    moved["q_opt"], moved["t_opt"] = tc.unit(moved["q_opt"] + 0.1), moved["t_opt"] + 1.0
    for m, ((n, e), (n2, e2)) in enumerate(zip(members, pg.split(members, moved, edges, off))):
        assert n2["q_opt"].tobytes() == moved["q_opt"][off[m]:off[m + 1]].tobytes() and n2["t_opt"].tobytes() == moved["t_opt"][off[m]:off[m + 1]].tobytes()
        assert all(n2[f].tobytes() == n[f].tobytes() for f in ("q", "t", "frame", "pad")) and e2.tobytes() == e.tobytes()


def test_an_alignment_keeps_the_members_own_residuals():
    """A o X_opt for every node and A o Z for every anchor: E = Z^-1 o X_i^-1 o X_j of a relative edge and E = Z'^-1 o X_j' of an anchor are
    unchanged up to the rounding of the compositions, 64 eps max(1, |t|max) per component (test_graph_trim_model.py's bound for the same
    composition; |t| over the poses before and after).  Chains: member 2 is aligned to member 1's placed estimates."""
    members, links = members_of(257)
    align = [0, 1, 1]
    nodes, edges, off = pg.join(members, links, align=align)
    out = pg.split(members, nodes, edges, off, align)
    worst = 0.0
    for m, ((n, e), (n2, e2)) in enumerate(zip(members, out)):
        if not align[m]:
            assert n2.tobytes() == n.tobytes() and e2.tobytes() == e.tobytes()
            continue
        scale = max(1.0, np.abs(n["t_opt"]).max(), np.abs(n2["t_opt"]).max(), np.abs(e["t"]).max(), np.abs(e2["t"]).max())
        dev = np.abs(jc.own_residuals(n2, e2) - jc.own_residuals(n, e)).max()
        worst = max(worst, dev / scale)
        print(f"member {m}: {len(n)} nodes, {len(e)} edges, {(e['i'] < 0).sum()} anchors, residuals differ by {dev:.3e}, scale {scale:.3g}")
        assert dev <= 64 * np.finfo(np.float64).eps * scale
        anchor = e["i"] < 0
        assert anchor.any() and e2[~anchor].tobytes() == e[~anchor].tobytes()
        assert all(e2[f].tobytes() == e[f].tobytes() for f in ("seq", "i", "j", "flags", "info"))
        assert all(n2[f].tobytes() == n[f].tobytes() for f in ("q", "t", "frame"))
        assert not np.array_equal(n2["q_opt"], n["q_opt"]) and not np.array_equal(e2["q"][anchor], e["q"][anchor])
    # the tree link's own residual is zero after the alignment: the member was placed by it
    l = links[0]
    jn = nodes
    r = pg.residual(jn["q_opt"], jn["t_opt"], edges[len(edges) - len(links):][:1])
    assert np.abs(r).max() <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(jn["t_opt"]).max(), np.abs(l["t"]).max())


def test_align_member_is_the_stated_composition():
    members, links = members_of(256)
    n, e = members[1]
    l = links[0]                                                        # member 1 is its seq_i side
    qg, tg = members[0][0]["q_opt"][0], members[0][0]["t_opt"][0]
    n2, e2, (qa, ta) = pg.align_member(n, e, qg, tg, l, int(l["i"]), True)
    want = pg.compose(*pg.compose(qg, tg, *pg.inverse(l["q"], l["t"])), *pg.inverse(n["q_opt"][l["i"]], n["t_opt"][l["i"]]))
    want = pg.stored_q(want[0]), want[1]
    assert abs(np.linalg.norm(qa) - 1.0) <= 2 * np.finfo(np.float64).eps
    assert qa.tobytes() == want[0].tobytes() and ta.tobytes() == want[1].tobytes()
    q2, t2 = pg.compose(qa, ta, n["q_opt"], n["t_opt"])
    assert n2["q_opt"].tobytes() == q2.tobytes() and n2["t_opt"].tobytes() == t2.tobytes()
    n3, _, (qb, tb) = pg.align_member(n, e, qg, tg, l, int(l["j"]) % len(n), False)      # the seq_j side: Z as it is
    want = pg.compose(*pg.compose(qg, tg, l["q"], l["t"]), *pg.inverse(n["q_opt"][int(l["j"]) % len(n)], n["t_opt"][int(l["j"]) % len(n)]))
    assert qb.tobytes() == pg.stored_q(want[0]).tobytes() and tb.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("laps,cut", jc.CUTS, ids=[str(c[0]) for c in jc.CUTS])
def test_a_cut_drive_solved_jointly_is_the_uncut_drive(laps, cut):
    """cut_drive at `cut` with the second session moved by 2 rad / 100 m: optimize_joint with align ends within 8 eps_ref of optimize of the
    uncut graph (measured: 6.3e-10, 6.8e-11, 1.1e-11; eps_ref is 1.0e-8), and the costs agree."""
    g = pg.drifted_laps(*laps)
    d = pg.cut_drive(g, cut, jc.FRAME)
    assert (d["links"]["i"][0], d["links"]["j"][0]) == (cut - 1, 0) and len(d["links"]) >= 2
    assert len(d["members"][0][1]) + len(d["members"][1][1]) + len(d["links"]) == len(d["whole"][1])
    assert np.abs(d["members"][1][0]["t"] - g["t"][cut:]).max() > 50.0
    out, res, _ = pg.optimize_joint(d["members"], d["links"], align=[0, 1], **OPTIONS)
    q, t, ref = pg.optimize(d["whole"][0]["q"], d["whole"][0]["t"], d["whole"][1], **OPTIONS)
    qj, tj = np.concatenate([n["q_opt"] for n, _ in out]), np.concatenate([n["t_opt"] for n, _ in out])
    dev = pg.pose_difference(qj, tj, q, t)
    print(f"{laps} cut at {cut}: {len(d['links'])} links, joint against uncut {dev:.3e} (tolerance {8 * pc.eps_ref():.2e}), cost {res['final_cost']:.12g} / {ref['final_cost']:.12g}")
    assert res["status"] == ref["status"] == 0 and res["nodes"] == len(g["q"]) and res["edges"] == len(d["whole"][1])
    assert dev <= 8 * pc.eps_ref()
    assert np.isclose(res["initial_cost"], ref["initial_cost"], rtol=1e-9) and abs(res["final_cost"] - ref["final_cost"]) <= 8 * pc.eps_ref()
    # without align the second session stays 100 m away: the joint solve is a different problem
    assert pg.join(d["members"], d["links"])[0]["t_opt"][cut:].tobytes() == d["members"][1][0]["t_opt"].tobytes()


def test_a_group_of_one_member_is_the_plain_solve():
    g = pg.drifted_laps(4, 40, 2)
    nodes, edges = pg.graph_nodes(g["q"], g["t"]), np.concatenate([g["odom"], g["loop"]])
    out, res, (jn, je) = pg.optimize_joint([(nodes, edges)], np.zeros(0, pg.LINK_DTYPE), **OPTIONS)
    q, t, ref = pg.optimize(g["q"], g["t"], edges, **OPTIONS)
    assert out[0][0]["q_opt"].tobytes() == q.tobytes() and out[0][0]["t_opt"].tobytes() == t.tobytes() and res == ref and je.tobytes() == edges.tobytes()
    # fewer than two nodes or no edge: nothing is written back
    out, res, _ = pg.optimize_joint([(nodes[:1], edges[:0])], np.zeros(0, pg.LINK_DTYPE), **OPTIONS)
    assert res["status"] == 1 and out[0][0].tobytes() == nodes[:1].tobytes()
