"""aloam_graph_optimize_robust on the MI355X: GNC-TLS over the flagged edges, against posegraph.optimize_robust.

One context holds every graph, entered through aloam_set_state / aloam_graph_add_nodes / aloam_graph_add_edges (posegraph_cases.enter).
The call moves the estimates, so every comparison has a sequence of its own: three copies of (case A, a clean graph, a one-node graph) for
the calls in two orders and alone, case B, an unflagged graph twice (the robust call against aloam_graph_optimize), the graph with a
non-finite flagged edge twice, case A again for the cap and the clean graph again for the skip branch.  All calls are made once (the
fixture) and the tests look at what they left.  The discrete outcome is held to the model's exactly: graph_robust_cases.py asserts the
margin condition on the model's trace.  Every comparison prints the device's figures."""
import ctypes as C

import numpy as np
import pytest

import graph_robust_cases as rc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg

pytestmark = pytest.mark.gpu
A0, CLEAN0, ONE0, A1, CLEAN1, ONE1, A2, CLEAN2, ONE2, B, PLAIN_R, PLAIN_P, BAD_R, BAD_P, A_CAP, CLEAN_SKIP = range(16)
SENTINEL = -7.0


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def one_node(case):
    return dict(q=case["q"][:1], t=case["t"][:1], odom=case["odom"][:0], info=case["info"], extra=case["odom"][:0], edges=case["odom"][:0], max_nodes=1, max_edges=1)


def unflagged(case):
    extra = case["extra"].copy()
    extra["flags"] = 0
    return dict(case, extra=extra, edges=np.concatenate([case["odom"], extra]))


def flagged_failing():
    _, bad = pc.failing_case()
    extra = bad["extra"].copy()
    extra["flags"][-1] = pg.EDGE_ROBUST                    # t = (1e200, 0, 0): s overflows
    return dict(bad, extra=extra, edges=np.concatenate([bad["odom"], extra]))


def graph(gpu, seq):
    return gpu.graph_export(seq), gpu.graph_export(seq, edges=True)


@pytest.fixture(scope="module")
def world(binding):
    a, clean, b = rc.case_a(), rc.clean_case(), rc.case_b()
    one, plain, bad = one_node(clean), unflagged(clean), flagged_failing()
    cases = [a, clean, one] * 3 + [b, plain, plain, bad, bad, a, clean]
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=len(cases), max_points=4096)
    gpu.graph_enable(max(c["max_nodes"] for c in cases), max(c["max_edges"] for c in cases))
    info = {s: pc.odom_info(c) if len(c["odom"]) else pg.info_upper(np.eye(6))[None] for s, c in enumerate(cases)}
    pc.enter(gpu, {s: (c["q"], c["t"]) for s, c in enumerate(cases)}, info)
    gpu.graph_add_edges(np.concatenate([pc.with_seq(c["extra"], s) for s, c in enumerate(cases) if len(c["extra"])]))
    before = {s: graph(gpu, s) for s in range(len(cases))}
    stride = max(len(c["edges"]) for c in cases) + 5
    out = {}

    def call(seqs, robust=None, **options):
        res, w = gpu.graph_optimize_robust(seqs, robust=robust, weights_stride=stride, sentinel=SENTINEL, **dict(OPTIONS, **options))
        for k, s in enumerate(seqs):
            out[s] = dict(res=res[k], weights=w[k], nodes=gpu.graph_export(s), edges=gpu.graph_export(s, edges=True))

    call([A0, CLEAN0, ONE0])
    call([ONE1, CLEAN1, A1])
    for s in (A2, CLEAN2, ONE2):
        call([s])
    call([B])
    call([PLAIN_R])
    plain_res = gpu.graph_optimize([PLAIN_P], **OPTIONS)
    plain_nodes = gpu.graph_export(PLAIN_P)
    call([BAD_R])
    call([A_CAP], robust=dict(max_outer_iterations=2))
    s_clean = pg.edge_chi2(clean["q"], clean["t"], clean["edges"])[clean["edges"]["flags"] != 0]
    call([CLEAN_SKIP], robust=dict(inlier_chi2=float(2.5 * s_clean.max())))
    yield dict(gpu=gpu, cases=cases, before=before, out=out, plain_res=plain_res, plain_nodes=plain_nodes, stride=stride)
    gpu.close()


def row(world, seq):
    o, n = world["out"][seq], len(world["cases"][seq]["edges"])
    assert (o["weights"][n:] == SENTINEL).all() and len(o["weights"]) == world["stride"]          # entries beyond the edge count are not written
    return rc.as_dict(o["res"]), o["weights"][:n], o["nodes"]


def untouched(world, seq):
    """The entered poses and the exported edges are byte-equal before and after; so are frame and pad."""
    (n0, e0), o = world["before"][seq], world["out"][seq]
    return bits(e0) == bits(o["edges"]) and all(bits(n0[f]) == bits(o["nodes"][f]) for f in ("q", "t", "frame", "pad")) and bits(n0[:1]) == bits(o["nodes"][:1])


def test_case_a_against_the_model(world):
    """60 nodes, two true loops and three false ones: 18 outer iterations, weights [1, 1, 0, 0, 0], the model's and the inlier-only solve's
    poses to 8 eps_ref."""
    case = rc.case_a()
    m = rc.model(case)
    assert m["margin"] >= rc.MARGIN and m["trace"][-1]["weights"].tolist() == [1, 1, 0, 0, 0]
    res, weights, nodes = row(world, A0)
    rc.check_against_model("device, case A", case, res, weights, nodes, rc.want_of(m), rc.inlier_solve("a"))
    assert untouched(world, A0)
    assert abs(res["truncated_cost"] - m["res"]["truncated_cost"]) <= 1e-9 * m["res"]["truncated_cost"]


def test_case_b_against_the_record_and_the_inlier_solve(world):
    """300 nodes (more than the workgroup has threads), six false loops: the model's outcome as recorded (14 outer iterations, weights
    [1, 1, 0 x 6]; its trace keeps 0.3 % from every threshold) and the chain_pcg solve of the graph without the false loops."""
    case, rec = rc.case_b(), rc.record_b()
    assert rec["margin"] >= rc.MARGIN and rec["weights"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    res, weights, nodes = row(world, B)
    rc.check_against_model("device, case B", case, res, weights, nodes, rec, rc.inlier_solve("b"))
    assert untouched(world, B)


def test_results_do_not_depend_on_the_list(world):
    """Case A, the clean graph and the one-node graph in one call, in another call in the opposite order, and each alone: the result, the
    weight row (with its sentinel tail) and the nodes are the same bytes."""
    for first, second, alone in ((A0, A1, A2), (CLEAN0, CLEAN1, CLEAN2), (ONE0, ONE1, ONE2)):
        o = [world["out"][s] for s in (first, second, alone)]
        assert bits(o[0]["res"]) == bits(o[1]["res"]) == bits(o[2]["res"])
        assert bits(o[0]["weights"]) == bits(o[1]["weights"]) == bits(o[2]["weights"])
        assert bits(o[0]["nodes"]) == bits(o[1]["nodes"]) == bits(o[2]["nodes"])
        assert all(untouched(world, s) for s in (first, second, alone))
    res, weights, nodes = row(world, ONE0)
    assert res["status"] == 1 and res["outer_iterations"] == 0 and len(weights) == 0 and (world["out"][ONE0]["weights"] == SENTINEL).all()
    res, weights, nodes = row(world, CLEAN0)
    clean = rc.clean_case()
    m = rc.model(clean)
    assert res["status"] == 0 and (weights == 1).all() and (res["inliers"], res["outliers"]) == (2, 0) and res["outer_iterations"] == m["res"]["outer_iterations"]
    assert pg.pose_difference(nodes["q_opt"], nodes["t_opt"], m["q"], m["t"]) <= 8 * pc.eps_ref()


def test_an_empty_r_is_the_plain_solve_bit_for_bit(world):
    """No flagged edge: one solve of the scaled copy with every weight 1.  w * Omega with w = 1.0 is Omega's bits and the flags were 0
    already, so the device functions read the same values as under aloam_graph_optimize; the loop around them is restated statement for
    statement and the build contracts nothing (-ffp-contract=off), so every operation is the same IEEE operation on the same bits; Huber is
    never active in either (no flag).  Hence the same bits, in the result and in the nodes."""
    res, weights, nodes = row(world, PLAIN_R)
    plain, pnodes = world["plain_res"][0], world["plain_nodes"]
    print(f"empty R: LM {res['lm_iterations']} PCG {res['pcg_iterations']} final_cost {res['final_cost']:.17g}; aloam_graph_optimize LM {int(plain['lm_iterations'])} "
          f"PCG {int(plain['pcg_iterations'])} final_cost {float(plain['final_cost']):.17g}")
    assert (res["status"], res["outer_iterations"], res["mu"], res["robust_edges"], res["s_max"]) == (0, 1, 0.0, 0, 0.0) and (weights == 1).all()
    assert bits(nodes) == bits(pnodes)
    for f in ("status", "termination", "lm_iterations", "accepted_steps", "pcg_iterations", "nodes", "edges", "final_cost", "gradient_max"):
        assert res[f] == plain[f], f
    assert abs(res["initial_cost"] - plain["initial_cost"]) <= 1e-12 * plain["initial_cost"]          # (summed over s, not over rho: another order)
    # nothing is stored between calls: a plain solve after the robust one is the plain solve after a plain one
    gpu = world["gpu"]
    again = gpu.graph_optimize([PLAIN_R, PLAIN_P], **OPTIONS)
    assert bits(again[0]) == bits(again[1]) and bits(gpu.graph_export(PLAIN_R)) == bits(gpu.graph_export(PLAIN_P))


def test_skip_and_cap(world):
    res, weights, nodes = row(world, CLEAN_SKIP)
    clean = rc.clean_case()
    q, t, _ = pg.optimize(clean["q"], clean["t"], unflagged(clean)["edges"], **OPTIONS)
    assert (res["status"], res["outer_iterations"], res["mu"], res["inliers"], res["outliers"], res["robust_edges"]) == (0, 1, 0.0, 2, 0, 2) and (weights == 1).all()
    assert pg.pose_difference(nodes["q_opt"], nodes["t_opt"], q, t) <= 8 * pc.eps_ref() and untouched(world, CLEAN_SKIP)
    res, weights, nodes = row(world, A_CAP)
    w = weights[rc.case_a()["edges"]["flags"] != 0]
    print(f"cap 2: weights {w.tolist()}, mu {res['mu']:.6g}")
    assert res["status"] == 0 and res["outer_iterations"] == 2 and ((w > 0) & (w < 1)).any() and res["inliers"] + res["outliers"] < res["robust_edges"] == 5
    assert abs(res["mu"] - rc.C2 / (2.0 * res["s_max"] - rc.C2) * rc.MU_STEP) <= 1e-12 * res["mu"] and untouched(world, A_CAP)


def test_a_non_finite_edge_fails_and_changes_nothing(world):
    res, weights, nodes = row(world, BAD_R)
    assert (res["status"], res["termination"], res["outer_iterations"], res["lm_iterations"]) == (2, 5, 0, 0) and (weights == 1).all()
    assert bits(nodes) == bits(world["before"][BAD_R][0]) and untouched(world, BAD_R)
    # aloam_graph_optimize afterwards behaves as on the same graph that no robust call has touched
    gpu = world["gpu"]
    after = gpu.graph_optimize([BAD_R, BAD_P], **OPTIONS)
    assert bits(after[0]) == bits(after[1]) and bits(gpu.graph_export(BAD_R)) == bits(gpu.graph_export(BAD_P))


def test_refusals_queue_nothing(binding, world):
    import torch
    gpu, L = world["gpu"], binding.lib()
    seqs = [A_CAP, CLEAN_SKIP]
    state = [tuple(bits(x) for x in graph(gpu, s)) for s in seqs]
    stride = world["stride"]
    dst = torch.full((2 * 128,), 0xAB, dtype=torch.uint8).pin_memory()
    wts = torch.full((2, stride), SENTINEL, dtype=torch.float64).pin_memory()

    def refused(code=binding.E_ARG, ids=seqs, dst_ptr=None, w_ptr=None, w_stride=stride, options=None, **robust):
        with pytest.raises(binding.AloamError) as err:
            gpu.graph_optimize_robust_into(ids, dst.data_ptr() if dst_ptr is None else dst_ptr, gpu.graph_options(**options) if options else None,
                                           gpu.graph_robust_options(**robust) if robust else None, wts.data_ptr() if w_ptr is None else w_ptr, w_stride)
        assert err.value.code == code, err.value

    for bad in (dict(max_outer_iterations=0), dict(inlier_chi2=0.0), dict(inlier_chi2=-1.0), dict(inlier_chi2=np.inf), dict(inlier_chi2=np.nan),
                dict(mu_step=1.0), dict(mu_step=0.5), dict(mu_step=np.inf), dict(mu_step=np.nan)):
        refused(**bad)
    refused(options=dict(pcg_max_iterations=0))
    refused(options=dict(gradient_tolerance=-1.0))
    refused(w_stride=len(rc.case_a()["edges"]) - 1)                                       # below the largest edge count listed
    refused(dst_ptr=np.zeros(2 * 128, np.uint8).ctypes.data)                              # pageable
    refused(w_ptr=np.zeros(2 * stride).ctypes.data)
    refused(ids=[A_CAP, A_CAP])                                                           # duplicates
    refused(ids=[A_CAP, len(world["cases"])])
    with pytest.raises(binding.AloamError) as err:                                        # dst NULL
        gpu._check(L.aloam_graph_optimize_robust(gpu.h, binding._p(np.array(seqs, np.int32)), 2, None, None, None, C.c_void_p(wts.data_ptr()), stride))
    assert err.value.code == binding.E_ARG
    gpu.synchronize()
    assert (dst.numpy() == 0xAB).all() and (wts.numpy() == SENTINEL).all()
    assert [tuple(bits(x) for x in graph(gpu, s)) for s in seqs] == state
    off = binding.Aloam(n_scans=16, min_range=0.3, batch=2, max_points=4096)
    assert L.aloam_graph_optimize_robust(off.h, binding._p(np.array([0], np.int32)), 1, None, None, C.c_void_p(dst.data_ptr()), None, 0) == binding.E_STATE   # before aloam_graph_enable
    off.close()
    # weights_dst may be NULL, and n = 0 is ALOAM_OK
    gpu.graph_optimize_robust_into([CLEAN_SKIP], dst.data_ptr(), gpu.graph_options(**OPTIONS), None, 0, 0)
    gpu.graph_optimize_robust_into([], 0, None, None, 0, 0)
    gpu.synchronize()
    assert np.frombuffer(dst.numpy()[:128].tobytes(), rc.RESULT_DTYPE)["solve"]["status"][0] == 0 and (dst.numpy()[128:] == 0xAB).all() and (wts.numpy() == SENTINEL).all()
