"""aloam_graph_marginals on the MI355X: the covariance of a candidate edge's residual under the graph, s_edge and the
innovation chi-square, against posegraph.marginals at the estimates the device exports.

One context holds every graph the comparisons need, entered through aloam_set_state / aloam_graph_add_nodes / aloam_graph_add_edges
(posegraph_cases.enter) and solved once with aloam_graph_optimize: the two 40-node graphs with dense information, the 515-node hub, the
40-node graph 5.3e6 m from the origin, and graphs of 2, 300 and 1 nodes.  Every tolerance is 8 x a figure the model measures on itself in
the run (graph_marginal_cases.py): eps_marg, the deviation between the model's dense route and its chain-PCG route at pcg_tolerance 1e-13.
Every comparison prints the device's deviation."""
import ctypes as C

import numpy as np
import pytest

import graph_marginal_cases as mc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg

pytestmark = pytest.mark.gpu
STEP100, STEP1E6, HUB, FAR, TWO, LAPS, ONE = range(7)
DEVICE_OPTIONS = dict(pcg_tolerance=mc.TOL)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def enter(binding, cases, solve=True):
    """A context with one sequence per case, entered and (solve) optimised; returns it and [(q, t, edges)] at the exported estimates."""
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=len(cases), max_points=4096)
    gpu.graph_enable(max(c["max_nodes"] for c in cases), max(c["max_edges"] for c in cases))
    info = {b: pc.odom_info(c) if len(c["odom"]) else pg.info_upper(np.eye(6))[None] for b, c in enumerate(cases)}       # (a lone node 0 has no odometry edge; enter() still indexes one)
    pc.enter(gpu, {b: (c["q"], c["t"]) for b, c in enumerate(cases)}, info)
    extra = [pc.with_seq(c["extra"], b) for b, c in enumerate(cases) if len(c["extra"])]
    gpu.graph_add_edges(np.concatenate(extra))
    if solve:
        res = gpu.graph_optimize(list(range(len(cases))), **OPTIONS)
        assert all(r["status"] == (1 if len(c["q"]) < 2 else 0) for r, c in zip(res, cases)), res
    est = []
    for b in range(len(cases)):
        n, e = gpu.graph_export(b), gpu.graph_export(b, edges=True)
        est.append((n["q_opt"], n["t_opt"], e))
    return gpu, est


def small(d, n):
    """The first n nodes of a drifted_laps dict as a case (its odometry edges alone)."""
    return dict(q=d["q"][:n], t=d["t"][:n], q_true=d["q_true"][:n], t_true=d["t_true"][:n], odom=d["odom"][:n - 1], info=d["info"], extra=d["odom"][:0],
                max_nodes=n, max_edges=max(1, n - 1))


@pytest.fixture(scope="module")
def world(binding):
    laps = pg.drifted_laps(1, 300, 2)
    cases = [pc.step_case(1e2), pc.step_case(1e6), pc.hub_case(), pc.moved(pc.step_case(1e2)), small(laps, 2),
             dict(laps, extra=laps["loop"], max_nodes=300, max_edges=301), small(laps, 1)]
    gpu, est = enter(binding, cases)
    yield dict(gpu=gpu, est=est, cases=cases)
    gpu.close()


def marginals(w, seq, cand, mode=pg.MARGINAL_MEASURED, **options):
    return w["gpu"].graph_marginals(mc.requests(pc.with_seq(cand, seq), mode), dict(DEVICE_OPTIONS, **options))


@pytest.mark.parametrize("seq,name", [(STEP100, "cond 1e2"), (STEP1E6, "cond 1e6")])
def test_against_the_model(world, seq, name):
    """Sigma_r, chi2 and s_edge of the seven requests within 8 eps_marg of the model's dense route; eps_marg is about 3e-14 at condition 1e2
    and 5e-10 at 1e6; pcg_iterations at most twice the model's."""
    q, t, edges = world["est"][seq]
    cand = mc.candidates(world["cases"][seq], seq)
    eps = mc.model_pair(q, t, edges, cand)["eps"]
    res = marginals(world, seq, cand)
    mc.check_against_model(name, res, q, t, edges, cand, eps)
    assert (res["chi2"] <= res["s_edge"]).all() and bits(res["cov"]) == bits(res["cov"].transpose(0, 2, 1))
    assert np.abs(res["q"] - cand["q"]).max() <= 2.3e-16 and bits(res["t"]) == bits(cand["t"])          # (q is stored normalised)
    assert (res["seq"] == seq).all() and (res["mode"] == 0).all()
    r = pg.linearize(q, t, cand)[0]
    assert np.abs(res["r"] - r).max() <= 1e-14 * max(1.0, np.abs(r).max())


def test_three_passes_and_a_hub(world):
    """515 nodes (three passes of the workgroup), node 7 in 302 edges: a far loop candidate and an anchor of the last node."""
    q, t, edges = world["est"][HUB]
    cand = mc.candidates(world["cases"][HUB], HUB)[[0, 2]]
    assert (cand["i"].tolist(), cand["j"].tolist()) == ([2, -1], [513, 514])
    eps = mc.model_pair(q, t, edges, cand)["eps"]
    res = marginals(world, HUB, cand)
    mc.check_against_model("515 nodes, node 7 of degree 302", res, q, t, edges, cand, eps)


def test_at_estimate(world):
    """AT_ESTIMATE: Sigma_r of the relative pose (and of a node against the fixed node's frame) within the same bound, Z = relative_pose of
    the exported estimates, r at rounding, chi2 and s_edge exactly 0; the request's own Z and info are not looked at."""
    q, t, edges = world["est"][STEP100]
    cand = mc.candidates(world["cases"][STEP100], STEP100)[:6].copy()
    eps = mc.model_pair(q, t, edges, mc.candidates(world["cases"][STEP100], STEP100))["eps"]
    cand["q"][1], cand["t"][2], cand["info"][3] = [np.nan, 0, 0, 2], np.inf, -1.0          # ignored, not validated
    res = marginals(world, STEP100, cand, pg.MARGINAL_AT_ESTIMATE)
    model = pg.marginals(q, t, edges, cand, pg.MARGINAL_AT_ESTIMATE)
    dev = mc.deviation(res, model)
    i, j = cand["i"], cand["j"]
    zq, zt = pg.relative_pose(np.where((i < 0)[:, None], pc.IDENT_Q, q[np.maximum(i, 0)]), np.where((i < 0)[:, None], 0.0, t[np.maximum(i, 0)]), q[j], t[j])
    dz = max(np.abs(res["q"] - zq).max(), np.abs(res["t"] - zt).max())
    print(f"AT_ESTIMATE: Sigma_r against the model {dev:.3e} (tolerance {8 * eps:.3e}); |r| {np.abs(res['r']).max():.1e}; Z against relative_pose {dz:.1e}; "
          f"sigma of the relative translation (m) {np.sqrt(res['cov'][:, 3, 3]).round(4).tolist()}")
    assert (res["status"] == 0).all() and (res["mode"] == 1).all() and dev <= 8 * eps
    assert np.abs(res["r"]).max() <= 1e-14 and not res["chi2"].any() and not res["s_edge"].any() and dz <= 1e-14


def test_results_do_not_depend_on_the_list(world):
    """One request alone; inside a call that mixes the graphs of 2, 40 and 300 nodes; that call reversed; and a call of more requests than
    there are scratch rows (a round takes 1024): the same result bytes."""
    c40, c300 = mc.candidates(world["cases"][STEP100], STEP100), mc.candidates(world["cases"][LAPS], LAPS)
    two = pg.marginal_request(TWO, [0, -1], [1, 1], mode=[0, 1])
    alone = marginals(world, STEP100, c40[:1])
    mixed = np.concatenate([two, mc.requests(c300[:3]), mc.requests(c40), two[::-1], mc.requests(c300[3:])])
    o = dict(DEVICE_OPTIONS)
    a, b = world["gpu"].graph_marginals(mixed, o), world["gpu"].graph_marginals(mixed[::-1].copy(), o)
    at = 2 + 3
    assert bits(a[at]) == bits(alone[0]) and bits(a) == bits(b[::-1])
    assert (a["status"] == 0).all() and (a["nodes"][[0, 2, at]] == [2, 300, 40]).all()
    many = np.concatenate([mixed] * 65)                                               # 1170 requests: two rounds
    assert len(many) > 1024
    big = world["gpu"].graph_marginals(many, o)
    assert bits(big) == bits(np.concatenate([a] * 65))
    device = world["gpu"].graph_marginals(mixed, o, pinned=False)                       # into device memory
    assert bits(device) == bits(a)


def test_a_call_of_six_rounds_wraps_the_request_ring(world):
    """5130 requests in one call: six rounds of at most 1024 through the pinned ring of four slots, so rounds five and six fill the slots
    of rounds one and two, whose copies were queued in the same call.  The result bytes are the 18-request result tiled, as the 1170-request
    call of test_results_do_not_depend_on_the_list compares."""
    c40, c300 = mc.candidates(world["cases"][STEP100], STEP100), mc.candidates(world["cases"][LAPS], LAPS)
    two = pg.marginal_request(TWO, [0, -1], [1, 1], mode=[0, 1])
    mixed = np.concatenate([two, mc.requests(c300[:3]), mc.requests(c40), two[::-1], mc.requests(c300[3:])])
    o = dict(DEVICE_OPTIONS)
    a = world["gpu"].graph_marginals(mixed, o)
    many = np.concatenate([mixed] * 285)
    assert len(mixed) == 18 and len(many) == 5130 > 4 * 1024
    big = world["gpu"].graph_marginals(many, o)
    assert bits(big) == bits(np.concatenate([a] * 285))


def test_the_graph_is_only_read(world):
    gpu = world["gpu"]
    before = [(bits(gpu.graph_export(b)), bits(gpu.graph_export(b, edges=True))) for b in (STEP100, TWO, ONE)]
    marginals(world, STEP100, mc.candidates(world["cases"][STEP100], STEP100))
    gpu.graph_marginals(pg.marginal_request(TWO, [0], [1], mode=1))
    assert [(bits(gpu.graph_export(b)), bits(gpu.graph_export(b, edges=True))) for b in (STEP100, TWO, ONE)] == before
    assert gpu.graph_marginals(np.zeros(0, pg.MARGINAL_REQUEST_DTYPE)).shape == (0,)


def test_the_gate(world):
    """On the device's own numbers: the six consistent candidates below the 6-dof 0.999 quantile, the one displaced by 1.5 m above it."""
    for seq, name in ((STEP100, "cond 1e2"), (STEP1E6, "cond 1e6"), (HUB, "hub")):
        res = marginals(world, seq, mc.candidates(world["cases"][seq], seq))
        print(f"{name}: chi2 {res['chi2'].round(2).tolist()} against {mc.GATE:.2f}; s_edge {res['s_edge'].round(1).tolist()}; PCG {res['pcg_iterations'].tolist()}")
        assert (res["status"] == 0).all() and (res["chi2"][:6] < mc.GATE).all() and res["chi2"][6] > mc.GATE


def test_woodbury_on_the_device(binding):
    """The marginal of a plain candidate, aloam_graph_add_edges of it, the marginal again with no solve in between:
    Sigma_r' = Sigma_r - Sigma_r S^-1 Sigma_r, S = Sigma_r + Omega^-1, within 8 x what the model measures for the same identity."""
    case = pc.step_case(1e2)
    gpu, [(q, t, edges)] = enter(binding, [dict(case, max_edges=case["max_edges"] + 1)])
    cand = mc.candidates(case)[:1]

    def identity(before, after):
        S = before["cov"][0] + np.linalg.inv(pg.info_full(cand["info"][0]))
        want = before["cov"][0] - before["cov"][0] @ np.linalg.solve(S, before["cov"][0])
        d = np.sqrt(np.diag(want))
        return float(np.max(np.abs(after["cov"][0] - want) / (d[:, None] * d[None, :])))

    eps = identity(pg.marginals(q, t, edges, cand), pg.marginals(q, t, np.concatenate([edges, cand]), cand))
    req = mc.requests(cand)
    before = gpu.graph_marginals(req, DEVICE_OPTIONS)
    gpu.graph_add_edges(cand)
    after = gpu.graph_marginals(req, DEVICE_OPTIONS)
    dev = identity(before, after)
    print(f"Woodbury: device {dev:.3e}, model {eps:.3e} (tolerance {8 * eps:.3e}); edges {before['edges'][0]} -> {after['edges'][0]}")
    gpu.close()
    assert before["status"][0] == 0 == after["status"][0] and after["edges"][0] == before["edges"][0] + 1
    assert dev <= 8 * eps


def test_statuses(world):
    """A one-node graph: NO_EDGES.  pcg_max_iterations 1: NOT_CONVERGED, 6 iterations, Sigma_r that of the model's one-iteration route within
    8 x the deviation between chain_solver and posegraph_cases.chain_solver_dense at that cap.  (-1, 0): nothing to solve, chi2 = s_edge."""
    gpu = world["gpu"]
    r = gpu.graph_marginals(pg.marginal_request(ONE, [-1], [0]))[0]
    assert (r["status"], r["nodes"], r["edges"], r["pcg_iterations"]) == (pg.MARGINAL_NO_EDGES, 1, 0, 0) and not r["cov"].any() and r["chi2"] == 0
    q, t, edges = world["est"][STEP100]
    cand = mc.candidates(world["cases"][STEP100], STEP100)
    res = marginals(world, STEP100, cand, pcg_max_iterations=1)
    a, b = (pg.marginals(q, t, edges, cand, solve=s(mc.TOL, 1)) for s in (pg.chain_solver, pc.chain_solver_dense))
    eps, dev = mc.deviation(a, b), mc.deviation(res, a)
    print(f"pcg_max_iterations 1: device against the model's one-iteration route {dev:.3e}; the model's two preconditioner solves {eps:.3e} (tolerance {8 * eps:.3e})")
    assert (res["status"] == pg.MARGINAL_NOT_CONVERGED).all() and (res["pcg_iterations"] == 6).all()
    assert dev <= 8 * eps
    zero = gpu.graph_marginals(pg.marginal_request(STEP100, [-1], [0], info=[np.diag([4.0, 5, 6, 7, 8, 9])], t=[[0.1, 0.2, 0.3]]), DEVICE_OPTIONS)[0]
    assert zero["status"] == 0 and zero["pcg_iterations"] == 0 and not zero["cov"].any() and zero["chi2"] == zero["s_edge"] > 0


def test_refusals_queue_nothing(binding, world):
    import torch
    gpu, L = world["gpu"], binding.lib()
    cand = mc.candidates(world["cases"][STEP100], STEP100)
    ok = mc.requests(cand[:2])
    sentinel = torch.full((2 * mc.RESULT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, pin_memory=True)
    graph = [(bits(gpu.graph_export(b)), bits(gpu.graph_export(b, edges=True))) for b in (STEP100, ONE)]
    launches = None

    def refused(req, options=None, dst=None, code=binding.E_ARG):
        with pytest.raises(binding.AloamError) as err:
            gpu.graph_marginals_into(req, sentinel.data_ptr() if dst is None else dst, gpu.graph_marginal_options(**options) if options else None)
        assert err.value.code == code, err.value

    for field, value in (("seq", 7), ("seq", -1), ("i", -2), ("i", 40), ("j", -1), ("j", 40), ("i", int(ok["edge"]["j"][1])), ("flags", 2)):
        bad = ok.copy(); bad["edge"][field][1] = value
        refused(bad)
    for mode in (2, -1):
        bad = ok.copy(); bad["mode"][1] = mode
        refused(bad)
    for what in ("q_norm", "q_nan", "t_inf", "info_nan", "indefinite"):
        bad = ok.copy()
        if what == "q_norm": bad["edge"]["q"][1] = [0, 0, 0, 1.00001]
        if what == "q_nan": bad["edge"]["q"][1] = [np.nan, 0, 0, 1]
        if what == "t_inf": bad["edge"]["t"][1] = [np.inf, 0, 0]
        if what == "info_nan": bad["edge"]["info"][1, 3] = np.nan
        if what == "indefinite": bad["edge"]["info"][1] = pg.info_upper(np.diag([1, 1, 1, 1, 1, -1.0]))
        refused(bad)
    for o in (dict(pcg_max_iterations=0), dict(pcg_tolerance=-1.0), dict(pcg_tolerance=np.nan), dict(huber_delta=0.0), dict(huber_delta=np.inf)):
        refused(ok, options=o)
    refused(ok, dst=np.zeros(2 * 440, np.uint8).ctypes.data)                           # pageable
    refused(ok, dst=0)
    on_device = torch.zeros(2 * 248, dtype=torch.uint8, device="cuda")                   # requests are read on the host
    with pytest.raises(binding.AloamError) as err:
        gpu._check(L.aloam_graph_marginals(gpu.h, C.c_void_p(on_device.data_ptr()), 2, None, C.c_void_p(sentinel.data_ptr())))
    assert err.value.code == binding.E_ARG
    gpu.synchronize()
    assert (sentinel.numpy() == 0xAB).all()
    assert [(bits(gpu.graph_export(b)), bits(gpu.graph_export(b, edges=True))) for b in (STEP100, ONE)] == graph
    off = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=4096)
    assert L.aloam_graph_marginals(off.h, binding._p(ok), 2, None, C.c_void_p(sentinel.data_ptr())) == binding.E_STATE   # before aloam_graph_enable
    off.close()


def test_far_from_the_origin(world):
    """The 40-node graph composed with G, |t| = 5.3e6 m: Sigma_r of relative candidates is that of the near graph within 8 x the band the model
    shows between its own far and near results."""
    near, far = world["est"][STEP100], world["est"][FAR]
    cand = mc.candidates(world["cases"][STEP100])[[0, 1, 4, 5, 6]]                       # the relative ones: anchors measure G o X
    m_near, m_far = pg.marginals(*near, pc.with_seq(cand, STEP100)), pg.marginals(*far, pc.with_seq(cand, FAR))
    band = mc.deviation(m_far, m_near)
    d_near, d_far = marginals(world, STEP100, cand), marginals(world, FAR, cand)
    dev = mc.deviation(d_far, d_near)
    print(f"|t| = 5.3e6 m: device far against near {dev:.3e}; the model's own band {band:.3e} (tolerance {8 * band:.3e}); chi2 far {d_far['chi2'].round(2).tolist()}")
    assert (d_far["status"] == 0).all() and dev <= 8 * band


def test_a_context_that_never_asks_is_unchanged(binding, sequence):
    import torch
    scans, _, _, model = sequence("VLP-16", 3, seed=3)
    out = []
    for ask in (False, True):
        gpu = binding.Aloam(n_scans=model.n_scans, min_range=model.min_range, batch=1, max_points=40000)
        gpu.profile_enable(True)
        gpu.graph_enable(8, 8)
        for s in scans:
            gpu.scan_register(s)
            gpu.odometry_step()
            gpu.graph_add_nodes([0], np.eye(6) * 100.0)
        if ask:
            r = gpu.graph_marginals(pg.marginal_request(0, [0, -1], [2, 1], mode=1))
            assert (r["status"] == 0).all() and (r["nodes"] == 3).all() and r["cov"][0, 3, 3] > 0
        rec = torch.zeros(C.sizeof(binding.AloamPoseRecord), dtype=torch.uint8, pin_memory=True)
        gpu.export_poses(rec.data_ptr())
        gpu.synchronize()
        got = {k: v.tobytes() for k, v in gpu.pose().items()}
        got.update(record=rec.numpy().tobytes(), stats=str(gpu.odom_stats()), features={k: v.tobytes() for k, v in gpu.features().items()},
                   corr=[a.tobytes() for a in gpu.correspondences()], nodes=bits(gpu.graph_export(0)), edges=bits(gpu.graph_export(0, edges=True)))
        prof = gpu.profile()
        assert prof["graph_marginals"]["launches"] == (1 if ask else 0)
        got["launches"] = {k: v["launches"] for k, v in prof.items() if k != "graph_marginals"}
        out.append(got)
        gpu.close()
    assert out[0] == out[1]
