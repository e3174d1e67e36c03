"""k_pose_graph on the MI355X step by step and with dense information ("what the tests reach").

test_gpu_posegraph.py compares the device with the model at the minimum, where a solve with the right gradient and a wrong H still arrives,
and every information matrix there is diag(a, a, a, b, b, b), which forgives a wrong rotation, a transposed off-diagonal block and a
dropped rotation-translation coupling.  Here every edge carries a dense, badly conditioned information of its own, Huber's delta is not 1,
and the solve is stopped after 0, 1, 2, 3 iterations, where H decides the answer: the linearisation alone against a longdouble restatement,
truncated solves against the model's two solvers, rejected steps, a PCG cut short, three passes of the workgroup with an incidence list
longer than it, exact invariances, coordinates of 10^6 m, a failing graph beside a healthy one, and the refused options.

Graphs are entered through aloam_set_state / aloam_graph_add_nodes / aloam_graph_add_edges and the model is fed what the device exports, as
in test_gpu_posegraph.py.  Every tolerance is 8 x a figure the model measures on itself in the run (posegraph_cases.py): eps_lin (f64
against longdouble), eps_step (dense solve against chain_pcg, the largest over the parametrised family), or the model's own band.  The
cases and the assertions are shared with the host emulation (test_posegraph_emulation.py); test_posegraph_model.py checks that the
truncated cases decide far from the acceptance threshold.  Every comparison prints the device's deviation."""
import numpy as np
import pytest

import posegraph_cases as pc
from posegraph_cases import OPTIONS, STEP_OPTIONS, pg

pytestmark = pytest.mark.gpu


def ctx(binding, B, max_nodes, max_edges):
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=B, max_points=4096)
    gpu.graph_enable(max_nodes, max_edges)
    return gpu


def entered(binding, cases):
    """A fresh context with one sequence per case; returns it and [(nodes, edges)] as the device exports them."""
    gpu = ctx(binding, len(cases), max(c["max_nodes"] for c in cases), max(c["max_edges"] for c in cases))
    pc.enter(gpu, {b: (c["q"], c["t"]) for b, c in enumerate(cases)}, {b: pc.odom_info(c) for b, c in enumerate(cases)})
    gpu.graph_add_edges(np.concatenate([pc.with_seq(c["extra"], b) for b, c in enumerate(cases)]))
    start = [(gpu.graph_export(b), gpu.graph_export(b, edges=True)) for b in range(len(cases))]
    for (n, e), c in zip(start, cases):
        assert len(n) == len(c["q"]) and len(e) == len(c["edges"])
    return gpu, start


def solve(binding, case, **options):
    """One case in a fresh context: (nodes before, edges, result, nodes after)."""
    gpu, [(nodes0, edges)] = entered(binding, [case])
    res = gpu.graph_optimize([0], **options)[0]
    out = gpu.graph_export(0)
    gpu.close()
    return nodes0, edges, res, out


def as_problem(nodes, edges):
    return nodes["q_opt"], nodes["t_opt"], edges


@pytest.fixture(scope="module")
def step_problems(binding):
    """The two 40-node graphs as the device holds them: what eps_lin and eps_step of the family are measured on."""
    gpu, start = entered(binding, [pc.step_case(c) for c in pc.CONDS])
    gpu.close()
    return [as_problem(n, e) for n, e in start]


@pytest.fixture(scope="module")
def hub(binding):
    gpu, [(nodes0, edges)] = entered(binding, [pc.hub_case()])
    gpu.close()
    return as_problem(nodes0, edges)


@pytest.mark.parametrize("delta", pc.DELTAS)
@pytest.mark.parametrize("cond", pc.CONDS)
def test_linearisation_alone(binding, step_problems, cond, delta):
    """(a) max_iterations = 0: cost and gradient of the first linearisation against the longdouble restatement, to 8 eps_lin."""
    nodes0, edges, res, out = solve(binding, pc.step_case(cond), **dict(STEP_OPTIONS, max_iterations=0, huber_delta=delta))
    pc.check_linearisation(f"cond {cond:g} delta {delta}", nodes0, edges, res, out, delta, pc.eps_lin(step_problems))


@pytest.mark.parametrize("k", pc.STEPS)
@pytest.mark.parametrize("delta", pc.DELTAS)
@pytest.mark.parametrize("cond", pc.CONDS)
def test_truncated_solves(binding, step_problems, cond, delta, k):
    """(b) the estimates after k iterations against the model's, to 8 eps_step of the family."""
    o = dict(STEP_OPTIONS, max_iterations=k, huber_delta=delta)
    nodes0, edges, res, out = solve(binding, pc.step_case(cond), **o)
    pc.check_truncated(f"cond {cond:g} delta {delta} k {k}", nodes0, edges, res, out, pc.eps_step(step_problems, pc.DELTAS, pc.STEPS), **o)


@pytest.mark.parametrize("k", pc.REJECTED_STEPS)
def test_rejected_steps(binding, k):
    """(c) three rejected steps, then accepted ones: while nothing is accepted the nodes stay bit for bit, afterwards as (b)."""
    case = pc.rejected_case()
    o = dict(STEP_OPTIONS, max_iterations=k)
    nodes0, edges, res, out = solve(binding, case, **o)
    eps = pc.eps_step([as_problem(nodes0, edges)], (1.0,), pc.REJECTED_STEPS)
    pc.check_truncated(f"rejected steps, k {k}", nodes0, edges, res, out, eps, **o)
    assert res["accepted_steps"] == pc.REJECTED_ACCEPTED[k - 1] and res["lm_iterations"] == k
    if pc.REJECTED_ACCEPTED[k - 1] == 0:
        assert res["status"] == 0 and pc.bits_equal(out, nodes0) and res["final_cost"] == res["initial_cost"]


@pytest.mark.parametrize("k", (1, 2))
def test_one_pcg_iteration_per_step(binding, k):
    """(d) pcg_max_iterations = 1 against chain_pcg with the same cap; eps_step between the model's two statements of the capped PCG."""
    o = dict(STEP_OPTIONS, max_iterations=k, pcg_max_iterations=1)
    nodes0, edges, res, out = solve(binding, pc.step_case(pc.CONDS[0]), **o)
    eps = pc.eps_step([as_problem(nodes0, edges)], (1.0,), (1, 2), pcg_max_iterations=1)
    pc.check_truncated(f"pcg_max_iterations 1, k {k}", nodes0, edges, res, out, eps, **o)
    assert res["pcg_iterations"] == k


@pytest.mark.parametrize("k", (1, 2))
def test_three_passes_and_a_long_incidence_list(binding, hub, k):
    """(e) 515 nodes, node 7 in 302 edges; and the same bytes from two fresh contexts: the order of the integer atomics does not show."""
    o = dict(STEP_OPTIONS, max_iterations=k)
    nodes0, edges, res, out = solve(binding, pc.hub_case(), **o)
    assert pc.bits_equal(nodes0["q_opt"], hub[0]) and pc.bits_equal(edges, hub[2])
    pc.check_truncated(f"515 nodes, node 7 of degree 302, k {k}", nodes0, edges, res, out, pc.eps_step([hub], (1.0,), (1, 2)), **o)
    _, _, res2, out2 = solve(binding, pc.hub_case(), **o)
    assert res2.tobytes() == res.tobytes() and out2.tobytes() == out.tobytes()


def test_a_huge_huber_delta_is_no_robust_edge(binding):
    """(f) every loop and anchor edge flagged with huber_delta = 1e6 (s never reaches 1e12): bit for bit the unflagged twin of the same call."""
    case = pc.step_case(pc.CONDS[0])
    plain, flagged = dict(case, extra=case["extra"].copy()), dict(case, extra=case["extra"].copy())
    plain["extra"]["flags"], flagged["extra"]["flags"] = 0, pg.EDGE_ROBUST
    gpu, start = entered(binding, [plain, flagged])
    assert pc.edge_s(*as_problem(*start[1])).max() < 1e12
    res = gpu.graph_optimize([0, 1], **dict(OPTIONS, huber_delta=1e6))
    out = [gpu.graph_export(b) for b in range(2)]
    gpu.close()
    print(f"huber_delta 1e6: {res[0]}")
    assert res[0]["status"] == 0 and res[0]["accepted_steps"] > 0
    assert res[0].tobytes() == res[1].tobytes() and out[0].tobytes() == out[1].tobytes()


def test_the_sign_of_an_entered_quaternion_does_not_show(binding):
    """(f) every third entered quaternion negated: t_opt bit for bit, q_opt bit for bit up to its sign."""
    case = pc.step_case(pc.CONDS[0])
    negated = dict(case, q=case["q"] * np.where(np.arange(40) % 3 == 1, -1.0, 1.0)[:, None])
    assert (negated["q"][:, 3] < 0).any()
    gpu, start = entered(binding, [case, negated])
    res = gpu.graph_optimize([0, 1], **OPTIONS)
    out = [gpu.graph_export(b) for b in range(2)]
    gpu.close()
    sign = np.where(np.arange(40) % 3 == 1, -1.0, 1.0)[:, None]
    print(f"negated quaternions: {res[1]}; largest |q_opt -+ q_opt'| {np.abs(out[0]['q_opt'] - sign * out[1]['q_opt']).max():.1e}, |t_opt - t_opt'| {np.abs(out[0]['t_opt'] - out[1]['t_opt']).max():.1e}")
    assert pc.bits_equal(start[1][0]["q"], negated["q"])                                  # entered as given
    assert res[0]["status"] == 0 and res[0]["accepted_steps"] > 0 and res[0].tobytes() == res[1].tobytes()
    assert pc.bits_equal(out[0]["t_opt"], out[1]["t_opt"]) and pc.bits_equal(out[0]["q_opt"], sign * out[1]["q_opt"])


def test_far_from_the_origin(binding):
    """(g) G o X0 solved against G o (X0 solved), G a rotation of (0.3, -1.1, 2.0) rad and a translation of (4.1e5, -5.3e6, 312) m: the
    band is the same difference taken with the model alone (eps |t|, about 1e-9), the device gets 8 x it."""
    near = pc.step_case(pc.CONDS[0])
    gpu, start = entered(binding, [near, pc.moved(near)])
    res = gpu.graph_optimize([0, 1], **OPTIONS)
    out = [gpu.graph_export(b) for b in range(2)]
    gpu.close()
    model = [pg.optimize(*as_problem(*s), **OPTIONS) for s in start]
    band = pg.pose_difference(model[1][0], model[1][1], *pg.compose(pc.FAR_Q, pc.FAR_T, model[0][0], model[0][1]))
    dev = pg.pose_difference(out[1]["q_opt"], out[1]["t_opt"], *pg.compose(pc.FAR_Q, pc.FAR_T, out[0]["q_opt"], out[0]["t_opt"]))
    to_model = pg.pose_difference(out[1]["q_opt"], out[1]["t_opt"], model[1][0], model[1][1])
    print(f"far from the origin: device G o X against G o (device X) {dev:.3e}; the model's band {band:.3e} (tolerance {8 * band:.3e}); device against model, far {to_model:.3e}; "
          f"device {res[1]}; model {model[1][2]}")
    assert res[0]["status"] == 0 and res[1]["status"] == 0 and res[1]["accepted_steps"] > 0
    assert 0.0 < band < 1e-7                                  # eps |t| = 1.2e-9 and its amplification, not a second minimum
    assert dev <= 8 * band and to_model <= 8 * band


def test_a_failing_graph_beside_a_healthy_one(binding):
    """(h) a loop edge with t = (1e200, 0, 0) is finite and accepted; its s overflows: FAILED, termination 5, nothing moved - and the
    healthy sequence of the same call gives the bytes it gives alone."""
    healthy, bad = pc.failing_case()
    gpu, start = entered(binding, [healthy, bad])
    res = gpu.graph_optimize([0, 1], **OPTIONS)
    out = [gpu.graph_export(b) for b in range(2)]
    gpu.close()
    print(f"failing: {res[1]}")
    r = res[1]
    assert (r["status"], r["termination"], r["lm_iterations"], r["accepted_steps"], r["pcg_iterations"]) == (binding.GRAPH_FAILED, 5, 0, 0, 0)
    assert r["initial_cost"] == np.inf and r["final_cost"] == np.inf and (r["nodes"], r["edges"]) == (40, len(bad["edges"]))
    assert pc.bits_equal(out[1], start[1][0])
    with np.errstate(all="ignore"):
        _, _, m = pg.optimize(*as_problem(*start[1]), **OPTIONS)
    assert (m["status"], m["termination"], m["lm_iterations"]) == (2, 5, 0)
    _, _, alone, out_alone = solve(binding, healthy, **OPTIONS)
    assert alone["status"] == 0 and alone["accepted_steps"] > 0
    assert res[0].tobytes() == alone.tobytes() and out[0].tobytes() == out_alone.tobytes()


def test_refused_options_queue_nothing(binding):
    """(i) E_ARG, and both graphs' bytes as they were; max_iterations = 0 is accepted (test_linearisation_alone)."""
    case = pc.step_case(pc.CONDS[0])
    gpu, start = entered(binding, [case, pc.rejected_case()])
    for bad in (dict(pcg_max_iterations=0), dict(pcg_tolerance=-1e-8), dict(function_tolerance=-1.0), dict(gradient_tolerance=-1e-300),
                dict(pcg_tolerance=np.nan), dict(function_tolerance=np.nan), dict(gradient_tolerance=np.nan), dict(function_tolerance=np.inf),
                dict(max_iterations=-1), dict(huber_delta=np.nan), dict(huber_delta=-1.0)):
        with pytest.raises(binding.AloamError) as err:
            gpu.graph_optimize([0, 1], **dict(OPTIONS, **bad))
        assert err.value.code == binding.E_ARG, (bad, err.value)
    now = [(gpu.graph_export(b), gpu.graph_export(b, edges=True)) for b in range(2)]
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(start, now))
    res = gpu.graph_optimize([0, 1], **dict(OPTIONS, max_iterations=0))
    assert all(r["status"] == 0 and r["lm_iterations"] == 0 for r in res)
    gpu.close()
