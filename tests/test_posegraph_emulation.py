"""k_pose_graph without a GPU: the kernel source compiled for the host (tests/posegraph_emulation: 256 std::threads stand for a workgroup, a
std::barrier for __syncthreads) under AddressSanitizer and UBSan as a stand-alone program, on one graph that takes every path - more nodes
than the workgroup has threads, loop edges in both orientations, anchors, a robust outlier edge - against the numpy model.  It checks the
kernel's arithmetic, indexing and barriers; what only the device can show (the compiler's code, the runtime) is test_gpu_posegraph.py's.
The second half runs the cases of test_gpu_posegraph_steps.py (posegraph_cases.py: dense information, a solve stopped after k iterations,
rejected steps, a capped PCG, 515 nodes with a hub of degree 302) with the assertions of the GPU tests, at the sizes that stay quick here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import posegraph_cases as pc
from posegraph_cases import OPTIONS, eps_ref, pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "posegraph_emulation")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("posegraph_emulation")
    hpp = open(os.path.join(CSRC, "posegraph_kernels.hpp")).read()
    for line in ('#include <hip/hip_runtime.h>', '#include "../../include/aloam_mi355x.h"', '#include "mapping_kernels.hpp"'):
        assert line in hpp
        hpp = hpp.replace(line, "")
    hpp = hpp.replace('#include "aloam_device.hpp"', '#include "emulation.hpp"')
    hip = open(os.path.join(CSRC, "posegraph_kernels.hip")).read()
    assert '#include "lm_device.hpp"' in hip and '#include "posegraph_kernels.hpp"' in hip
    hip = hip.replace('#include "lm_device.hpp"', '#include "emulation.hpp"').replace('#include "posegraph_kernels.hpp"', '#include "posegraph_kernels_host.hpp"')
    (d / "posegraph_kernels_host.hpp").write_text(hpp)
    (d / "posegraph_kernels_host.cpp").write_text(hip)
    exe = d / "emulate"
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + str(d), "-I" + EMU,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(EMU, "main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def _solve(emulator, name, q0, t0, edges):
    """The emulated kernel on one graph against the model: returns the exported nodes after the checks both tests share."""
    d, exe = emulator
    nodes = np.zeros(len(q0), pg.NODE_DTYPE)
    nodes["q"], nodes["t"] = q0, t0
    nodes["q_opt"], nodes["t_opt"] = q0, t0
    nodes.tofile(d / "nodes.bin")
    edges.tofile(d / "edges.bin")
    r = subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "edges.bin"), "3", str(d / "out.bin"), "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "GUARD" not in r.stdout and not r.stderr, r.stdout + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("status 1 ") and lines[1].startswith("status 0 "), r.stdout        # the one-node item: NO_EDGES
    out = np.fromfile(d / "out.bin", pg.NODE_DTYPE)
    q, t, m = pg.optimize(q0, t0, edges, **OPTIONS)
    _, _, mc = pg.chain_pcg(q0, t0, edges, **OPTIONS)
    dev = pg.pose_difference(out["q_opt"], out["t_opt"], q, t)
    pcg = int(lines[1].split(" pcg ")[1].split()[0])
    print(f"{name}: {lines[1]}\nmodel {m}\nemulated kernel vs model: {dev:.3e} (tolerance {8 * eps_ref():.1e}); PCG {pcg}, model chain_pcg {mc['pcg_iterations']}")
    assert dev <= 8 * eps_ref() and pcg <= 2 * mc["pcg_iterations"]
    assert out["q"].tobytes() == nodes["q"].tobytes() and out["t"].tobytes() == nodes["t"].tobytes()      # the entered poses never change
    assert abs(pg.cost(out["q_opt"], out["t_opt"], edges) - m["final_cost"]) <= 8 * eps_ref() < m["initial_cost"] - m["final_cost"]
    return out


def test_the_kernel_source_solves_a_mixed_graph_on_the_host(emulator):
    g = pg.drifted_laps(1, 270, 2)
    rng = np.random.default_rng(5)
    back = pg.make_edges(0, [200], [20], *pg.relative_pose(g["q_true"][200], g["t_true"][200], g["q_true"][20], g["t_true"][20]), g["info"])   # i > j
    anchors = np.concatenate([pg.anchor_from_localization(j, g["q_true"][j], g["t_true"][j] + 0.02 * rng.standard_normal(3), g["info"]) for j in (90, 269)])
    _solve(emulator, "270 nodes, 3 loops, 2 anchors", g["q"], g["t"], np.concatenate([g["odom"], g["loop"], back, anchors]))


def test_the_kernel_source_discounts_a_robust_outlier_on_the_host(emulator):
    g = pg.drifted_laps(7, 30, 2)
    outlier = g["loop"][:1].copy()
    outlier["i"], outlier["j"] = 3, 22
    outlier["t"] += [3.0, -2.0, 0.5]
    outlier["flags"] = pg.EDGE_ROBUST
    _solve(emulator, "30 nodes, a robust outlier", g["q"], g["t"], np.concatenate([g["odom"], g["loop"], outlier]))


# ---- the cases of test_gpu_posegraph_steps.py -------------------------------------------------------------------------------------------
def run(emulator, case, **options):
    """The emulated kernel on a case of posegraph_cases with the given options: (nodes as entered, result, nodes afterwards)."""
    d, exe = emulator
    nodes = np.zeros(len(case["q"]), pg.NODE_DTYPE)
    nodes["q"], nodes["t"], nodes["q_opt"], nodes["t_opt"], nodes["frame"] = case["q"], case["t"], case["q"], case["t"], -1
    nodes.tofile(d / "nodes.bin")
    case["edges"].tofile(d / "edges.bin")
    keys = ("max_iterations", "pcg_max_iterations", "pcg_tolerance", "huber_delta", "function_tolerance")
    r = subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "edges.bin"), "3", str(d / "out.bin")] + [f"{k}={options[k]!r}" for k in keys if k in options],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "GUARD" not in r.stdout and not r.stderr, r.stdout + r.stderr[-3000:]
    w = r.stdout.splitlines()[1].split()
    res = dict(status=int(w[1]), termination=int(w[3]), lm_iterations=int(w[5]), accepted_steps=int(w[7]), pcg_iterations=int(w[9]), nodes=int(w[11]),
               edges=int(w[13]), initial_cost=float(w[15]), final_cost=float(w[17]), gradient_max=float(w[19]))
    assert res["nodes"] == len(nodes) and res["edges"] == len(case["edges"])
    return nodes, res, np.fromfile(d / "out.bin", pg.NODE_DTYPE)


def problems(cases):
    return [(c["q"], c["t"], c["edges"]) for c in cases]


STEP_PROBLEMS = lambda: problems(pc.step_case(c) for c in pc.CONDS)


@pytest.mark.parametrize("delta", pc.DELTAS)
@pytest.mark.parametrize("cond", pc.CONDS)
def test_linearisation_alone_on_the_host(emulator, cond, delta):
    case = pc.step_case(cond)
    nodes0, res, out = run(emulator, case, **dict(pc.STEP_OPTIONS, max_iterations=0, huber_delta=delta))
    pc.check_linearisation(f"cond {cond:g} delta {delta}", nodes0, case["edges"], res, out, delta, pc.eps_lin(STEP_PROBLEMS()))


@pytest.mark.parametrize("delta", pc.DELTAS)
@pytest.mark.parametrize("cond", pc.CONDS)
def test_truncated_solves_on_the_host(emulator, cond, delta):
    case = pc.step_case(cond)
    eps = pc.eps_step(STEP_PROBLEMS(), pc.DELTAS, pc.STEPS)
    for k in pc.STEPS:
        o = dict(pc.STEP_OPTIONS, max_iterations=k, huber_delta=delta)
        nodes0, res, out = run(emulator, case, **o)
        pc.check_truncated(f"cond {cond:g} delta {delta} k {k}", nodes0, case["edges"], res, out, eps, **o)


def test_rejected_steps_on_the_host(emulator):
    case = pc.rejected_case()
    eps = pc.eps_step(problems([case]), (1.0,), pc.REJECTED_STEPS)
    accepted = []
    for k in pc.REJECTED_STEPS:
        o = dict(pc.STEP_OPTIONS, max_iterations=k)
        nodes0, res, out = run(emulator, case, **o)
        pc.check_truncated(f"rejected steps, k {k}", nodes0, case["edges"], res, out, eps, **o)
        accepted.append(res["accepted_steps"])
    assert accepted == pc.REJECTED_ACCEPTED


def test_one_pcg_iteration_per_step_on_the_host(emulator):
    case = pc.step_case(pc.CONDS[0])
    eps = pc.eps_step(problems([case]), (1.0,), (1, 2), pcg_max_iterations=1)
    for k in (1, 2):
        o = dict(pc.STEP_OPTIONS, max_iterations=k, pcg_max_iterations=1)
        nodes0, res, out = run(emulator, case, **o)
        pc.check_truncated(f"pcg_max_iterations 1, k {k}", nodes0, case["edges"], res, out, eps, **o)


def test_three_passes_and_a_long_incidence_list_on_the_host(emulator):
    case = pc.hub_case()
    o = dict(pc.STEP_OPTIONS, max_iterations=1)
    eps = pc.eps_step(problems([case]), (1.0,), (1,))
    nodes0, res, out = run(emulator, case, **o)
    pc.check_truncated("515 nodes, node 7 of degree 302, k 1", nodes0, case["edges"], res, out, eps, **o)
    _, res2, out2 = run(emulator, case, **o)                     # the atomics' order must not show
    assert res2 == res and out2.tobytes() == out.tobytes()


def test_exact_properties_on_the_host(emulator):
    """Three iterations are enough for a property that holds bit for bit at any."""
    case = pc.step_case(pc.CONDS[0])
    o = dict(pc.STEP_OPTIONS, max_iterations=3)
    plain, flagged = case["extra"].copy(), case["extra"].copy()
    plain["flags"], flagged["flags"] = 0, pg.EDGE_ROBUST
    a = run(emulator, dict(case, edges=np.concatenate([case["odom"], plain])), **dict(o, huber_delta=1e6))
    b = run(emulator, dict(case, edges=np.concatenate([case["odom"], flagged])), **dict(o, huber_delta=1e6))
    assert a[1]["accepted_steps"] == 3 and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    sign = np.where(np.arange(40) % 3 == 1, -1.0, 1.0)[:, None]
    c, d = run(emulator, case, **o), run(emulator, dict(case, q=sign * case["q"]), **o)
    assert c[1]["accepted_steps"] == 3 and c[1] == d[1]
    assert c[2]["t_opt"].tobytes() == d[2]["t_opt"].tobytes() and c[2]["q_opt"].tobytes() == (sign * d[2]["q_opt"]).tobytes()


def test_an_overflowing_edge_fails_on_the_host(emulator):
    nodes0, res, out = run(emulator, pc.failing_case()[1], **OPTIONS)
    print(res)
    assert (res["status"], res["termination"], res["lm_iterations"], res["accepted_steps"], res["pcg_iterations"]) == (2, 5, 0, 0, 0)
    assert res["initial_cost"] == np.inf == res["final_cost"] and out.tobytes() == nodes0.tobytes()
