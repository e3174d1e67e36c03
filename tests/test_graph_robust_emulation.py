"""k_graph_robust without a GPU: the kernel source and the device functions of posegraph_kernels.hip it reaches, compiled for the host
(tests/posegraph_emulation/emulation.hpp, included and not edited: 256 std::threads stand for a workgroup, a std::barrier for __syncthreads)
under AddressSanitizer and UBSan as a stand-alone program, on case A of graph_robust_cases.py against the numpy model, with the assertions
of test_gpu_graph_robust.py.  It checks the kernel's arithmetic, indexing and barriers; what only the device can show is the GPU test's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_robust_cases as rc
import posegraph_cases as pc
from posegraph_cases import OPTIONS, pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "posegraph_emulation")
MAIN = os.path.join(ROOT, "tests", "graph_robust_emulation", "main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")


def _swap(text, pairs):
    for old, new in pairs:
        assert old in text, old
        text = text.replace(old, new)
    return text


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("graph_robust_emulation")
    read = lambda f: open(os.path.join(CSRC, f)).read()
    (d / "posegraph_kernels_host.hpp").write_text(_swap(read("posegraph_kernels.hpp"), [
        ('#include <hip/hip_runtime.h>', ''), ('#include "../../include/aloam_mi355x.h"', ''), ('#include "mapping_kernels.hpp"', ''),
        ('#include "aloam_device.hpp"', '#include "emulation.hpp"')]))
    (d / "posegraph_kernels_host.cpp").write_text(_swap(read("posegraph_kernels.hip"), [
        ('#include "lm_device.hpp"', '#include "emulation.hpp"'), ('#include "posegraph_kernels.hpp"', '#include "posegraph_kernels_host.hpp"')]))
    (d / "graphrobust_kernels_host.hpp").write_text(_swap(read("graphrobust_kernels.hpp"), [('#include "posegraph_kernels.hpp"', '#include "posegraph_kernels_host.hpp"')]))
    (d / "graphrobust_kernels_host.cpp").write_text(_swap(read("graphrobust_kernels.hip"), [
        ('#include "posegraph_kernels.hip"', '#include "posegraph_kernels_host.cpp"'), ('#include "graphrobust_kernels.hpp"', '#include "graphrobust_kernels_host.hpp"')]))
    exe = d / "emulate"
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + str(d), "-I" + EMU,
                        "-I" + os.path.join(ROOT, "include"), MAIN, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run(emulator, q, t, edges, **options):
    """The emulated kernel on one graph entered at (q, t): its result (as_dict), its weight row, the nodes afterwards, and the line of the
    one-node graph listed first."""
    d, exe = emulator
    nodes = np.zeros(len(q), pg.NODE_DTYPE)
    nodes["q"], nodes["t"], nodes["q_opt"], nodes["t_opt"], nodes["frame"] = q, t, q, t, -1
    nodes.tofile(d / "nodes.bin"); edges.tofile(d / "edges.bin")
    r = subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "edges.bin"), "3", str(d / "out.bin")] + [f"{k}={v!r}" for k, v in options.items()], capture_output=True, text=True)
    assert r.returncode == 0 and "GUARD" not in r.stdout and "CHANGED" not in r.stdout and not r.stderr, r.stdout + r.stderr[-3000:]
    raw = open(d / "out.bin", "rb").read()
    res = np.frombuffer(raw[:128], rc.RESULT_DTYPE)[0]
    weights = np.frombuffer(raw[128:128 + 8 * len(edges)], np.float64)
    out = np.frombuffer(raw[128 + 8 * len(edges):], pg.NODE_DTYPE)
    assert len(out) == len(q)
    return rc.as_dict(res), weights, out, r.stdout.splitlines()[0]


def test_the_kernel_source_takes_the_models_decisions_on_case_a(emulator):
    """Case A: the false loops end at weight 0 and the true loops at 1 after the model's 18 outer iterations; the poses are the model's and
    the inlier-only solve's to 8 eps_ref.  The margin condition holds on the model's trace, so the discrete outcome must be equal."""
    case = rc.case_a()
    m = rc.model(case)
    assert m["margin"] >= rc.MARGIN and m["res"]["outer_iterations"] == 18 and m["trace"][-1]["weights"].tolist() == [1, 1, 0, 0, 0]
    res, weights, out, first = run(emulator, case["q"], case["t"], case["edges"], **OPTIONS)
    assert first.startswith("status 1 termination 0 lm 0 accepted 0 pcg 0 nodes 1 edges 0 outer 0 robust 0 inliers 0 outliers 0 mu 0 s_max 0"), first     # the one-node graph: NO_EDGES
    rc.check_against_model("emulated kernel, case A", case, res, weights, out, rc.want_of(m), rc.inlier_solve("a"))
    assert abs(res["truncated_cost"] - m["res"]["truncated_cost"]) <= 1e-9 * m["res"]["truncated_cost"]
    assert abs(res["initial_cost"] - m["res"]["initial_cost"]) <= 1e-12 * m["res"]["initial_cost"]


def test_the_cap_leaves_undecided_weights_on_the_host(emulator):
    case = rc.case_a()
    m = rc.model(case, max_outer_iterations=2)
    res, weights, out, _ = run(emulator, case["q"], case["t"], case["edges"], max_outer_iterations=2, **OPTIONS)
    w = weights[case["edges"]["flags"] != 0]
    print(f"cap 2: weights {w.tolist()} (model {m['trace'][-1]['weights'].tolist()})")
    assert res["status"] == 0 and res["outer_iterations"] == 2 and res["inliers"] + res["outliers"] < res["robust_edges"] == 5
    assert ((w > 0) & (w < 1)).any() and ((m["trace"][-1]["weights"] > 0) & (m["trace"][-1]["weights"] < 1)).any()
    assert abs(res["mu"] - rc.C2 / (2.0 * res["s_max"] - rc.C2) * rc.MU_STEP) <= 1e-12 * res["mu"]


def test_skip_empty_and_failure_on_the_host(emulator):
    """The skip branch (an inlier_chi2 above twice the largest flagged s), an empty R, and a non-finite flagged edge."""
    case = rc.clean_case()
    s = pg.edge_chi2(case["q"], case["t"], case["edges"])[case["edges"]["flags"] != 0]
    res, weights, out, _ = run(emulator, case["q"], case["t"], case["edges"], inlier_chi2=float(2.5 * s.max()), **OPTIONS)
    plain = case["edges"].copy(); plain["flags"] = 0
    q, t, _ = pg.optimize(case["q"], case["t"], plain, **OPTIONS)
    assert (res["status"], res["outer_iterations"], res["mu"], res["inliers"], res["outliers"]) == (0, 1, 0.0, 2, 0) and (weights == 1).all()
    assert pg.pose_difference(out["q_opt"], out["t_opt"], q, t) <= 8 * pc.eps_ref()
    res, weights, out2, _ = run(emulator, case["q"], case["t"], plain, **OPTIONS)
    assert (res["status"], res["outer_iterations"], res["mu"], res["robust_edges"], res["s_max"]) == (0, 1, 0.0, 0, 0.0) and (weights == 1).all()
    assert pc.bits_equal(out2, out)                      # the same weighted problem, so the same bits
    _, bad = pc.failing_case()
    edges = bad["edges"].copy(); edges["flags"][-1] = pg.EDGE_ROBUST
    res, weights, out, _ = run(emulator, bad["q"], bad["t"], edges, **OPTIONS)
    assert (res["status"], res["termination"], res["outer_iterations"], res["lm_iterations"]) == (2, 5, 0, 0) and (weights == 1).all()
    assert pc.bits_equal(out["q_opt"], bad["q"]) and pc.bits_equal(out["t_opt"], bad["t"])
