"""k_graph_marginals without a GPU: the kernel source and the device functions of posegraph_kernels.hip it reaches, compiled for the host
(tests/posegraph_emulation/emulation.hpp: 256 std::threads stand for a workgroup, a std::barrier for __syncthreads) under AddressSanitizer
and UBSan as a stand-alone program, against the numpy model on step_case(1e2) with the seven requests of the gate.  It checks the kernel's
arithmetic, indexing and barriers; what only the device can show is test_gpu_graph_marginals.py's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_marginal_cases as mc
from posegraph_cases import pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "posegraph_emulation")
MAIN = os.path.join(ROOT, "tests", "graph_marginal_emulation", "main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")


def _swap(text, pairs):
    for old, new in pairs:
        assert old in text, old
        text = text.replace(old, new)
    return text


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("graph_marginal_emulation")
    read = lambda f: open(os.path.join(CSRC, f)).read()
    (d / "posegraph_kernels_host.hpp").write_text(_swap(read("posegraph_kernels.hpp"), [
        ('#include <hip/hip_runtime.h>', ''), ('#include "../../include/aloam_mi355x.h"', ''), ('#include "mapping_kernels.hpp"', ''),
        ('#include "aloam_device.hpp"', '#include "emulation.hpp"')]))
    (d / "posegraph_kernels_host.cpp").write_text(_swap(read("posegraph_kernels.hip"), [
        ('#include "lm_device.hpp"', '#include "emulation.hpp"'), ('#include "posegraph_kernels.hpp"', '#include "posegraph_kernels_host.hpp"')]))
    (d / "graphmarginal_kernels_host.hpp").write_text(_swap(read("graphmarginal_kernels.hpp"), [('#include "posegraph_kernels.hpp"', '#include "posegraph_kernels_host.hpp"')]))
    (d / "graphmarginal_kernels_host.cpp").write_text(_swap(read("graphmarginal_kernels.hip"), [
        ('#include "posegraph_kernels.hip"', '#include "posegraph_kernels_host.cpp"'), ('#include "graphmarginal_kernels.hpp"', '#include "graphmarginal_kernels_host.hpp"')]))
    exe = d / "emulate"
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + str(d), "-I" + EMU,
                        "-I" + os.path.join(ROOT, "include"), MAIN, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run(emulator, q, t, edges, req, **options):
    """The emulated kernel on one graph at the estimates (q, t): the results of the requests, and the line of the one-node request put first."""
    d, exe = emulator
    nodes = np.zeros(len(q), pg.NODE_DTYPE)
    nodes["q"], nodes["t"], nodes["q_opt"], nodes["t_opt"], nodes["frame"] = q, t, q, t, -1
    nodes.tofile(d / "nodes.bin"); edges.tofile(d / "edges.bin"); req.tofile(d / "req.bin")
    r = subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "edges.bin"), str(d / "req.bin"), "3", str(d / "out.bin")] + [f"{k}={v!r}" for k, v in options.items()],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "GUARD" not in r.stdout and "CHANGED" not in r.stdout and not r.stderr, r.stdout + r.stderr[-3000:]
    return np.fromfile(d / "out.bin", mc.RESULT_DTYPE), r.stdout.splitlines()[0]


def test_the_kernel_source_gives_the_models_marginals_on_the_host(emulator):
    case, q, t = mc.solved(1e2)
    cand = mc.candidates(case)
    eps = mc.model_pair(q, t, case["edges"], cand)["eps"]
    res, first = run(emulator, q, t, case["edges"], mc.requests(cand), pcg_tolerance=mc.TOL)
    assert first.startswith("status 1 mode 0 seq 1 i -1 j 0 pcg 0 nodes 1 edges 0 chi2 0 s_edge 0"), first      # the one-node graph: NO_EDGES
    mc.check_against_model("emulated kernel, cond 1e2", res, q, t, case["edges"], cand, eps)
    assert (res["chi2"][:6] < mc.GATE).all() and res["chi2"][6] > mc.GATE
    assert (res["q"] == cand["q"]).all() and (res["t"] == cand["t"]).all() and (res["mode"] == 0).all() and (res["seq"] == 0).all()
    lin = pg.linearize(q, t, cand)
    assert np.abs(res["r"] - lin[0]).max() <= 1e-14 * max(1.0, np.abs(lin[0]).max())


def test_at_estimate_and_the_fixed_node_on_the_host(emulator):
    """AT_ESTIMATE: Z of the estimates, r at rounding, chi2 = s_edge = 0; the request (-1, 0) has no column to solve."""
    case, q, t = mc.solved(1e2)
    cand = np.concatenate([mc.candidates(case)[:3], pg.marginal_request(0, [-1], [0])["edge"]])
    mode = np.array([1, 1, 1, 0], np.int32)
    eps = mc.model_pair(q, t, case["edges"], mc.candidates(case))["eps"]
    res, _ = run(emulator, q, t, case["edges"], mc.requests(cand, mode), pcg_tolerance=mc.TOL)
    model = pg.marginals(q, t, case["edges"], cand, mode)
    dev = mc.deviation(res, model)
    print(f"AT_ESTIMATE: against the model {dev:.3e} (tolerance {8 * eps:.3e}); |r| {np.abs(res['r']).max():.1e}; PCG {res['pcg_iterations'].tolist()}")
    assert (res["status"] == 0).all() and dev <= 8 * eps
    assert np.abs(res["r"][:3]).max() <= 1e-14 and (res["chi2"][:3] == 0).all() and (res["s_edge"][:3] == 0).all()
    assert np.abs(res["q"][:3] - model["q"][:3]).max() <= 1e-14 and np.abs(res["t"][:3] - model["t"][:3]).max() <= 1e-14
    assert res["pcg_iterations"][3] == 0 and not res["cov"][3].any() and res["chi2"][3] == res["s_edge"][3] > 0


def test_a_capped_column_is_reported_on_the_host(emulator):
    case, q, t = mc.solved(1e2)
    cand = mc.candidates(case)[:2]
    res, _ = run(emulator, q, t, case["edges"], mc.requests(cand), pcg_max_iterations=1)
    one = pg.marginals(q, t, case["edges"], cand, solve=pg.marginal_solver(1e-10, 1))
    assert (res["status"] == pg.MARGINAL_NOT_CONVERGED).all() and (res["pcg_iterations"] == 6).all() and (one["status"] == pg.MARGINAL_NOT_CONVERGED).all()
    assert mc.deviation(res, one) <= 1e-9
