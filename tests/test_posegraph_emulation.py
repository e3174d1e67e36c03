"""k_pose_graph without a GPU: the kernel source compiled for the host (tests/posegraph_emulation: 256 std::threads stand for a workgroup, a
std::barrier for __syncthreads) under AddressSanitizer and UBSan as a stand-alone program, on one graph that takes every path - more nodes
than the workgroup has threads, loop edges in both orientations, anchors, a robust outlier edge - against the numpy model.  It checks the
kernel's arithmetic, indexing and barriers; what only the device can show (the compiler's code, the runtime) is test_gpu_posegraph.py's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

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
