"""Pose-graph marginals, host side (no GPU): the records and entry points in the header, the binding, the model and the library; the
profiling slot; what can be refused without a device; the tools' options."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def test_the_model_uses_the_same_records_and_constants(binding):
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert pg.MARGINAL_REQUEST_DTYPE == binding.GRAPH_MARGINAL_REQUEST_DTYPE
    assert (pg.MARGINAL_MEASURED, pg.MARGINAL_AT_ESTIMATE) == (binding.GRAPH_MARGINAL_MEASURED, binding.GRAPH_MARGINAL_AT_ESTIMATE) == (0, 1)
    assert (pg.MARGINAL_OK, pg.MARGINAL_NO_EDGES, pg.MARGINAL_NOT_CONVERGED, pg.MARGINAL_FAILED) == (0, 1, 2, 3) == \
        (binding.GRAPH_MARGINAL_OK, binding.GRAPH_MARGINAL_NO_EDGES, binding.GRAPH_MARGINAL_NOT_CONVERGED, binding.GRAPH_MARGINAL_FAILED)
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "enum { ALOAM_GRAPH_MARGINAL_MEASURED = 0, ALOAM_GRAPH_MARGINAL_AT_ESTIMATE = 1 };" in d
    assert ("enum { ALOAM_GRAPH_MARGINAL_OK = 0, ALOAM_GRAPH_MARGINAL_NO_EDGES = 1, ALOAM_GRAPH_MARGINAL_NOT_CONVERGED = 2, "
            "ALOAM_GRAPH_MARGINAL_FAILED = 3 };") in d
    internal = open(os.path.join(ROOT, "a-loam_amd", "csrc", "information_device.hpp")).read()
    assert "kInfoPivotTol = %g" % pg.INFO_PIVOT_TOL in internal
    r = pg.marginal_request(3, [1, -1], [4, 2], mode=[0, 1])
    assert r.dtype == pg.MARGINAL_REQUEST_DTYPE and r["edge"]["seq"].tolist() == [3, 3] and r["mode"].tolist() == [0, 1] and r["edge"]["i"].tolist() == [1, -1]
    assert abs(pg.chi2_gate() - 22.4577) < 1e-4 and abs(pg.chi2_gate(3, 0.95) - 7.8147) < 1e-4


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in ("aloam_graph_marginals", "aloam_graph_marginal_default_options"):
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_marginals", "graph_marginals_into", "graph_marginal_options"):
        assert callable(getattr(binding.Aloam, m, None)), m
    o = binding.AloamGraphMarginalOptions()
    binding.lib().aloam_graph_marginal_default_options(C.byref(o))
    assert (o.pcg_max_iterations, o.pcg_tolerance, o.huber_delta) == (200, 1e-10, 1.0)
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert pg.MARGINAL_DEFAULTS == dict(pcg_max_iterations=200, pcg_tolerance=1e-10, huber_delta=1.0)
    assert binding.lib().aloam_graph_marginals(None, None, 0, None, None) == binding.E_ARG      # a null context


def test_header_states_the_definition():
    txt = open(HEADER).read()
    block = txt[txt.index("---- pose-graph marginals"):txt.index("typedef struct aloam_graph_marginal_request")]
    assert txt.index("---- loop edges measured on the device") < txt.index("---- pose-graph marginals") < txt.index("---- intermediate arrays")
    for word in ("chi2 = r^T (Sigma_r + Omega^-1)^-1 r", "(q_opt, t_opt)", "node 0 fixed", "no\n *     Levenberg-Marquardt damping", "never robustified",
                 "H y_c = (J^T)_c", "(M + M^T) / 2", "RIGHT tangent of Z", "takes 0 iterations", "s_edge = r^T Omega r", "With Sigma_r = 0, chi2 is s_edge",
                 "Z := X_i^-1 o X_j", "ignored and not validated", "ALOAM_GRAPH_MARGINAL_OK", "NO_EDGES", "NOT_CONVERGED", "FAILED", "ALOAM_E_STATE before aloam_graph_enable",
                 "n = 0 is ALOAM_OK", "pinned\n *   staging ring", "any number of times", "do not depend on n, on r, on the\n *   round", "writes\n * nothing in them", "1 GiB",
                 "launches exactly what it launched\n * before"):
        assert word in block, word


def test_the_profiling_slot_leaves_the_pinned_ones_where_they_are(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names.index("graph_marginals") == names.index("map_register") + 1 == names.index("export_clouds") - 1
    # what the older ABI tests pin, restated: every later slot keeps its neighbours
    assert names[names.index("export_clouds"):] == ["export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register", "save_sequences",
                                                    "load_sequences", "score_corrections", "apply_corrections"]


def test_the_edge_checks_are_shared_and_the_old_unit_is_included_not_copied():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    host = open(os.path.join(csrc, "capi_graphmarginal.hip")).read()
    assert "graph_edge_check(c, it.rq.edge" in host and "graph_edge_check(c, e, true)" in open(os.path.join(csrc, "capi_posegraph.hip")).read()
    unit = open(os.path.join(csrc, "graphmarginal_kernels.hip")).read()
    assert '#define ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY\n#include "posegraph_kernels.hip"' in unit
    for reused in ("graph_build_incidence", "graph_linearize_edges", "graph_linearize_nodes", "graph_factor_chain", "graph_apply_chain", "graph_matvec", "graph_dot",
                   "edge_residual", "edge_rho", "pg_relative"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
    assert "atomicAdd" not in unit and "atomicAdd(double" not in open(os.path.join(csrc, "posegraph_kernels.hip")).read()


def test_loop_results_go_into_the_gate(binding):
    lr = importlib.import_module("a-loam_amd.loopreg")
    pg = importlib.import_module("a-loam_amd.posegraph")
    res = np.zeros(1, binding.GRAPH_LOOP_RESULT_DTYPE)
    res["q"], res["t"], res["info"] = [0, 0, 0, 2.0], [1, 2, 3], pg.info_upper(np.eye(6) * 3)
    r = lr.request_from_result(res[0], 4, 9, 1)
    e = lr.edge_from_result(res[0], 1, 4, 9, robust=False)
    assert r.dtype == pg.MARGINAL_REQUEST_DTYPE and r["edge"].tobytes() == e.tobytes() and r["mode"][0] == pg.MARGINAL_MEASURED
    assert (r["edge"]["seq"][0], r["edge"]["i"][0], r["edge"]["j"][0]) == (1, 4, 9) and r["edge"]["q"][0].tolist() == [0, 0, 0, 1]
    res["status"] = binding.LOOP_SOLVE_FAILED
    assert lr.request_from_result(res[0], 4, 9, 1) is None


@pytest.mark.parametrize("tool,option", [("graph_marginal_rate.py", "--shapes"), ("loop_closure_drive.py", "--device-loops")])
def test_the_tools_have_their_options(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
