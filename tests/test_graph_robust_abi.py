"""The robust pose-graph solve, host side (no GPU): the records and entry points in the header, the binding and the library; the defaults;
what can be refused without a device; the words of the definition in the header; the profiling slots, which it leaves alone; the tools'
options."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def test_the_result_dtype_nests_the_plain_result(binding):
    dt = binding.GRAPH_ROBUST_RESULT_DTYPE
    assert dt.fields["solve"][0] == binding.GRAPH_RESULT_DTYPE and dt.fields["solve"][1] == 0 and dt.fields["outer_iterations"][1] == 64
    import graph_robust_cases as rc
    assert rc.RESULT_DTYPE == dt


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in ("aloam_graph_optimize_robust", "aloam_graph_robust_default_options"):
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_optimize_robust", "graph_optimize_robust_into", "graph_robust_options"):
        assert callable(getattr(binding.Aloam, m, None)), m
    o = binding.AloamGraphRobustOptions()
    binding.lib().aloam_graph_robust_default_options(C.byref(o))
    assert (o.max_outer_iterations, o.inlier_chi2, o.mu_step) == (100, 22.46, 1.4) and (o.pad, o.reserved) == (0, 0.0)
    import importlib
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert pg.ROBUST_DEFAULTS == dict(inlier_chi2=22.46, mu_step=1.4, max_outer_iterations=100)
    assert abs(pg.chi2_gate() - o.inlier_chi2) < 5e-3                              # the 6-dof quantile at p = 0.999, rounded
    assert binding.lib().aloam_graph_optimize_robust(None, None, 0, None, None, None, None, 0) == binding.E_ARG      # a null context


def test_header_states_the_definition():
    txt = open(HEADER).read()
    block = txt[txt.index("---- the robust solve"):txt.index("int aloam_graph_optimize_robust(")]
    assert txt.index("---- graph records") < txt.index("---- the robust solve") < txt.index("---- intermediate arrays")
    plain = txt[txt.index("---- pose graphs"):txt.index("---- keyframe clouds")]
    assert "robust solve" not in plain and "aloam_graph_optimize_robust" not in plain          # a section of its own: the pose-graph block is sliced by older tests
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("GNC-TLS", "graduated non-convexity", "truncated least-squares", "Yang, Antonante, Tzoumas, Carlone", "GncOptimizer", "s_e = r^T Omega r",
                 "Omega_e <- w_e Omega_e for e in R and every flag cleared", "There is no Huber in this call: huber_delta is unused", "s_max = max over R",
                 "ALOAM_GRAPH_FAILED with termination 5", "2 s_max - c2 <= 0", "outer_iterations = 1, mu = 0", "counts as an inlier", "mu = c2 / (2 s_max - c2)",
                 "lo = mu / (mu + 1) * c2", "hi = (mu + 1) / mu * c2", "w_e = 1 if s_e <= lo", "w_e = 0 if s_e >= hi", "w_e = sqrt(c2 * mu * (mu + 1) / s_e) - mu",
                 "every weight was exactly 0 or 1", "mu *= mu_step", "only if no inner solve ended as a failure", "accepts nothing is not a failure",
                 "ALOAM_GRAPH_NO_EDGES", "flag loop and anchor edges only", "no host synchronisation", "nothing is queued on any error", "max_outer_iterations >= 1",
                 "inlier_chi2 > 0 and finite", "mu_step > 1 and finite", "classified like dst", "at least the largest edge count listed", "1.0 for unflagged edges",
                 "entries beyond the edge count are not written", "independent of n, of i and of the other sequences listed", "changes only q_opt / t_opt",
                 "byte for byte", "nothing is stored between calls", "should keep being solved with the robust call", "n * row_edges * 256 B", "profiling slot pose_graph",
                 "launches exactly what it launched before"):
        assert word in flat, word


def test_the_profiling_slots_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert not any("robust" in n for n in names)
    assert names[names.index("map_register"):] == ["map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register",
                                                   "save_sequences", "load_sequences", "score_corrections", "apply_corrections"]


def test_the_old_unit_is_included_not_copied_and_left_alone():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    unit = open(os.path.join(csrc, "graphrobust_kernels.hip")).read()
    assert '#define ALOAM_GRAPH_DEVICE_FUNCTIONS_ONLY\n#include "posegraph_kernels.hip"' in unit
    for reused in ("graph_build_incidence", "graph_cost", "graph_linearize_edges", "graph_linearize_nodes", "graph_factor_chain", "graph_apply_chain", "graph_matvec",
                   "graph_dot", "edge_residual", "pg_exp_half", "block_max"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
    assert "atomicAdd" not in unit and "K_POSE_GRAPH" in open(os.path.join(csrc, "capi_graphrobust.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert all(f in mk for f in ("graphrobust_kernels.hip", "capi_graphrobust.hip", "graphrobust_kernels.hpp"))


@pytest.mark.parametrize("tool,option", [("graph_robust_rate.py", "--false-loops"), ("loop_closure_drive.py", "--false-loops")])
def test_the_tools_have_their_options(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
