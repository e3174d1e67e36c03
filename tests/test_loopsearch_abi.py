"""A pose grid searched around a loop guess, host side (no GPU): the records and entry points in the header, the binding and the library;
the default grid; the profiling list; the units in the Makefile; what can be refused without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from test_posegraph_abi import HEADER, ROOT

CALLS = ("aloam_graph_loop_default_search", "aloam_graph_search_loops")
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_loop_search", "graph_search_loops_into", "graph_search_loops"):
        assert callable(getattr(binding.Aloam, m, None)), m
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert d.index("aloam_graph_register_loops(") < d.index("aloam_graph_loop_default_search(") < d.index("aloam_graph_search_loops(") < d.index("aloam_graph_marginals(")
    txt = open(HEADER).read()
    assert txt.index("---- loop edges measured on the device") < txt.index("---- a pose grid searched around a loop guess") < txt.index("---- pose-graph marginals")
    loopreg = __import__("importlib").import_module("a-loam_amd.loopreg")
    assert callable(loopreg.search_grid) and callable(loopreg.search_best)


def test_the_default_grid_is_relocalizes_steps(binding):
    g = binding.AloamGraphLoopSearch()
    binding.lib().aloam_graph_loop_default_search(C.byref(g))
    assert (g.radius_m, g.step_m, g.yaw_deg, g.yaw_step_deg) == (3.0, 0.5, 12.5, 2.5)
    binding.lib().aloam_graph_loop_default_search(None)
    import loopsearch_model
    assert loopsearch_model.DEFAULT_GRID == (3.0, 0.5, 12.5, 2.5)


def test_a_null_context_is_an_argument_error(binding):
    assert binding.lib().aloam_graph_search_loops(None, None, 0, None, None, None, None, None) == binding.E_ARG


def test_header_states_the_definition():
    txt = open(HEADER).read()
    block = txt[txt.index("---- a pose grid searched around a loop guess"):txt.index("typedef struct aloam_graph_loop_search {")]
    block = " ".join(block.replace("\n *", " ").split())
    for word in ("no host synchronisation", "keeps its behaviour and its launches", "floor(radius_m / step_m + 1e-9)", "floor(yaw_deg / yaw_step_deg + 1e-9)",
                 "K = (2a + 1)(2m + 1)^2", "yaw outermost, then y, then x", "q_c = dq q_g", "dq = (0, 0, sin h, cos h)", "h = (dyaw * (pi / 180)) / 2",
                 "t_c = t_g + (dx, dy, 0)", "the centre node is the guess bit for bit", "Roll, pitch and z are not searched", "computed on the host", "a <= 31",
                 "no transformAssociateToMap", "round 0 of a registration started from that node", "HuberLoss(0.1)", "NaN ranks as +infinity", "then the lower index",
                 "the centre node (the guess) is taken", "`parameters` := the best node's pose", "Z in the loop result is still the request's guess", "best = -1",
                 "1 <= K <= 2^14", "min(max_requests, 2^18 / K)", "ALOAM_E_HIP and nothing of it stays allocated", "do not depend on n", "no floating-point atomics",
                 "byte for byte what aloam_graph_register_loops writes", "every f64 operation is separately rounded"):
        assert word in block, word


def test_the_profiling_names_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names[names.index("export_clouds"):] == ["export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register", "save_sequences",
                                                    "load_sequences", "score_corrections", "apply_corrections"]
    assert not [n for n in names if "search" in n]


def test_the_makefile_builds_the_new_units_and_they_keep_to_themselves():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "loopsearch_kernels.hip" in src and "loopsearch_kernels.hpp" in hdr and "map_score_device.hpp" in hdr
    unit = open(os.path.join(CSRC, "loopsearch_kernels.hip")).read()
    assert "loopreg" not in unit and "atomicAdd(double" not in unit and "atomicAdd" not in unit
    assert '#include "map_score_device.hpp"' in unit and '#include "map_score_device.hpp"' in open(os.path.join(CSRC, "relocalize_kernels.hip")).read()
    # one copy of the per-point body: the shared header holds it, neither unit restates it
    assert "void score_point(" in open(os.path.join(CSRC, "map_score_device.hpp")).read()
    for f in ("loopsearch_kernels.hip", "relocalize_kernels.hip"):
        assert "void score_point(" not in open(os.path.join(CSRC, f)).read(), f
    host = open(os.path.join(CSRC, "capi_loopreg.hip")).read()
    assert "launch_loop_search(" in host and host.count("launch_map_associate(") == 1     # one body behind both entry points


@pytest.mark.parametrize("tool", ["loop_register_rate.py", "loop_closure_drive.py"])
def test_the_tools_answer_help_with_search(tool):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--search" in r.stdout, r.stdout + r.stderr
