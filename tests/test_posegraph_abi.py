"""Pose graphs, host side (no GPU): the records and entry points in the header, the binding and the library; the profiling slot; what can
be refused without a device; where the per-sequence counts live."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CALLS = ("aloam_graph_default_options", "aloam_graph_enable", "aloam_graph_add_nodes", "aloam_graph_add_edges", "aloam_graph_export",
         "aloam_graph_export_edges", "aloam_graph_clear", "aloam_graph_info", "aloam_graph_optimize")


def test_the_model_uses_the_same_records(binding):
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert pg.NODE_DTYPE == binding.GRAPH_NODE_DTYPE and pg.EDGE_DTYPE == binding.GRAPH_EDGE_DTYPE and pg.EDGE_ROBUST == binding.GRAPH_EDGE_ROBUST


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_enable", "graph_add_nodes", "graph_add_edges", "graph_optimize", "graph_optimize_into", "graph_export", "graph_export_into",
              "graph_clear", "graph_info"):
        assert callable(getattr(binding.Aloam, m, None)), m
    assert (binding.GRAPH_OK, binding.GRAPH_NO_EDGES, binding.GRAPH_FAILED) == (0, 1, 2)
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "enum { ALOAM_GRAPH_EDGE_ROBUST = 1 };" in d and "enum { ALOAM_GRAPH_OK = 0, ALOAM_GRAPH_NO_EDGES = 1, ALOAM_GRAPH_FAILED = 2 };" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                                   # the graph is not part of a sequence record
    o = binding.AloamGraphOptions()
    binding.lib().aloam_graph_default_options(C.byref(o))
    assert (o.max_iterations, o.function_tolerance, o.gradient_tolerance, o.pcg_tolerance) == (20, 1e-10, 1e-10, 1e-8)
    assert o.pcg_max_iterations >= 1 and o.huber_delta > 0


def test_header_states_the_problem_and_the_lifetime():
    txt = open(HEADER).read()
    block = txt[txt.index("---- pose graphs"):txt.index("typedef struct aloam_graph_node")]
    for word in ("E = Z^-1 o X_i^-1 o X_j", "negated when its w < 0", "r = (2 q_E.xyz, t_E)", "HuberLoss(huber_delta)", "Node 0 is held fixed", "LEFT perturbation",
                 "aloam_pose_information.info", "anchor", "X_opt[k-1] o Z", "ALOAM_E_CAPACITY", "within 1e-6 of unit norm", "positive definite",
                 "NOT part of a sequence record", "aloam_reset_sequences", "aloam_load_sequences", "clears a slot's graph", "pageable",
                 "not above the initial one", "do not depend on n", "block-tridiagonal chain"):
        assert word in block, word


def test_profiling_slot_follows_pose_information(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names.index("pose_graph") == names.index("pose_information") + 1
    # what the older ABI tests pin, restated
    assert names.index("pose_information") == names.index("export_clouds") + 1
    assert names[-3] == "load_sequences" and names[-2:] == ["score_corrections", "apply_corrections"]


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids = (C.c_int * 1)(0)
    out = (C.c_int * 4)()
    info = np.zeros(21)
    edge = np.zeros(1, binding.GRAPH_EDGE_DTYPE)
    assert L.aloam_graph_enable(None, 4, 4) == binding.E_ARG
    assert L.aloam_graph_add_nodes(None, ids, 1, info.ctypes.data_as(C.c_void_p)) == binding.E_ARG
    assert L.aloam_graph_add_edges(None, edge.ctypes.data_as(C.c_void_p), 1) == binding.E_ARG
    assert L.aloam_graph_export(None, 0, 0, 0, None) == binding.E_ARG
    assert L.aloam_graph_export_edges(None, 0, 0, 0, None) == binding.E_ARG
    assert L.aloam_graph_clear(None, ids, 1) == binding.E_ARG
    assert L.aloam_graph_info(None, 0, out) == binding.E_ARG
    assert L.aloam_graph_optimize(None, ids, 1, None, None) == binding.E_ARG


def test_counts_are_seqhost_fields_assigned_by_the_events_only():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    internal = open(os.path.join(csrc, "capi_internal.hpp")).read()
    seqhost = internal[internal.index("struct SeqHost {"):internal.index("struct aloam_ctx {")]
    assert "graph_nodes" in seqhost and "graph_edges" in seqhost
    assign = re.compile(r"\bgraph_(nodes|edges)\s*(=[^=]|\+=|-=|\+\+|--)|(\+\+|--)\s*[\w.\->\[\]]*graph_(nodes|edges)\b")
    for f in os.listdir(csrc):
        if f.endswith(".hip") and f != "capi_seq.hip":
            txt = open(os.path.join(csrc, f)).read()
            assert not assign.search(txt), f
    events = open(os.path.join(csrc, "capi_seq.hip")).read()
    for name in ("on_graph_nodes_added", "on_graph_edges_added", "on_graph_cleared"):
        assert name in events and name in internal, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("on_graph_nodes_added", "on_graph_edges_added", "on_graph_cleared"):
        assert "| `%s`" % name[3:] in design, name                               # §7b's table has their rows (it drops the on_)


def test_the_rate_tool_has_its_options():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pose_graph_rate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--repeats" in r.stdout, r.stdout + r.stderr
