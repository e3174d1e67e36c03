"""The in-place trim of pose graphs, host side (no GPU): the entry point in the header, the binding and the library; the words of the
definition in the header; the profiling slots and the records, which it leaves alone; the event that sets the counts; the unit's reuse of
the pose device functions and its one chunk constant; the Makefile; the tools' options."""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")


def test_the_call_is_declared_exported_and_bound(binding):
    binding.build()
    assert "aloam_graph_trim" in binding.declared_symbols() and hasattr(binding.lib(), "aloam_graph_trim")
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T aloam_graph_trim\b", out)
    assert callable(getattr(binding.Aloam, "graph_trim", None))
    pg = importlib.import_module("a-loam_amd.posegraph")
    gr = importlib.import_module("a-loam_amd.graph_records")
    assert callable(pg.trim) and callable(pg.trim_classes) and callable(gr.trim_keyframes) and callable(gr.descriptors)
    assert binding.lib().aloam_graph_trim(None, None, None, 0, None) == binding.E_ARG                                 # a null context


def test_header_states_the_definition():
    txt = open(HEADER).read()
    assert txt.index("---- loop candidates by pose proximity") < txt.index("---- trimming a graph in place") < txt.index("---- intermediate arrays")
    assert txt.index("int aloam_graph_propose_loops(") < txt.index("---- trimming a graph in place")
    block = txt[txt.index("---- trimming a graph in place"):txt.index("int aloam_graph_trim(")]
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("f = first[k] is the old index of the node that becomes node 0", "Nodes [0, f) are dropped", "becomes node n - f, a bit copy of its 128 bytes",
                 "the node every solver holds fixed", "conditions on the dropped nodes and on node f at their current estimates", "does not marginalise",
                 "in their stored order (a stable compaction)", "j > f and (i >= f or i == -1): kept", "i' = i - f (or -1), j' = j - f",
                 "Z, info and flags are bit copies", "j > f and 0 <= i < f: anchored", "Z' = X_opt[i] o Z", "quat_mul(q_opt_i, q_Z)",
                 "quat_rotate(q_opt_i, t_Z) + t_opt_i", "every f64 operation rounded on its own", "stored as computed, not renormalised",
                 "E = Z'^-1 o X_j is the old Z^-1 o X_i^-1 o X_j", "residual, tangent, Huber weight and information are unchanged",
                 "i > f and j == f: kept, i' = i - f, j' = 0", "i > f and 0 <= j < f: removed and counted as removed_reverse", "no exact anchor form exists",
                 "only ever produce i < j", "touches no node above f", "removed and counted as removed_fixed", "d = desc[f].first[cls] and m = cursor[cls] - d",
                 "Points [d, d + m) move to [0, m)", "with first -= d, counts unchanged", "the cursor becomes m", "nodes kept without clouds stay",
                 "{nodes, edges, anchored, removed_fixed, removed_reverse, corner points freed, surf points freed, 0}", "may be NULL",
                 "Checked before anything is queued", "seqs distinct and in range", "0 <= first[k] < nodes", "first[k] == 0 is allowed and changes nothing",
                 "ALOAM_E_STATE before aloam_graph_enable", "n = 0 is ALOAM_OK", "pinned staging ring", "SYNCHRONISES the context's stream once",
                 "as aloam_graph_export_map does", "the host holds no copy of the edge endpoints", "once per many keyframes",
                 "aloam_graph_export_map or aloam_graph_save", "do not depend on n, on its position in the list or on the other sequences",
                 "unlisted sequences are untouched", "profiling slot pose_graph", "launches exactly what it launched before"):
        assert word in flat, word
    assert "typedef" not in block and "enum" not in block                           # no new record, no new enumerator


def test_the_profiling_slots_and_the_records_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert not any("trim" in n for n in names)
    assert names[names.index("map_register"):] == ["map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register",
                                                   "save_sequences", "load_sequences", "score_corrections", "apply_corrections"]
    assert "trim" not in open(os.path.join(ROOT, "a-loam_amd", "records.py")).read().lower()
    assert "K_POSE_GRAPH" in open(os.path.join(CSRC, "capi_graphtrim.hip")).read()
    assert "typedef struct" not in open(os.path.join(CSRC, "graphtrim_kernels.hpp")).read()


def test_the_counts_change_in_one_event():
    events = open(os.path.join(CSRC, "capi_seq.hip")).read()
    internal = open(os.path.join(CSRC, "capi_internal.hpp")).read()
    host = open(os.path.join(CSRC, "capi_graphtrim.hip")).read()
    assert "void on_graph_trimmed(aloam_ctx* c, int seq, int nodes, int edges)" in events and "on_graph_trimmed" in internal and "on_graph_trimmed(" in host
    assert not re.search(r"\bgraph_(nodes|edges)\s*(=[^=]|\+=|-=|\+\+|--)", host)
    assert host.count("hipStreamSynchronize(") == 1                                  # the one synchronisation, behind the launches
    assert host.index("launch_graph_trim(") < host.index("hipStreamSynchronize(") < host.index("on_graph_trimmed(")
    assert "| `graph_trimmed`" in open(os.path.join(ROOT, "DESIGN.md")).read()        # §7b's table has its row (it drops the on_)


def test_the_unit_calls_the_pose_functions_and_names_its_chunk_once():
    unit = open(os.path.join(CSRC, "graphtrim_kernels.hip")).read()
    assert '#include "map_search_device.hpp"' in unit
    for reused in ("quat_mul", "quat_rotate"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
    code = re.sub(r"//[^\n]*", "", unit)
    assert not re.search(r"atomic\w*\([^)]*(double|float)", code) and "while" not in code                             # no float atomics, no spinning
    assert code.count("loads_complete();\n    __syncthreads();") == 3                                                  # tail, edge tiles, node row
    assert "__ballot(" in unit and "__builtin_amdgcn_mbcnt_hi(" in unit
    hpp = open(os.path.join(CSRC, "graphtrim_kernels.hpp")).read()
    assert len(re.findall(r"constexpr int kTrimChunk = \d+;", hpp)) == 1
    every = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC))
    assert len(re.findall(r"kTrimChunk\s*=[^=]", every)) == 1


def test_the_makefile_lists_the_three_files():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(f in mk for f in ("graphtrim_kernels.hip", "capi_graphtrim.hip", "graphtrim_kernels.hpp"))
    assert "-ffp-contract=off" in mk


@pytest.mark.parametrize("tool,option", [("loop_closure_drive.py", "--window"), ("graph_trim_rate.py", "--repeats")])
def test_the_tools_have_their_options(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
