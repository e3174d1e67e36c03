"""The loop proposal by pose proximity, host side (no GPU): the entry point in the header, the binding and the library; the words of the
definition in the header; the profiling slots and the records, which it leaves alone; the unit's reuse of the relative-pose device functions;
the Makefile; the tools' options."""
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
    assert "aloam_graph_propose_loops" in binding.declared_symbols() and hasattr(binding.lib(), "aloam_graph_propose_loops")
    for m in ("graph_propose_loops", "graph_propose_loops_into"):
        assert callable(getattr(binding.Aloam, m, None)), m
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert callable(pg.propose_loops) and callable(pg.unclosed) and pg.PROPOSE_MAX_K == 16
    assert binding.lib().aloam_graph_propose_loops(None, None, 0, 1, 3.0, 0.0, 20, 3, 6, 4, None, None, None) == binding.E_ARG      # a null context


def test_header_states_the_definition():
    txt = open(HEADER).read()
    assert txt.index("---- the robust solve") < txt.index("---- loop candidates by pose proximity") < txt.index("---- intermediate arrays")
    block = txt[txt.index("---- loop candidates by pose proximity"):txt.index("int aloam_graph_propose_loops(")]
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("every f64 operation separately rounded", "(q, t) or its estimate (q_opt, t_opt), chosen by pose", "i in [0, j - min_gap]", "none when j < min_gap",
                 "(dx, dy, dz) = t_i - t_j", "d2 = (dx*dx + dy*dy) + dz*dz", "r = (double)(j - i) * growth_m_per_node + radius_m", "i is a hit when d2 <= r*r",
                 "at most K rounds", "the least (d2, i)", "lower d2 first, then lower i", "|i' - i| <= separation", "counts[q] is the number taken",
                 "first = max(0, i - half_window)", "count = i + half_window - first + 1", "q_d = conj(q_i) q_j", "t_d = conj(q_i) (t_j - t_i)",
                 "pad and reserved are zero", "dist2[q][k] = d2", "all-zero bytes", "nothing outside them is written", "checked before anything is queued",
                 "0 <= j < the sequence's nodes", "pose 0 or 1", "finite and >= 0", "min_gap >= 1", "0 <= half_window < min_gap", "separation >= 0", "1 <= K <= 16",
                 "classified like the exports", "dst and dist2 8-byte aligned and counts 4-byte aligned", "ALOAM_E_STATE before aloam_graph_enable", "n = 0 is ALOAM_OK",
                 "any number of times", "no host synchronisation", "pinned staging ring", "runs in rounds", "reads the graph and writes nothing in it",
                 "independent of n, of its position in the list, of the round and of the other queries", "profiling slot pose_graph",
                 "launches exactly what it launched before"):
        assert word in flat, word
    assert "typedef" not in block and "enum" not in block                           # no new record, no new enumerator


def test_the_profiling_slots_and_the_records_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert not any("propose" in n for n in names)
    assert names[names.index("map_register"):] == ["map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register",
                                                   "save_sequences", "load_sequences", "score_corrections", "apply_corrections"]
    records = open(os.path.join(ROOT, "a-loam_amd", "records.py")).read()
    assert "propose" not in records.lower()
    assert "K_POSE_GRAPH" in open(os.path.join(CSRC, "capi_graphpropose.hip")).read()
    assert "typedef struct" not in open(os.path.join(CSRC, "graphpropose_kernels.hpp")).read()


def test_the_unit_includes_the_relative_pose_functions_and_names_its_capacity_once():
    unit = open(os.path.join(CSRC, "graphpropose_kernels.hip")).read()
    assert '#include "map_search_device.hpp"' in unit
    for reused in ("quat_mul", "quat_rotate"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
        assert re.search(r"\b%s\(" % reused, open(os.path.join(CSRC, "loopreg_kernels.hip")).read())
    assert "atomicAdd(&s_hits" in unit and not re.search(r"atomic\w*\([^)]*(d2|double|float)", unit)                 # the one atomic is an integer's
    assert "__ballot(" in unit and "__builtin_amdgcn_mbcnt_hi(" in unit
    hpp = open(os.path.join(CSRC, "graphpropose_kernels.hpp")).read()
    assert len(re.findall(r"constexpr int kProposeHits = \d+;", hpp)) == 1
    every = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC))
    assert len(re.findall(r"kProposeHits\s*=[^=]", every)) == 1


def test_the_makefile_lists_the_three_files():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(f in mk for f in ("graphpropose_kernels.hip", "capi_graphpropose.hip", "graphpropose_kernels.hpp"))


@pytest.mark.parametrize("tool,option", [("loop_closure_drive.py", "--proximity"), ("graph_propose_rate.py", "--repeats")])
def test_the_tools_have_their_options(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
