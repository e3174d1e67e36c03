"""Keyframe clouds and the map at the graph's poses, host side (no GPU): the records and entry points in the header, the binding and the
library; the profiling slot; what can be refused without a device; the tools' options."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from test_posegraph_abi import HEADER, ROOT

CALLS = ("aloam_graph_keyframes_enable", "aloam_graph_export_keyframes", "aloam_graph_keyframe_info", "aloam_graph_export_map")


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_keyframes_enable", "graph_export_keyframes", "graph_export_keyframes_into", "graph_keyframe_info", "graph_export_map",
              "graph_export_map_into"):
        assert callable(getattr(binding.Aloam, m, None)), m
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "enum { ALOAM_GRAPH_POSE_ENTERED = 0, ALOAM_GRAPH_POSE_OPTIMIZED = 1 };" in d
    assert (binding.GRAPH_POSE_ENTERED, binding.GRAPH_POSE_OPTIMIZED) == (0, 1)
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                                   # keyframe clouds are not part of a sequence record
    assert d.index("aloam_graph_optimize(") < d.index("aloam_graph_keyframes_enable(")     # the section follows the pose graphs


def test_header_states_the_definition_and_where_it_synchronises():
    txt = open(HEADER).read()
    block = txt[txt.index("---- keyframe clouds and the map"):txt.index("typedef struct aloam_graph_map_request")]
    for word in ("sensor frame", "kept whole or not at all", "keyframe store full", "ALOAM_E_CAPACITY once", "rewinds", "aloam_reset_sequences",
                 "not part of a sequence record", "int((v + 25) / 50)", "-75", "node order, then point order", "input-order sum", "always applied",
                 "ascending in (cube[0], cube[1], cube[2])", "size query", "BOTH", "do not depend on n", "SYNCHRONISES", "once, after the transform pass",
                 "never pass through host", "grows the map pools first", "-512 .. 511", "launches exactly what it launched before"):
        assert word in block, word


def test_profiling_slot_follows_pose_graph(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names.index("graph_map") == names.index("pose_graph") + 1 == names.index("pose_information") + 2
    assert names[-3] == "load_sequences" and names[-2:] == ["score_corrections", "apply_corrections"]


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    out = (C.c_longlong * 8)()
    off = (C.c_longlong * 4)()
    assert L.aloam_graph_keyframes_enable(None, 16, 16) == binding.E_ARG
    assert L.aloam_graph_export_keyframes(None, 0, 0, 0, 0, None, 0, off) == binding.E_ARG
    assert L.aloam_graph_keyframe_info(None, 0, out) == binding.E_ARG
    assert L.aloam_graph_export_map(None, None, 0, None, 0, None, 0, off, None) == binding.E_ARG


def test_the_stacks_flag_is_a_seqhost_field_assigned_by_the_events_only():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    internal = open(os.path.join(csrc, "capi_internal.hpp")).read()
    assert "has_stacks" in internal[internal.index("struct SeqHost {"):internal.index("struct aloam_ctx {")]
    assign = re.compile(r"\bhas_stacks\s*=[^=]")
    for f in os.listdir(csrc):
        if f.endswith(".hip") and f != "capi_seq.hip":
            assert not assign.search(open(os.path.join(csrc, f)).read()), f
    assert len(assign.findall(open(os.path.join(csrc, "capi_seq.hip")).read())) == 2       # a mapping step sets it, a reset clears it


def test_the_makefile_builds_the_new_unit_like_the_others():
    mk = open(os.path.join(ROOT, "a-loam_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "graphmap_kernels.hip" in src and "capi_graphmap.hip" in src and "graphmap_kernels.hpp" in hdr


@pytest.mark.parametrize("tool,option", [("graph_map_rate.py", "--repeats"), ("loop_closure_drive.py", "--radius")])
def test_the_tools_answer_help(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
