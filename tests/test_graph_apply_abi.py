"""aloam_graph_apply, host side (no GPU): the entry point, the enums and the two records in the header, the binding and the library; the
event in capi_seq.hip and its row in DESIGN §7b; what the header says about the map, the rebase and the stored places."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def test_the_records_are_whole_doubles(binding):
    """(Their layouts are rows of test_abi_records.py.)"""
    assert binding.GRAPH_APPLY_REQUEST_DTYPE.itemsize % 8 == 0 and binding.GRAPH_APPLY_RESULT_DTYPE.itemsize % 8 == 0


def test_the_call_is_declared_exported_and_bound(binding):
    binding.build()
    assert "aloam_graph_apply" in binding.declared_symbols() and hasattr(binding.lib(), "aloam_graph_apply")
    for m in ("graph_apply", "graph_apply_into", "graph_apply_requests"):
        assert callable(getattr(binding.Aloam, m, None)), m
    assert (binding.GRAPH_APPLY_POSE, binding.GRAPH_APPLY_MAP) == (1, 2)
    assert (binding.GRAPH_APPLIED, binding.GRAPH_APPLY_NO_NODES, binding.GRAPH_APPLY_NO_ROOM) == (0, 1, 2)
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "enum { ALOAM_GRAPH_APPLY_POSE = 1, ALOAM_GRAPH_APPLY_MAP = 2 };" in d
    assert "enum { ALOAM_GRAPH_APPLIED = 0, ALOAM_GRAPH_APPLY_NO_NODES = 1, ALOAM_GRAPH_APPLY_NO_ROOM = 2 };" in d
    assert d.index("aloam_graph_apply(") > d.index("aloam_graph_export_map(")                  # behind the keyframe section
    assert binding.lib().aloam_graph_apply(None, None, 0, None) == binding.E_ARG


def test_the_header_says_what_an_apply_does_and_does_not():
    txt = open(HEADER).read()
    block = txt[txt.index("---- a solved graph carried into the live state"):txt.index("typedef struct aloam_graph_apply_request")]
    for word in ("q_D = normalise(q_opt conj(q))", "t_D = t_opt - q_D t", "LAST node", "rebased", "bit copies", "KEYFRAMES ONLY", "not spilled", "SYNCHRONISES",
                 "ALOAM_GRAPH_APPLY_NO_ROOM", "ALOAM_E_CAPACITY", "frozen", "attached", "listed twice", "n = 0 is ALOAM_OK", "do not depend on n",
                 "a place's pose is to be taken from its node", "odometry state and frameCount are not touched", "never pass"):
        assert word in " ".join(block.split()), word
    node = txt[txt.index("typedef struct aloam_graph_node"):txt.index("} aloam_graph_node;")]
    assert "changed only by aloam_graph_apply" in node and "never changed" not in node


def test_the_event_is_in_capi_seq_and_in_the_table():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    assert "int on_graph_applied(" in open(os.path.join(csrc, "capi_seq.hip")).read()
    assert "on_graph_applied" in open(os.path.join(csrc, "capi_internal.hpp")).read()
    host = open(os.path.join(csrc, "capi_graphapply.hip")).read()
    assert "on_graph_applied(" in host and not re.search(r"\b(scorable|info_map)\s*=[^=]", host)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `graph_applied`" in design and "7m" in design
    # k_graph_add_nodes and its translation unit do not know about the apply
    unit = open(os.path.join(csrc, "posegraph_kernels.hip")).read()
    assert "aloam_graph_apply" not in unit and "graphapply" not in unit


def test_the_tools_have_their_options():
    for tool, opt in (("graph_apply_rate.py", "--repeats"), ("loop_closure_drive.py", "--apply")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and opt in r.stdout, r.stdout + r.stderr
