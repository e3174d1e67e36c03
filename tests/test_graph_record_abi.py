"""Graph records, host side (no GPU): the header struct and the two entry points in the header, the binding and the library; what can be
refused without a device; where the new code lives; the profiling slots it leaves alone; the tools' options."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")


def test_the_magic_the_version_and_the_parts(binding):
    """(The layout of aloam_graph_record_header is a row of test_abi_records.py, which also holds these against the header's.)"""
    assert (binding.GRAPH_RECORD_MAGIC, binding.GRAPH_RECORD_VERSION, binding.GRAPH_PART_GRAPH, binding.GRAPH_PART_KEYFRAMES) == (0x52474C41, 1, 1, 2)


def test_the_enums_and_the_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in ("aloam_graph_save", "aloam_graph_load"):
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_save_into", "graph_save", "graph_load"):
        assert callable(getattr(binding.Aloam, m, None)), m
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "enum { ALOAM_GRAPH_RECORD_MAGIC = 0x52474c41 , ALOAM_GRAPH_RECORD_VERSION = 1 };" in d.replace(",", " ,").replace("  ", " ")
    assert "enum { ALOAM_GRAPH_PART_GRAPH = 1, ALOAM_GRAPH_PART_KEYFRAMES = 2 };" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                                   # sequence records keep their format
    assert "int aloam_graph_save(aloam_ctx* ctx, const int* seqs, int n, void* dst, long long cap_bytes, long long* dst_offsets );" in d
    assert "int aloam_graph_load(aloam_ctx* ctx, const int* slots, int n, const void* src, const long long* src_offsets );" in d


def test_the_header_states_the_format_and_the_refusals():
    txt = open(HEADER).read()
    block = txt[txt.index("---- graph records"):txt.index("typedef struct aloam_graph_record_header")]
    for word in ("header (128) | nodes[N] | edges[E]", "zeros up to a multiple of 256", "16-byte units", "depend on the graph alone", "always written",
                 "only when it ends at or before cap_bytes", "size query", "no host synchronisation", "pageable", "synchronises the context's stream once",
                 "a refused load changes nothing", "is not empty", "if and only if the store is enabled", "ALOAM_E_CAPACITY", "\"payload\"",
                 "-1 <= i < nodes, 0 <= j < nodes, i != j", "back to back from 0", "trusted", "no checksum", "rewritten to the target slot", "append cursors",
                 "left alone", "continue bit for bit", "save_sequences", "load_sequences", "ALOAM_SEQ_RECORD_VERSION is unchanged"):
        assert word in block, word
    # the sentences about what a sequence record leaves out stay in place
    assert "The graph is NOT part of a sequence record" in txt and "it is not part of a sequence record" in txt


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids = (C.c_int * 1)(0)
    off = (C.c_longlong * 2)(0, 256)
    buf = (C.c_char * 256)()
    assert L.aloam_graph_save(None, ids, 1, None, 0, off) == binding.E_ARG
    assert L.aloam_graph_load(None, ids, 1, buf, off) == binding.E_ARG


def test_the_new_units_are_built_and_the_event_has_its_row():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "graphrecord_kernels.hip" in src and "capi_graphrecords.hip" in src and "graphrecord_kernels.hpp" in hdr
    internal = open(os.path.join(CSRC, "capi_internal.hpp")).read()
    assert "void on_graph_loaded(aloam_ctx* c, int seq, int nodes, int edges);" in internal
    assert "void on_graph_loaded(aloam_ctx* c, int seq, int nodes, int edges) {" in open(os.path.join(CSRC, "capi_seq.hip")).read()
    host = open(os.path.join(CSRC, "capi_graphrecords.hip")).read()
    assert "on_graph_loaded(" in host and not re.search(r"\bgraph_(nodes|edges)\s*(=[^=]|\+=|-=|\+\+|--)", host)
    assert "| `graph_loaded`" in open(os.path.join(ROOT, "DESIGN.md")).read()      # §7b's table has its row (it drops the on_)
    kernels = open(os.path.join(CSRC, "graphrecord_kernels.hpp")).read()
    assert "__host__ __device__ inline GraphRecLayout graph_rec_layout(" in kernels   # the layout is stated once, for the host and the device
    assert "graph_rec_layout(" in host and "launch_export_scan(" in open(os.path.join(CSRC, "graphrecord_kernels.hip")).read()


def test_no_profiling_slot_was_added(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names[names.index("export_clouds"):] == ["export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register", "save_sequences",
                                                    "load_sequences", "score_corrections", "apply_corrections"]
    assert names.index("graph_marginals") == names.index("map_register") + 1 == names.index("export_clouds") - 1
    assert not any("record" in n for n in names)


@pytest.mark.parametrize("tool,options", [("graph_record_rate.py", ("--repeats", "--cases", "--points")), ("loop_closure_drive.py", ("--resume-at", "--apply", "--device-loops", "--search"))])
def test_the_tools_answer_help_with_their_options(tool, options):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for o in options:
        assert o in r.stdout, o
