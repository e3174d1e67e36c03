"""The links measured on the device, host side (no GPU): the record and the three entry points in the header, the binding and the library;
the section's place and words; the profiling slots and the existing kernel units, which the feature leaves alone; the new unit's reuse of
the pose device functions and of the proposal's capacities; the Makefile; the tools' options.  What the calls do is tested on the GPU
(tests/test_gpu_graph_links.py)."""
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
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")
CALLS = ("aloam_graph_register_links", "aloam_graph_search_links", "aloam_graph_propose_links")
FIELDS = [("seq_i", 0), ("i", 4), ("first", 8), ("count", 12), ("seq_j", 16), ("j", 20), ("pose", 24), ("pad", 28), ("q", 32), ("t", 64), ("reserved", 88)]


def test_the_calls_are_declared_exported_and_bound(binding):
    binding.build()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert name in binding.declared_symbols() and hasattr(binding.lib(), name) and re.search(r" T %s\b" % name, out), name
    for method in ("graph_register_links", "graph_register_links_into", "graph_search_links", "graph_search_links_into", "graph_propose_links",
                   "graph_propose_links_into", "graph_link_requests"):
        assert callable(getattr(binding.Aloam, method, None)), method
    pg, lr = importlib.import_module("a-loam_amd.posegraph"), importlib.import_module("a-loam_amd.loopreg")
    assert callable(pg.propose_links) and callable(pg.frame_from_link) and callable(lr.link_request) and callable(lr.link_from_result)
    L = binding.lib()
    assert L.aloam_graph_register_links(None, None, 0, None, None) == binding.E_ARG                                   # a null context
    assert L.aloam_graph_search_links(None, None, 0, None, None, None, None, None) == binding.E_ARG
    assert L.aloam_graph_propose_links(None, None, None, 0, 1, 3.0, 3, 6, 4, None, None, None) == binding.E_ARG


def test_the_record_is_what_a_c_compiler_makes_of_the_header(binding, tmp_path):
    """As tests/test_graph_joint_abi.py holds its two records: one C99 program prints sizeof and every offsetof; the size written here, the
    compiler's, ctypes' and the dtype's agree, and so do every member's name, order, offset, element type and shape, read from the header's
    own text.  The guess sits at byte 32, where aloam_graph_loop_request has it."""
    lk = importlib.import_module("a-loam_amd.link_records")
    name, cls, dt = "aloam_graph_link_request", binding.AloamGraphLinkRequest, binding.GRAPH_LINK_REQUEST_DTYPE
    assert cls is lk.AloamGraphLinkRequest and dt is lk.GRAPH_LINK_REQUEST_DTYPE and dt == lk.record_dtype(cls)
    assert {n for n, v in vars(lk).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure} == {"AloamGraphLinkRequest"}
    assert {n for n, v in vars(lk).items() if isinstance(v, np.dtype)} == {"GRAPH_LINK_REQUEST_DTYPE"}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), text, flags=re.S).group(1)
    members = []
    for stmt in filter(None, (" ".join(x.split()) for x in body.split(";"))):
        ctype, decls = stmt.split(" ", 1)
        for decl in decls.split(","):
            member, dims = re.fullmatch(r"(\w+)((?:\[\d+\])*)", decl.strip()).groups()
            members.append((ctype, member, tuple(int(d) for d in re.findall(r"\[(\d+)\]", dims))))
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "aloam_mi355x.h"', "int main(void) {", f'  printf("S %zu\\n", sizeof({name}));']
    src += [f'  printf("M {m} %zu\\n", offsetof({name}, {m}));' for _, m, _ in members]
    src += ['  printf("G %zu\\n", offsetof(aloam_graph_loop_request, q));', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    size, offsets, guess = None, {}, None
    for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        kind, *f = line.split()
        if kind == "S":
            size = int(f[0])
        elif kind == "G":
            guess = int(f[0])
        else:
            offsets[f[0]] = int(f[1])
    assert 96 == size == C.sizeof(cls) == dt.itemsize
    assert [m for _, m, _ in members] == [n for n, _ in cls._fields_] == list(dt.names) == [n for n, _ in FIELDS]
    scalars = {"int": (C.c_int, np.int32), "double": (C.c_double, np.float64)}
    for (ctype, member, dims), (_, ftype), (_, stated) in zip(members, cls._fields_, FIELDS):
        assert offsets[member] == getattr(cls, member).offset == dt.fields[member][1] == stated, member
        elem, shape = ftype, ()
        while issubclass(elem, C.Array):
            shape, elem = shape + (elem._length_,), elem._type_
        assert elem is scalars[ctype][0] and shape == dims and dt.fields[member][0].shape == dims and dt.fields[member][0].base == np.dtype(scalars[ctype][1]), member
    loop = binding.AloamGraphLoopRequest
    assert guess == offsets["q"] == 32 == loop.q.offset and offsets["t"] == loop.t.offset and offsets["reserved"] == loop.reserved.offset
    assert "32" in re.search(r"struct %s \{[^\n]*" % name, open(HEADER).read()).group(0)          # the header states where the guess sits


def test_the_section_stands_where_it_must_and_says_what_it_must():
    txt = open(HEADER).read()
    assert txt.index("int aloam_graph_optimize_joint_robust(") < txt.index("---- links measured on the device") < txt.index("---- intermediate arrays")
    assert txt.index("---- joined graphs") < txt.index("---- links measured on the device")
    block = txt[txt.index("---- links measured on the device"):txt.index("---- intermediate arrays")]
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("word for word, with two substitutions", "No pose of seq_j is read", "the guess carries everything about their relation", "seq_i != seq_j",
                 "held against seq_i's node count", "0 <= j < seq_j's node count", 'there is no "j outside the window" rule', "ALOAM_E_STATE before aloam_graph_loops_enable",
                 "n = 0 is ALOAM_OK", "profiling slot loop_register", "made by the first link call that needs it", "nothing of it stays allocated",
                 "after a link call as after a loop call", "rounded on its own", "X_j' = X_j when frames is NULL", "the bits are X_j's", "quat_mul(q_A, q_j)",
                 "quat_rotate(q_A, t_j) + t_A", "all nodes [0, nodes(seq_i))", "no minimum gap and no growth term", "d2 = (dx*dx + dy*dy) + dz*dz",
                 "d2 <= radius_m * radius_m", "lower d2 first, then lower i", "|i' - i| <= separation", "first = max(0, i - half_window)",
                 "count = min(i + half_window, nodes(seq_i) - 1) - first + 1", "clamped at BOTH ends", "q_d = conj(q_i) q_j'", "t_d = conj(q_i) (t_j' - t_i)",
                 "pad and reserved are zero", "all-zero bytes", "nothing outside them is written", "A = (X_i o Z) o X_j^-1", "unit to 1e-6", "1 <= K <= 16",
                 "ALOAM_E_STATE before aloam_graph_enable", "no host synchronisation", "profiling slot pose_graph", "The guess sits at byte 32",
                 "launches exactly what it launched before"):
        assert word in flat, word
    assert len(re.findall(r"typedef struct", block)) == 1 and "enum" not in block and "typedef struct aloam_graph_link_request {" not in block


def test_the_profiling_slots_the_records_and_the_other_units_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert not any("link" in n for n in names)
    assert names[names.index("map_register"):] == ["map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register",
                                                   "save_sequences", "load_sequences", "score_corrections", "apply_corrections"]
    for module in ("records.py", "joint_records.py"):
        assert "link_request" not in open(os.path.join(ROOT, "a-loam_amd", module)).read().lower(), module
    for unit in ("loopreg_kernels.hip", "loopreg_kernels.hpp", "loopsearch_kernels.hip", "loopsearch_kernels.hpp", "graphpropose_kernels.hip", "graphpropose_kernels.hpp"):
        assert "link" not in open(os.path.join(CSRC, unit)).read().lower(), unit    # the kernels behind the gather are launched as they are
    assert "K_LOOP_REGISTER" in open(os.path.join(CSRC, "capi_loopreg.hip")).read() and "K_POSE_GRAPH" in open(os.path.join(CSRC, "capi_graphlink.hip")).read()


def test_the_unit_reuses_what_exists_and_keeps_to_itself():
    unit, hpp = open(os.path.join(CSRC, "graphlink_kernels.hip")).read(), open(os.path.join(CSRC, "graphlink_kernels.hpp")).read()
    assert "loopreg" not in unit and "loopreg" not in hpp
    for inc in ("graphmap_kernels.hpp", "mapping_kernels.hpp", "graphpropose_kernels.hpp"):
        assert '#include "%s"' % inc in hpp, inc
    assert '#include "map_search_device.hpp"' in unit
    for reused in ("quat_mul", "quat_rotate", "associate_to_map", "vox_enlist"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
    assert "atomicAdd(&s_hits" in unit and len(re.findall(r"atomic\w*\(", unit)) == 1                                       # the one atomic is an integer's
    assert not re.search(r"atomic\w*\([^)]*(d2|double|float)", unit)
    assert "__ballot(" in unit and "__builtin_amdgcn_mbcnt_hi(" in unit and "kProposeHits" in unit and "kProposeMaxK" in unit
    every = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC))
    assert len(re.findall(r"kProposeHits\s*=[^=]", every)) == 1 and len(re.findall(r"kProposeMaxK\s*=[^=]", every)) == 1
    host = open(os.path.join(CSRC, "capi_loopreg.hip")).read()
    assert host.count("launch_map_associate(") == 1 and host.count("launch_link_gather(") == 1 and host.count("launch_loop_gather(") == 1
    entry = open(os.path.join(CSRC, "capi_graphlink.hip")).read()
    assert "launch_map_associate(" not in entry and entry.count("register_loops(c, nullptr, req") == 2 and "hipStreamSynchronize" not in entry
    assert "hipStreamSynchronize" not in host[host.index("int aloam::register_loops"):host.index("int aloam_graph_loop_export_target")]


def test_the_makefile_lists_the_three_files():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "graphlink_kernels.hip" in src and "capi_graphlink.hip" in src and "graphlink_kernels.hpp" in hdr and "-ffp-contract=off" in mk


@pytest.mark.parametrize("tool,option", [("loop_register_rate.py", "--links"), ("loop_closure_drive.py", "--two-sessions")])
def test_the_tools_have_their_options(tool, option):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
