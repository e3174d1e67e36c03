"""The map of joined sequences, host side (no GPU): the call and its two records in the header, the binding and the library; the section's
place; the Makefile; the kernel unit of the per-request map, which the feature leaves alone; the tools' options.  What the call does is
tested on the GPU (tests/test_gpu_graph_map_joint.py)."""
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
CALL = "aloam_graph_export_map_joint"
# record: (class, dtype, bytes, [(member, offset), ...]); the sizes and offsets are written out here and come from nowhere else
RECORDS = {"aloam_graph_map_part": ("AloamGraphMapPart", "GRAPH_MAP_PART_DTYPE", 16, [("seq", 0), ("first", 4), ("count", 8), ("frame", 12)]),
           "aloam_graph_map_group": ("AloamGraphMapGroup", "GRAPH_MAP_GROUP_DTYPE", 16, [("part_first", 0), ("part_count", 4), ("pose", 8), ("pad", 12)])}


def test_the_call_is_declared_exported_and_bound(binding):
    binding.build()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert CALL in binding.declared_symbols() and hasattr(binding.lib(), CALL) and re.search(r" T %s\b" % CALL, out)
    for method in ("graph_export_map_joint", "graph_export_map_joint_into", "graph_map_groups"):
        assert callable(getattr(binding.Aloam, method, None)), method
    assert callable(importlib.import_module("a-loam_amd.atlas").tiles_from_parts)
    assert binding.lib().aloam_graph_export_map_joint(None, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == binding.E_ARG   # a null context
    parts, groups = binding.Aloam.graph_map_groups([([(0, 0, 1, -1), (2, 3, 4, 0)], 1), ([], 0), ([(1, 0, 7, -1)], 0)])
    assert parts.dtype == binding.GRAPH_MAP_PART_DTYPE and groups.dtype == binding.GRAPH_MAP_GROUP_DTYPE
    assert parts.tolist() == [(0, 0, 1, -1), (2, 3, 4, 0), (1, 0, 7, -1)] and groups.tolist() == [(0, 2, 1, 0), (2, 0, 0, 0), (2, 1, 0, 0)]


def test_the_records_are_what_a_c_compiler_makes_of_the_header(binding, tmp_path):
    """As tests/test_graph_link_abi.py holds its record: one C99 program prints sizeof and every offsetof; the size written here, the
    compiler's, ctypes' and the dtype's agree, and so do every member's name, order, offset and element type, read from the header's text."""
    mj = importlib.import_module("a-loam_amd.map_joint_records")
    assert {n for n, v in vars(mj).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure} == {r[0] for r in RECORDS.values()}
    assert {n for n, v in vars(mj).items() if isinstance(v, np.dtype)} == {r[1] for r in RECORDS.values()}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    members = {}
    for name in RECORDS:
        body = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), text, flags=re.S).group(1)
        members[name] = []
        for stmt in filter(None, (" ".join(x.split()) for x in body.split(";"))):
            ctype, decls = stmt.split(" ", 1)
            assert ctype == "int"
            members[name] += [re.fullmatch(r"\w+", d.strip()).group(0) for d in decls.split(",")]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "aloam_mi355x.h"', "int main(void) {"]
    for name in RECORDS:
        src.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        src += [f'  printf("M {name} {m} %zu\\n", offsetof({name}, {m}));' for m in members[name]]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes, offsets = {}, {}
    for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        kind, *f = line.split()
        if kind == "S":
            sizes[f[0]] = int(f[1])
        else:
            offsets[f[0], f[1]] = int(f[2])
    for name, (cls_name, dtype_name, size, fields) in RECORDS.items():
        cls, dt = getattr(binding, cls_name), getattr(binding, dtype_name)
        assert cls is getattr(mj, cls_name) and dt is getattr(mj, dtype_name) and dt == mj.record_dtype(cls)
        assert size == sizes[name] == C.sizeof(cls) == dt.itemsize, name
        assert members[name] == [n for n, _ in cls._fields_] == list(dt.names) == [n for n, _ in fields], name
        for (member, stated), (_, ftype) in zip(fields, cls._fields_):
            assert offsets[name, member] == getattr(cls, member).offset == dt.fields[member][1] == stated, (name, member)
            assert ftype is C.c_int and dt.fields[member][0] == np.dtype(np.int32), (name, member)


def test_the_section_stands_where_it_must_and_says_what_it_must():
    txt = open(HEADER).read()
    assert txt.index("int aloam_graph_optimize_joint_robust(") < txt.index("---- the map of joined sequences") < txt.index("---- links measured on the device")
    block = txt[txt.index("---- the map of joined sequences"):txt.index("---- links measured on the device")]
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("int aloam_graph_export_map_joint(", "struct aloam_graph_map_part {", "struct aloam_graph_map_group {", "in part order", "the bits are X_k's",
                 "quat_mul(q_A, q_k)", "quat_rotate(q_A, t_k) + t_A", "nothing renormalised", "unit to 1e-6", "frame in [-1, n_frames)", "pad 0",
                 "tile parts contiguously and in order", "n_groups <= 32768", "ALOAM_E_STATE before aloam_graph_keyframes_enable", "n_groups = 0 is ALOAM_OK",
                 "ALOAM_E_CAPACITY before anything is queued", "profiling slot graph_map", "byte for byte aloam_graph_export_map",
                 "launches exactly what it launched before", "Nothing about joins is stored".lower()):
        assert word in flat, word
    assert "typedef struct aloam_graph_map_part {" not in block and "enum" not in block      # struct, then typedef; ALOAM_GRAPH_POSE_* are reused


def test_the_makefile_lists_the_new_files():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "graphmapjoint_kernels.hip" in src and "capi_graphmapjoint.hip" in src and "graphmapjoint_kernels.hpp" in hdr and "-ffp-contract=off" in mk


def test_the_per_request_unit_is_left_alone_and_both_entries_share_one_back_half():
    for unit in ("graphmap_kernels.hip", "graphmap_kernels.hpp"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "k_graph_map_transform_parts" not in text and "k_graph_map_group_parts" not in text and "GmPart" not in text, unit
    unit = open(os.path.join(CSRC, "graphmapjoint_kernels.hip")).read()
    for reused in ("quat_mul", "quat_rotate", "associate_to_map", "cube_coord", "atlas_key", "last_le"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated
    assert not re.search(r"atomic\w*\([^)]*(double|float)", unit) and "__shared__" not in unit
    internal = open(os.path.join(CSRC, "capi_internal.hpp")).read()
    assert internal.count("int graph_map_run(") == 1
    for entry in ("capi_graphmap.hip", "capi_graphmapjoint.hip"):
        text = open(os.path.join(CSRC, entry)).read()
        assert "return graph_map_run(c, " in text, entry
    joint = open(os.path.join(CSRC, "capi_graphmapjoint.hip")).read()
    assert "hipStreamSynchronize" not in joint and "launch_voxel_filter" not in joint and "K_GRAPH_MAP" not in joint      # all of that is the shared half's


@pytest.mark.parametrize("tool,option,word", [("loop_closure_drive.py", "--two-sessions", "aloam_graph_export_map_joint"), ("graph_map_rate.py", "--joint", "aloam_graph_export_map_joint")])
def test_the_tools_have_their_options(tool, option, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout and word in " ".join(r.stdout.split()), r.stdout + r.stderr
