"""The joined pose graphs, host side (no GPU): the records and the three entry points in the header, the binding and the library; the words
the header must say; the profiling slots and the kernel units, which the feature leaves alone; the new unit's reuse of the pose device
functions; the Makefile; the tool's options.  What the calls do is tested on the GPU (tests/test_gpu_graph_joint.py)."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CSRC = os.path.join(ROOT, "a-loam_amd", "csrc")
CALLS = ("aloam_graph_optimize_joint", "aloam_graph_optimize_joint_robust", "aloam_graph_joint_export")


def test_the_calls_are_declared_exported_and_bound(binding):
    binding.build()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert name in binding.declared_symbols() and hasattr(binding.lib(), name) and re.search(r" T %s\b" % name, out), name
    for method in ("graph_optimize_joint", "graph_optimize_joint_into", "graph_optimize_joint_robust", "graph_joint_export", "joint_lists"):
        assert callable(getattr(binding.Aloam, method, None)), method
    pg = importlib.import_module("a-loam_amd.posegraph")
    assert all(callable(getattr(pg, f)) for f in ("join", "align_member", "split", "optimize_joint", "cut_drive", "make_links", "tree_links"))
    L = binding.lib()
    assert L.aloam_graph_optimize_joint(None, None, None, 0, None, 0, None, 0, None, None) == binding.E_ARG              # a null context
    assert L.aloam_graph_optimize_joint_robust(None, None, None, 0, None, 0, None, 0, None, None, None, None, 0) == binding.E_ARG
    assert L.aloam_graph_joint_export(None, 0, None, 0, None, 0, None) == binding.E_ARG


def test_the_records_are_what_a_c_compiler_makes_of_the_header(binding, tmp_path):
    """As test_abi_records.py holds the records of records.py: one C99 program prints sizeof of the two records and offsetof of every
    member; the size written here, the compiler's, ctypes' and the dtype's agree, and so do every member's name, order, offset, element type
    and shape.  The members are read from the header's own text."""
    import numpy as np
    jr = importlib.import_module("a-loam_amd.joint_records")
    rows = (("aloam_graph_link", "AloamGraphLink", "GRAPH_LINK_DTYPE", 256), ("aloam_graph_joint_group", "AloamGraphJointGroup", "GRAPH_JOINT_GROUP_DTYPE", 16))
    mirrors = {n for n, v in vars(jr).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert mirrors == {r[1] for r in rows} and {n for n, v in vars(jr).items() if isinstance(v, np.dtype)} == {r[2] for r in rows}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    members = {}
    for name, _, _, _ in rows:
        body = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), text, flags=re.S).group(1)
        found = []
        for stmt in filter(None, (" ".join(x.split()) for x in body.split(";"))):
            ctype, decls = stmt.split(" ", 1)
            for decl in decls.split(","):
                member, dims = re.fullmatch(r"(\w+)((?:\[\d+\])*)", decl.strip()).groups()
                found.append((ctype, member, tuple(int(d) for d in re.findall(r"\[(\d+)\]", dims))))
        members[name] = found
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "aloam_mi355x.h"', "int main(void) {"]
    for name in members:
        src.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        src += [f'  printf("M {name} {m} %zu\\n", offsetof({name}, {m}));' for _, m, _ in members[name]]
    (tmp_path / "layout.c").write_text("\n".join(src + ["  return 0;", "}"]) + "\n")
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
    scalars = {"int": (C.c_int, np.int32), "double": (C.c_double, np.float64)}
    for name, cls_name, dtype_name, size in rows:
        cls, dt = getattr(binding, cls_name), getattr(binding, dtype_name)
        assert cls is getattr(jr, cls_name) and dt is getattr(jr, dtype_name) and dt == jr.record_dtype(cls)
        assert size == sizes[name] == C.sizeof(cls) == dt.itemsize
        assert [m for _, m, _ in members[name]] == [n for n, _ in cls._fields_] == list(dt.names)
        for (ctype, member, dims), (_, ftype) in zip(members[name], cls._fields_):
            assert offsets[name, member] == getattr(cls, member).offset == dt.fields[member][1], (name, member)
            elem, shape = ftype, ()
            while issubclass(elem, C.Array):
                shape, elem = shape + (elem._length_,), elem._type_
            assert elem is scalars[ctype][0] and shape == dims and dt.fields[member][0].shape == dims and dt.fields[member][0].base == np.dtype(scalars[ctype][1]), (name, member)


def test_the_records_have_the_stated_layout(binding):
    """Sizes and offsets as the issue states them."""
    link, group = binding.AloamGraphLink, binding.AloamGraphJointGroup
    assert C.sizeof(link) == 256 and C.sizeof(group) == 16
    assert [(n, getattr(link, n).offset) for n, _ in link._fields_] == [("seq_i", 0), ("i", 4), ("seq_j", 8), ("j", 12), ("flags", 16), ("pad", 20), ("q", 32),
                                                                          ("t", 64), ("info", 88)]
    assert [(n, getattr(group, n).offset) for n, _ in group._fields_] == [("member_first", 0), ("member_count", 4), ("link_first", 8), ("link_count", 12)]
    assert binding.GRAPH_LINK_DTYPE.itemsize == 256 and binding.GRAPH_JOINT_GROUP_DTYPE.itemsize == 16
    # a link's Z and info are an edge's, 16 bytes further in
    edge = binding.AloamGraphEdge
    assert all(getattr(link, f).offset == getattr(edge, f).offset + 16 and getattr(link, f).size == getattr(edge, f).size for f in ("q", "t", "info"))
    m, a, l, g = binding.Aloam.joint_lists([([3, 1], None), ([0, 2, 4], importlib.import_module("a-loam_amd.posegraph").make_links(0, [1, 2], 2, [0, 0], [[0, 0, 0, 1]] * 2, [[0, 0, 0]] * 2, __import__("numpy").eye(6)), [0, 1, 0])])
    assert m.tolist() == [3, 1, 0, 2, 4] and a.tolist() == [0, 0, 0, 1, 0] and len(l) == 2 and g.tolist() == [(0, 2, 0, 0), (2, 3, 0, 2)]


def test_header_states_what_the_issue_says_it_must():
    """The section's place, its two records, and the three things the issue says the header must say: the links are not stored, the host
    shifts its link indices after a trim, aligning a member again re-composes its anchors."""
    txt = open(HEADER).read()
    assert txt.index("---- trimming a graph in place") < txt.index("---- joined graphs") < txt.index("---- intermediate arrays")
    assert txt.index("int aloam_graph_loop_export_target(") < txt.index("int aloam_graph_joint_export(")
    block = txt[txt.index("---- joined graphs"):txt.index("int aloam_graph_optimize_joint_robust(")]
    flat = " ".join(block.replace("\n *", " ").split())
    for word in ("The links are NOT STORED", "passes them on every call", "shifts its own link indices of that member by -first",
                 "aligning a member again re-composes its anchors"):
        assert word in flat, word
    assert len(re.findall(r"typedef struct", block)) == 2 and "enum" not in block                    # two records, no new enumerator


def test_the_profiling_slots_and_the_other_units_are_unchanged(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert not any("joint" in n for n in names)
    assert names[names.index("map_register"):] == ["map_register", "graph_marginals", "export_clouds", "pose_information", "pose_graph", "graph_map", "loop_register",
                                                   "save_sequences", "load_sequences", "score_corrections", "apply_corrections"]
    for unit in ("posegraph_kernels.hip", "graphrobust_kernels.hip", "posegraph_kernels.hpp", "graphrobust_kernels.hpp"):
        assert "joint" not in open(os.path.join(CSRC, unit)).read().lower(), unit              # the solve is launched as it is


def test_the_unit_calls_the_pose_functions():
    unit = open(os.path.join(CSRC, "graphjoint_kernels.hip")).read()
    for reused in ("quat_mul", "quat_rotate"):
        assert re.search(r"\b%s\(" % reused, unit) and not re.search(r"__device__[^;{]*\b%s\(" % reused, unit), reused      # called, not restated


def test_the_makefile_lists_the_three_files():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(f in mk for f in ("graphjoint_kernels.hip", "capi_graphjoint.hip", "graphjoint_kernels.hpp"))
    assert "-ffp-contract=off" in mk


def test_the_rate_tool_has_its_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "graph_joint_rate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--repeats" in r.stdout and "--members" in r.stdout, r.stdout + r.stderr
