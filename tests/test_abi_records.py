"""Every record and enumerator of include/aloam_mi355x.h against its mirror in a-loam_amd/records.py (no GPU).

One C99 program, generated from the header's own text and compiled once, prints sizeof of every record, offsetof of every member - down
through nested records - and the value of every enumerator.  Each row of RECORDS is then held against it four ways: the size written
here, the C compiler's, ctypes' and the dtype's; every member's name, order, offset, element type and shape.  Two tests keep RECORDS
complete, one holds the mirrored constants."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")

# (record of the header, class, dtype or None, bytes); the sizes are written out here and come from nowhere else
RECORDS = (("aloam_config", "AloamConfig", None, 40),
           ("aloam_odom_stats", "AloamOdomStats", None, 72),
           ("aloam_range_decoder", "AloamRangeDecoder", None, 80),
           ("aloam_pose_record", "AloamPoseRecord", None, 240),
           ("aloam_map_correction", "AloamMapCorrection", "MAP_CORRECTION_DTYPE", 64),
           ("aloam_map_score", "AloamMapScore", "MAP_SCORE_DTYPE", 32),
           ("aloam_map_tile", "AloamMapTile", "MAP_TILE_DTYPE", 32),
           ("aloam_place", "AloamPlace", "PLACE_DTYPE", 4880),
           ("aloam_place_match", "AloamPlaceMatch", "PLACE_MATCH_DTYPE", 16),
           ("aloam_seq_record_header", "AloamSeqRecordHeader", None, 128),
           ("aloam_pose_information", "AloamPoseInformation", "POSE_INFORMATION_DTYPE", 1048),
           ("aloam_graph_node", "AloamGraphNode", "GRAPH_NODE_DTYPE", 128),
           ("aloam_graph_edge", "AloamGraphEdge", "GRAPH_EDGE_DTYPE", 240),
           ("aloam_graph_options", "AloamGraphOptions", None, 40),
           ("aloam_graph_result", "AloamGraphResult", "GRAPH_RESULT_DTYPE", 64),
           ("aloam_graph_map_request", "AloamGraphMapRequest", "GRAPH_MAP_REQUEST_DTYPE", 16),
           ("aloam_graph_map_stats", "AloamGraphMapStats", "GRAPH_MAP_STATS_DTYPE", 32),
           ("aloam_graph_apply_request", "AloamGraphApplyRequest", "GRAPH_APPLY_REQUEST_DTYPE", 16),
           ("aloam_graph_apply_result", "AloamGraphApplyResult", "GRAPH_APPLY_RESULT_DTYPE", 104),
           ("aloam_graph_loop_request", "AloamGraphLoopRequest", "GRAPH_LOOP_REQUEST_DTYPE", 96),
           ("aloam_graph_loop_options", "AloamGraphLoopOptions", None, 8),
           ("aloam_graph_loop_result", "AloamGraphLoopResult", "GRAPH_LOOP_RESULT_DTYPE", 448),
           ("aloam_graph_loop_search", "AloamGraphLoopSearch", "GRAPH_LOOP_SEARCH_DTYPE", 32),
           ("aloam_graph_loop_search_result", "AloamGraphLoopSearchResult", "GRAPH_LOOP_SEARCH_RESULT_DTYPE", 160),
           ("aloam_graph_marginal_request", "AloamGraphMarginalRequest", "GRAPH_MARGINAL_REQUEST_DTYPE", 248),
           ("aloam_graph_marginal_options", "AloamGraphMarginalOptions", None, 24),
           ("aloam_graph_marginal_result", "AloamGraphMarginalResult", "GRAPH_MARGINAL_RESULT_DTYPE", 440),
           ("aloam_graph_record_header", "AloamGraphRecordHeader", "GRAPH_RECORD_HEADER_DTYPE", 128),
           ("aloam_graph_robust_options", "AloamGraphRobustOptions", None, 32),
           ("aloam_graph_robust_result", "AloamGraphRobustResult", "GRAPH_ROBUST_RESULT_DTYPE", 128))
BY_C_NAME = {r[0]: r for r in RECORDS}
# row-major matrices that the header declares flat and the mirrors 2-D: the only members whose shape may differ from the C declaration's
FLAT_MATRICES = {("aloam_pose_information", "info"): (6, 6), ("aloam_pose_information", "eigenvectors"): (6, 6),
                 ("aloam_pose_information", "trans_info"): (3, 3), ("aloam_pose_information", "trans_eigenvectors"): (3, 3),
                 ("aloam_pose_information", "rot_info"): (3, 3), ("aloam_pose_information", "rot_eigenvectors"): (3, 3),
                 ("aloam_graph_marginal_result", "cov"): (6, 6)}
SCALARS = {"int": (C.c_int, np.int32), "unsigned int": (C.c_uint, np.uint32), "unsigned": (C.c_uint, np.uint32), "float": (C.c_float, np.float32),
           "double": (C.c_double, np.float64), "long long": (C.c_longlong, np.int64)}
# enumerators of the header that Python code has no use for
NOT_MIRRORED = ("OK", "SUM_INPUT_ORDER", "SUM_REFERENCE_ORDER")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_records():
    """{record: [(type, member, dims), ...]} from the struct bodies, in order.  A statement is a type followed by declarators, `name`,
    `name[N]` or `name[N][M]`, with commas between them; the type is whatever stands before the first one (pointers: it ends in '*'); a
    dimension is a number or an enumerator."""
    out = {}
    for name, body in re.findall(r"typedef struct (aloam_\w+) \{(.*?)\} \1;", _header(), flags=re.S):
        members = []
        for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
            first, *rest = [d.strip() for d in stmt.split(",")]
            m = re.fullmatch(r"(.*[\s*])(\w+(?:\[\w+\])*)", first)
            ctype = re.sub(r"\s*\*", "*", m.group(1).strip())
            for decl in [m.group(2)] + rest:
                member, dims = re.fullmatch(r"(\w+)((?:\[\w+\])*)", decl).groups()
                members.append((ctype, member, tuple(re.findall(r"\[(\w+)\]", dims))))
        out[name] = members
    return out


def header_enumerators():
    return [e for block in re.findall(r"\benum\s*\{(.*?)\}", _header(), flags=re.S) for e in re.findall(r"\b(ALOAM_\w+)\s*(?:=|,|$)", block.strip())]


def _member_paths(recs, name, prefix=""):
    for ctype, member, _ in recs[name]:
        yield prefix + member
        if ctype in recs:
            yield from _member_paths(recs, ctype, prefix + member + ".")


@pytest.fixture(scope="module")
def in_c(tmp_path_factory):
    """What a C99 compiler makes of the header: ({record: size}, {(record, member path): offset}, {enumerator: value})."""
    recs = header_records()
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "aloam_mi355x.h"', "int main(void) {"]
    for name in recs:
        src.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        src += [f'  printf("M {name} {p} %zu\\n", offsetof({name}, {p}));' for p in _member_paths(recs, name)]
    src += [f'  printf("E {e} %lld\\n", (long long){e});' for e in header_enumerators()]
    src += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_records")
    (d / "layout.c").write_text("\n".join(src) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(d / "layout.c"), "-o", str(d / "layout")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr                                    # the header is plain C99
    sizes, offsets, enums = {}, {}, {}
    for line in subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        kind, *f = line.split()
        if kind == "S":
            sizes[f[0]] = int(f[1])
        elif kind == "M":
            offsets[f[0], f[1]] = int(f[2])
        else:
            enums[f[0]] = int(f[1])
    return sizes, offsets, enums


def _element(t):
    """(element type, shape) of a ctypes field type: arrays of arrays collapse into one shape."""
    shape = ()
    while issubclass(t, C.Array):
        shape, t = shape + (t._length_,), t._type_
    return t, shape


def _check_members(binding, in_c, recs, top, c_name, cls, dt, prefix="", base=0):
    _, offsets, enums = in_c
    names = [m for _, m, _ in recs[c_name]]
    assert names == [n for n, _ in cls._fields_], (c_name, names)         # every member of the header is mirrored, in its order
    assert dt is None or list(dt.names) == names, (c_name, dt.names)
    for (ctype, member, dims), (_, ftype) in zip(recs[c_name], cls._fields_):
        where = (top, prefix + member)
        off = offsets[where]
        assert off == base + getattr(cls, member).offset, where
        assert dt is None or off == base + dt.fields[member][1], where
        shape = tuple(int(d) if d.isdigit() else enums[d] for d in dims)
        if (c_name, member) in FLAT_MATRICES:
            assert len(shape) == 1 and shape[0] == int(np.prod(FLAT_MATRICES[c_name, member])), where
            shape = FLAT_MATRICES[c_name, member]
        elem, fshape = _element(ftype)
        assert fshape == shape, where
        sub = dt.fields[member][0] if dt is not None else None
        assert sub is None or sub.shape == shape, where
        if ctype in recs:                                                 # a nested record: its mirror is the table's, and so are its insides
            _, sub_cls, sub_dtype, _ = BY_C_NAME[ctype]
            assert elem is getattr(binding, sub_cls) and shape == (), where
            assert sub is None or sub_dtype is None or sub == getattr(binding, sub_dtype), where
            _check_members(binding, in_c, recs, top, ctype, elem, sub, prefix + member + ".", off)
        elif ctype.endswith("*"):
            assert elem is C.POINTER(SCALARS[ctype[:-1].replace("const ", "")][0]) and dt is None, where
        else:
            assert elem is SCALARS[ctype][0], where
            assert sub is None or sub.base == np.dtype(SCALARS[ctype][1]), where


@pytest.mark.parametrize("c_name,cls_name,dtype_name,size", RECORDS, ids=[r[0] for r in RECORDS])
def test_record_has_the_header_layout(binding, in_c, c_name, cls_name, dtype_name, size):
    cls = getattr(binding, cls_name)
    dt = getattr(binding, dtype_name) if dtype_name else None
    assert size == in_c[0][c_name] == C.sizeof(cls)
    assert dt is None or dt.itemsize == size
    _check_members(binding, in_c, header_records(), c_name, c_name, cls, dt)


def test_every_record_of_the_header_has_a_row():
    assert set(header_records()) == set(BY_C_NAME) and len(BY_C_NAME) == len(RECORDS)


def test_every_structure_of_the_module_has_a_row(binding):
    records = importlib.import_module("a-loam_amd.records")
    mirrors = {n for n, v in vars(records).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert mirrors == {r[1] for r in RECORDS}
    dtypes = {n for n, v in vars(records).items() if isinstance(v, np.dtype)}
    assert dtypes == {r[2] for r in RECORDS if r[2]}
    for n in mirrors | dtypes:
        assert getattr(binding, n) is getattr(records, n), n              # the binding hands out the same objects
    for _, cls_name, dtype_name, _ in RECORDS:
        assert dtype_name is None or getattr(records, dtype_name) == records.record_dtype(getattr(records, cls_name))


def test_constants_are_the_headers_enumerators(binding, in_c):
    enums = in_c[2]
    assert len(enums) == len(header_enumerators()) >= 60
    missing = []
    for name, value in enums.items():
        assert name.startswith("ALOAM_")
        if hasattr(binding, name[6:]):
            assert getattr(binding, name[6:]) == value, name
        else:
            missing.append(name[6:])
    assert tuple(missing) == NOT_MIRRORED
    records = importlib.import_module("a-loam_amd.records")
    for n, v in vars(records).items():                                    # and nothing is mirrored that the header does not have
        if n.isupper() and isinstance(v, int):
            assert enums.get("ALOAM_" + n) == v, n
