"""The records of the header's section "the map of joined sequences" (include/aloam_mi355x.h), each declared once: aloam_graph_map_part
and aloam_graph_map_group.  They stand beside a-loam_amd/records.py, a-loam_amd/joint_records.py and a-loam_amd/link_records.py in a
module of their own, and are declared in the header as a struct followed by its typedef, as the joint and link records are: each of those
three modules is held closed by a test.  tests/test_graph_map_joint_abi.py holds these two against what a C compiler makes of the header.
binding.py re-exports them.
"""
from __future__ import annotations

import ctypes as C

from .records import record_dtype


class AloamGraphMapPart(C.Structure):
    """Nodes [first, first + count) of one sequence under a frame (-1: the poses as stored) (aloam_graph_map_part, 16 bytes)."""
    _fields_ = [("seq", C.c_int), ("first", C.c_int), ("count", C.c_int), ("frame", C.c_int)]


class AloamGraphMapGroup(C.Structure):
    """The parts of one joined map in a call's list and the poses it is built at (aloam_graph_map_group, 16 bytes)."""
    _fields_ = [("part_first", C.c_int), ("part_count", C.c_int), ("pose", C.c_int), ("pad", C.c_int)]


GRAPH_MAP_PART_DTYPE = record_dtype(AloamGraphMapPart)
GRAPH_MAP_GROUP_DTYPE = record_dtype(AloamGraphMapGroup)
