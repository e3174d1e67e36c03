"""The records of the header's section "joined graphs" (include/aloam_mi355x.h), each declared once: aloam_graph_link and
aloam_graph_joint_group.  They stand beside a-loam_amd/records.py, in a module of their own, and are declared in the header as a struct
followed by its typedef: tests/test_abi_records.py keeps a closed table of the records of records.py and of the header's
`typedef struct name { ... } name;` declarations, and tests/test_graph_joint_abi.py holds these two against what a C compiler makes of
the header in the same way.  binding.py re-exports them; posegraph.py takes its link dtype from here.
"""
from __future__ import annotations

import ctypes as C

from .records import record_dtype


class AloamGraphLink(C.Structure):
    """Node j of seq_j measured in the frame of node i of seq_i (aloam_graph_link, 256 bytes); a-loam_amd/posegraph.py join() holds the definitions."""
    _fields_ = [("seq_i", C.c_int), ("i", C.c_int), ("seq_j", C.c_int), ("j", C.c_int), ("flags", C.c_int), ("pad", C.c_int * 3),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("info", C.c_double * 21)]


class AloamGraphJointGroup(C.Structure):
    """The members and links of one joined graph in a call's lists (aloam_graph_joint_group, 16 bytes)."""
    _fields_ = [("member_first", C.c_int), ("member_count", C.c_int), ("link_first", C.c_int), ("link_count", C.c_int)]


GRAPH_LINK_DTYPE = record_dtype(AloamGraphLink)
GRAPH_JOINT_GROUP_DTYPE = record_dtype(AloamGraphJointGroup)
