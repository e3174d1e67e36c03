"""The record of the header's section "links measured on the device" (include/aloam_mi355x.h), declared once: aloam_graph_link_request.
It stands beside a-loam_amd/records.py and a-loam_amd/joint_records.py in a module of its own, and is declared in the header as a struct
followed by its typedef, as the two joint records are: tests/test_abi_records.py keeps a closed table of the records of records.py, and
tests/test_graph_joint_abi.py holds joint_records.py to exactly two.  tests/test_graph_link_abi.py holds this one against what a C
compiler makes of the header.  binding.py re-exports it; posegraph.py and loopreg.py take their link-request dtype from here.
"""
from __future__ import annotations

import ctypes as C

from .records import record_dtype


class AloamGraphLinkRequest(C.Structure):
    """Node j of seq_j registered against nodes [first, first + count) of seq_i in the frame of node i (aloam_graph_link_request, 96 bytes;
    the guess at byte 32, as in aloam_graph_loop_request)."""
    _fields_ = [("seq_i", C.c_int), ("i", C.c_int), ("first", C.c_int), ("count", C.c_int), ("seq_j", C.c_int), ("j", C.c_int), ("pose", C.c_int),
                ("pad", C.c_int), ("q", C.c_double * 4), ("t", C.c_double * 3), ("reserved", C.c_double)]


GRAPH_LINK_REQUEST_DTYPE = record_dtype(AloamGraphLinkRequest)
