"""Graph records in numpy: the byte format aloam_graph_save writes and aloam_graph_load reads (include/aloam_mi355x.h, "graph records";
DESIGN.md §7r), stated once more without the device.

A record is `header | nodes[N] | edges[E] [ | descriptors[N] | corner points | surf points ] | zeros up to a multiple of 256`; every
section is a whole number of 16-byte units.  pack() builds one from what Aloam.graph_export, graph_export(edges=True) and
graph_export_keyframes return, parse() takes one apart into those arrays, check() names what aloam_graph_load would refuse.
trim_keyframes() is the keyframe store's part of aloam_graph_trim, on the same descriptors."""
from __future__ import annotations

import numpy as np

from .posegraph import EDGE_DTYPE, EDGE_ROBUST, NODE_DTYPE
from .records import GRAPH_RECORD_HEADER_DTYPE as HEADER_DTYPE                    # aloam_graph_record_header, 128 bytes

DESC_DTYPE = np.dtype([("first", np.int32, 2), ("count", np.int32, 2)])          # KfDesc: where a node's clouds lie in the point sections
MAGIC, VERSION = 0x52474C41, 1                                                    # the bytes "ALGR"
PART_GRAPH, PART_KEYFRAMES = 1, 2
ALIGN = 256
E_ARG, E_CAPACITY, E_STATE = -1, -4, -6                                           # ALOAM_E_*


def layout(nodes, edges, kf_points=None):
    """Byte offsets of the sections from the counts; kf_points = (corner, surf) with the keyframe part, None without it."""
    L = {"nodes": HEADER_DTYPE.itemsize}
    L["edges"] = L["nodes"] + NODE_DTYPE.itemsize * int(nodes)
    L["end"] = L["edges"] + EDGE_DTYPE.itemsize * int(edges)
    L["desc"] = L["corner"] = L["surf"] = L["end"]
    if kf_points is not None:
        L["corner"] = L["desc"] + DESC_DTYPE.itemsize * int(nodes)
        L["surf"] = L["corner"] + 16 * int(kf_points[0])
        L["end"] = L["surf"] + 16 * int(kf_points[1])
    L["bytes"] = (L["end"] + ALIGN - 1) // ALIGN * ALIGN
    return L


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def pack(nodes, edges, keyframes=None, resolutions=None, seq=0):
    """One record as a uint8 array.  nodes / edges: structured arrays as exported.  keyframes: None, or per class (corner, surf) the pair
    (points float32 [n, 4], offsets int64 [N + 1]) that graph_export_keyframes returns for all N nodes; resolutions: the context's
    (mapping_line_resolution, mapping_plane_resolution), required with keyframes.  seq: the slot the record is saved from."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    N, E = len(nodes), len(edges)
    kf_points = None
    if keyframes is not None:
        assert resolutions is not None, "the keyframe part carries the mapping resolutions"
        pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 4) for p, _ in keyframes]
        offs = [np.asarray(o, np.int64) for _, o in keyframes]
        assert all(len(o) == N + 1 and o[0] == 0 and o[-1] == len(p) for p, o in zip(pts, offs))
        kf_points = (len(pts[0]), len(pts[1]))
    L = layout(N, E, kf_points)
    rec = np.zeros(L["bytes"], np.uint8)
    h = rec[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
    h["magic"], h["version"], h["bytes"] = MAGIC, VERSION, L["bytes"]
    h["parts"] = PART_GRAPH | (PART_KEYFRAMES if keyframes is not None else 0)
    h["nodes"], h["edges"], h["seq"] = N, E, seq
    h["node_bytes"], h["edge_bytes"], h["desc_bytes"], h["point_bytes"] = NODE_DTYPE.itemsize, EDGE_DTYPE.itemsize, DESC_DTYPE.itemsize, 16
    rec[L["nodes"]:L["edges"]] = nodes.view(np.uint8).reshape(-1)
    rec[L["edges"]:L["edges"] + EDGE_DTYPE.itemsize * E] = edges.view(np.uint8).reshape(-1)
    if keyframes is not None:
        h["kf_points"] = kf_points
        h["line_res_bits"], h["plane_res_bits"] = _bits(resolutions[0]), _bits(resolutions[1])
        rec[L["desc"]:L["corner"]] = descriptors(keyframes).view(np.uint8).reshape(-1)
        rec[L["corner"]:L["surf"]] = pts[0].view(np.uint8).reshape(-1)
        rec[L["surf"]:L["end"]] = pts[1].view(np.uint8).reshape(-1)
    return rec


def header(blob, offset=0):
    return np.frombuffer(np.ascontiguousarray(blob, np.uint8)[offset:offset + HEADER_DTYPE.itemsize].tobytes(), HEADER_DTYPE)[0]


def parse(blob, offset=0):
    """The record at `offset` of blob, back to pack()'s arguments: a dict with nodes, edges, keyframes, resolutions, seq and bytes."""
    blob = np.ascontiguousarray(blob, np.uint8)
    h = header(blob, offset)
    kf = bool(h["parts"] & PART_KEYFRAMES)
    N, E = int(h["nodes"]), int(h["edges"])
    L = layout(N, E, tuple(int(v) for v in h["kf_points"]) if kf else None)
    rec = blob[offset:offset + L["bytes"]]

    def section(a, b, dt):
        return np.frombuffer(rec[L[a]:b].tobytes(), dt).copy()
    out = {"nodes": section("nodes", L["edges"], NODE_DTYPE), "edges": section("edges", L["edges"] + EDGE_DTYPE.itemsize * E, EDGE_DTYPE),
           "keyframes": None, "resolutions": None, "seq": int(h["seq"]), "bytes": int(h["bytes"])}
    if kf:
        d = section("desc", L["corner"], DESC_DTYPE)
        pts = (section("corner", L["surf"], np.float32).reshape(-1, 4), section("surf", L["end"], np.float32).reshape(-1, 4))
        out["keyframes"] = tuple((pts[cls], np.concatenate([d["first"][:, cls], [len(pts[cls])]]).astype(np.int64)) for cls in (0, 1))
        out["resolutions"] = tuple(float(np.array([h[k]], np.uint32).view(np.float32)[0]) for k in ("line_res_bits", "plane_res_bits"))
    return out


def descriptors(keyframes):
    """The descriptor row of the N nodes from the per-class (points, offsets [N + 1]) pairs that graph_export_keyframes returns."""
    offs = [np.asarray(o, np.int64) for _, o in keyframes]
    d = np.zeros(len(offs[0]) - 1, DESC_DTYPE)
    for cls in (0, 1):
        d["first"][:, cls] = offs[cls][:-1]
        d["count"][:, cls] = np.diff(offs[cls])
    return d


def trim_keyframes(desc, corner, surf, first):
    """The keyframe store of one sequence behind aloam_graph_trim(first).  desc: DESC_DTYPE [N]; corner / surf: the points
    the rows hold, [cursor, 4] each.  Per class d = desc[first].first and m = cursor - d: points [d, d + m) move to [0, m), descriptor
    n >= first moves to n - first with first -= d and its counts unchanged, the cursor becomes m.  Returns (desc', corner', surf', freed)
    with freed = [d corner, d surf] (copies; points as bits)."""
    desc = np.ascontiguousarray(desc, DESC_DTYPE)
    f = int(first)
    assert 0 <= f < len(desc), "0 <= first < nodes"
    d = desc["first"][f].astype(np.int64)
    out = desc[f:].copy()
    out["first"] -= d.astype(np.int32)
    pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 4)[int(d[cls]):].copy() for cls, p in enumerate((corner, surf))]
    return out, pts[0], pts[1], d


def check(blob, offset=0, length=None, max_nodes=None, max_edges=None, kf_capacity=None, resolutions=None):
    """What aloam_graph_load says about the record at `offset` (`length`: the difference of its offsets, default: to the end of blob) in a
    context with rows of max_nodes / max_edges (None: no limit), keyframe rows of kf_capacity = (corner, surf) points (None: the store is
    not enabled) and the mapping `resolutions`.  None when it loads, else (error code, name): the header field, or "payload: ..." for what
    the check kernel finds.  The order is the load's."""
    blob = np.ascontiguousarray(blob, np.uint8)
    length = len(blob) - offset if length is None else length
    if offset < 0 or offset % 16 or length < HEADER_DTYPE.itemsize or length % ALIGN:
        return E_ARG, "offsets"
    h = header(blob, offset)
    if h["magic"] != MAGIC:
        return E_ARG, "magic"
    if h["version"] != VERSION:
        return E_ARG, "version"
    if h["bytes"] != length:
        return E_ARG, "bytes"
    if (h["node_bytes"], h["edge_bytes"], h["desc_bytes"], h["point_bytes"]) != (NODE_DTYPE.itemsize, EDGE_DTYPE.itemsize, DESC_DTYPE.itemsize, 16):
        return E_ARG, "section sizes"
    if not h["parts"] & PART_GRAPH or h["parts"] & ~(PART_GRAPH | PART_KEYFRAMES):
        return E_ARG, "parts"
    kf = bool(h["parts"] & PART_KEYFRAMES)
    if kf != (kf_capacity is not None):
        return E_ARG, "parts"
    N, E, P = int(h["nodes"]), int(h["edges"]), [int(v) for v in h["kf_points"]]
    if N < 0 or E < 0 or min(P) < 0 or (not kf and max(P) > 0):
        return E_ARG, "counts"
    L = layout(N, E, P if kf else None)
    if L["bytes"] != h["bytes"]:
        return E_ARG, "bytes"
    want = (_bits(resolutions[0]), _bits(resolutions[1])) if kf else (0, 0)
    if h["line_res_bits"] != want[0]:
        return E_ARG, "mapping_line_resolution"
    if h["plane_res_bits"] != want[1]:
        return E_ARG, "mapping_plane_resolution"
    if max_nodes is not None and N > max_nodes:
        return E_CAPACITY, "nodes"
    if max_edges is not None and E > max_edges:
        return E_CAPACITY, "edges"
    if kf and (P[0] > kf_capacity[0] or P[1] > kf_capacity[1]):
        return E_CAPACITY, "kf_points"
    r = parse(blob, offset)
    e = r["edges"]
    if np.any((e["i"] < -1) | (e["i"] >= N) | (e["j"] < 0) | (e["j"] >= N) | (e["i"] == e["j"])):
        return E_ARG, "payload: edge index"
    if np.any(e["flags"] & ~EDGE_ROBUST):
        return E_ARG, "payload: edge flags"
    if kf:
        d = np.frombuffer(blob[offset + L["desc"]:offset + L["corner"]].tobytes(), DESC_DTYPE)
        first, count = d["first"].astype(np.int64), d["count"].astype(np.int64)
        start = np.concatenate([np.zeros((1, 2), np.int64), (first + count)[:-1]]) if N else first
        if np.any(count < 0) or np.any(first != start):
            return E_ARG, "payload: descriptor chain"
        total = (first[-1] + count[-1]).tolist() if N else [0, 0]
        if total != P:
            return E_ARG, "payload: descriptor total"
    return None
