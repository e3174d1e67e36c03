"""The graph record format in numpy (a-loam_amd/graph_records.py, no GPU): pack and parse are inverses, every section lies on 16 bytes and a
record on 256, the padding is zero, and check() names each refusal of aloam_graph_load on hand-damaged records."""
import importlib

import numpy as np
import pytest

LEAF = (0.4, 0.8)


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("a-loam_amd.graph_records")


def graph(R, n_nodes, n_edges, seed=3):
    rng = np.random.default_rng(seed)
    nodes = np.zeros(n_nodes, R.NODE_DTYPE)
    for k in ("q", "t", "q_opt", "t_opt"):
        nodes[k] = rng.normal(size=nodes[k].shape)
    nodes["frame"] = np.arange(n_nodes)
    edges = np.zeros(n_edges, R.EDGE_DTYPE)
    if n_edges:
        edges["seq"] = 2
        edges["i"] = np.arange(n_edges) % max(n_nodes - 1, 1)
        edges["j"] = edges["i"] + 1
        edges["i"][-1] = -1                                                      # an anchor
        edges["flags"][0] = R.EDGE_ROBUST
        edges["q"], edges["t"], edges["info"] = rng.normal(size=(n_edges, 4)), rng.normal(size=(n_edges, 3)), rng.normal(size=(n_edges, 21))
    return nodes, edges


def clouds(counts, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for cls in (0, 1):
        off = np.concatenate([[0], np.cumsum([c[cls] for c in counts])]).astype(np.int64)
        out.append((rng.normal(size=(int(off[-1]), 4)).astype(np.float32), off))
    return tuple(out)


CASES = {"empty": (0, 0, None), "empty with the store": (0, 0, []), "no keyframe part": (5, 7, None),
         "a node kept without clouds": (4, 5, [(30, 100), (0, 70), (0, 0), (41, 9)]), "one node, empty corner cloud": (1, 0, [(0, 33)])}


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_parse_inverts_pack(R, name):
    n, e, counts = CASES[name]
    nodes, edges = graph(R, n, e)
    kf = clouds(counts) if counts is not None else None
    rec = R.pack(nodes, edges, kf, LEAF if kf else None, seq=2)
    p = R.parse(np.concatenate([np.full(512, 0xEE, np.uint8), rec, np.full(256, 0xEE, np.uint8)]), offset=512)   # position independent
    assert same(p["nodes"], nodes) and same(p["edges"], edges) and p["seq"] == 2 and p["bytes"] == len(rec)
    assert same(p["keyframes"], kf)
    assert p["resolutions"] == (tuple(float(np.float32(v)) for v in LEAF) if kf else None)
    # the layout
    h = R.header(rec)
    L = R.layout(n, e, h["kf_points"] if kf else None)
    assert all(v % 16 == 0 for v in L.values()) and L["bytes"] % 256 == 0 and L["bytes"] == len(rec) == h["bytes"] and L["bytes"] - L["end"] < 256
    assert not rec[L["end"]:].any() and not rec[64:128].any()                    # padding of the record and of the header
    assert (h["magic"], h["version"]) == (0x52474C41, 1) and rec[:4].tobytes() == b"ALGR"
    assert h["parts"] == (3 if kf else 1) and (h["node_bytes"], h["edge_bytes"], h["desc_bytes"], h["point_bytes"]) == (128, 240, 16, 16)
    assert (h["line_res_bits"], h["plane_res_bits"]) == ((0x3ECCCCCD, 0x3F4CCCCD) if kf else (0, 0))
    if kf:
        d = np.frombuffer(rec[L["desc"]:L["corner"]].tobytes(), R.DESC_DTYPE)
        assert d["count"].tolist() == [list(c) for c in counts]
        fill = np.concatenate([np.zeros((1, 2), int), np.cumsum(np.array(counts, int).reshape(-1, 2), 0)])[:-1]
        assert d["first"].tolist() == fill.tolist()                              # every descriptor carries the fill position, a node without clouds too
        assert h["kf_points"].tolist() == [sum(c[0] for c in counts), sum(c[1] for c in counts)]
    else:
        assert L["desc"] == L["corner"] == L["surf"] == L["end"] and h["kf_points"].tolist() == [0, 0]
    ctx = dict(max_nodes=8, max_edges=8, kf_capacity=(1000, 1000) if kf else None, resolutions=LEAF)
    assert R.check(rec, **ctx) is None


def test_layout_matches_the_header_strides(R):
    L = R.layout(3, 2, (5, 7))
    assert (L["nodes"], L["edges"], L["desc"], L["corner"], L["surf"], L["end"], L["bytes"]) == (128, 512, 992, 1040, 1120, 1232, 1280)
    assert R.layout(0, 0)["bytes"] == 256 and R.layout(0, 0, (0, 0))["bytes"] == 256 and R.layout(1, 0)["bytes"] == 256 and R.layout(1, 0, (0, 0))["bytes"] == 512


def test_check_names_each_refusal(R):
    nodes, edges = graph(R, 4, 5)
    counts = [(30, 100), (0, 70), (0, 0), (41, 9)]
    rec = R.pack(nodes, edges, clouds(counts), LEAF, seq=1)
    ctx = dict(max_nodes=8, max_edges=8, kf_capacity=(100, 200), resolutions=LEAF)
    L = R.layout(4, 5, (71, 179))

    def verdict(change, **kw):
        r = np.array(rec)
        change(r)
        return R.check(r, **{**ctx, **kw})

    def header(**fields):
        def change(r):
            for k, v in fields.items():
                r[:128].view(R.HEADER_DTYPE)[k] = v
        return change

    def edge(k, **fields):
        def change(r):
            for f, v in fields.items():
                r[L["edges"]:L["edges"] + 240 * 5].view(R.EDGE_DTYPE)[f][k] = v
        return change

    def desc(k, field, delta):
        def change(r):
            r[L["desc"]:L["corner"]].view(R.DESC_DTYPE)[field][k] += delta
        return change
    assert verdict(lambda r: None) is None
    assert verdict(header(magic=0x51534C41)) == (R.E_ARG, "magic")
    assert verdict(header(version=2)) == (R.E_ARG, "version")
    assert verdict(header(bytes=len(rec) + 256)) == (R.E_ARG, "bytes")
    assert R.check(rec, length=len(rec) - 256, **ctx) == (R.E_ARG, "bytes")
    assert R.check(rec[:len(rec) - 16], **ctx) == (R.E_ARG, "offsets")
    assert verdict(header(edge_bytes=232)) == (R.E_ARG, "section sizes")
    assert verdict(header(parts=1)) == (R.E_ARG, "parts") and verdict(header(parts=7)) == (R.E_ARG, "parts")
    assert verdict(lambda r: None, kf_capacity=None) == (R.E_ARG, "parts")
    assert verdict(header(nodes=-1)) == (R.E_ARG, "counts")
    assert verdict(header(nodes=40)) == (R.E_ARG, "bytes")                       # bytes inconsistent with the counts
    assert verdict(lambda r: None, resolutions=(0.2, 0.8)) == (R.E_ARG, "mapping_line_resolution")
    assert verdict(lambda r: None, resolutions=(0.4, 0.4)) == (R.E_ARG, "mapping_plane_resolution")
    assert verdict(lambda r: None, max_nodes=3) == (R.E_CAPACITY, "nodes")
    assert verdict(lambda r: None, max_edges=4) == (R.E_CAPACITY, "edges")
    assert verdict(lambda r: None, kf_capacity=(70, 200)) == (R.E_CAPACITY, "kf_points")
    assert verdict(lambda r: None, kf_capacity=(100, 178)) == (R.E_CAPACITY, "kf_points")
    assert verdict(edge(1, j=4)) == (R.E_ARG, "payload: edge index")
    assert verdict(edge(1, i=2, j=2)) == (R.E_ARG, "payload: edge index")
    assert verdict(edge(1, i=-2)) == (R.E_ARG, "payload: edge index")
    assert verdict(edge(4, i=-1, j=3)) is None                                   # an anchor of the last node
    assert verdict(edge(2, flags=2)) == (R.E_ARG, "payload: edge flags")
    assert verdict(desc(2, "first", (0, 1))) == (R.E_ARG, "payload: descriptor chain")
    assert verdict(desc(1, "count", (-1, 0))) == (R.E_ARG, "payload: descriptor chain")
    assert verdict(desc(0, "first", (1, 0))) == (R.E_ARG, "payload: descriptor chain")      # node 0 starts at 0
    assert verdict(desc(3, "count", (1, 0))) == (R.E_ARG, "payload: descriptor total")
    assert verdict(header(kf_points=(71, 180))) == (R.E_ARG, "payload: descriptor total")   # the same length, another total
    none = R.pack(nodes, edges)
    assert R.check(none, max_nodes=8, max_edges=8) is None and R.check(none, **ctx) == (R.E_ARG, "parts")


def test_the_model_and_the_binding_share_the_records(R, binding):
    assert R.HEADER_DTYPE == binding.GRAPH_RECORD_HEADER_DTYPE and R.HEADER_DTYPE.itemsize == 128
    assert (R.NODE_DTYPE, R.EDGE_DTYPE) == (binding.GRAPH_NODE_DTYPE, binding.GRAPH_EDGE_DTYPE)
    assert (R.MAGIC, R.VERSION, R.PART_GRAPH, R.PART_KEYFRAMES) == (binding.GRAPH_RECORD_MAGIC, binding.GRAPH_RECORD_VERSION, binding.GRAPH_PART_GRAPH, binding.GRAPH_PART_KEYFRAMES)
    assert (R.E_ARG, R.E_CAPACITY, R.E_STATE) == (binding.E_ARG, binding.E_CAPACITY, binding.E_STATE)
