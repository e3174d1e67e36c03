"""The constructed graphs and clouds of the in-place trim (aloam_graph_trim), shared by the model's test and the GPU test.
Every builder is seeded and small.  Edge patterns are lists of (i, j) against a given `first`; clouds are points that carry their own
identity in their bits (class, node, index within the class row), so a point that moved to the wrong place is a different point."""
import importlib
import os
import re

import numpy as np

pg = importlib.import_module("a-loam_amd.posegraph")
gr = importlib.import_module("a-loam_amd.graph_records")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "a-loam_amd", "csrc", "graphtrim_kernels.hpp")


def constant(name):
    """An integer constant of graphtrim_kernels.hpp, read from its text."""
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(HPP).read()).group(1))


CHUNK = constant("kTrimChunk")
EDGE_COUNTS = (0, 1, 255, 256, 257, 600)
PATTERNS = ("kept", "removed", "alternating", "reverse", "anchors", "robust", "endpoints")
N_EDGE_GRAPH, F_EDGE_GRAPH = 40, 17                  # the graph the edge patterns live on, and its `first`
NODE_CASES = ((5, 0), (5, 1), (5, 4), (600, 255), (600, 256), (600, 257))          # (nodes, first)
# (d, m) of a class: points dropped in front, points that stay.  The two classes of cloud case k take CLOUD_CASES[k] and [(k + 3) % 8].
CLOUD_CASES = ((5, 0), (7, 3), (6, 6), (6, 7), (1, 3 * CHUNK + 5), (CHUNK - 1, 2 * CHUNK + 3), (CHUNK, 2 * CHUNK + 3), (CHUNK + 1, 2 * CHUNK + 3))
KF_CAPACITY = 4 * CHUNK                              # points per class row: holds the largest cursor above, 3 CHUNK + 6


def unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def random_nodes(seed, n):
    """n nodes with unrelated entered poses and estimates (a trim copies them; nothing here solves)."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros(n, pg.NODE_DTYPE)
    nodes["q"], nodes["t"] = unit(rng.standard_normal((n, 4))), rng.uniform(-50, 50, (n, 3))
    nodes["q_opt"], nodes["t_opt"] = unit(rng.standard_normal((n, 4))), rng.uniform(-50, 50, (n, 3))
    nodes["frame"] = 7 + 3 * np.arange(n)
    nodes["pad"] = 0
    return nodes


def pattern_pairs(pattern, count, n, f):
    """`count` pairs (i, j) on a graph of n nodes trimmed at f (1 < f < n - 2), in the named pattern."""
    k = np.arange(count)
    above = n - f - 1                                            # nodes above f
    if pattern == "kept":                                        # rule 1, and rule 3 every seventh
        i = f + k % (above - 1)
        j = i + 1
        third = k % 7 == 3
        i, j = np.where(third, f + 1 + k % above, i), np.where(third, f, j)
    elif pattern == "removed":                                   # rule 5: nothing above f
        i, j = k % f, k % f + 1
    elif pattern in ("alternating", "robust"):                   # keep / anchor / remove
        kind = k % 3
        i = np.where(kind == 0, f + (k // 3) % above, k % f)
        j = np.where(kind == 1, f + 1 + (k // 3) % above, i + 1)
    elif pattern == "reverse":                                   # rule 4 among kept ones and rule 3
        kind = k % 4
        i = f + 1 + k % above
        j = np.where(kind == 0, k % f, np.where(kind == 1, f, np.where(kind == 2, f - 1, f + 1 + (k + 1) % above)))
        j = np.where(i == j, f, j)
    elif pattern == "anchors":                                   # i = -1 at every j: kept above f, constants at and below
        i, j = np.full(count, -1), (k * 7) % n
    elif pattern == "endpoints":                                 # every pair of -1, 0, f - 1, f, f + 1, last
        ends = (-1, 0, f - 1, f, f + 1, n - 1)
        pairs = [(a, b) for a in ends for b in ends if b >= 0 and a != b]
        i, j = (np.array([pairs[x % len(pairs)][c] for x in k], np.int64).reshape(-1) for c in (0, 1))
    else:
        raise KeyError(pattern)
    return np.asarray(i, np.int64), np.asarray(j, np.int64)


def random_edges(seed, i, j, robust=None, seq=0):
    rng = np.random.default_rng(seed)
    n = len(i)
    a = rng.standard_normal((n, 6, 6))
    info = a @ a.transpose(0, 2, 1) + 6.0 * np.eye(6)
    flags = (rng.integers(0, 2, n) == 1) if robust is None else robust
    return pg.make_edges(seq, i, j, unit(rng.standard_normal((n, 4))), rng.uniform(-20, 20, (n, 3)), info, robust=flags)


def edge_case(pattern, count, seed=0):
    """(nodes, edges, first) of one edge case; `robust` flags about half of its edges, the others none."""
    i, j = pattern_pairs(pattern, count, N_EDGE_GRAPH, F_EDGE_GRAPH)
    robust = None if pattern == "robust" else np.zeros(count, bool)
    return random_nodes(1000 + seed, N_EDGE_GRAPH), random_edges(2000 + seed + count, i, j, robust), F_EDGE_GRAPH


def points(cls, node, first, count):
    """`count` points of one node: x = index in the class row, y = class, z = node, w = a fixed pattern, as the bits of float32."""
    p = np.zeros((count, 4), np.uint32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = first + np.arange(count), cls, node, 0x3F800000
    return p.view(np.float32)


def clouds(counts):
    """counts: int [N, 2] points per node and class.  Returns the keyframes argument of graph_records.pack: per class (points, offsets)."""
    counts = np.asarray(counts, np.int64).reshape(-1, 2)
    out = []
    for cls in (0, 1):
        off = np.concatenate([[0], np.cumsum(counts[:, cls])])
        pts = [points(cls, k, int(off[k]), int(counts[k, cls])) for k in range(len(counts))]
        out.append((np.concatenate(pts) if pts else np.zeros((0, 4), np.float32), off))
    return tuple(out)


def small_counts(n):
    """A few points per node, some nodes without a corner cloud."""
    k = np.arange(n)
    return np.stack([k % 3, 1 + k % 2], 1)


def cloud_case(k):
    """(nodes, counts [4, 2], first = 2): two nodes hold the d points that go, two the m points that stay, per class its own (d, m)."""
    counts = np.zeros((4, 2), np.int64)
    for cls, (d, m) in enumerate((CLOUD_CASES[k], CLOUD_CASES[(k + 3) % len(CLOUD_CASES)])):
        counts[:, cls] = (d // 2, d - d // 2, m // 2, m - m // 2)
    return random_nodes(3000 + k, 4), counts, 2


def model(nodes, edges, keyframes, first):
    """The whole model on what was exported before the trim: (nodes', edges', keyframes', out[8])."""
    n2, e2, stats = pg.trim(nodes, edges, first)
    freed = [0, 0]
    if keyframes is not None:
        desc, corner, surf, freed = gr.trim_keyframes(gr.descriptors(keyframes), keyframes[0][0], keyframes[1][0], first)
        keyframes = tuple((p, np.concatenate([desc["first"][:, cls], [len(p)]]).astype(np.int64)) for cls, p in enumerate((corner, surf)))
    return n2, e2, keyframes, np.array(list(stats) + [int(freed[0]), int(freed[1]), 0], np.int32)
