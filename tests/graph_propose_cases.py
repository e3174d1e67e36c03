"""The constructed graphs of the loop proposal by pose proximity (aloam_graph_propose_loops), shared by the model's test and
the GPU test.  GRAPHS: name -> nodes (NODE_DTYPE); CASES: a list of dict(name, graph, j, pose, params[, expect]).  Coordinates are small
integers or halves, so d2 and r r are exact and equal distances are exactly equal: every outcome below is decided by the definition alone.
The `laps` graphs are drifted_laps chains with real-valued coordinates; this file asserts, for every query on them, that no two d2 and no
d2 and r r lie close enough for a rounding to decide anything."""
import importlib
import os
import re

import numpy as np

pg = importlib.import_module("a-loam_amd.posegraph")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "a-loam_amd", "csrc", "graphpropose_kernels.hpp")


def constant(name):
    """An integer constant of graphpropose_kernels.hpp, read from its text."""
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(HPP).read()).group(1))


HITS = constant("kProposeHits")
FAR = 1.0e4                          # filler nodes lie on a line that starts this far out, 10 m apart: outside every radius used here


def make_nodes(t, q=None, t_opt=None, q_opt=None):
    t = np.asarray(t, np.float64)
    n = np.zeros(len(t), pg.NODE_DTYPE)
    n["t"] = t
    n["q"] = np.array([0.0, 0.0, 0.0, 1.0]) if q is None else q
    n["t_opt"] = t if t_opt is None else t_opt
    n["q_opt"] = n["q"] if q_opt is None else q_opt
    n["frame"] = -1
    return n


def filler(count):
    t = np.zeros((count, 3))
    t[:, 0] = FAR + 10.0 * np.arange(count)
    return t


def params(radius_m, min_gap, half_window=0, separation=0, K=1, growth_m_per_node=0.0):
    return dict(radius_m=float(radius_m), growth_m_per_node=float(growth_m_per_node), min_gap=int(min_gap), half_window=int(half_window),
                separation=int(separation), K=int(K))


GRAPHS, CASES = {}, []


def case(name, graph, j, p, expect=None, pose=pg.POSE_OPTIMIZED):
    CASES.append(dict(name=name, graph=graph, j=int(j), pose=int(pose), params=p, expect=expect))


# ---- ends: the first and the last iteration of every strided loop, every wave and workgroup boundary -----------------------------------
# Nodes 0 .. 599 on a line, 4 m apart.  FIRST is a query node next to node 0 alone: its eligible count is set through min_gap.  For the
# other version min_gap is fixed (GAP) and node E - 1 + GAP sits between the line's nodes E - 1 and E: both inside the radius, only E - 1 eligible.
ENDS_COUNTS = (1, 63, 64, 65, 255, 256, 257, 600)
GAP, FIRST = 700, 1400


def _ends():
    t = filler(FIRST + 1)
    t[:600] = 0.0
    t[:600, 0] = 4.0 * np.arange(600)
    t[FIRST] = (-1.0, 1.0, 0.0)                                                   # d2 = 2 to node 0, 26 to node 1
    for e in ENDS_COUNTS:
        t[e - 1 + GAP] = (4.0 * (e - 1) + 1.0, 1.0, 0.0)                          # d2 = 2 to node e - 1, 10 to node e, 26 to node e - 2
    GRAPHS["ends"] = make_nodes(t)
    for e in ENDS_COUNTS:
        case("ends/first/%d" % e, "ends", FIRST, params(4.0, FIRST - e + 1, K=3), expect=[0])
        case("ends/last/%d" % e, "ends", e - 1 + GAP, params(4.0, GAP, K=3), expect=[e - 1])


# ---- none ------------------------------------------------------------------------------------------------------------------------------
def _none():
    GRAPHS["one"] = make_nodes(np.zeros((1, 3)))
    case("none/one node", "one", 0, params(5.0, 1, K=2), expect=[])
    case("none/j below min_gap", "ends", 5, params(1000.0, 10, K=2), expect=[])
    case("none/all outside", "ends", 1200, params(3.0, 10, K=2), expect=[])


# ---- rim: d2 == r r exactly ------------------------------------------------------------------------------------------------------------
def _rim():
    t = filler(41)
    t[40] = (0.0, 0.0, 0.0)
    t[7] = (3.0, 4.0, 0.0)                                                        # d2 = 25
    t[20] = (0.0, 6.0, 0.0)                                                       # d2 = 36: outside 5 m, inside once the radius grows
    GRAPHS["rim"] = make_nodes(t)
    case("rim/on it", "rim", 40, params(5.0, 10, K=4), expect=[7])
    case("rim/just inside it", "rim", 40, params(np.nextafter(5.0, 0.0), 10, K=4), expect=[])
    # growth 0.0625 (exact in binary): node 20 gets r = 20 * 0.0625 + 5 = 6.25, node 7 gets r = 33 * 0.0625 + 5
    case("rim/growth", "rim", 40, params(5.0, 10, K=4, growth_m_per_node=0.0625), expect=[7, 20])


# ---- ties: equal d2 in different threads and waves -------------------------------------------------------------------------------------
def _ties():
    t = filler(501)
    t[500] = (0.0, 0.0, 0.0)
    t[3], t[200], t[450] = (3.0, 4.0, 0.0), (-3.0, 4.0, 0.0), (0.0, 0.0, 5.0)     # d2 = 25 three times
    t[5] = (1.0, 0.0, 0.0)
    GRAPHS["ties"] = make_nodes(t)
    case("ties/three", "ties", 500, params(5.0, 10, K=4), expect=[5, 3, 200, 450])
    case("ties/three, K short", "ties", 500, params(5.0, 10, K=2), expect=[5, 3])
    case("ties/two, the lowest shadowed", "ties", 500, params(5.0, 10, separation=2, K=4), expect=[5, 200, 450])
    case("ties/last two only", "ties", 500, params(5.0, 10, separation=197, K=4), expect=[5, 450])


# ---- passes: three runs of seven consecutive hits --------------------------------------------------------------------------------------
def _passes():
    t = filler(121)
    t[120] = (0.0, 0.0, 0.0)
    for start, y in ((10, 1.0), (40, 1.5), (70, 2.0)):
        for k in range(7):
            t[start + k] = (k - 3.0, y, 0.0)                                      # d2 = (k - 3)^2 + y^2 <= 13: the ends of a run tie
    GRAPHS["passes"] = make_nodes(t)
    want = {(0, 16): [13, 12, 14, 43, 42, 44, 73, 11, 15, 72, 74, 41, 45, 71, 75, 10],
            (2, 16): [13, 43, 73, 10, 16, 40, 46, 70, 76], (6, 16): [13, 43, 73], (50, 16): [13, 73]}
    for sep in (0, 2, 6, 50):
        for K in (1, 3, 16):
            case("passes/sep %d K %d" % (sep, K), "passes", 120, params(4.0, 20, half_window=5, separation=sep, K=K), expect=want[(sep, 16)][:K])


# ---- window ----------------------------------------------------------------------------------------------------------------------------
def _window():
    t = filler(21)
    t[20] = (0.0, 0.0, 0.0)
    t[0], t[2], t[15] = (1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (3.0, 0.0, 0.0)
    GRAPHS["window"] = make_nodes(t)
    case("window/clipped and full", "window", 20, params(4.0, 5, half_window=4, K=3), expect=[0, 2, 15])


# ---- crowd: around the capacity of the hit list -----------------------------------------------------------------------------------------
# Nodes 0 .. 3 HITS on the z axis, node i at (3 HITS - i) / 2: the query node 3 HITS sits at the origin, the nearest hits have the highest
# indices, and a radius of h / 2 gives exactly h hits.
def _crowd():
    n = 3 * HITS
    t = np.zeros((n + 1, 3))
    t[:, 2] = 0.5 * (n - np.arange(n + 1))
    GRAPHS["crowd"] = make_nodes(t)
    for h in (HITS - 1, HITS, HITS + 1, 3 * HITS):
        case("crowd/%d hits" % h, "crowd", n, params(0.5 * h, 1, K=4), expect=[n - 1, n - 2, n - 3, n - 4])
        wide = HITS + 76
        case("crowd/%d hits, wide separation" % h, "crowd", n, params(0.5 * h, 1, separation=wide, K=16),
             expect=[i for i in (n - 1, n - 2 - wide, n - 3 - 2 * wide) if i >= n - h])


# ---- estimates: t_opt / q_opt differ from t / q -----------------------------------------------------------------------------------------
def _estimates():
    rng = np.random.default_rng(7)
    q = pg.qexp(rng.uniform(-1.0, 1.0, (31, 3)))
    q_opt = pg.qexp(rng.uniform(-1.0, 1.0, (31, 3)))
    t, t_opt = filler(31), filler(31)
    t[30] = t_opt[30] = (1.0, 2.0, 3.0)
    t[4], t[9] = (2.0, 2.0, 3.0), (1.0, 4.5, 3.0)
    t_opt[4], t_opt[12] = (1.0, 2.0, 6.0), (0.5, 2.0, 3.0)
    GRAPHS["estimates"] = make_nodes(t, q, t_opt, q_opt)
    case("estimates/entered", "estimates", 30, params(3.0, 10, half_window=2, K=4), expect=[4, 9], pose=pg.POSE_ENTERED)
    case("estimates/optimized", "estimates", 30, params(3.0, 10, half_window=2, K=4), expect=[12, 4], pose=pg.POSE_OPTIMIZED)


# ---- laps: a drifted chain ---------------------------------------------------------------------------------------------------------------
LAPS_SEEDS, LAPS_QUERIES, LAPS_GROWTH = (1, 2, 3), (39, 45, 90, 130, 199), (0.0, 0.02)
LAPS_REL_GAP, LAPS_RIM = 1e-9, 1e-9


def laps_graph(seed):
    return pg.drifted_laps(seed, 200, 0, per_lap=40)


def laps_margins(t, j, p):
    """(the smallest relative gap between two neighbouring d2 of the eligible nodes, the smallest |d2 - r r| / r r)."""
    i = np.arange(max(0, j - p["min_gap"] + 1))
    if not len(i):
        return np.inf, np.inf
    d = t[i] - t[j]
    d2 = (d * d).sum(1)
    r = (j - i) * p["growth_m_per_node"] + p["radius_m"]
    s = np.sort(d2)
    gap = (np.diff(s) / s[1:]).min() if len(s) > 1 else np.inf
    return float(gap), float((np.abs(d2 - r * r) / (r * r)).min())


def _laps():
    for seed in LAPS_SEEDS:
        g = laps_graph(seed)
        GRAPHS["laps%d" % seed] = make_nodes(g["t"], g["q"])
        for growth in LAPS_GROWTH:
            for j in LAPS_QUERIES:
                p = params(3.0, 20, half_window=3, separation=6, K=4, growth_m_per_node=growth)
                # Margins: a d2 carries a few ulps (1e-16 relative) of rounding, and a chain entered on the device differs from this one by the
                # rounding of 200 compositions (1e-13).  With gaps a thousand times that, no rounding decides an order or a radius test.
                gap, rim = laps_margins(g["t"], j, p)
                assert gap >= LAPS_REL_GAP and rim >= LAPS_RIM, (seed, j, growth, gap, rim)
                case("laps/seed %d j %d growth %g" % (seed, j, growth), "laps%d" % seed, j, p,
                     expect=[160, 120, 80, 40] if (seed, j) == (1, 199) else None)


for build in (_ends, _none, _rim, _ties, _passes, _window, _crowd, _estimates, _laps):
    build()


def poses(nodes, pose):
    return (nodes["q_opt"], nodes["t_opt"]) if pose == pg.POSE_OPTIMIZED else (nodes["q"], nodes["t"])


def model(c, nodes=None, seq=0):
    """posegraph.propose_loops on a case (on `nodes` when given: the GPU test feeds what it exported)."""
    nodes = GRAPHS[c["graph"]] if nodes is None else nodes
    q, t = poses(nodes, c["pose"])
    return pg.propose_loops(q, t, c["j"], seq=seq, pose=c["pose"], **c["params"])
