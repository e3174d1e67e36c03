"""aloam_graph_propose_loops on the MI355X against posegraph.propose_loops, byte for byte: dst, counts and dist2.

One context holds every graph of graph_propose_cases.py, entered in one aloam_graph_load of records made with graph_records.pack; the three
`laps` chains are also entered through aloam_set_state / aloam_graph_add_nodes (posegraph_cases.enter) in slots of their own.  The model is
fed the exported nodes.  All calls are made once (the fixture) and the tests look at what they left."""
import importlib

import numpy as np
import pytest

import graph_propose_cases as gc
import posegraph_cases as pc
from graph_propose_cases import pg

gr = importlib.import_module("a-loam_amd.graph_records")

pytestmark = pytest.mark.gpu
NAMES = list(gc.GRAPHS)
SEQ = {name: s for s, name in enumerate(NAMES)}
ENTERED = {"laps%d" % seed: len(NAMES) + k for k, seed in enumerate(gc.LAPS_SEEDS)}
BATCH = len(NAMES) + len(ENTERED)
SHARED = gc.params(3.0, 20, half_window=3, separation=6, K=4, growth_m_per_node=0.02)          # the parameters of the mixed lists
ROUND = gc.constant("kProposeStageItems")
SENTINEL, TAIL = 0xA5, 64


def mixed_queries():
    """(seq, j) over every graph, loaded and entered: the laps queries, and the first, a middle and the last node of every other graph."""
    qs = []
    for name, s in SEQ.items():
        n = len(gc.GRAPHS[name])
        qs += [(s, j) for j in (gc.LAPS_QUERIES if name.startswith("laps") else sorted({0, n // 2, n - 1}))]
    qs += [(s, j) for s in ENTERED.values() for j in gc.LAPS_QUERIES]
    return qs


def expected(world, seq, j, p, pose):
    req, count, d2 = pg.propose_loops(*gc.poses(world["nodes"][seq], pose), j, seq=seq, pose=pose, **p)
    return req.tobytes(), count, d2.tobytes()


def got(out, k):
    req, counts, d2 = out
    return req[k].tobytes(), int(counts[k]), d2[k].tobytes()


@pytest.fixture(scope="module")
def world(binding):
    import torch
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=BATCH, max_points=4096)
    gpu.graph_enable(max(len(g) for g in gc.GRAPHS.values()), 256)
    recs = [gr.pack(gc.GRAPHS[name], np.zeros(0, pg.EDGE_DTYPE), seq=SEQ[name]) for name in NAMES]
    gpu.graph_load([SEQ[name] for name in NAMES], np.concatenate(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]))
    laps = {name: gc.laps_graph(int(name[4:])) for name in ENTERED}
    pc.enter(gpu, {s: (laps[name]["q"], laps[name]["t"]) for name, s in ENTERED.items()}, laps["laps1"]["info"])
    gpu.synchronize()
    nodes = {s: gpu.graph_export(s) for s in range(BATCH)}
    edges = {s: gpu.graph_export(s, edges=True) for s in ENTERED.values()}
    w = dict(gpu=gpu, nodes=nodes, B=binding)
    # ---- every case, a call of its own; the laps cases also on the entered chains
    w["cases"] = [(c, SEQ[c["graph"]]) for c in gc.CASES] + [(c, ENTERED[c["graph"]]) for c in gc.CASES if c["graph"] in ENTERED]
    w["case_out"] = [gpu.graph_propose_loops([(s, c["j"])], pose=c["pose"], **c["params"]) for c, s in w["cases"]]
    # ---- batch independence, with one set of parameters
    qs = mixed_queries()
    w["mixed"] = qs
    w["forward"] = gpu.graph_propose_loops(qs, **SHARED)
    w["backward"] = gpu.graph_propose_loops(qs[::-1], **SHARED)
    w["device"] = gpu.graph_propose_loops(qs, pinned=False, **SHARED)
    w["alone"] = [gpu.graph_propose_loops([q], **SHARED) for q in qs]
    w["thrice"] = gpu.graph_propose_loops([qs[3], qs[0], qs[3], qs[3]], **SHARED)
    w["long"] = gpu.graph_propose_loops((qs * (ROUND // len(qs) + 2))[:ROUND + 5], **SHARED)
    # ---- sentinels behind the destinations; dist2 = NULL
    n, K = len(qs), SHARED["K"]
    sizes = dict(dst=n * K * pg.LOOP_REQUEST_DTYPE.itemsize, counts=n * 4, dist2=n * K * 8)
    buf = {k: torch.full((v + TAIL,), SENTINEL, dtype=torch.uint8, pin_memory=True) for k, v in sizes.items()}
    gpu.graph_propose_loops_into(qs, buf["dst"].data_ptr(), buf["counts"].data_ptr(), buf["dist2"].data_ptr(), **SHARED)
    gpu.synchronize()
    w["sentinel"] = {k: v.numpy().copy() for k, v in buf.items()}
    nul = {k: torch.full((v + TAIL,), SENTINEL, dtype=torch.uint8, pin_memory=True) for k, v in sizes.items()}
    gpu.graph_propose_loops_into(qs, nul["dst"].data_ptr(), nul["counts"].data_ptr(), 0, **SHARED)
    gpu.synchronize()
    w["null"] = {k: v.numpy().copy() for k, v in nul.items()}
    w["sizes"] = sizes
    w["after"] = ({s: gpu.graph_export(s) for s in range(BATCH)}, {s: gpu.graph_export(s, edges=True) for s in ENTERED.values()})
    w["edges"] = edges
    yield w
    gpu.close()


def test_every_case_against_the_model(world):
    bad = []
    for (c, s), out in zip(world["cases"], world["case_out"]):
        want = expected(world, s, c["j"], c["params"], c["pose"])
        have = got(out, 0)
        taken = out[0][0]["i"][:have[1]].tolist()
        print(c["name"], "seq", s, "count", have[1], "taken", taken)
        if have != want or (c["expect"] is not None and s < len(NAMES) and taken != c["expect"]):
            bad.append((c["name"], s, taken))
    assert not bad, bad


def test_the_list_and_the_rescan_give_the_same_bytes(world):
    """The crowd cases straddle the capacity of the list: one hit fewer and one hit more than it holds differ in nothing but the hit that
    is out of reach of K = 4 rounds."""
    outs = {c["name"]: out for (c, s), out in zip(world["cases"], world["case_out"]) if c["graph"] == "crowd"}
    a, b, c, d = (outs["crowd/%d hits" % h] for h in (gc.HITS - 1, gc.HITS, gc.HITS + 1, 3 * gc.HITS))
    assert got(a, 0) == got(b, 0) == got(c, 0) == got(d, 0) and got(a, 0)[1] == 4
    wide = outs["crowd/%d hits, wide separation" % (3 * gc.HITS)]
    assert got(wide, 0)[1] == 3 and wide[0][0]["i"][:3].tolist() == [3 * gc.HITS - 1, 2 * gc.HITS - 78, gc.HITS - 155]


def test_entered_and_loaded_chains(world):
    """Behind aloam_graph_add_nodes the estimates are the device's own compositions: the same nodes are taken as on the loaded chain."""
    by = {}
    for (c, s), out in zip(world["cases"], world["case_out"]):
        if c["graph"] in ENTERED:
            by.setdefault(c["name"], []).append(out[0][0]["i"][:int(out[1][0])].tolist())
    assert len(by) == 30 and all(len(v) == 2 and v[0] == v[1] and len(v[0]) >= 1 for v in by.values()), by


def test_a_query_does_not_depend_on_its_batch(world):
    qs = world["mixed"]
    n = len(qs)
    for k, (s, j) in enumerate(qs):
        want = expected(world, s, j, SHARED, pg.POSE_OPTIMIZED)
        assert got(world["forward"], k) == want, (s, j)
        assert got(world["backward"], n - 1 - k) == want and got(world["device"], k) == want and got(world["alone"][k], 0) == want, (s, j)
    assert any(got(world["forward"], k)[1] > 0 for k in range(n))
    t = world["thrice"]
    assert got(t, 0) == got(t, 2) == got(t, 3) == got(world["forward"], 3) and got(t, 1) == got(world["forward"], 0)
    long = world["long"]
    assert len(long[1]) == ROUND + 5 > ROUND
    for k in range(ROUND + 5):
        assert got(long, k) == got(world["forward"], k % n), k


def test_nothing_is_written_behind_the_destinations(world):
    f, sizes = world["forward"], world["sizes"]
    whole = dict(dst=f[0].tobytes(), counts=f[1].astype(np.int32).tobytes(), dist2=f[2].tobytes())
    for k, size in sizes.items():
        for which in ("sentinel", "null"):
            b = world[which][k]
            assert (b[size:] == SENTINEL).all() and len(b) == size + TAIL, (which, k)
            if not (which == "null" and k == "dist2"):
                assert b[:size].tobytes() == whole[k], (which, k)
    assert (world["null"]["dist2"] == SENTINEL).all()                               # dist2 = NULL: nothing of it is touched


def test_the_graph_is_only_read(world):
    nodes, edges = world["after"]
    assert all(nodes[s].tobytes() == world["nodes"][s].tobytes() for s in nodes)
    assert all(edges[s].tobytes() == world["edges"][s].tobytes() and len(edges[s]) == 199 for s in edges)


def test_refusals_leave_the_destinations_alone(world):
    import torch
    gpu, B = world["gpu"], world["B"]
    K = 4
    buf = {k: torch.full((v,), SENTINEL, dtype=torch.uint8, pin_memory=True) for k, v in dict(dst=2 * K * 96 + 16, counts=2 * 4 + 16, dist2=2 * K * 8 + 16).items()}
    ptr = {k: v.data_ptr() for k, v in buf.items()}
    good = dict(queries=[(SEQ["ties"], 500), (SEQ["rim"], 40)], dst=ptr["dst"], counts=ptr["counts"], dist2=ptr["dist2"], pose=1, radius_m=5.0,
                growth_m_per_node=0.0, min_gap=10, half_window=3, separation=2, K=K)
    pageable = np.zeros(4096, np.uint8)
    refused = [dict(queries=[(-1, 0)]), dict(queries=[(BATCH, 0)]), dict(queries=[(SEQ["rim"], -1)]), dict(queries=[(SEQ["rim"], 41)]),
               dict(queries=[(SEQ["ties"], 500), (SEQ["one"], 1)]), dict(pose=2), dict(pose=-1), dict(radius_m=float("nan")), dict(radius_m=float("inf")),
               dict(radius_m=-1.0), dict(growth_m_per_node=float("nan")), dict(growth_m_per_node=float("inf")), dict(growth_m_per_node=-0.5),
               dict(min_gap=0), dict(half_window=-1), dict(half_window=10), dict(separation=-1), dict(K=0), dict(K=17),
               dict(dst=pageable.ctypes.data), dict(counts=pageable.ctypes.data), dict(dist2=pageable.ctypes.data), dict(dst=0), dict(counts=0),
               dict(dst=ptr["dst"] + 4), dict(counts=ptr["counts"] + 2), dict(dist2=ptr["dist2"] + 4)]
    for change in refused:
        a = dict(good, **change)
        with pytest.raises(B.AloamError) as e:
            gpu.graph_propose_loops_into(a.pop("queries"), a.pop("dst"), a.pop("counts"), a.pop("dist2"), **a)
        assert e.value.code == B.E_ARG, change
    L = B.lib()
    qs = np.array(good["queries"], np.int32)
    tail = (1, 5.0, 0.0, 10, 3, 2, K, ptr["dst"], ptr["counts"], ptr["dist2"])
    assert L.aloam_graph_propose_loops(gpu.h, qs.ctypes.data, -1, *tail) == B.E_ARG and L.aloam_graph_propose_loops(gpu.h, None, 2, *tail) == B.E_ARG
    assert L.aloam_graph_propose_loops(gpu.h, None, 0, *tail) == 0                 # n = 0 is ALOAM_OK
    gpu.synchronize()
    assert all((v.numpy() == SENTINEL).all() for v in buf.values())
    a = dict(good)
    gpu.graph_propose_loops_into(a.pop("queries"), a.pop("dst"), a.pop("counts"), a.pop("dist2"), **a)      # and the call they vary is accepted
    gpu.synchronize()
    assert buf["counts"].numpy()[:8].view(np.int32).tolist() == [3, 1]


def test_state_error_before_graph_enable(binding):
    import torch
    gpu = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=4096)
    try:
        buf = torch.full((512,), SENTINEL, dtype=torch.uint8, pin_memory=True)
        with pytest.raises(binding.AloamError) as e:
            gpu.graph_propose_loops_into([(0, 0)], buf.data_ptr(), buf.data_ptr() + 256, 0, radius_m=3.0, min_gap=1)
        assert e.value.code == binding.E_STATE
        gpu.synchronize()
        assert (buf.numpy() == SENTINEL).all()
    finally:
        gpu.close()
