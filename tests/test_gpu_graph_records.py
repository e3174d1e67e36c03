"""Graph records on the MI355X (aloam_graph_save / aloam_graph_load): the saved bytes are graph_records.pack of the three exports, byte for
byte; a record loaded into another slot or another context gives the same graph, the same solve, the same map and the same loop
registration; a sequence record and a graph record taken together continue bit for bit; every refusal leaves every slot as it was.

The context and the feeding are those of test_gpu_graph_map.py (hand-made clouds through aloam_set_last + aloam_mapping_step, solver off),
with a fourth sequence that never gets a node: its graph is the empty one and its slot the free target of the loads."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_graph_map import INFO, KF_CORNER, KF_SURF, LEAF, POSES_1, Q_ID, cloud, context

pytestmark = pytest.mark.gpu
MAP = 3                                                                          # ALOAM_GRAPH_APPLY_POSE | ALOAM_GRAPH_APPLY_MAP
CHUNK = 4096 * 16                                                                # bytes of one unit of work of the pack


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("a-loam_amd.graph_records")


@pytest.fixture(scope="module")
def pg():
    return importlib.import_module("a-loam_amd.posegraph")


def feed(gpu, inputs, add):
    """One mapping step of every sequence - inputs[b] = (corner, surf, q, t) - then a node for the sequences in `add`."""
    for b, (corner, surf, q, t) in enumerate(inputs):
        gpu.set_last(corner, surf, b)
        gpu.set_full_cloud(surf[:4], b)
        gpu.set_state([0, 0, 0, 1], [0, 0, 0], np.array(q, np.float64), np.array(t, np.float64), b)
    gpu.mapping_step()
    if add:
        gpu.graph_add_nodes(add, INFO)


def inputs_of(rng, k):
    """Sequence 0: an empty corner cloud.  1: the rotated keyframes of POSES_1.  2: about 1000 + 4050 points.  3: never a node."""
    f2 = np.concatenate([cloud(rng, 3750, (24, 24, 24)), cloud(rng, 250, (20, 20, 20), (50, 0, 0)), cloud(rng, 50, (20, 20, 20), (0, 50, 0))])
    f2[:, 3] = np.sort(f2[:, 3])
    return [(np.zeros((0, 4), np.float32), cloud(rng, 300, (20, 20, 2)), Q_ID, (1.0, 2.0, 0.5)),
            (cloud(rng, 300, (30, 30, 10)), cloud(rng, 1500, (40, 40, 20)), *POSES_1[min(k, 6)]),
            (cloud(rng, 1000, (24, 24, 24)), f2, Q_ID, (0.01 * k, -0.01 * k, 0.0)),
            (cloud(rng, 40, (5, 5, 2)), cloud(rng, 200, (8, 8, 2)), Q_ID, (0.0, 0.0, 0.0))]


def extra_edges(pg, nodes, seq):
    """A loop edge, an anchor and a robust edge of a sequence with at least seven nodes, each a few centimetres off the entered poses."""
    def rel(i, j, dt):
        q, t = pg.relative_pose(nodes["q"][i], nodes["t"][i], nodes["q"][j], nodes["t"][j])
        return q, t + np.array(dt)
    loop, robust = rel(1, 5, (0.05, -0.02, 0.01)), rel(0, 6, (-0.03, 0.04, 0.0))
    return np.concatenate([pg.make_edges(seq, 1, 5, loop[0], loop[1], np.eye(6) * 50.0),
                           pg.make_edges(seq, -1, 3, nodes["q"][3], nodes["t"][3] + np.array((0.1, 0.0, -0.1)), np.eye(6) * 400.0),
                           pg.make_edges(seq, 0, 6, robust[0], robust[1], np.eye(6) * 25.0, robust=True)])


def build_world(binding, pg, steps=18):
    """Sequence 0: one node with an empty corner cloud.  1: seven rotated nodes with a loop edge, an anchor and a robust edge.  2: eighteen
    nodes of about 1000 + 4050 points.  3: an empty graph.  Built the same way every time."""
    rng = np.random.default_rng(41)
    gpu = context(binding, batch=4)
    gpu.graph_loops_enable(2, 1 << 14, 1 << 16)
    for k in range(steps):
        feed(gpu, inputs_of(rng, k), [2] + ([1] if k < 7 else []) + ([0] if k == 0 else []))
    for b in (1, 2):
        gpu.graph_add_edges(extra_edges(pg, gpu.graph_export(b), b))
    return gpu


def model_record(gpu, R, b, keyframes=True):
    kf = tuple(gpu.graph_export_keyframes(b, feature_class=cls) for cls in (0, 1)) if keyframes else None
    return R.pack(gpu.graph_export(b), gpu.graph_export(b, edges=True), kf, LEAF if keyframes else None, seq=b)


def records(gpu, seqs, pinned=True):
    """The records of `seqs`, one uint8 array each."""
    blob, off = gpu.graph_save(seqs, pinned=pinned)
    blob = blob if pinned else blob.cpu().numpy()
    return [np.array(blob[off[i]:off[i + 1]]) for i in range(len(seqs))]


def graph_state(gpu, b, keyframes=True):
    """What the C ABI tells about the graph of slot b, with the edges' seq (the slot's own number) taken out."""
    e = gpu.graph_export(b, edges=True)
    assert (e["seq"] == b).all()
    e["seq"] = 0
    info = gpu.graph_info(b)
    out = [(info["nodes"], info["edges"]), gpu.graph_export(b).tobytes(), e.tobytes()]
    if keyframes:
        for cls in (0, 1):
            pts, off = gpu.graph_export_keyframes(b, feature_class=cls)
            out += [pts.tobytes(), off.tolist()]
        out.append(gpu.graph_keyframe_info(b)["points"])
    return out


def without_slot(rec, R):
    """A record with the header's source slot and the edges' seq (both name the slot it was saved from) set to 0."""
    rec = np.array(rec)
    h = R.header(rec)
    L = R.layout(h["nodes"], h["edges"], h["kf_points"] if h["parts"] & R.PART_KEYFRAMES else None)
    rec[:128].view(R.HEADER_DTYPE)["seq"] = 0
    rec[L["edges"]:L["edges"] + 240 * int(h["edges"])].view(R.EDGE_DTYPE)["seq"] = 0
    return rec


@pytest.fixture(scope="module")
def world(binding, pg, R):
    """Shared by the tests that leave it as it is: slot 3 is loaded into and cleared again, refusals change nothing."""
    gpu = build_world(binding, pg)
    yield {"gpu": gpu, "records": records(gpu, [0, 1, 2, 3])}
    gpu.close()


# ---- 1. the saved bytes are the model's ----------------------------------------------------------------------------------------------------
def test_save_equals_the_model(binding, pg, R):
    gpu = build_world(binding, pg)
    try:
        def same(pinned):
            got = records(gpu, [0, 1, 2, 3], pinned=pinned)
            for b in range(4):
                want = model_record(gpu, R, b)
                assert len(got[b]) == len(want) and np.array_equal(got[b], want), (b, pinned)
            return got
        got = same(True)
        same(False)                                                              # into device memory
        h = [R.header(r) for r in got]
        assert [(int(x["nodes"]), int(x["edges"])) for x in h] == [(1, 0), (7, 9), (18, 20), (0, 0)]
        assert h[0]["kf_points"][0] == 0 and h[0]["kf_points"][1] > 0            # one node with an empty corner cloud
        assert len(got[3]) == 256 and not got[3][64:].any()                      # the empty graph: a header and zeros
        L = R.layout(18, 20, h[2]["kf_points"])
        assert L["bytes"] > 20 * CHUNK and all(L[k] % CHUNK for k in ("edges", "desc", "corner", "surf", "end", "bytes"))   # many chunks, no section ends on one
        assert (gpu.graph_optimize([1, 2])["status"] == binding.GRAPH_OK).all()
        opt = same(True)
        assert not np.array_equal(opt[1], got[1])                                # q_opt, t_opt moved
        assert gpu.graph_apply([(1, 0, 7, MAP), (2, 0, 18, 1)])["status"].tolist() == [binding.GRAPH_APPLIED] * 2
        app = same(True)
        assert not np.array_equal(app[1], opt[1])                                # q, t rebased
        same(False)
    finally:
        gpu.close()


def test_a_node_kept_without_clouds_and_a_context_without_the_store(binding, pg, R):
    rng = np.random.default_rng(7)
    tiny = context(binding, batch=4, keyframes=(700, 1 << 17))                   # the corner row holds two of the three 300-point clouds
    bare = context(binding, batch=4, keyframes=None)
    try:
        for k in range(3):
            inp = inputs_of(rng, k)
            for g in (tiny, bare):
                feed(g, inp, [1])
        with pytest.raises(binding.AloamError) as e:
            tiny.synchronize()
        assert "keyframe store full" in str(e.value) and tiny.graph_keyframe_info(1)["dropped_nodes"] == 1
        rec = records(tiny, [1])[0]
        assert np.array_equal(rec, model_record(tiny, R, 1))
        p = R.parse(rec)
        assert np.diff(p["keyframes"][0][1]).tolist()[2] == 0 and np.diff(p["keyframes"][1][1]).tolist()[2] == 0 and p["keyframes"][0][1][2] > 0
        tiny.graph_load([3], rec, [0, len(rec)])                                 # the descriptor of the node without clouds survives the trip
        tiny.synchronize()
        assert graph_state(tiny, 3)[:-1] == graph_state(tiny, 1)[:-1]
        assert tiny.graph_keyframe_info(3)["points"] == tiny.graph_keyframe_info(1)["points"] and tiny.graph_keyframe_info(3)["dropped_nodes"] == 0
        rec = records(bare, [1])[0]
        assert np.array_equal(rec, model_record(bare, R, 1, keyframes=False)) and R.header(rec)["parts"] == R.PART_GRAPH
        bare.graph_load([0], rec, [0, len(rec)])
        bare.synchronize()
        assert graph_state(bare, 0, keyframes=False) == graph_state(bare, 1, keyframes=False)
    finally:
        tiny.close()
        bare.close()


# ---- 2. caps ---------------------------------------------------------------------------------------------------------------------------------
def test_caps_and_offsets(binding, world):
    import torch
    gpu, recs = world["gpu"], world["records"]
    sizes = [len(r) for r in recs[:3]]
    want = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    off = torch.full((4,), -1, dtype=torch.int64).pin_memory()
    gpu.graph_save_into([0, 1, 2], 0, 0, off.data_ptr())                         # the size query writes offsets only
    gpu.synchronize()
    assert off.tolist() == want
    buf = torch.full((want[3],), 0xAB, dtype=torch.uint8).pin_memory()
    off.fill_(-1)
    gpu.graph_save_into([0, 1, 2], buf.data_ptr(), want[1] + 256, off.data_ptr())   # holds record 0, not record 1
    gpu.synchronize()
    assert off.tolist() == want
    got = buf.numpy()
    assert np.array_equal(got[:want[1]], recs[0]) and (got[want[1]:] == 0xAB).all()
    gpu.graph_save_into([0, 1, 2], buf.data_ptr(), want[3], off.data_ptr())
    gpu.synchronize()
    for i in range(3):                                                           # a record saved in a call of three equals the same record saved alone
        assert np.array_equal(got[want[i]:want[i + 1]], records(gpu, [i])[0]), i
        assert np.array_equal(got[want[i]:want[i + 1]], recs[i]), i
    assert np.array_equal(records(gpu, [2, 0])[0], recs[2])                      # nor does it depend on its position
    blob, off0 = gpu.graph_save([])
    assert off0.tolist() == [0]


# ---- 3. load elsewhere -------------------------------------------------------------------------------------------------------------------
def loop_request(gpu, pg, b):
    n = gpu.graph_export(b)
    q, t = pg.relative_pose(n["q"][4], n["t"][4], n["q"][9], n["t"][9])
    return (b, 4, 9, 0, 9, 0, q, t)


def test_load_elsewhere(binding, pg, R):
    a = build_world(binding, pg)
    b = context(binding, batch=3, nodes=64, edges=128, keyframes=(1 << 16, 1 << 18))
    b.graph_loops_enable(2, 1 << 14, 1 << 16)
    try:
        blob, off = a.graph_save([1, 2])
        b.graph_load([0, 2], blob, off)                                          # sequence 1 -> slot 0 of the other context, sequence 2 -> its slot 2
        a.graph_load([3], blob[off[1]:], [0, off[2] - off[1]])                   # sequence 2 -> the free slot of its own context
        b.synchronize()
        a.synchronize()
        assert graph_state(b, 0) == graph_state(a, 1) and graph_state(b, 2) == graph_state(a, 2) == graph_state(a, 3)
        assert b.graph_info(0)["max_nodes"] == 64 and b.graph_info(1)["nodes"] == 0
        # A save of the loaded slot is the record that was loaded but for the header's source slot; where the slot's number differs the
        # edges differ in their seq too, which names the slot that holds them (aloam_graph_export_edges)
        back = records(b, [0, 2]) + records(a, [3])
        assert np.array_equal(back[1], blob[off[1]:off[2]])                      # slot 2 from slot 2: every byte
        assert np.array_equal(without_slot(back[0], R), without_slot(blob[off[0]:off[1]], R))
        assert np.array_equal(without_slot(back[2], R), without_slot(blob[off[1]:off[2]], R))
        assert R.header(back[0])["seq"] == 0 and R.header(back[2])["seq"] == 3 and R.header(blob, off[0])["seq"] == 1
        # the same solve, the same map, the same loop registration
        ra, rb = a.graph_optimize([1, 2, 3]), b.graph_optimize([0, 2])
        assert (ra["status"] == binding.GRAPH_OK).all() and ra[:2].tobytes() == rb.tobytes() and ra[1].tobytes() == ra[2].tobytes()
        assert graph_state(b, 0) == graph_state(a, 1) and graph_state(b, 2) == graph_state(a, 2) == graph_state(a, 3)
        for (ga, sa), (gb, sb) in (((a, 1), (b, 0)), ((a, 2), (b, 2)), ((a, 2), (a, 3))):
            ta, tb = ga.graph_export_map([(sa, 0, 7, binding.GRAPH_POSE_OPTIMIZED)]), gb.graph_export_map([(sb, 0, 7, binding.GRAPH_POSE_OPTIMIZED)])
            assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes() and len(ta[0]) > 0, (sa, sb)
        la = a.graph_register_loops([loop_request(a, pg, 2), loop_request(a, pg, 3)])
        lb = b.graph_register_loops([loop_request(b, pg, 2)])
        assert la[0]["target_raw"].min() > 0 and la[0].tobytes() == la[1].tobytes() == lb[0].tobytes()
    finally:
        a.close()
        b.close()


# ---- 4. continue -------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_record_and_a_graph_record_continue_bit_for_bit(binding, pg, sequence):
    scans = sequence("VLP-16", 3, seed=5, columns=250)[0]
    a = build_world(binding, pg, steps=7)
    b = context(binding, batch=2, nodes=64, edges=128, keyframes=(1 << 16, 1 << 18))
    try:
        seq_blob, seq_off = a.save_sequences([1])
        blob, off = a.graph_save([1])
        b.load_sequences([0], seq_blob, seq_off)
        b.graph_load([0], blob, off)
        rng = np.random.default_rng(99)
        for k in range(3):
            inp = inputs_of(rng, k)
            q, t = POSES_1[6][0], (POSES_1[6][1][0] + 2.0 * (k + 1), POSES_1[6][1][1] - 1.0 * (k + 1), POSES_1[6][1][2])
            inp[1] = (inp[1][0], inp[1][1], q, t)
            for g, n, mine in ((a, 4, inp), (b, 2, [inp[1], inp[3]])):
                g.scan_register([scans[k]] * n)                                  # a loaded slot meets an odometry step before it may map
                g.odometry_step()
                feed(g, mine, [1] if g is a else [0])
        for g, s in ((a, 1), (b, 0)):
            n = g.graph_export(s)
            assert len(n) == 10
            q, t = pg.relative_pose(n["q"][2], n["t"][2], n["q"][8], n["t"][8])
            g.graph_add_edges(np.concatenate([pg.make_edges(s, 2, 8, q, t + np.array((0.04, 0.0, -0.02)), np.eye(6) * 80.0, robust=True),
                                              pg.make_edges(s, -1, 9, n["q"][9], n["t"][9] + np.array((0.2, -0.1, 0.0)), np.eye(6) * 300.0)]))
        ra, rb = a.graph_optimize([1])[0], b.graph_optimize([0])[0]
        assert ra["status"] == binding.GRAPH_OK and ra.tobytes() == rb.tobytes()
        pa, pb = a.graph_apply([(1, 0, 10, MAP)])[0], b.graph_apply([(0, 0, 10, MAP)])[0]
        assert pa["status"] == binding.GRAPH_APPLIED and pa.tobytes() == pb.tobytes()
        assert graph_state(a, 1) == graph_state(b, 0)
        assert a.graph_info(1)["edges"] == 9 + 3 + 2                              # three odometry edges from the loaded last node on, two added
        for key, v in a.map_pose(1).items():
            assert v.tobytes() == b.map_pose(0)[key].tobytes(), key
        for key, v in a.pose(1).items():
            assert np.asarray(v).tobytes() == np.asarray(b.pose(0)[key]).tobytes(), key
        for cls in (0, 1):
            ca, cb = a.map_cubes(cls, 1), b.map_cubes(cls, 0)
            assert sorted(ca) == sorted(cb) and len(ca) > 0
            assert all(ca[k].tobytes() == cb[k].tobytes() for k in ca), cls
    finally:
        a.close()
        b.close()


# ---- 5. sources --------------------------------------------------------------------------------------------------------------------------
def test_sources_and_a_fork(binding, world, tmp_path):
    import torch
    gpu, recs = world["gpu"], world["records"]
    want = graph_state(gpu, 2)
    recs[2].tofile(tmp_path / "graph.rec")
    paged = np.fromfile(tmp_path / "graph.rec", np.uint8)                        # pageable memory, read back from a file
    pinned = torch.from_numpy(recs[2]).pin_memory()
    device = torch.from_numpy(recs[2]).cuda()
    for src in (paged, pinned, device):
        gpu.graph_load([3], src, [0, len(recs[2])])
        gpu.synchronize()
        assert graph_state(gpu, 3) == want
        gpu.graph_clear([3])
    off_dev = torch.tensor([0, len(recs[2])], dtype=torch.int64, device="cuda")   # the offsets in device memory too
    ids = np.array([3], np.int32)
    assert binding.lib().aloam_graph_load(gpu.h, ids.ctypes.data_as(C.c_void_p), 1, C.c_void_p(device.data_ptr()), C.c_void_p(off_dev.data_ptr())) == 0
    gpu.synchronize()
    assert graph_state(gpu, 3) == want
    gpu.graph_clear([3])
    gpu.synchronize()
    assert records(gpu, [3])[0].tobytes() == recs[3].tobytes()                   # the world is as it was
    b = context(binding, batch=3)
    try:
        one = recs[1]
        b.graph_load([2, 0], np.concatenate([one, one]), [0, len(one), 2 * len(one)])   # position independent: its bytes once per slot
        b.synchronize()
        assert graph_state(b, 2) == graph_state(b, 0) == graph_state(gpu, 1) and b.graph_info(1)["nodes"] == 0
    finally:
        b.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def damaged(R, rec, header=None, edge=None, desc=None):
    rec = np.array(rec)
    h = rec[:128].view(R.HEADER_DTYPE)
    L = R.layout(h["nodes"][0], h["edges"][0], h["kf_points"][0])
    for k, v in (header or {}).items():
        h[k] = v
    if edge:
        e = rec[L["edges"]:L["edges"] + 240 * int(h["edges"][0])].view(R.EDGE_DTYPE)
        for k, v in edge[1].items():
            e[k][edge[0]] = v
    if desc:
        d = rec[L["desc"]:L["corner"]].view(R.DESC_DTYPE)
        d[desc[1]][desc[0]] += desc[2]
    return rec


def test_every_refusal_leaves_every_slot_as_it_was(binding, pg, R, world):
    gpu, recs = world["gpu"], world["records"]
    good = recs[1]
    n = int(R.header(good)["nodes"])

    ctx = dict(kf_capacity=(KF_CORNER, KF_SURF), resolutions=LEAF, max_nodes=32, max_edges=64)

    def refused(g, slots, rec, code, word, offsets=None, model=None):
        """The load is refused with `code` and `word` in its text; model: what graph_records.check calls the same refusal in the world's context."""
        offsets = [0, len(rec)] if offsets is None else offsets
        with pytest.raises(binding.AloamError) as e:
            g.graph_load(slots, rec, offsets)
        assert e.value.code == code and word in str(e.value), (str(e.value), word)
        if model:
            assert R.check(rec, length=offsets[1], **ctx) == (code, model), model
    refused(gpu, [1], good, binding.E_STATE, "not empty")
    refused(gpu, [3, 3], np.concatenate([good, good]), binding.E_ARG, "repeated", [0, len(good), 2 * len(good)])
    refused(gpu, [3], damaged(R, good, {"magic": 0x51534C41}), binding.E_ARG, "magic", model="magic")
    refused(gpu, [3], damaged(R, good, {"version": 2}), binding.E_ARG, "version", model="version")
    refused(gpu, [3], damaged(R, good, {"bytes": len(good) + 256}), binding.E_ARG, "length", model="bytes")
    refused(gpu, [3], good, binding.E_ARG, "length", [0, len(good) - 256], model="bytes")
    refused(gpu, [3], damaged(R, good, {"nodes": n + 64}), binding.E_ARG, "counts", model="bytes")
    refused(gpu, [3], damaged(R, good, {"parts": R.PART_GRAPH}), binding.E_ARG, "parts", model="parts")
    refused(gpu, [3], damaged(R, good, {"line_res_bits": 0x3F000000}), binding.E_ARG, "mapping_line_resolution", model="mapping_line_resolution")
    refused(gpu, [3], damaged(R, good, {"plane_res_bits": 0x3F000000}), binding.E_ARG, "mapping_plane_resolution", model="mapping_plane_resolution")
    refused(gpu, [3], damaged(R, good, edge=(2, {"j": n})), binding.E_ARG, "payload", model="payload: edge index")
    refused(gpu, [3], damaged(R, good, edge=(7, {"i": 4, "j": 4})), binding.E_ARG, "payload", model="payload: edge index")
    refused(gpu, [3], damaged(R, good, edge=(8, {"i": -2})), binding.E_ARG, "payload", model="payload: edge index")
    refused(gpu, [3], damaged(R, good, edge=(0, {"flags": 2})), binding.E_ARG, "payload", model="payload: edge flags")
    refused(gpu, [3], damaged(R, good, desc=(3, "first", (0, 1))), binding.E_ARG, "payload", model="payload: descriptor chain")
    refused(gpu, [3], damaged(R, good, desc=(3, "count", (-400, 0))), binding.E_ARG, "payload", model="payload: descriptor chain")
    refused(gpu, [3], damaged(R, good, desc=(n - 1, "count", (1, 0))), binding.E_ARG, "payload", model="payload: descriptor total")   # the total disagrees with the header
    assert R.check(good, **ctx) is None
    gpu.synchronize()
    after = records(gpu, [0, 1, 2, 3])
    assert all(np.array_equal(x, y) for x, y in zip(after, recs))
    # targets that differ from the source
    for kw, rec, code, word in (({"nodes": 16}, recs[2], binding.E_CAPACITY, "max_nodes"), ({"edges": 8}, recs[2], binding.E_CAPACITY, "max_edges"),
                                ({"keyframes": (100, 1 << 17)}, recs[2], binding.E_CAPACITY, "corner"), ({"keyframes": (1 << 15, 1000)}, recs[2], binding.E_CAPACITY, "surf"),
                                ({"keyframes": None}, good, binding.E_ARG, "parts")):
        g = context(binding, batch=2, **kw)
        try:
            before = records(g, [0, 1])
            refused(g, [0], rec, code, word)
            refused(g, [1, 0], np.concatenate([recs[3] if kw.get("keyframes", 1) else before[0], rec]), code, word, [0, 256, 256 + len(rec)])
            g.synchronize()
            assert all(np.array_equal(x, y) for x, y in zip(records(g, [0, 1]), before))
            if kw.get("keyframes", 1) is None:
                refused(gpu, [3], before[0], binding.E_ARG, "parts")             # and a record without clouds into a context that keeps them
        finally:
            g.close()
    bare = binding.Aloam(n_scans=16, min_range=0.3, batch=1, max_points=4096)
    try:
        with pytest.raises(binding.AloamError) as e:
            bare.graph_save([0])
        assert e.value.code == binding.E_STATE
        refused(bare, [0], good, binding.E_STATE, "not enabled")
    finally:
        bare.close()
    assert all(np.array_equal(x, y) for x, y in zip(records(gpu, [0, 1, 2, 3]), recs))
