"""k_solve keeps its factor records in LDS from the first evaluation of a solve on (odometry_solve_device.hpp; ALOAM_SOLVE_STAGE, default on).  With
ALOAM_SOLVE_STAGE=0 every evaluation reads the records from global memory.  Both forms perform the same operations on the same operands in the same order,
so every case here runs in a context of either kind and demands the two agree BIT FOR BIT on para_q, para_t, q_w, t_w, both outer iterations' costs, the
iteration, success and correspondence counts and the termination codes; and the context that keeps the records must match the oracle within the bounds
of test_gpu_parity.test_lm_branch_coverage.

A thread of the solve owns records t, t + 128, ... of a class (its slots); what goes wrong in this code goes wrong per slot and per thread: a slot marked
valid that is not, a thread without a record, a class with fewer records than threads.  An invalid record here is a query farther than 5 m from every point
of the last cloud (the association's own rule), put at chosen indices of real feature lists."""
from types import SimpleNamespace

import numpy as np
import pytest

import assoc_cases
import lm_scenarios
from test_gpu_parity import _assert_pose_close, _mk

pytestmark = pytest.mark.gpu

INT_STATS = ("corner_corr", "plane_corr", "lm_iterations", "lm_successful", "termination")
GOOD = (np.array(lm_scenarios.GOOD[0]) / np.linalg.norm(lm_scenarios.GOOD[0]), np.array(lm_scenarios.GOOD[1]))


def _bits(stats, pose):
    """Everything the two kinds of context must agree on, as bytes (NaN costs compare by their bits)."""
    return b"".join(np.asarray(stats[k], np.float64 if "cost" in k else np.int64).tobytes() for k in sorted(stats)) + \
        b"".join(np.asarray(pose[k], np.float64).tobytes() for k in ("q_lc", "t_lc", "q_w", "t_w"))


def _assert_matches_oracle(so, po, sg, pg, ctx):
    """The bounds of test_lm_branch_coverage."""
    for key in INT_STATS:
        assert so[key] == sg[key], (ctx, key, so, sg)
    for k in range(2):
        a, b = so["final_cost"][k], sg["final_cost"][k]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * abs(a) + 1e-16, (ctx, so, sg)
    _assert_pose_close(po, pg, ctx)


def kept_slots(n_scans, distortion=False):
    """(plane slots, edge slots, bytes) a solve keeps, restated from the issue: 48 / 44 bytes per slot (4 more with distortion) for each of 128 threads,
    80 KiB less the 448 bytes of the block reduction, planes first, then the edges that still fit."""
    per_p, per_e, room = (48 + 4 * distortion) * 128, (44 + 4 * distortion) * 128, 80 * 1024 - 448
    kp = min(-(-n_scans * 24 // 128), room // per_p)
    ke = min(-(-n_scans * 12 // 128), (room - kp * per_p) // per_e)
    return kp, ke, kp * per_p + ke * per_e


class Pair:
    """A context that keeps the records in LDS and one that does not, otherwise alike.  That the two really differ is read back from the library
    (aloam_get_solve_lds): agreement of two contexts that both ignored the switch would prove nothing."""

    def __init__(self, binding, monkeypatch, model, **kw):
        monkeypatch.delenv("ALOAM_SOLVE_STAGE", raising=False)
        self.kept = _mk(binding, model, **kw)
        monkeypatch.setenv("ALOAM_SOLVE_STAGE", "0")
        self.plain = _mk(binding, model, **kw)
        monkeypatch.delenv("ALOAM_SOLVE_STAGE")
        want = kept_slots(model.n_scans, bool(kw.get("distortion", False)))
        assert want[0] > 0 and self.kept.solve_lds() == want and self.plain.solve_lds() == (0, 0, 0), (self.kept.solve_lds(), self.plain.solve_lds(), want)

    def both(self):
        return self.kept, self.plain

    def close(self):
        self.kept.close()
        self.plain.close()


@pytest.fixture(scope="module")
def scenarios(O, sequence):
    return lm_scenarios.build(O, sequence)


@pytest.fixture(scope="module")
def problems(O, sequence):
    """problem(sensor) -> (model, features of the third sweep, last corner cloud, last surf cloud), from three registered sweeps; built once."""
    cache = {}

    def get(name):
        if name not in cache:
            scans, R, t, model = sequence(name, 3, seed=9, columns=512)
            orc = O.Oracle(n_scans=model.n_scans, min_range=model.min_range, ring_from_field=model.ring_from_field)
            feats = []
            for x in scans:
                feats.append(orc.scan_register(x))
                orc.odometry_step()
            # The synthetic sensors leave some rings without returns; the feature lists are filled up to the capacity of a sweep (12 and 24 per ring) with
            # points of the sweep's own less-sharp / less-flat clouds, so that a thread of the solve has every slot its sensor can give it.
            f = dict(feats[2])
            for k, pool, per_ring in (("sharp", "less_sharp", 12), ("flat", "less_flat", 24)):
                more = f[pool][np.linspace(0, len(f[pool]) - 1, model.n_scans * per_ring - len(f[k])).astype(int)]
                both = np.concatenate([f[k], more])
                f[k] = both[np.argsort(both[:, 3].astype(int), kind="stable")]
            cache[name] = (model, f, feats[1]["less_sharp"], feats[1]["less_flat"])
        return cache[name]
    return get


def _far(points, invalid):
    """The listed features moved a kilometre off (distinct places, ring and time kept): no point of the last cloud within 5 m of them at any pose tried here."""
    out = points.copy()
    idx = np.flatnonzero(invalid)
    out[idx, 0] = 1000.0 + 7.0 * np.arange(len(idx), dtype=np.float32)
    out[idx, 1] = -1000.0
    out[idx, 2] = 500.0
    return out


def _scene(f, corner, surf, n_sharp=None, n_flat=None, bad_sharp=None, bad_flat=None):
    """The problem with its feature lists cut to n_sharp / n_flat and the features that bad_*(n) marks (a boolean mask) made invalid."""
    sharp = f["sharp"][:len(f["sharp"]) if n_sharp is None else n_sharp]
    flat = f["flat"][:len(f["flat"]) if n_flat is None else n_flat]
    ms = np.zeros(len(sharp), bool) if bad_sharp is None else np.asarray(bad_sharp(len(sharp)), bool)
    mf = np.zeros(len(flat), bool) if bad_flat is None else np.asarray(bad_flat(len(flat)), bool)
    return SimpleNamespace(sharp=_far(sharp, ms), flat=_far(flat, mf), less_sharp=corner, less_flat=surf, n_valid=(int((~ms).sum()), int((~mf).sum())))


def _step(dev, s, pose=GOOD, **seq):
    assoc_cases.feed(dev, s, pose, **seq)
    dev.odometry_step()
    return dev.odom_stats(**seq), dev.pose(**seq)


ALL = lambda n: np.ones(n, bool)
PATTERNS = {
    # name: (n_sharp, n_flat, invalid sharp, invalid flat)
    "nothing-valid": (None, None, ALL, ALL),
    "edges-only": (None, None, None, ALL),
    "one-plane": (None, None, ALL, "all but one that has a correspondence"),
    "every-second-plane": (None, None, None, lambda n: np.arange(n) % 2 == 1),
    "every-128th-plane": (None, None, None, lambda n: np.arange(n) % 128 != 5),
    "first-and-last-invalid": (None, None, lambda n: np.isin(np.arange(n), (0, n - 1)), lambda n: np.isin(np.arange(n), (0, n - 1))),
    "flat127": (None, 127, None, None), "flat128": (None, 128, None, None), "flat129": (None, 129, None, None), "flat-full": (None, None, None, None),
    "sharp0": (0, None, None, None), "sharp1": (1, None, None, None),
}


@pytest.mark.parametrize("lm,outer", [(4, 2), (0, 2), (8, 2), (2, 3), (4, 1)])
def test_lm_scenarios_kept_and_plain(O, binding, monkeypatch, scenarios, lm, outer):
    """The problems that leave the happy path (rejected steps, bad warm starts, non-finite residuals, fewer rows than parameters), at iteration limits from
    0 (the records are written to LDS and never read) to 8 (read eight times)."""
    model, scs = scenarios
    pair = Pair(binding, monkeypatch, model, max_points=40000, lm_max_iterations=lm, outer_iterations=outer)
    orc = O.Oracle(n_scans=64, min_range=model.min_range, lm_max_iterations=lm, outer_iterations=outer)
    done = set()
    for sc in scs:
        name = sc[0].replace("-lm4", "").replace("-lm8", "").replace("-outer6", "")     # the scenario's own limits are replaced by this case's
        if name in done:
            continue
        done.add(name)
        sk, pk = lm_scenarios.run(pair.kept, sc)
        sp, pp = lm_scenarios.run(pair.plain, sc)
        assert _bits(sk, pk) == _bits(sp, pp), (name, sk, sp, pk, pp)
        so, po = lm_scenarios.run(orc, sc)
        _assert_matches_oracle(so, po, sk, pk, name)
    assert len(done) >= 70
    pair.close()


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_validity_patterns(O, binding, monkeypatch, problems, pattern):
    """HDL-64: twelve plane slots and six edge slots per thread, of which the LDS holds the twelve and one."""
    model, f, corner, surf = problems("HDL-64")
    assert len(f["flat"]) == 64 * 24 and len(f["sharp"]) == 64 * 12
    ns, nf, bad_s, bad_f = PATTERNS[pattern]
    pair = Pair(binding, monkeypatch, model, max_points=40000)
    if pattern == "one-plane":
        _step(pair.kept, _scene(f, corner, surf))
        pq = pair.kept.correspondences()[3]
        keep_one = int(pq[len(pq) // 2])
        bad_f = lambda n: np.arange(n) != keep_one
    s = _scene(f, corner, surf, ns, nf, bad_s, bad_f)
    sk, pk = _step(pair.kept, s)
    sp, pp = _step(pair.plain, s)
    print(pattern, sk)
    assert _bits(sk, pk) == _bits(sp, pp), (pattern, sk, sp, pk, pp)
    assert sk["corner_corr"][0] <= s.n_valid[0] and sk["plane_corr"][0] <= s.n_valid[1]
    if pattern == "nothing-valid":
        assert sk["termination"] == [4, 4] and sk["corner_corr"] == [0, 0] and sk["plane_corr"] == [0, 0]
        assert np.array_equal(pk["q_lc"], GOOD[0]) and np.array_equal(pk["t_lc"], GOOD[1]), pk       # the pose is left as it was
    if pattern == "edges-only":
        assert sk["plane_corr"] == [0, 0] and sk["corner_corr"][0] > 100
    if pattern == "one-plane":
        assert sk["corner_corr"] == [0, 0] and sk["plane_corr"][0] == 1
    if pattern == "every-128th-plane":
        assert 0 < sk["plane_corr"][0] <= 12
    orc = O.Oracle(n_scans=64, min_range=model.min_range)
    so, po = _step(orc, s)
    _assert_matches_oracle(so, po, sk, pk, pattern)
    pair.close()


@pytest.mark.parametrize("sensor,n_sharp", [("VLP-16", None), ("VLP-16", 100), ("HDL-64", None), ("ROWS128", None)])
def test_sensors(O, binding, monkeypatch, problems, sensor, n_sharp):
    """VLP-16: three plane slots per thread; 192 edge records give threads 0 - 63 two slots and the others one, and the first 100 of them alone leave
    threads 100 - 127 beyond the edge count, with no edge slot at all.  HDL-64: the LDS is full.  128 rings: 24 plane slots per thread, of which thirteen
    fit and no edge slot does - the others come from global memory in every pass, in slot order behind the kept ones."""
    model, f, corner, surf = problems(sensor)
    assert len(f["flat"]) == model.n_scans * 24 and len(f["sharp"]) == model.n_scans * 12
    s = _scene(f, corner, surf, n_sharp=n_sharp)
    pair = Pair(binding, monkeypatch, model, max_points=model.n_scans * 512 + 4096)
    sk, pk = _step(pair.kept, s)
    sp, pp = _step(pair.plain, s)
    print(sensor, n_sharp, pair.kept.solve_lds(), sk)
    assert _bits(sk, pk) == _bits(sp, pp), (sensor, sk, sp, pk, pp)
    assert sk["plane_corr"][1] > model.n_scans * 8 and sk["corner_corr"][1] > (model.n_scans * 2 if n_sharp is None else n_sharp // 2), sk
    assert n_sharp is None or sk["corner_corr"][1] <= n_sharp < 128
    orc = O.Oracle(n_scans=model.n_scans, min_range=model.min_range, ring_from_field=model.ring_from_field)
    so, po = _step(orc, s)
    _assert_matches_oracle(so, po, sk, pk, sensor)
    pair.close()


def test_distortion_mode(O, binding, monkeypatch, sequence):
    """One free-running sequence with distortion = 1: the interpolation fraction of a record travels through LDS too (52 and 48 bytes per slot)."""
    scans, R, t, model = sequence("HDL-64", 3, seed=9, columns=512)
    pair = Pair(binding, monkeypatch, model, max_points=40000, distortion=True)
    orc = O.Oracle(n_scans=model.n_scans, min_range=model.min_range, distortion=True)
    for k, x in enumerate(scans):
        orc.scan_register(x)
        po = orc.odometry_step()
        for g in pair.both():
            g.scan_register(x)
            g.odometry_step()
        sk, pk = pair.kept.odom_stats(), pair.kept.pose()
        assert _bits(sk, pk) == _bits(pair.plain.odom_stats(), pair.plain.pose()), k
        _assert_matches_oracle(orc.odom_stats(), po, sk, pk, f"distortion, sweep {k}")
    assert pair.kept.solve_lds()[:2] == (12, 0)                  # 52 bytes per plane slot: the twelve fit, no edge slot beside them
    assert sk["plane_corr"][1] > 700 and sk["lm_iterations"][1] > 0 and np.linalg.norm(pk["t_lc"]) > 0.5, (sk, pk)
    pair.close()


def test_batch_of_five_with_an_idle_and_a_first_frame_sequence(O, binding, monkeypatch, problems):
    """Sequence 0 sits the step out, sequence 1 meets its first frame, 2 - 4 solve problems of different sizes.  The first two keep their state bit for bit."""
    model, f, corner, surf = problems("HDL-64")
    scenes = [_scene(f, corner, surf), _scene(f, corner, surf), _scene(f, corner, surf), _scene(f, corner, surf, n_sharp=5, n_flat=129),
              _scene(f, corner, surf, n_sharp=300, n_flat=1000, bad_flat=lambda n: np.arange(n) % 3 == 0)]
    pair = Pair(binding, monkeypatch, model, batch=5, max_points=40000)
    out = []
    for g in pair.both():
        for b, s in enumerate(scenes):
            assoc_cases.feed(g, s, GOOD, seq=b)
        g.reset_sequences([1])
        g.set_features(assoc_cases.posed(scenes[1], GOOD), seq=1)
        g.synchronize()
        before = [g.pose(seq=b) for b in range(5)]
        g.set_active([0, 1, 1, 1, 1])
        g.odometry_step()
        g.set_active(None)
        g.synchronize()
        after = [(g.odom_stats(seq=b), g.pose(seq=b)) for b in range(5)]
        for b in (0, 1):
            for k in ("q_lc", "t_lc", "q_w", "t_w"):
                assert np.array_equal(before[b][k], after[b][1][k]), (b, k, before[b], after[b][1])
        out.append(after)
    for b in range(5):
        assert _bits(*out[0][b]) == _bits(*out[1][b]), (b, out[0][b], out[1][b])
    counts = [out[0][b][0]["plane_corr"][1] for b in (2, 3, 4)]
    assert counts[0] > 1000 and 0 < counts[1] <= 129 and 129 < counts[2] < 700, counts
    for b in (2, 3, 4):
        orc = O.Oracle(n_scans=64, min_range=model.min_range)
        so, po = _step(orc, scenes[b])
        _assert_matches_oracle(so, po, out[0][b][0], out[0][b][1], f"batch sequence {b}")
    pair.close()


def test_pose_information_is_the_same(binding, monkeypatch, problems):
    """aloam_export_pose_information(ALOAM_INFO_ODOMETRY) evaluates the records once more with the solver's own function: from poses that are bit-equal
    the records must be too."""
    model, f, corner, surf = problems("HDL-64")
    s = _scene(f, corner, surf, bad_flat=lambda n: np.arange(n) % 5 == 2)
    pair = Pair(binding, monkeypatch, model, max_points=40000)
    recs = []
    for g in pair.both():
        st, pose = _step(g, s)
        rec = g.export_pose_information(binding.INFO_ODOMETRY, [0])
        assert int(rec[0]["status"]) == binding.INFO_OK and int(rec[0]["n_plane"]) == st["plane_corr"][1]
        recs.append((_bits(st, pose), rec.tobytes()))
    assert recs[0] == recs[1]
    pair.close()
