"""Place recognition, the numpy model alone (no GPU, no library): scan-context descriptors of a 300 m street drive find the stored place
and the yaw of queries rendered aside of it and turned; the sign convention of the shift; and the input checks the GPU tests rely on."""
import importlib
import math

import numpy as np
import pytest
import torch

from places_common import MATCH_DRIVE, MATCH_T, db_slots, kept, query_slots

pl = importlib.import_module("a-loam_amd.places")

QUERY_FRAMES = (21, 55, 97, 131, 171)
MOVES = ((0.0, 0.0), (1.5, 30.0), (-2.0, 180.0))         # metres sideways (the sensor's +y), degrees of extra yaw


def _rz(deg):
    a = math.radians(deg)
    return torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


@pytest.fixture(scope="module")
def street(syn):
    world = syn.make_street_world(7)
    R, t = syn.trajectory_travel(200, 1.6, seed=7)
    model = syn.sensor_model("HDL-64", columns=512)
    gen = torch.Generator().manual_seed(77 + 7)

    def render(Rk, tk):
        s = syn.render_scan(world, model, Rk, tk, 0.02, gen, max_range=syn.STREET_MAX_RANGE, cull=True).numpy()
        return pl.scan_context(kept(s, model.min_range))
    db = np.stack([render(R[k], t[k]) for k in range(0, 200, 2)])
    return R, t, db, render


def test_moved_and_turned_queries_find_their_place_and_yaw(street):
    R, t, db, render = street
    for k in QUERY_FRAMES:
        far = np.abs(2 * np.arange(len(db)) - k) > 8
        for side, yaw in MOVES:
            q = render(R[k] @ _rz(yaw), t[k] + R[k] @ torch.tensor([0.0, side, 0.0], dtype=torch.float64))
            ent, sh, di = pl.match(q, db, 1)
            d_far = pl.match(q, db[far], 1)[2][0]
            print(f"frame {k} side {side:+.1f} m yaw {yaw:5.1f} deg: entry {ent[0]} (frame {2 * ent[0]}) shift {sh[0]} d {di[0]:.3f}; best entry > 8 frames away {d_far:.3f}")
            assert abs(2 * int(ent[0]) - k) <= 2, (k, side, yaw, ent, di)
            want = round(yaw / pl.SECTOR_DEG) % pl.SECTORS
            assert min((int(sh[0]) - want) % pl.SECTORS, (want - int(sh[0])) % pl.SECTORS) <= 1, (k, side, yaw, sh)


def test_a_query_with_thirty_degrees_of_extra_yaw_matches_with_shift_five():
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((40000, 3)) * [25.0, 25.0, 1.5]).astype(np.float32)
    a = math.radians(30.0)                               # the sensor turned by +30 deg sees every point 30 deg further clockwise
    q = p.copy()
    q[:, 0] = (math.cos(a) * p[:, 0] + math.sin(a) * p[:, 1]).astype(np.float32)
    q[:, 1] = (-math.sin(a) * p[:, 0] + math.cos(a) * p[:, 1]).astype(np.float32)
    d, shift = pl.distance(pl.scan_context(q), pl.scan_context(p))
    assert shift == 5 and d < 0.02, (d, shift)
    # and the guess puts the sensor at the stored pose turned by +30 deg about its own z
    qc, tc = pl.guess_from_match([0, 0, 0, 1], [4.0, -2.0, 0.5], shift, [0, 0, 0, 1], [0, 0, 0])
    assert np.allclose(qc, [0, 0, math.sin(a / 2), math.cos(a / 2)]) and np.allclose(tc, [4.0, -2.0, 0.5])
    # an odometry pose that is not the identity is taken out again: map pose = correction * odometry pose
    oq, ot = np.array([0, 0, math.sin(0.2), math.cos(0.2)]), np.array([1.0, 2.0, 3.0])
    qc, tc = pl.guess_from_match([0, 0, 0, 1], [4.0, -2.0, 0.5], 0, oq, ot)
    from importlib import import_module
    rl = import_module("a-loam_amd.relocalize")
    assert np.allclose(rl._qmul(qc, oq), [0, 0, 0, 1]) and np.allclose(rl._qrot(qc, ot) + tc, [4.0, -2.0, 0.5])


def test_distance_rules():
    rng = np.random.default_rng(5)
    c = rng.random((pl.RINGS, pl.SECTORS)).astype(np.float32)
    c[:, 10:20] = 0
    assert pl.distance(c, c) == (pytest.approx(0.0, abs=1e-12), 0)
    d, s = pl.distance(np.roll(c, 7, axis=1), c)         # the stored place seen 7 sectors turned: Q[:, j] = C[:, j + 7] -> shift -7
    assert s == (pl.SECTORS - 7) and d == pytest.approx(0.0, abs=1e-12)
    assert pl.distance(np.zeros_like(c), c) == (math.inf, -1)
    ent, sh, di = pl.match(c, np.stack([c * 0, c, c]), 3)
    assert ent.tolist() == [1, 2, -1] and sh.tolist() == [0, 0, -1]      # ties rank by index; an entry without a valid shift is left out


def test_gpu_match_inputs_are_well_separated(sequence):
    """Input check of test_gpu_places.py: on every query it uses, consecutive entries among the model's T + 1 best differ by more than
    2e-4 in distance, twenty times the bound on the device's f32 error (1e-5): the device cannot rank them otherwise for a legitimate
    reason.  If this fails, change the seed of places_common.MATCH_DRIVE, not the tolerance."""
    kw = dict(MATCH_DRIVE)
    scans, R, t, model = sequence(kw.pop("name"), kw.pop("frames"), **kw)
    desc = np.stack([pl.scan_context(kept(s, model.min_range)) for s in scans])
    db = desc[db_slots()]
    for b in query_slots():
        d = np.sort(pl.shift_distances(desc[b], db).min(axis=1))[:MATCH_T + 1]
        assert np.all(np.diff(d) > 2e-4), (b, d)


def test_border_exception_is_rare_on_the_model_side(sequence):
    """At most 12 of a sweep's 1200 cells may depend on points within 4 ulp of a sector border (2 - 3 such points per 131 k-point sweep are
    expected): the cap the GPU descriptor test allows for, asserted on the sweeps it uses."""
    for name, cols, seed in (("HDL-64", 2048, 31), ("VLP-16", 600, 5)):
        scans, R, t, model = sequence(name, 2, seed=seed, columns=cols)
        for s in scans:
            lo, hi = pl.scan_context_bounds(kept(s, model.min_range))
            assert int((lo != hi).sum()) <= 12, (name, int((lo != hi).sum()))
