"""pick_sector and the second pass of k_ring_features on the rings of selection_cases.py, in both ring-capacity classes.

tests/test_selection_cases.py proves on the CPU what every ring forces (redo chains, marks carried through sectors shorter than five
points, ties over lanes and over registers of a lane, kills that leave lanes 0 .. 63, every reach at the word borders of the gap bits,
curvatures one ulp around the threshold, registers 8 .. 10 of the <4096> instance) and which mistake it would catch.  Here the rings go
through the device, eight to a sweep, all sweeps of a class in one batched call, and every array is compared bit for bit with a fresh
oracle per sweep: the five clouds, the ring ranges and, over the indices the reference reads, curvature and labels per point.  The
curvatures of all rings but one are exact in f32, so nothing is tolerated.

The context's default ring capacity is 4107, i.e. the <4096> instance (aloam_default_config); the <2048> instance, the one the benchmark
runs, is asked for with max_ring_points = 2059."""
import time

import numpy as np
import pytest
from conftest import bits_equal

import selection_cases as sc

pytestmark = pytest.mark.gpu
FEATURES = ("cloud", "sharp", "less_sharp", "flat", "less_flat")
_REF = {}


def reference(O, long_context):
    """per sweep: input, scene names, and the oracle's clouds, ring ranges, curvature and labels; computed once"""
    if long_context not in _REF:
        out = []
        for x, names in sc.sweeps(long_context):
            orc = O.Oracle(n_scans=sc.RINGS, min_range=0.3, ring_from_field=True)
            fo = orc.scan_register(x)
            curv, lab, _ = orc.per_point()
            out.append((x, names, fo, orc.ring_ranges(), curv, lab))
        _REF[long_context] = out
    return _REF[long_context]


def _compare(gpu, b, ref, ctx):
    x, names, fo, (so, co), curv_o, lab_o = ref
    fg = gpu.features(b)
    for k in FEATURES:
        assert fo[k].shape == fg[k].shape, (ctx, names, k, fo[k].shape, fg[k].shape)
        assert bits_equal(fo[k], fg[k]), (ctx, names, k)
    sg, cg = gpu.ring_ranges(b)
    assert np.array_equal(so, sg) and np.array_equal(co, cg), (ctx, names)
    curv_g, lab_g = gpu.per_point(b)
    for r, (s0, c0) in enumerate(zip(so, co)):
        if c0 >= 17:
            sel = slice(s0 + 5, s0 + c0 - 6)                       # the indices the reference ever reads (scanRegistration.cpp:249-251)
            assert bits_equal(curv_o[sel], curv_g[sel]), (ctx, names[r], "curvature", np.flatnonzero(curv_o[sel].view(np.uint32) != curv_g[sel].view(np.uint32))[:8] + 5)
            assert np.array_equal(lab_o[sel], lab_g[sel]), (ctx, names[r], "labels", [(int(i) + 5, int(lab_o[sel][i]), int(lab_g[sel][i])) for i in np.flatnonzero(lab_o[sel] != lab_g[sel])[:8]])


@pytest.mark.parametrize("max_ring_points", [2059, 4107])
def test_selection_scenes_match_the_oracle_bit_for_bit(O, binding, max_ring_points):
    """all sweeps of the class in one batched call, then once more with the sweeps in reversed order: ring tickets and look-back granules of
    every sequence are reused by rings of other lengths.  The 4107 class ends with a sweep whose rings are a ring too short to be looked at, a
    one-point-sector ring, an empty ring id and a 4107-point ring side by side: zero-count, early-exit and full workgroups in one look-back chain"""
    ref = reference(O, max_ring_points > 2059)
    t0 = time.perf_counter()
    gpu = binding.Aloam(n_scans=sc.RINGS, min_range=0.3, ring_from_field=True, batch=len(ref), max_points=max(len(r[0]) for r in ref) + 64,
                        max_ring_points=max_ring_points)
    for order in (list(range(len(ref))), list(range(len(ref)))[::-1]):
        gpu.scan_register([ref[i][0] for i in order])
        for b, i in enumerate(order):
            _compare(gpu, b, ref[i], (max_ring_points, "sweep", i, "as sequence", b))
    gpu.close()
    print("selection scenes, max_ring_points %d: %d sweeps, %d rings, %d points, %d sharp / %d less sharp / %d flat / %d less flat compared twice, device part %.2f s"
          % (max_ring_points, len(ref), sum(1 for r in ref for k in r[1] if k), sum(len(r[0]) for r in ref), *(sum(len(r[2][k]) for r in ref) for k in FEATURES[1:]), time.perf_counter() - t0))
