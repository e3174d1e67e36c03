"""The odometry association kernels (k_associate_pair / k_associate_nearly / k_associate_flagged and the grid builders of
a-loam_amd/csrc/odometry_kernels.hip) on constructed geometry: the scenes of tests/assoc_cases.py, whose path and sensitivity facts
tests/test_assoc_cases.py proves without a GPU, against the CPU oracle.  Library and oracle run with lm_max_iterations = 0, so the recorded
correspondences are those of the pose handed in and nothing but the search is under test.  Bar, as in test_gpu_parity.py: query index lists equal,
records bit for bit equal to the oracle's after the same astype(float32), odom_stats counts equal, last_cloud_order() what the scene says."""
import numpy as np
import pytest

import assoc_cases as ac
from conftest import bits_equal
from test_gpu_parity import _assert_pose_close

pytestmark = pytest.mark.gpu
_ORACLE = {}


def _oracle(O, name, pose_name, lm=0):
    """One oracle run per (scene, pose, solver setting), shared by the tests that need it and left unchanged."""
    key = (name, pose_name, lm)
    if key not in _ORACLE:
        s = ac.scene(name)
        orc = O.Oracle(n_scans=s.n_scans, min_range=0.1, ring_from_field=s.n_scans > 64, **({} if lm is None else {"lm_max_iterations": lm}))
        ac.feed(orc, s, ac.POSES[pose_name])
        orc.odometry_step()
        _ORACLE[key] = (orc.correspondences(), orc.odom_stats(), orc.pose())
    return _ORACLE[key]


def _assert_same_search(s, want, got, stats_o, stats_g, order, ctx):
    eo, plo, eqo, pqo = want
    eg, plg, eqg, pqg = got
    agree = ac.tag_agreement(s, ac.per_query(s, want), ac.per_query(s, got))
    for (cls, tag), (n, bad) in agree.items():
        print(f"{ctx} {cls:6s} {tag:24s} {n - bad:4d} / {n:4d} records agree")
    assert np.array_equal(eqo, eqg) and np.array_equal(pqo, pqg), (ctx, agree)
    assert bits_equal(eo.astype(np.float32), eg) and bits_equal(plo.astype(np.float32), plg), (ctx, agree)
    for key in ("corner_corr", "plane_corr"):
        assert stats_o[key] == stats_g[key], (ctx, key, stats_o, stats_g)
    assert order == s.order, (ctx, order, s.order)


def _gpu(binding, s, batch=1, lm=0):
    return binding.Aloam(n_scans=s.n_scans, min_range=0.1, ring_from_field=s.n_scans > 64, batch=batch, max_points=s.max_points, **({} if lm is None else {"lm_max_iterations": lm}))


@pytest.mark.parametrize("pose_name", sorted(ac.POSES))
@pytest.mark.parametrize("name", ac.SMALL)
def test_scene_matches_oracle(O, binding, name, pose_name):
    """S1 dense block, S2 unequal halves, S3 far 1-NN, S4 ring window, S5 ties and borders, S7 the nearly-sorted and the flagged forms of S1 and S5,
    S8 S1 on the 128-ring instances - at the identity pose and at one with a real rotation and translation."""
    s = ac.scene(name)
    want, stats_o, _ = _oracle(O, name, pose_name)
    gpu = _gpu(binding, s)
    ac.feed(gpu, s, ac.POSES[pose_name])
    gpu.odometry_step()
    _assert_same_search(s, want, gpu.correspondences(), stats_o, gpu.odom_stats(), gpu.last_cloud_order(), (name, pose_name))
    gpu.close()


def test_build_limits_65535_and_65536_points(O, binding):
    """S6: surf_last of exactly 65535 points (the fused build's 16-bit counters, two to a word, one bucket of tens of thousands of entries) and of 65536
    (the per-grid builder), a few dozen queries each."""
    for name in ac.BUILD_LIMITS:
        s = ac.scene(name)
        want, stats_o, _ = _oracle(O, name, "identity")
        gpu = _gpu(binding, s)
        ac.feed(gpu, s, ac.IDENTITY)
        gpu.odometry_step()
        _assert_same_search(s, want, gpu.correspondences(), stats_o, gpu.odom_stats(), gpu.last_cloud_order(), (name,))
        gpu.close()


def test_five_unequal_sequences_in_one_batch(O, binding):
    """S9: S1, S2, an empty scene, S5 and a flagged S7 variant as five sequences of one context: every sequence equals its own oracle run although their
    loads differ by three orders of magnitude."""
    scenes = [ac.scene(n) for n in ac.BATCH]
    poses = ["identity", "rotated", "identity", "rotated", "identity"]
    gpu = binding.Aloam(n_scans=16, min_range=0.1, batch=len(scenes), max_points=max(s.max_points for s in scenes), lm_max_iterations=0)
    for b, (s, p) in enumerate(zip(scenes, poses)):
        ac.feed(gpu, s, ac.POSES[p], seq=b)
    gpu.odometry_step()
    for b, (s, p) in enumerate(zip(scenes, poses)):
        want, stats_o, _ = _oracle(O, s.name, p)
        _assert_same_search(s, want, gpu.correspondences(b), stats_o, gpu.odom_stats(b), gpu.last_cloud_order(b), (b, s.name, p))
    gpu.close()


@pytest.mark.parametrize("name", ["S1", "S2a", "S3", "S4", "S5", "S6-65535", "S1-lowered1", "S8"])
def test_one_scene_of_each_group_with_the_default_solver(O, binding, name):
    """The same inputs through the default solver settings (two outer iterations, four LM iterations each): the first association is the one above, the
    second runs at the pose the first solve left; the pose is held to the bound of test_gpu_parity._assert_pose_close."""
    s = ac.scene(name)
    _, stats_o, pose_o = _oracle(O, name, "rotated", lm=None)
    gpu = _gpu(binding, s, lm=None)
    ac.feed(gpu, s, ac.ROTATED)
    gpu.odometry_step()
    stats_g = gpu.odom_stats()
    print(name, "oracle", stats_o, "device", stats_g)
    _assert_pose_close(pose_o, gpu.pose(), name)
    assert stats_o["corner_corr"][0] == stats_g["corner_corr"][0] and stats_o["plane_corr"][0] == stats_g["plane_corr"][0]
    gpu.close()
