"""Register / LDS / scratch budgets of the pose-information kernels, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in
the manner of the other test_*_budgets.py.  The figures are those of DESIGN §7j."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def information(tmp_path_factory):
    return _kernels("information_kernels", tmp_path_factory)


def _nothing_spilled(k):
    return k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0


def test_the_unit_holds_the_three_kernels_and_nothing_else(information):
    assert set(information) == {"k_pose_information_odom<false>", "k_pose_information_odom<true>", "k_pose_information_map"}


def test_odometry_kernels_keep_everything_in_registers(information):
    """128 threads as k_solve (the evaluation strides by that count).  Measured: 162 VGPRs / 64 SGPRs without distortion, 184 / 106 with it -
    the 6 x 6 matrix, its eigenvectors and the 28 sums, none of the Levenberg-Marquardt state (k_solve: 432 / 458).  Nothing spilled, no
    scratch; LDS = the 2 x 28 doubles of the block reduction."""
    for name, vgprs in (("k_pose_information_odom<false>", 176), ("k_pose_information_odom<true>", 200)):
        k = information[name]
        assert k[".max_flat_workgroup_size"] == 128, k
        assert k[".vgpr_count"] <= vgprs and k.get(".agpr_count", 0) == 0, k
        assert _nothing_spilled(k), k
        assert k[".group_segment_fixed_size"] == 2 * 28 * 8, k


def test_mapping_kernel_keeps_everything_in_registers(information):
    """256 threads as k_map_solve.  Measured: 250 VGPRs / 66 SGPRs (k_map_solve: 506), nothing spilled, no scratch; static LDS = the 4 x 28
    doubles of the block reduction (the tile prefixes are dynamic LDS, sized per launch as for k_map_solve)."""
    k = information["k_pose_information_map"]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert k[".vgpr_count"] <= 256 and k.get(".agpr_count", 0) == 0, k
    assert _nothing_spilled(k), k
    assert k[".group_segment_fixed_size"] == 4 * 28 * 8, k
