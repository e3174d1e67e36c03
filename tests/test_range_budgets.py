"""Register / LDS / scratch budgets of the two kernels that read a sweep handed in as a range image, from the code-object metadata hipcc emits
for gfx950 (no GPU needed), in the manner of the other test_*_budgets.py.  The figures are those of DESIGN §7i."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def registration(tmp_path_factory):
    return _kernels("registration_kernels", tmp_path_factory)


def test_front_range_keeps_eight_waves_per_simd_without_scratch(registration):
    """k_front_range: 256 threads, 58 VGPRs / 70 SGPRs, nothing spilled, no scratch: eight waves per SIMD by both register files.  It decodes a point
    a second time for its store instead of holding four points across the look-back (k_front holds them: 64 registers with six spilled).  LDS: the
    8 KB rank table and two words of k_front + the six per-row tables of 128 entries = 11 272 bytes; eight workgroups per CU take 88 KB of the 160."""
    k = registration["k_front_range"]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert k[".vgpr_count"] <= 64 and k[".sgpr_count"] <= 80, k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert occupancy_waves(k) == 8, k
    assert k[".group_segment_fixed_size"] == registration["k_front"][".group_segment_fixed_size"] + 6 * 128 * 4, k
    assert 8 * k[".group_segment_fixed_size"] <= 160 * 1024


def test_find_ends_range_uses_no_scratch(registration):
    """k_find_ends_range: one workgroup of 1024 threads per sweep, 40 VGPRs (the limit of such a workgroup is 128), the row tables in LDS."""
    k = registration["k_find_ends_range"]
    assert k[".max_flat_workgroup_size"] == 1024 and k[".vgpr_count"] <= 64, k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert k[".group_segment_fixed_size"] == registration["k_find_ends"][".group_segment_fixed_size"] + 6 * 128 * 4, k


def test_the_float_kernels_keep_their_figures(registration):
    """Sharing the bodies with the range kernels leaves k_find_ends and k_front what they were: 11 / 64 VGPRs, six spilled registers in k_front."""
    assert registration["k_find_ends"][".vgpr_count"] <= 11 and registration["k_find_ends"][".private_segment_fixed_size"] == 0
    k = registration["k_front"]
    assert k[".vgpr_count"] <= 64 and k[".vgpr_spill_count"] <= 6 and k[".private_segment_fixed_size"] <= 28 and k[".group_segment_fixed_size"] == 8200, k
