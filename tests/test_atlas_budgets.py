"""Register / LDS / scratch budgets of the map-spill and atlas kernels, read from the code-object metadata hipcc emits for gfx950 (no GPU needed), in
the manner of test_kernel_budgets.py.  The figures are those of DESIGN §7g."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def atlas_kernels(tmp_path_factory):
    return _kernels("atlas_kernels", tmp_path_factory)


def test_spill_kernels_use_no_scratch(atlas_kernels):
    assert set(atlas_kernels) == {"k_map_spill", "k_spill_count", "k_spill_gather", "k_spill_clear", "k_atlas_window", "k_atlas_merge_segments"}
    for name, k in atlas_kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, k)
        assert k.get(".agpr_count", 0) == 0, (name, k)


def test_spill_kernel_figures_are_those_measured(atlas_kernels):
    """k_map_spill: 74 VGPRs / 91 SGPRs / 1056 bytes of LDS (the 256-int scan buffer and eight ints) - six waves per SIMD by the vector
    file, far more than the one workgroup per sequence that ever runs, and on almost every step the workgroup returns after the shift test.
    k_spill_gather: 48 / 54, no LDS (eight points in flight per thread in copy_points)."""
    k = atlas_kernels["k_map_spill"]
    assert k[".vgpr_count"] <= 74 and k[".sgpr_count"] <= 91 and k[".group_segment_fixed_size"] <= 1056, k
    assert occupancy_waves(k) >= 6, k
    g = atlas_kernels["k_spill_gather"]
    assert g[".vgpr_count"] <= 48 and g[".sgpr_count"] <= 54 and g[".group_segment_fixed_size"] == 0, g
    for name in ("k_spill_count", "k_spill_clear"):
        assert atlas_kernels[name][".vgpr_count"] <= 8 and atlas_kernels[name][".group_segment_fixed_size"] == 0, name


def test_atlas_window_figures_are_those_measured(atlas_kernels):
    """k_atlas_window: 60 VGPRs / 86 SGPRs / 42924 bytes of LDS (the 4852-entry prefix and the 4851 first-point indices the flat copy
    searches, and the 1024-int scan buffer): one workgroup of 1024 threads = four waves per SIMD, which 60 registers allow twice over;
    three such workgroups fit a CU's 160 KiB.  k_atlas_merge_segments: 20 / 22, no LDS."""
    k = atlas_kernels["k_atlas_window"]
    assert k[".vgpr_count"] <= 60 and k[".sgpr_count"] <= 86 and k[".group_segment_fixed_size"] <= 42924, k
    assert occupancy_waves(k) >= 8, k
    m = atlas_kernels["k_atlas_merge_segments"]
    assert m[".vgpr_count"] <= 20 and m[".sgpr_count"] <= 22 and m[".group_segment_fixed_size"] == 0, m
