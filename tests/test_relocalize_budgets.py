"""Register / LDS / scratch budgets of the hypothesis-scoring kernels, read from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of test_kernel_budgets.py."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def relocalize(tmp_path_factory):
    return _kernels("relocalize_kernels", tmp_path_factory)


def test_scoring_kernels_keep_everything_in_registers(relocalize):
    assert set(relocalize) == {"k_score_corrections", "k_score_finalize", "k_apply_corrections"}
    for name, k in relocalize.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, k)


def test_fused_search_and_fit_runs_four_waves_per_simd(relocalize):
    """k_score_corrections holds the search (k_map_search: 63 / 65 VGPRs) and the f64 fits (k_map_fit: 104 / 146 VGPRs) in one register
    allocation and hands the five neighbours over in registers: 128 VGPRs measured, the last count that still admits four waves per SIMD
    (512 / 128).  One register more would halve nothing - it would drop to three waves - so the line is pinned here.  LDS is only the
    workgroup reduction (96 bytes), far below what would limit four workgroups per CU."""
    k = relocalize["k_score_corrections"]
    assert k[".vgpr_count"] <= 128 and k.get(".agpr_count", 0) == 0, k
    assert occupancy_waves(k) >= 4, k
    assert k[".group_segment_fixed_size"] <= 256, k
    f = relocalize["k_score_finalize"]
    assert f[".vgpr_count"] <= 64 and f[".group_segment_fixed_size"] <= 4096, f     # 256 x (int, int, double) of the best-candidate reduction
