"""Register / LDS / scratch budgets of the loop-search kernels, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in the
manner of test_loopreg_budgets.py.  The figures are those of DESIGN §7q.  k_loop_search runs the per-point body of k_score_corrections and
must not need more vector registers than it (128: four waves per SIMD)."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, static LDS bytes), pinned at what the build gives
BUDGETS = {"k_loop_search": (256, 128, 73, 152), "k_loop_search_pick": (256, 61, 34, 4096)}


@pytest.fixture(scope="module")
def loopsearch(tmp_path_factory):
    return _kernels("loopsearch_kernels", tmp_path_factory)


def test_the_unit_holds_the_two_kernels_and_nothing_else(loopsearch):
    assert set(loopsearch) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(loopsearch, name):
    """Nothing spilled, no private segment: the yaw table is read from the kernel arguments by a computed index, not copied to scratch."""
    k = loopsearch[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k


def test_the_search_keeps_the_occupancy_of_the_hypothesis_scoring(loopsearch):
    k = loopsearch["k_loop_search"]
    assert k[".vgpr_count"] <= 128 and occupancy_waves(k) >= 4, k
    assert k[".kernarg_segment_size"] <= 4096, k
