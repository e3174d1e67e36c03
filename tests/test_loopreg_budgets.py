"""Register / LDS / scratch budgets of the loop-registration kernels, from the code-object metadata hipcc emits for gfx950 (no GPU needed),
in the manner of the other test_*_budgets.py.  The figures are those of DESIGN §7n."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, static LDS bytes), pinned at what the build gives; k_loop_grid's bucket table is dynamic LDS
BUDGETS = {"k_loop_gather": (256, 62, 87, 56), "k_loop_grid": (1024, 24, 26, 0), "k_loop_result": (64, 122, 27, 0), "k_loop_export_target": (256, 46, 32, 0)}


@pytest.fixture(scope="module")
def loopreg(tmp_path_factory):
    return _kernels("loopreg_kernels", tmp_path_factory)


def test_the_unit_holds_the_four_kernels_and_nothing_else(loopreg):
    """Association, fit, solve, information and the voxel filter are the mapping step's kernels in their own units: none is instantiated here."""
    assert set(loopreg) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(loopreg, name):
    """Nothing spilled, no scratch - the result kernel included: its 6 x 6 matrices are indexed by compile-time constants only."""
    k = loopreg[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k
