"""Register / LDS / scratch budget of the loop proposal's kernel, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in the
manner of test_graph_robust_budgets.py.  The figures are those of DESIGN §7v."""
import os

import pytest

from graph_propose_cases import HITS, constant
from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPR_AGPR_SGPR = (64, 0, 85)


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphpropose_kernels", tmp_path_factory)


def test_the_unit_holds_its_kernel_and_nothing_else(unit):
    assert set(unit) == {"k_graph_propose"}


def test_the_kernel_keeps_its_state_in_registers_and_its_list_in_lds(unit):
    """One workgroup of 256 threads per query.  Nothing spilled, vector or scalar, no scratch, no dynamic stack.  LDS = the list (a double and
    an int per entry), per wave and per round a (d2, i) pair, and the hit counter; rounded up to 8 bytes.  With kProposeHits = 1024 that is
    12.2 KiB: the register file admits eight workgroups of four waves per CU, and 160 KiB of LDS holds thirteen such lists."""
    k = unit["k_graph_propose"]
    waves, max_k = 256 // 64, constant("kProposeMaxK")
    assert k[".max_flat_workgroup_size"] == 256, k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k
    lds = 8 * (HITS + waves + max_k) + 4 * (HITS + waves + max_k) + 4
    assert k[".group_segment_fixed_size"] == (lds + 7) // 8 * 8 and 8 * k[".group_segment_fixed_size"] <= 160 * 1024, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == VGPR_AGPR_SGPR, k
    assert occupancy_waves(k) >= 8, k
