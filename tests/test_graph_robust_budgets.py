"""Register / LDS / scratch budget of the robust pose-graph solve's kernels, from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of test_posegraph_budgets.py.  The unit includes posegraph_kernels.hip for its device functions and must not bring
its kernels along.  The figures are those of DESIGN §7s."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphrobust_kernels", tmp_path_factory)


def test_the_unit_holds_its_two_kernels_and_nothing_else(unit):
    assert set(unit) == {"k_graph_robust_incidence", "k_graph_robust"}


def test_the_incidence_kernel_is_k_graph_incidence_again(unit):
    """26 VGPRs, the 256-int scan in LDS, as k_graph_incidence; one scalar register more for the longer argument record."""
    k = unit["k_graph_robust_incidence"]
    assert k[".max_flat_workgroup_size"] == 256 and k[".group_segment_fixed_size"] == 256 * 4, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (26, 0, 33), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k


def test_the_solve_keeps_its_blocks_in_registers(unit):
    """One workgroup of 256 threads per graph, one wave per SIMD, as k_pose_graph.  What lives across the outer loop lies in LDS, which is
    what keeps the scalar registers from spilling: nothing spilled, vector or scalar, no scratch, no dynamic stack.  LDS = the 4 doubles of
    block_sum, the factorisation's flag, the two option records (40 and 32 bytes), the outer loop's state (64) and the result (128)."""
    k = unit["k_graph_robust"]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == VGPR_AGPR_SGPR, k
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k
    assert k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 4 * 8 + 8 + 40 + 32 + 64 + 128, k


VGPR_AGPR_SGPR = (282, 26, 102)
