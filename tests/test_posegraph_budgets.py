"""Register / LDS / scratch budgets of the pose-graph kernels, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in the
manner of the other test_*_budgets.py.  The figures are those of DESIGN §7k."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def posegraph(tmp_path_factory):
    return _kernels("posegraph_kernels", tmp_path_factory)


def _no_scratch(k):
    return k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0


def test_the_unit_holds_the_three_kernels_and_nothing_else(posegraph):
    assert set(posegraph) == {"k_graph_add_nodes", "k_graph_incidence", "k_pose_graph"}


def test_store_and_incidence_kernels_are_small(posegraph):
    """k_graph_add_nodes: 72 VGPRs / 16 SGPRs, no LDS; k_graph_incidence: 26 / 32 with the 256-int scan in LDS.  Pinned at what the build gives."""
    k = posegraph["k_graph_add_nodes"]
    assert k[".max_flat_workgroup_size"] == 64 and k[".group_segment_fixed_size"] == 0, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (72, 0, 16), k
    assert _no_scratch(k) and k[".sgpr_spill_count"] == 0, k
    k = posegraph["k_graph_incidence"]
    assert k[".max_flat_workgroup_size"] == 256 and k[".group_segment_fixed_size"] == 256 * 4, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (26, 0, 32), k
    assert _no_scratch(k) and k[".sgpr_spill_count"] == 0, k


def test_the_solve_keeps_its_blocks_in_registers(posegraph):
    """One workgroup of 256 threads per graph, one wave per SIMD: the 512 registers of a lane are there to be used.  The build gives 286 (256
    VGPRs and 30 AGPRs; the node pass holds a 6 x 6 Jacobian, the upper triangle of its block sum and the information matrix) and 98 SGPRs:
    nothing spilled, vector or scalar, no scratch, no dynamic stack (the one call, pg_exp_half, passes everything in registers).  LDS = the
    4 doubles of block_sum, the factorisation's flag and the options (40 bytes)."""
    k = posegraph["k_pose_graph"]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (286, 30, 98), k
    assert _no_scratch(k) and not k.get(".uses_dynamic_stack", False), k
    assert k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 4 * 8 + 8 + 40, k
