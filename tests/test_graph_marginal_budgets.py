"""Register / LDS / scratch budget of the pose-graph marginals' kernel, from the code-object metadata hipcc emits for gfx950 (no GPU needed),
in the manner of test_posegraph_budgets.py.  The unit includes posegraph_kernels.hip for its device functions and must not bring its kernels
along.  The figures are those of DESIGN §7p."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphmarginal_kernels", tmp_path_factory)


def test_the_unit_holds_the_one_kernel_and_nothing_else(unit):
    assert set(unit) == {"k_graph_marginals"}


def test_the_kernel_keeps_its_blocks_in_registers(unit):
    """One workgroup of 256 threads per request, one wave per SIMD, as k_pose_graph: the build gives 250 VGPRs, no AGPRs and 71 SGPRs, nothing
    spilled, no scratch, no dynamic stack.  LDS = the 4 doubles of block_sum, the 256-int scan of the incidence build, the factorisation's
    flag and the candidate (its edge, r, J_i, J_j, Sigma_r and the one thread's four 6 x 6 matrices: 2304 bytes)."""
    k = unit["k_graph_marginals"]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (250, 0, 71), k
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k
    assert k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 4 * 8 + 256 * 4 + 8 + (240 + 8 * (6 + 36 + 36 + 36 + 4 * 36)), k
