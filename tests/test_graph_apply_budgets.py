"""Register / LDS / scratch budget of the graph-apply kernel, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in the
manner of the other test_*_budgets.py.  The figures are those of DESIGN §7m."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, LDS bytes), pinned at what the build gives.  LDS: the scan (1024 ints), the prefix and the source offset
# of every window cube (4852 + 4851 ints), the poses (21 doubles) and the centre.
BUDGETS = {"k_graph_apply": (1024, 64, 86, 43088)}


@pytest.fixture(scope="module")
def graphapply(tmp_path_factory):
    return _kernels("graphapply_kernels", tmp_path_factory)


def test_the_unit_holds_the_one_kernel(graphapply):
    assert set(graphapply) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(graphapply, name):
    """Nothing in scratch, no spilled register, vector or scalar: the result record is built in registers, the class loop reads the
    structs indexed by class through selects, and the four loads in flight are named registers."""
    k = graphapply[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k
