"""Register / LDS / scratch budgets of the graph-record kernels, from the code-object metadata hipcc emits for gfx950 (no GPU needed), in
the manner of the other test_*_budgets.py.  The figures are those of DESIGN §7r."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, LDS bytes), pinned at what the build gives
BUDGETS = {"k_graph_rec_count": (64, 10, 17, 0), "k_graph_rec_offsets": (64, 4, 12, 0), "k_graph_rec_pack": (256, 72, 102, 0),
           "k_graph_rec_check": (256, 18, 48, 4), "k_graph_rec_unpack": (256, 62, 102, 0)}


@pytest.fixture(scope="module")
def graphrecord(tmp_path_factory):
    return _kernels("graphrecord_kernels", tmp_path_factory)


def test_the_unit_holds_the_five_kernels_and_nothing_else(graphrecord):
    assert set(graphrecord) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(graphrecord, name):
    """None of the five keeps anything in scratch or spills a register, vector or scalar: the persistent pack and unpack hold a record's
    layout as ints in 16-byte units, and the only LDS is the check's verdict word."""
    k = graphrecord[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k
