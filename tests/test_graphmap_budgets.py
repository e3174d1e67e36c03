"""Register / LDS / scratch budgets of the keyframe and graph-map kernels, from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of the other test_*_budgets.py.  The figures are those of DESIGN §7l."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, LDS bytes), pinned at what the build gives
BUDGETS = {"k_keyframe_capture": (256, 46, 46, 0), "k_keyframe_export": (256, 46, 36, 0), "k_graph_map_transform": (256, 94, 38, 0),
           "k_graph_map_group": (256, 26, 25, 0), "k_graph_map_offsets": (1024, 26, 32, 1024 * 8), "k_graph_map_emit": (256, 46, 30, 0)}


@pytest.fixture(scope="module")
def graphmap(tmp_path_factory):
    return _kernels("graphmap_kernels", tmp_path_factory)


def test_the_unit_holds_the_six_kernels_and_nothing_else(graphmap):
    assert set(graphmap) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(graphmap, name):
    """None of the six keeps anything in scratch or spills a register, vector or scalar - the grouping kernel included: a point's place
    comes from one look-up and one integer atomic per distinct cube in the wave, and the structs indexed by class are read through selects."""
    k = graphmap[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k
