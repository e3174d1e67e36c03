"""Register / LDS / scratch budgets of the two kernels of the map of joined sequences, from the code-object metadata hipcc emits for gfx950
(no GPU needed), in the manner of tests/test_graphmap_budgets.py.  The figures are those of DESIGN §7za."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
# kernel: (workgroup, VGPRs, SGPRs, LDS bytes), pinned at what the build gives; neither stages the pose in LDS
BUDGETS = {"k_graph_map_transform_parts": (256, 74, 69, 0), "k_graph_map_group_parts": (256, 26, 25, 0)}


@pytest.fixture(scope="module")
def joint(tmp_path_factory):
    return _kernels("graphmapjoint_kernels", tmp_path_factory)


@pytest.fixture(scope="module")
def graphmap(tmp_path_factory):
    return _kernels("graphmap_kernels", tmp_path_factory)


def test_the_unit_holds_the_two_kernels_and_nothing_else(joint):
    assert set(joint) == set(BUDGETS)


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_registers_and_lds_are_what_the_build_gives(joint, name):
    """Neither keeps anything in scratch or spills a register, vector or scalar: the class-indexed structs are read through selects, and the
    frame is loaded where the node changes, not held across the loop."""
    k = joint[name]
    wg, vgpr, sgpr, lds = BUDGETS[name]
    assert k[".max_flat_workgroup_size"] == wg and k[".group_segment_fixed_size"] == lds, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == (vgpr, 0, sgpr), k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    assert not k.get(".uses_dynamic_stack", False), k


def test_the_transform_over_parts_keeps_the_occupancy_of_the_transform_over_requests(joint, graphmap):
    """The same work plus one composed pose per node: the wave's part and piece sit in scalar registers, so the kernel needs no more vector
    registers than k_graph_map_transform and as many waves fit a SIMD."""
    assert occupancy_waves(joint["k_graph_map_transform_parts"]) >= occupancy_waves(graphmap["k_graph_map_transform"])
    assert occupancy_waves(joint["k_graph_map_group_parts"]) >= occupancy_waves(graphmap["k_graph_map_group"])
