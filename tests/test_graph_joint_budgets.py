"""Register / LDS / scratch budget of the two kernels of the joined pose graphs, from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of test_graph_trim_budgets.py.  The figures are those of DESIGN §7y."""
import os

import pytest

from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ("k_joint_gather", "k_joint_scatter")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphjoint_kernels", tmp_path_factory)


def test_the_unit_holds_its_two_kernels_and_nothing_else(unit):
    assert set(unit) == set(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_a_record_lives_in_registers(unit, name):
    """A record is held in vector registers between its loads and its stores: nothing spilled, vector or scalar, no scratch, no dynamic
    stack, no AGPRs - a record array that the compiler could not keep in registers would show as scratch here."""
    k = unit[name]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k
    assert k.get(".agpr_count", 0) == 0, k


def test_the_budgets(unit):
    """Gather: a 240-byte edge is 60 registers, the composition with A (seven doubles, uniform) works beside it: 96 VGPRs, 48 SGPRs, five
    waves per SIMD.  Scatter: a 128-byte node is 32 registers: 38 VGPRs, 29 SGPRs, eight waves.  Neither uses LDS."""
    gather, scatter = (unit[n] for n in KERNELS)
    assert gather[".group_segment_fixed_size"] == 0 and scatter[".group_segment_fixed_size"] == 0
    assert 60 <= gather[".vgpr_count"] <= 96 and gather[".sgpr_count"] <= 48 and occupancy_waves(gather) >= 5, gather
    assert 32 <= scatter[".vgpr_count"] <= 40 and scatter[".sgpr_count"] <= 32 and occupancy_waves(scatter) == 8, scatter
