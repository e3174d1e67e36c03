"""Register / LDS / scratch budget of the three kernels of the in-place trim, from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of test_graph_propose_budgets.py.  The figures are those of DESIGN §7x."""
import os

import pytest

from graph_trim_cases import CHUNK, constant
from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ("k_trim_cloud_head", "k_trim_cloud_tail", "k_graph_trim")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphtrim_kernels", tmp_path_factory)


def test_the_unit_holds_its_three_kernels_and_nothing_else(unit):
    assert set(unit) == set(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_a_step_lives_in_registers(unit, name):
    """What a step moves is held in vector registers between its loads and its stores: nothing spilled, vector or scalar, no scratch, no
    dynamic stack - a record array that the compiler could not keep in registers would show as scratch or as LDS here."""
    k = unit[name]
    assert k[".max_flat_workgroup_size"] == 256, k
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False), k
    assert k.get(".agpr_count", 0) == 0, k


def test_the_budgets(unit):
    """Head: kTrimHeadUnroll 16-byte values per lane.  Tail: kTrimChunk / 256 = 8 of them, 32 registers.  k_graph_trim: a 240-byte edge is
    60 registers, the composition of an anchored one works beside it; its LDS is the per-wave counts of two tiles and three counters."""
    head, tail, trim = (unit[n] for n in KERNELS)
    waves = 256 // 64
    assert head[".group_segment_fixed_size"] == 0 and tail[".group_segment_fixed_size"] == 0
    assert trim[".group_segment_fixed_size"] == 4 * (2 * waves + 3)
    assert 4 * constant("kTrimHeadUnroll") <= head[".vgpr_count"] <= 32 and occupancy_waves(head) == 8, head
    assert 4 * CHUNK // 256 <= tail[".vgpr_count"] <= 64 and occupancy_waves(tail) == 8, tail
    assert 60 <= trim[".vgpr_count"] <= 128 and trim[".sgpr_count"] <= 80 and occupancy_waves(trim) >= 4, trim
