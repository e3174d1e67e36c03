"""Register / LDS / scratch budget of the two kernels of the links measured on the device, from the code-object metadata hipcc emits for
gfx950 (no GPU needed), in the manner of test_graph_propose_budgets.py.  The figures are those of DESIGN §7z."""
import os

import pytest

from graph_propose_cases import HITS, constant
from test_kernel_budgets import HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

GATHER_VGPR_AGPR_SGPR = (62, 0, 86)
PROPOSE_VGPR_AGPR_SGPR = (66, 0, 72)


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    return _kernels("graphlink_kernels", tmp_path_factory)


def test_the_unit_holds_its_two_kernels_and_nothing_else(unit):
    assert set(unit) == {"k_link_gather", "k_link_propose"}


def clean(k):
    return k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0 and not k.get(".uses_dynamic_stack", False)


def test_the_gather_keeps_its_points_in_registers(unit):
    """256 threads, four 16-byte loads in flight per lane.  Nothing spilled, no scratch, no dynamic stack, no AGPRs; LDS = the seven doubles
    of T_k and nothing else (a local array of points that the compiler promotes to LDS would show here as 16 KiB).  Eight waves per SIMD."""
    k = unit["k_link_gather"]
    assert k[".max_flat_workgroup_size"] == 256 and clean(k), k
    assert k[".group_segment_fixed_size"] == 7 * 8, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == GATHER_VGPR_AGPR_SGPR, k
    assert occupancy_waves(k) >= 8, k


def test_the_proposal_keeps_its_state_in_registers_and_its_list_in_lds(unit):
    """One workgroup of 256 threads per query.  Nothing spilled, no scratch, no dynamic stack, no AGPRs.  LDS = the list (a double and an int
    per entry), per wave and per round a (d2, i) pair, the eight doubles of X_j', and the hit counter; rounded up to 8 bytes: 12.3 KiB, so
    160 KiB of LDS holds thirteen lists.  66 VGPRs admit seven waves per SIMD, seven workgroups of four waves per CU."""
    k = unit["k_link_propose"]
    waves, max_k = 256 // 64, constant("kProposeMaxK")
    assert k[".max_flat_workgroup_size"] == 256 and clean(k), k
    lds = 8 * (HITS + waves + max_k + 7) + 4 * (HITS + waves + max_k) + 4         # (+ 7: q and t of X_j')
    assert k[".group_segment_fixed_size"] == (lds + 7) // 8 * 8 and 8 * k[".group_segment_fixed_size"] <= 160 * 1024, k
    assert (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"]) == PROPOSE_VGPR_AGPR_SGPR, k
    assert occupancy_waves(k) >= 7, k
