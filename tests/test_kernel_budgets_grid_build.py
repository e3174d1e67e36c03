"""The persistent "last"-form grid build (k_build_grids_fused_last, beside the scan registration) keeps the budget of k_build_grids_fused: it is
the same body in a loop, and four of its waves share a SIMD with the registration's.  "Does not spill" is what test_kernel_budgets.py means by it: no
vector register spilled and nothing in scratch.  (Around the loop the compiler keeps 29 loop-invariant scalars in lanes of one vector register, as it does
in k_build_grids_fused_next: one v_readlane where a scalar load stood, inside the 64 registers.)"""
import os

import pytest
from test_kernel_budgets import HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_persistent_last_build_keeps_the_fused_budget(tmp_path_factory):
    odometry = _kernels("odometry_kernels", tmp_path_factory)
    k = odometry["k_build_grids_fused_last"]
    assert k[".vgpr_count"] <= 64, k
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k
    for name in ("k_build_grids_fused", "k_build_grids_fused_next"):
        assert name in odometry, name
