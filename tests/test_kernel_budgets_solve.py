"""Register and LDS budgets of the odometry solve, from the code-object metadata hipcc emits for gfx950 and from the header's own size computation
(no GPU needed), in the manner of the other test_*_budgets.py.

k_solve runs one wave per SIMD on purpose, so two of its two-wave workgroups share a CU and its 160 KiB of LDS: the factor records a solve keeps there
(odometry_solve_device.hpp, solve_stage()) plus the block reduction's static array may take at most 80 KiB, or half the chip's solves wait for LDS.  The
records fetched ahead live in registers: the kernels must stay within the 512 of a lane with nothing spilled to scratch."""
import os
import subprocess

import pytest

from test_kernel_budgets import CSRC, HIPCC, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

PROBE = r"""
#include <cstdio>
#include "odometry_solve_device.hpp"
int main() {
  for (int distort = 0; distort < 2; ++distort)
    for (int R : {16, 32, 64, 128}) {
      constexpr int kStatic = aloam::kSolveStaticLds;
      const aloam::SolveStage s = aloam::solve_stage(R, distort != 0);
      std::printf("%d %d %d %d %d %d %d %d\n", R, distort, s.plane_slots, s.edge_slots, s.bytes, kStatic, aloam::solve_slots(R * aloam::kFlatPerRing), aloam::solve_slots(R * aloam::kSharpPerRing));
    }
  static_assert(aloam::solve_stage(64, false).bytes + aloam::kSolveStaticLds <= 80 * 1024, "HDL-64: two workgroups per CU");
  return 0;
}
"""


@pytest.fixture(scope="module")
def odometry(tmp_path_factory):
    return _kernels("odometry_kernels", tmp_path_factory)


@pytest.fixture(scope="module")
def information(tmp_path_factory):
    return _kernels("information_kernels", tmp_path_factory)


@pytest.fixture(scope="module")
def stages(tmp_path_factory):
    """{(R, distortion): (plane slots kept, edge slots kept, dynamic LDS bytes, static LDS bytes, plane slots, edge slots)} as the HOST computes them:
    the header's constexpr helper compiled into a host-only program (no device code, no HIP call)."""
    d = tmp_path_factory.mktemp("solve_stage")
    src, exe = d / "probe.hip", d / "probe"
    src.write_text(PROBE)
    r = subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    return {(r[0], bool(r[1])): r[2:] for r in rows}


def test_solve_kernels_fit_the_register_file(odometry, information):
    """Measured: k_solve<false> 440 registers (256 + 184 accumulation), k_solve<true> 474, with two records fetched ahead; k_pose_information_odom 162 /
    190 with one and none (its own budgets: tests/test_information_budgets.py)."""
    for k in (odometry["k_solve<false>"], odometry["k_solve<true>"], information["k_pose_information_odom<false>"], information["k_pose_information_odom<true>"]):
        assert k[".vgpr_count"] <= 512 and k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k


def test_static_lds_is_what_the_header_says(odometry, stages):
    for name in ("k_solve<false>", "k_solve<true>"):
        assert odometry[name][".group_segment_fixed_size"] == stages[(64, False)][3] == 2 * 28 * 8, odometry[name]


def test_hdl64_leaves_room_for_two_workgroups_per_cu(stages):
    kept_p, kept_e, dynamic, static, slots_p, slots_e = stages[(64, False)]
    assert static + dynamic <= 81920, stages[(64, False)]
    assert (kept_p, kept_e, slots_p, slots_e) == (12, 1, 12, 6) and dynamic == 1536 * 48 + 128 * 44       # every plane slot, and the edge slot that is left


@pytest.mark.parametrize("R", [16, 32, 64, 128])
@pytest.mark.parametrize("distortion", [False, True])
def test_every_sensor_stays_inside_half_a_cu(stages, R, distortion):
    kept_p, kept_e, dynamic, static, slots_p, slots_e = stages[(R, distortion)]
    per_p, per_e = (48 + 4 * distortion) * 128, (44 + 4 * distortion) * 128
    assert 0 <= kept_p <= slots_p == -(-R * 24 // 128) and 0 <= kept_e <= slots_e == -(-R * 12 // 128)
    assert dynamic == kept_p * per_p + kept_e * per_e and static + dynamic <= 81920
    # nothing is left out that would have fitted: planes first, then edges
    assert kept_p == slots_p or static + (kept_p + 1) * per_p > 81920
    assert kept_e == slots_e or static + dynamic + per_e > 81920
    if R <= 32:
        assert (kept_p, kept_e) == (slots_p, slots_e)          # 16 and 32 rings keep every record
