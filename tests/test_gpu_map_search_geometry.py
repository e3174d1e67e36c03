"""The scan-to-map search and fit (k_mapgrid_build, k_map_search, k_map_fit of a-loam_amd/csrc/mapping_kernels.hip, map_search_device.hpp) on the
constructed frame of tests/map_search_cases.py, whose path, sensitivity and margin facts tests/test_map_search_cases.py proves without a GPU.  The
oracle's cubes go in through set_map / set_map_frame, the constructed stack through mapping_step_inputs, at lm_max_iterations = 0.  Compared: the
map_info counts with Oracle.mapping_step on the same input, and map_factors record by record with the numpy model - cp bit for bit, a line as the
unordered pair {a, b}, plane (n, d) and line ends within 100 times the spread measured on the CPU between the oracle's Eigen stand-ins and numpy."""
import numpy as np
import pytest

import map_search_cases as mc

pytestmark = pytest.mark.gpu


def test_constructed_map_frame_matches_oracle_and_model(O, binding):
    ev = mc.evaluated()
    s = ev.scene
    tol = mc.device_tolerance()
    gpu = binding.Aloam(n_scans=16, min_range=0.3, max_points=4096, lm_max_iterations=0)
    gpu.mapping_enable(mc.LEAF, mc.LEAF, pool_points=mc.POOL_POINTS)
    assert gpu.map_pool_info()["pool_points"] == mc.POOL_POINTS and mc.table_size(mc.POOL_POINTS) == s.H      # the table size the bucket facts were stated for
    for cls in (0, 1):
        gpu.set_map(ev.cubes[cls], cls)
    gpu.set_map_frame((ev.info["cenW"], ev.info["cenH"], ev.info["cenD"]), [0, 0, 0, 1.0], [0, 0, 0.0], len(s.map_frames))
    gpu.mapping_step_inputs([0, 0, 0, 1.0], [0, 0, 0.0], s.stack[0], s.stack[1], s.stack[1][:4])
    gpu.synchronize()
    info = gpu.map_info()
    lines, planes = gpu.map_factors()
    assert gpu.map_pool_info()["growths"] == 0
    gpu.close()
    agree, worst, problems = mc.compare_factors(ev, lines, planes, tol)
    for (cls, tag), (n, bad) in agree.items():
        print(f"{cls:6s} {tag:40s} {n - bad:3d} / {n:3d} queries agree")
    print(f"largest deviation of a line end / plane component from the model: {worst:.3e} (tolerance {tol:.3e} = 100 x the measured spread {mc.measured_spread():.3e})")
    for key in mc.INFO_KEYS:
        assert info[key] == ev.info[key], (key, info, ev.info)
    assert not problems, problems
    assert (len(lines), len(planes)) == (len(ev.model[0]), len(ev.model[1])) == (ev.info["corner_num1"], ev.info["surf_num1"])
