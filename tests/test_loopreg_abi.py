"""Loop edges measured on the device, host side (no GPU): the records and entry points in the header, the binding and the library; the
profiling slot; what can be refused without a device."""
import ctypes as C
import os
import re

import pytest

from test_posegraph_abi import HEADER, ROOT

CALLS = ("aloam_graph_loops_enable", "aloam_graph_loop_default_options", "aloam_graph_register_loops", "aloam_graph_loop_export_target")


def test_calls_are_declared_exported_and_bound(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("graph_loops_enable", "graph_register_loops", "graph_register_loops_into", "graph_loop_target", "graph_loop_requests", "graph_loop_options"):
        assert callable(getattr(binding.Aloam, m, None)), m
    d = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert ("enum { ALOAM_LOOP_OK = 0, ALOAM_LOOP_NO_CLOUDS = 1, ALOAM_LOOP_TARGET_TOO_SMALL = 2, ALOAM_LOOP_TOO_LARGE = 3, "
            "ALOAM_LOOP_SOLVE_FAILED = 4 };") in d
    assert (binding.LOOP_OK, binding.LOOP_NO_CLOUDS, binding.LOOP_TARGET_TOO_SMALL, binding.LOOP_TOO_LARGE, binding.LOOP_SOLVE_FAILED) == (0, 1, 2, 3, 4)
    assert d.index("aloam_graph_apply(") < d.index("aloam_graph_loops_enable(") < d.index("aloam_get_ring_ranges(")   # behind "a solved graph carried into the live state"
    assert d.index("aloam_get_map_factors(") < d.index("aloam_graph_loop_export_target(") < d.index("aloam_profile_enable(")   # with the intermediate arrays
    assert C.sizeof(binding.AloamGraphLoopOptions) == 8


def test_the_default_options_are_the_reference_mapping_values(binding):
    o = binding.AloamGraphLoopOptions()
    binding.lib().aloam_graph_loop_default_options(C.byref(o))
    assert (o.outer_iterations, o.lm_max_iterations) == (2, 4)
    binding.lib().aloam_graph_loop_default_options(None)


def test_header_states_the_definition():
    txt = open(HEADER).read()
    block = txt[txt.index("---- loop edges measured on the device"):txt.index("typedef struct aloam_graph_loop_request")]
    block = " ".join(block.replace("\n *", " ").split())                       # the comment's line breaks are not part of what it says
    for word in ("does not synchronise the host", "launches exactly what it launched before", "conj(q_i) q_k", "node order, then point order", "input-order sum",
                 "frame of node i", "more than 10 points", "more than 50", "REQUEST's options", "LEFT tangent", "on the RIGHT", "T^T info_left T",
                 "blockdiag(R_Z, R_Z)", "ALOAM_GRAPH_EDGE_ROBUST", "caller's decision", "nothing stays allocated behind a refusal", "unit to 1e-6",
                 "pinned staging ring", "rounds over the same scratch", "do not depend on n", "decided on the device", "Z is the guess"):
        assert word in block, word


def test_profiling_slot_follows_graph_map(binding):
    L = binding.lib()
    names = [L.aloam_profile_kernel_name(k).decode() for k in range(L.aloam_profile_kernel_count())]
    assert names.index("loop_register") == names.index("graph_map") + 1 == names.index("save_sequences") - 1
    assert names[-3] == "load_sequences" and names[-2:] == ["score_corrections", "apply_corrections"]    # what the older ABI tests pin


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    cnt = C.c_int(0)
    assert L.aloam_graph_loops_enable(None, 1, 16, 16) == binding.E_ARG
    assert L.aloam_graph_register_loops(None, None, 0, None, None) == binding.E_ARG
    assert L.aloam_graph_loop_export_target(None, 0, 0, None, 0, C.byref(cnt)) == binding.E_ARG


def test_the_makefile_builds_the_new_units_and_the_old_kernels_are_left_alone():
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "loopreg_kernels.hip" in src and "capi_loopreg.hip" in src and "loopreg_kernels.hpp" in hdr
    # the feature's kernels live in their own unit and call the mapping step's launchers; no other kernel file knows of it
    for f in os.listdir(csrc):
        if f.endswith("_kernels.hip") and f != "loopreg_kernels.hip":
            assert "loopreg" not in open(os.path.join(csrc, f)).read(), f
    host = open(os.path.join(csrc, "capi_loopreg.hip")).read()
    for call in ("launch_map_associate(", "launch_map_solve(", "launch_pose_information_map(", "launch_voxel_filter("):
        assert call in host, call
    assert "hipStreamSynchronize" not in host[host.index("int aloam_graph_register_loops"):host.index("int aloam_graph_loop_export_target")]


@pytest.mark.parametrize("tool,option", [("loop_register_rate.py", "--shapes"), ("loop_closure_drive.py", "--device-loops")])
def test_the_tools_answer_help(tool, option):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and option in r.stdout, r.stdout + r.stderr
