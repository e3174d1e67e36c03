"""Pose information, host side (no GPU): the two entry points and the record in the header, the binding and the library; what can be
refused without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return " ".join(txt.split())


def test_header_declares_the_calls_and_the_record():
    d = _declarations()
    assert "int aloam_export_pose_information(aloam_ctx* ctx, int which, const int* seqs, int n, aloam_pose_information* dst );" in d
    assert ("int aloam_get_map_factors(aloam_ctx* ctx, int seq, double* lines, int cap_lines, int* n_lines, double* planes, int cap_planes, "
            "int* n_planes);") in d
    assert "enum { ALOAM_INFO_ODOMETRY = 0, ALOAM_INFO_MAPPING = 1 };" in d
    assert "enum { ALOAM_INFO_OK = 0, ALOAM_INFO_NONE = 1, ALOAM_INFO_NO_FACTORS = 2, ALOAM_INFO_SINGULAR = 3 };" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                          # records are unchanged


def test_header_documents_the_definition():
    txt = open(HEADER).read()
    block = txt[txt.index("---- pose information"):txt.index("typedef struct aloam_pose_information")]
    for word in ("last outer iteration", "second iteration", "FAILURE", "HuberLoss(0.1)", "No Jacobi", "EigenQuaternionParameterization::Plus",
                 "LEFT", "theta = 2 d", "diag(1/2, 1/2, 1/2, 1, 1, 1)", "last sweep's frame", "map", "largest magnitude", "lowest index",
                 "H_tt - H_tr H_rr^-1 H_rt", "H_rr - H_rt H_tt^-1 H_tr", "sigma^2 = 2 cost / (rows - 6)", "ALOAM_INFO_NONE", "ALOAM_INFO_NO_FACTORS",
                 "ALOAM_INFO_SINGULAR", "aloam_reset_sequences", "aloam_load_sequences", "aloam_set_state", "aloam_set_features", "aloam_set_last",
                 "aloam_set_map", "aloam_set_map_frame", "aloam_apply_map_corrections", "pageable", "ALOAM_E_ARG", "ALOAM_E_STATE",
                 "do not depend on n", "sat out the last step"):
        assert word in block, word


def test_binding_and_library_export_the_calls(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in ("aloam_export_pose_information", "aloam_get_map_factors"):
        assert name in syms and hasattr(binding.lib(), name), name
    assert "aloam_pose_information" not in syms                               # a record, not a function
    for m in ("export_pose_information", "export_pose_information_into", "map_factors"):
        assert callable(getattr(binding.Aloam, m, None)), m
    assert (binding.INFO_ODOMETRY, binding.INFO_MAPPING) == (0, 1)
    assert (binding.INFO_OK, binding.INFO_NONE, binding.INFO_NO_FACTORS, binding.INFO_SINGULAR) == (0, 1, 2, 3)
    names = [binding.lib().aloam_profile_kernel_name(k).decode() for k in range(binding.lib().aloam_profile_kernel_count())]
    assert "pose_information" in names and names.index("pose_information") == names.index("export_clouds") + 1


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids = (C.c_int * 1)(0)
    n = C.c_int(0)
    assert L.aloam_export_pose_information(None, 0, ids, 1, None) == binding.E_ARG
    assert L.aloam_get_map_factors(None, 0, None, 0, C.byref(n), None, 0, C.byref(n)) == binding.E_ARG


def test_host_state_is_in_seqhost_and_not_in_a_record():
    """The two "information valid" flags are SeqHost fields changed by the events of capi_seq.hip and by nothing else."""
    csrc = os.path.join(ROOT, "a-loam_amd", "csrc")
    internal = open(os.path.join(csrc, "capi_internal.hpp")).read()
    seqhost = internal[internal.index("struct SeqHost {"):internal.index("struct aloam_ctx {")]
    assert "info_odom" in seqhost and "info_map" in seqhost
    for f in os.listdir(csrc):
        if f.endswith(".hip") and f != "capi_seq.hip":
            txt = open(os.path.join(csrc, f)).read()
            assert not re.search(r"\binfo_(odom|map)\s*=[^=]", txt), f                # read elsewhere, assigned only by the events


def test_tools_have_the_option():
    tool = os.path.join(ROOT, "tools", "run_kitti.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pose-information" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pose_information_rate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--repeats" in r.stdout, r.stdout + r.stderr
