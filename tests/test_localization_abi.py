"""Localization against a frozen prior map, host side (no GPU): the entry point aloam_set_map_frozen in the header and the binding, and the
prior-map options of the KITTI runner."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return " ".join(txt.split())


def test_header_declares_set_map_frozen():
    assert "int aloam_set_map_frozen(aloam_ctx* ctx, const int* frozen);" in _declarations()


def test_header_documents_the_contract():
    txt = open(HEADER).read()
    block = txt[txt.index("aloam_set_map_frozen:"):txt.index("int aloam_set_map_frozen(")]
    for word in ("aloam_set_map_frame", "aloam_get_map_info", "ALOAM_E_STATE", "aloam_mapping_enable", "aloam_set_active",
                 "aloam_reset_sequences", "aloam_load_sequences", "ALOAM_SEQ_RECORD_VERSION", ":737-783", ":788-801"):
        assert word in block, word
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in txt                        # records are unchanged


def test_binding_declares_and_wraps_set_map_frozen(binding):
    assert "aloam_set_map_frozen" in binding.declared_symbols()
    assert callable(getattr(binding.Aloam, "set_map_frozen", None))


def test_library_exports_set_map_frozen(binding):
    binding.build()
    assert hasattr(binding.lib(), "aloam_set_map_frozen")


def test_kitti_runner_has_prior_map_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for opt in ("--save-map", "--prior-map", "--initial-pose"):
        assert opt in r.stdout, opt


def test_kitti_runner_refuses_prior_map_with_several_sequences(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_kitti.py"), "--seqs", "00", "01", "--prior-map", str(tmp_path / "m.npz")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--prior-map" in r.stderr


def test_mapping_node_builds_and_links_with_the_hip_runtime(binding, tmp_path):
    """The node's `save_map` path (pinned memory through the HIP runtime API) compiles with a plain C++ compiler given the ROCm headers and
    links against libamdhip64; the tests' own node build (tests/host/Makefile) has no ROCm include path and compiles the other branch."""
    binding.build()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    host = os.path.join(ROOT, "a-loam_amd", "host")
    flags = ["-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "oracle", "ref_shim", "include"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
             "-I" + os.path.join(ROOT, "include"), "-I" + host, "-I" + os.path.join(rocm, "include")]
    obj, exe = str(tmp_path / "node.o"), str(tmp_path / "node_laser_mapping")
    r = subprocess.run(["g++", *flags, "-Dmain=node_main", "-c", os.path.join(host, "laser_mapping_node.cpp"), "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout
    assert "hipHostMalloc" in syms and "aloam_set_map_frozen" in syms and "aloam_load_sequences" in syms
    lib = os.path.join(ROOT, "a-loam_amd", "lib")
    r = subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "host", "drive_laser_mapping.cpp"), obj, "-o", exe, "-L" + lib, "-laloam_mi355x",
                        "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
