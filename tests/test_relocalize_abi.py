"""Scoring and applying map-pose hypotheses, host side (no GPU): the two entry points and their records in the header, the binding and the
library; what can be refused without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return " ".join(txt.split())


def test_header_declares_both_calls_and_records():
    d = _declarations()
    assert ("int aloam_score_map_corrections(aloam_ctx* ctx, const int* seqs, int n, const aloam_map_correction* cand, int K, "
            "aloam_map_score* scores , int* best );") in d
    assert "int aloam_apply_map_corrections(aloam_ctx* ctx, const int* seqs, int n, const aloam_map_correction* cand, int K, const int* choice );" in d
    assert "typedef struct aloam_map_correction { double q_wmap_wodom[4], t_wmap_wodom[3], pad; } aloam_map_correction;" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                          # records are unchanged


def test_header_documents_the_contract():
    txt = open(HEADER).read()
    block = txt[txt.index("aloam_score_map_corrections:"):txt.index("typedef struct aloam_map_correction")]
    for word in ("ALOAM_MAP_CORNER_STACK", "aloam_get_map_info", "aloam_set_map_frame", "another 50 m cube", "ALOAM_E_STATE", "ALOAM_E_ARG",
                 "aloam_reset_sequences", "aloam_load_sequences", "aloam_set_map", "aloam_export_clouds", "aloam_synchronize", "pageable",
                 "ties: the lower cost; ties: the lower index", "no floating-point atomics", ":142-146", ":554"):
        assert word in block, word


def test_record_offsets_and_the_candidates_bytes(binding):
    """(test_abi_records.py holds both records against the C compiler's layout; two offsets are written out here once more.)"""
    assert C.sizeof(binding.AloamMapCorrection) == 64 and C.sizeof(binding.AloamMapScore) == 32
    assert binding.MAP_CORRECTION_DTYPE.itemsize == 64 and binding.MAP_SCORE_DTYPE.itemsize == 32
    assert binding.MAP_CORRECTION_DTYPE.fields["t_wmap_wodom"][1] == 32 and binding.MAP_SCORE_DTYPE.fields["cost"][1] == 16
    c = binding.map_corrections([[0, 0, 0, 1], [0, 0, 1, 0]], [[1, 2, 3], [4, 5, 6]])
    assert c.shape == (2,) and c.tobytes() == np.array([0, 0, 0, 1, 1, 2, 3, 0, 0, 0, 1, 0, 4, 5, 6, 0], np.float64).tobytes()


def test_binding_and_library_export_both_calls(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in ("aloam_score_map_corrections", "aloam_apply_map_corrections"):
        assert name in syms and hasattr(binding.lib(), name), name
    assert "aloam_map_score" not in syms and "aloam_map_correction" not in syms     # records, not functions
    for m in ("score_map_corrections", "score_map_corrections_into", "apply_map_corrections", "apply_map_corrections_from"):
        assert callable(getattr(binding.Aloam, m, None)), m
    names = [binding.lib().aloam_profile_kernel_name(k).decode() for k in range(binding.lib().aloam_profile_kernel_count())]
    assert names[-2:] == ["score_corrections", "apply_corrections"] and names.index("load_sequences") == len(names) - 3   # appended


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids = (C.c_int * 1)(0)
    cand = binding.map_corrections([[0, 0, 0, 1]], [[0, 0, 0]])
    assert L.aloam_score_map_corrections(None, ids, 1, C.c_void_p(cand.ctypes.data), 1, None, None) == binding.E_ARG
    assert L.aloam_apply_map_corrections(None, ids, 1, C.c_void_p(cand.ctypes.data), 1, None) == binding.E_ARG


def test_kitti_runner_has_the_relocalize_option():
    import sys
    tool = os.path.join(ROOT, "tools", "run_kitti.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--relocalize RADIUS_M YAW_DEG" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, "--selftest", "--relocalize", "3.5", "12.5"], capture_output=True, text=True)
    assert r.returncode != 0 and "--relocalize needs --prior-map" in r.stderr
