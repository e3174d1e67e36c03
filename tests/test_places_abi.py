"""Place recognition, host side (no GPU): the entry points and the two records in the header, the binding and the library; what can be
refused without a device; the runner's options; and that no profiling slot was added."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CALLS = ("aloam_places_enable", "aloam_places_add", "aloam_places_match", "aloam_places_export", "aloam_places_load", "aloam_places_clear",
         "aloam_places_info")


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return " ".join(txt.split())


def test_header_declares_the_calls_and_the_records():
    d = _declarations()
    assert "enum { ALOAM_PLACE_RINGS = 20, ALOAM_PLACE_SECTORS = 60 };" in d
    assert "int aloam_places_enable(aloam_ctx* ctx, int capacity, float max_range, float sensor_height);" in d
    assert "int aloam_places_add(aloam_ctx* ctx, const int* seqs, int n);" in d
    assert "int aloam_places_match(aloam_ctx* ctx, const int* seqs, int n, const int* ranges , int T, aloam_place_match* dst );" in d
    assert "int aloam_places_export(aloam_ctx* ctx, int first, int count, aloam_place* dst);" in d
    assert "int aloam_places_load(aloam_ctx* ctx, const aloam_place* src, int count);" in d
    assert "int aloam_places_clear(aloam_ctx* ctx);" in d
    assert "int aloam_places_info(aloam_ctx* ctx, int out[4]);" in d
    assert "typedef struct aloam_place_match { int entry, shift; float distance; int pad; } aloam_place_match;" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                          # records are unchanged


def test_header_documents_the_contract():
    txt = open(HEADER).read()
    block = txt[txt.index("---- place recognition"):txt.index("enum { ALOAM_PLACE_RINGS")]
    for word in ("IROS 2018", "beside the reference", "launches exactly what it launched before", "sqrtf(x * x + y * y)", "atan2f", "ring slabs",
                 "at most once per registered sweep", "the count before the call + i", "aloam_export_poses", "ALOAM_E_CAPACITY", "ALOAM_E_STATE",
                 "sat out the last registration", "ties to the lower shift", "(distance, index)", "+s * 6 deg", "1 <= T <= 8",
                 "f32-input matrix cores", "fixed K order", "finite and non-negative", "pageable", "ALOAM_SEQ_RECORD_VERSION",
                 "aloam_reset_sequences and aloam_load_sequences leave it alone"):
        assert word in block, word


def test_record_offsets_and_the_descriptors_shape(binding):
    """(test_abi_records.py holds both records against the C compiler's layout; the offsets are written out here once more.)"""
    fields = ("cells", "q", "t", "slot", "frame", "n_points", "pad")
    mfields = ("entry", "shift", "distance", "pad")
    assert C.sizeof(binding.AloamPlace) == 4880 and binding.PLACE_DTYPE.itemsize == 4880
    assert C.sizeof(binding.AloamPlaceMatch) == 16 and binding.PLACE_MATCH_DTYPE.itemsize == 16
    assert [getattr(binding.AloamPlace, f).offset for f in fields] == [0, 4800, 4832, 4856, 4860, 4864, 4868]
    assert [binding.PLACE_DTYPE.fields[f][1] for f in fields] == [0, 4800, 4832, 4856, 4860, 4864, 4868]
    assert [binding.PLACE_MATCH_DTYPE.fields[f][1] for f in mfields] == [0, 4, 8, 12]
    assert binding.PLACE_DTYPE["cells"].shape == (binding.PLACE_SECTORS, binding.PLACE_RINGS) == (60, 20)   # sector-major


def test_binding_and_library_export_the_calls(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    for m in ("places_enable", "places_add", "places_match", "places_match_into", "places_export", "places_export_into", "places_load",
              "places_clear", "places_info"):
        assert callable(getattr(binding.Aloam, m, None)), m
    places = importlib.import_module("a-loam_amd.places")
    for f in ("scan_context", "distance", "match", "guess_from_match"):
        assert callable(getattr(places, f, None)), f
    assert (places.RINGS, places.SECTORS) == (binding.PLACE_RINGS, binding.PLACE_SECTORS)
    names = [binding.lib().aloam_profile_kernel_name(k).decode() for k in range(binding.lib().aloam_profile_kernel_count())]
    assert names[-2:] == ["score_corrections", "apply_corrections"]       # no new profiling slot


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids, out = (C.c_int * 2)(0, 0), (C.c_int * 4)()
    assert L.aloam_places_enable(None, 16, 80.0, 2.0) == binding.E_ARG
    assert L.aloam_places_add(None, ids, 1) == binding.E_ARG
    assert L.aloam_places_match(None, ids, 1, ids, 1, None) == binding.E_ARG
    assert L.aloam_places_export(None, 0, 0, None) == binding.E_ARG
    assert L.aloam_places_load(None, None, 0) == binding.E_ARG
    assert L.aloam_places_clear(None) == binding.E_ARG
    assert L.aloam_places_info(None, out) == binding.E_ARG


def test_kitti_runner_has_the_place_options():
    tool = os.path.join(ROOT, "tools", "run_kitti.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--place-spacing" in r.stdout and "--global-relocalize" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, "--selftest", "--global-relocalize"], capture_output=True, text=True)
    assert r.returncode != 0 and "--global-relocalize needs --prior-atlas" in r.stderr
