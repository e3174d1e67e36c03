"""Map tiles and the map spill, host side (no GPU): the entry points and the 32-byte tile in the header, the binding and the library; what
can be refused without a device."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aloam_mi355x.h")
CALLS = ("aloam_map_spill_enable", "aloam_export_map_spill", "aloam_get_map_spill_info", "aloam_atlas_load", "aloam_atlas_attach", "aloam_atlas_info")


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return " ".join(txt.split())


def test_header_declares_the_calls_and_the_tile():
    d = _declarations()
    assert "int aloam_map_spill_enable(aloam_ctx* ctx, int max_tiles, int max_points);" in d
    assert ("int aloam_export_map_spill(aloam_ctx* ctx, const int* seqs, int n, aloam_map_tile* tiles_dst, long long cap_tiles, float* points_dst_xyzw, "
            "long long cap_points, long long* dst_offsets , int clear);") in d
    assert "int aloam_get_map_spill_info(aloam_ctx* ctx, int seq, int out[8]);" in d
    assert "typedef struct aloam_map_tile { int cube[3]; int feature_class; int count; int frame; long long first_point; } aloam_map_tile;" in d
    assert "int aloam_atlas_load(aloam_ctx* ctx, const aloam_map_tile* tiles, long long n_tiles, const float* points_xyzw, long long n_points);" in d
    assert "int aloam_atlas_attach(aloam_ctx* ctx, const int* attached );" in d
    assert "int aloam_atlas_info(aloam_ctx* ctx, long long out[12]);" in d
    assert "ALOAM_SEQ_RECORD_VERSION = 1" in d                          # records are unchanged


def test_header_documents_the_contract():
    txt = open(HEADER).read()
    block = txt[txt.index("---- map tiles and the map spill"):txt.index("typedef struct aloam_map_tile")]
    for word in (":312-321", ":323-507", "ascending window index", "BEFORE the step", "whole or not at all", "ALOAM_E_CAPACITY", "map spill full",
                 "aloam_reset_sequences", "aloam_load_sequences", "drains a slot before it reuses it", "aloam_export_clouds", "pageable",
                 "BOTH ranges", "size query", "Idle sequences spill nothing", "launches exactly what it launched before"):
        assert word in block, word
    block = txt[txt.index("---- the atlas:"):txt.index("int aloam_atlas_load(")]
    for word in (":323-507", ":788-801", "n_tiles = 0 unloads", "ALOAM_E_STATE", "ALOAM_E_CAPACITY", "load factor <= 1/2", "input-order sum",
                 "aloam_set_voxel_sum_order", "marked stale", "aloam_set_map_frame(cen, guess, 0)", "aloam_apply_map_corrections does not",
                 "must be frozen", "queues", "sliding sums", "device bytes"):
        assert word in block, word


def test_tile_offsets_and_the_models_dtype(binding):
    """(test_abi_records.py holds the tile against the C compiler's layout; the offsets are written out here once more.)"""
    fields = ("cube", "feature_class", "count", "frame", "first_point")
    atlas = importlib.import_module("a-loam_amd.atlas")
    assert C.sizeof(binding.AloamMapTile) == 32 and binding.MAP_TILE_DTYPE.itemsize == 32 and atlas.TILE_DTYPE == binding.MAP_TILE_DTYPE
    assert [getattr(binding.AloamMapTile, f).offset for f in fields] == [0, 12, 16, 20, 24]
    assert [binding.MAP_TILE_DTYPE.fields[f][1] for f in fields] == [0, 12, 16, 20, 24]


def test_binding_and_library_export_the_calls(binding):
    binding.build()
    syms = binding.declared_symbols()
    for name in CALLS:
        assert name in syms and hasattr(binding.lib(), name), name
    assert "aloam_map_tile" not in syms                                   # a record, not a function
    for m in ("map_spill_enable", "export_map_spill", "export_map_spill_into", "map_spill_info", "atlas_load", "atlas_attach", "atlas_info"):
        assert callable(getattr(binding.Aloam, m, None)), m
    names = [binding.lib().aloam_profile_kernel_name(k).decode() for k in range(binding.lib().aloam_profile_kernel_count())]
    assert names[-2:] == ["score_corrections", "apply_corrections"]       # no new profiling slot: the spill runs inside map_begin


def test_a_null_context_is_an_argument_error(binding):
    L = binding.lib()
    ids, out = (C.c_int * 1)(0), (C.c_int * 8)()
    assert L.aloam_map_spill_enable(None, 16, 16) == binding.E_ARG
    assert L.aloam_export_map_spill(None, ids, 1, None, 0, None, 0, None, 0) == binding.E_ARG
    assert L.aloam_get_map_spill_info(None, 0, out) == binding.E_ARG
    assert L.aloam_atlas_load(None, None, 0, None, 0) == binding.E_ARG
    assert L.aloam_atlas_attach(None, None) == binding.E_ARG
    assert L.aloam_atlas_info(None, (C.c_longlong * 12)()) == binding.E_ARG


def test_kitti_runner_has_both_atlas_options():
    tool = os.path.join(ROOT, "tools", "run_kitti.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--save-atlas FILE.npz" in r.stdout and "--prior-atlas FILE.npz" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, "--selftest", "--prior-atlas", "a.npz", "--prior-map", "m.npz"], capture_output=True, text=True)
    assert r.returncode != 0 and "--prior-atlas and --prior-map exclude each other" in r.stderr
    r = subprocess.run([sys.executable, tool, "--selftest", "--save-atlas", "a.npz"], capture_output=True, text=True)
    assert r.returncode != 0 and "--save-atlas needs --mapping" in r.stderr
