"""Register / LDS / scratch budgets of the place-recognition kernels, read from the code-object metadata hipcc emits for gfx950 (no GPU
needed), in the manner of test_atlas_budgets.py.  The figures are those of DESIGN §7h."""
import os
import re

import pytest

from test_kernel_budgets import CSRC, HIPCC, _kernels, occupancy_waves

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def places(tmp_path_factory):
    return _kernels("places_kernels", tmp_path_factory)


def test_place_kernels_use_no_scratch(places):
    assert set(places) == {"k_place_descriptor", "k_place_add", "k_place_finish", "k_place_match", "k_place_select"}
    for name, k in places.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, k)


def test_descriptor_figures_are_those_measured(places):
    """k_place_descriptor: 36 VGPRs / 72 SGPRs / 9600 bytes of LDS (the 1200 cells as unsigned for the atomic max, and as floats for the
    column norms): one workgroup of 512 threads = two waves per SIMD per sweep, eight by the register files; LDS would allow sixteen such
    workgroups per CU.  It streams 16 B per point and is bound by HBM, not by any of this."""
    k = places["k_place_descriptor"]
    assert k[".vgpr_count"] <= 36 and k[".sgpr_count"] <= 72 and k[".group_segment_fixed_size"] == 9600, k
    assert occupancy_waves(k) == 8, k
    assert k.get(".agpr_count", 0) == 0, k


def test_match_figures_are_those_measured(places):
    """k_place_match: 92 registers of the unified file (48 of them accumulation registers) / 28 SGPRs / 9600 bytes of LDS (the doubled query): five
    waves per SIMD by the vector file = five workgroups of four waves per CU, 48 KB of a CU's 160 KB of LDS.  One wave per SIMD with two
    independent accumulators already issues v_mfma_f32_32x32x2_f32 back to back (64 cycles each, 64 cycles of dependent latency); the other
    four hide the global loads of the entries.  k_place_select: 18 / 42 / 32 bytes."""
    k = places["k_place_match"]
    assert k[".vgpr_count"] <= 92 and k[".sgpr_count"] <= 28 and k[".group_segment_fixed_size"] == 9600, k   # (.vgpr_count counts the unified file: the accumulation registers are in it)
    assert occupancy_waves(k) >= 5, k
    s = places["k_place_select"]
    assert s[".vgpr_count"] <= 18 and s[".sgpr_count"] <= 42 and s[".group_segment_fixed_size"] <= 32, s
    for name in ("k_place_add", "k_place_finish"):
        assert places[name][".vgpr_count"] <= 32 and places[name][".group_segment_fixed_size"] == 0, name


def test_the_match_runs_on_the_f32_matrix_cores(tmp_path_factory):
    """The product is v_mfma_f32_32x32x2_f32 on f32 operands (no reduced-precision inputs), fed by 16-byte LDS and global loads; the source
    holds no inline assembly."""
    import subprocess
    out = tmp_path_factory.mktemp("isa") / "places.s"
    from test_kernel_budgets import FLAGS
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), os.path.join(CSRC, "places_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = out.read_text()
    body = txt[txt.index("k_place_match"):txt.index("k_place_select")]
    assert len(re.findall(r"v_mfma_f32_32x32x2_f32", body)) >= 8
    assert not re.findall(r"v_mfma_f32_\d+x\d+x\d+_(?:f16|bf16|bf8|fp8|xf32)", txt)
    assert "ds_read_b128" in body and "global_load_dwordx4" in body
    assert "asm" not in open(os.path.join(CSRC, "places_kernels.hip")).read().replace("assembly", "")
