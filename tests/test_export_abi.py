"""CPU-side checks of the batched export's boundary (aloam_export_poses / aloam_export_clouds): the library exports both entries, the ctypes
mirror of aloam_pose_record has the layout a C compiler gives the header's, and the id constants of the binding are the header's."""
import re
import subprocess


def test_library_exports_the_batched_export(binding):
    L = binding.lib()
    for name in ("aloam_export_poses", "aloam_export_clouds"):
        assert name in binding.declared_symbols()
        assert hasattr(L, name)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aloam_[a-z_0-9]+)", out))
    assert {"aloam_export_poses", "aloam_export_clouds"} <= exported


def test_export_id_constants_match_the_header(binding, tmp_path):
    names = {"ALOAM_EXPORT_MAP": binding.EXPORT_MAP, "ALOAM_EXPORT_MAX_IDS": binding.EXPORT_MAX_IDS,
             "ALOAM_MAP_REGISTERED": binding.MAP_REGISTERED, "ALOAM_MAP_CORNER_STACK": binding.MAP_CORNER_STACK,
             "ALOAM_MAP_SURF_STACK": binding.MAP_SURF_STACK, "ALOAM_MAP_SURROUND": binding.MAP_SURROUND, "ALOAM_MAP_FULL": binding.MAP_FULL,
             "ALOAM_CLOUD_FULL": binding.CLOUD_FULL, "ALOAM_CLOUD_SURF_LAST": binding.CLOUD_SURF_LAST}
    src = ['#include <stdio.h>', f'#include "{binding.HEADER_PATH}"', "int main(void) {"]
    src += [f'  printf("{n} %d\\n", (int){n});' for n in names]
    src += ["  return 0;", "}"]
    c = tmp_path / "ids.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "ids"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert {k: int(v) for k, v in got.items()} == names
    # the map ids of an export do not collide with the cloud ids
    assert binding.EXPORT_MAP + binding.MAP_REGISTERED > binding.CLOUD_SURF_LAST
