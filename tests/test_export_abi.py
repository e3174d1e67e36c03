"""CPU-side checks of the batched export's boundary (aloam_export_poses / aloam_export_clouds): the library exports both entries, the ctypes
mirror of aloam_pose_record has the layout a C compiler gives the header's, and the id constants of the binding are the header's."""
import ctypes as C
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


def test_pose_record_mirror_matches_the_header_layout(binding, tmp_path):
    cls = binding.AloamPoseRecord
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{binding.HEADER_PATH}"', "int main(void) {",
           '  printf("%zu", sizeof(aloam_pose_record));']
    src += [f'  printf(" {n}:%zu", offsetof(aloam_pose_record, {n}));' for n, _ in cls._fields_]
    src += ['  printf("\\n");', "  return 0;", "}"]
    c = tmp_path / "pose_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "pose_layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    parts = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(parts[0]) == C.sizeof(cls) == 240
    for tok, (name, _) in zip(parts[1:], cls._fields_):
        n, off = tok.split(":")
        assert n == name and int(off) == getattr(cls, name).offset, tok
    # every field of the header's struct is mirrored, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(binding.HEADER_PATH).read(), flags=re.S)
    body = re.search(r"typedef struct aloam_pose_record \{(.*?)\} aloam_pose_record;", hdr, flags=re.S).group(1)
    declared = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[,;]", body)
    assert declared == [n for n, _ in cls._fields_], declared


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
