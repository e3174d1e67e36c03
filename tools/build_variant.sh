#!/bin/bash
# tools/build_variant.sh <name> <extra hipcc flags...> — an A/B build of the library next to the product one
# (a-loam_amd/lib/variants/lib<name>.so, git-ignored, travels to the GPU box); select it with ALOAM_MI355X_LIB=<path>.
# Built by a-loam_amd/csrc/Makefile, so the variant has every source file of the product; its objects go to lib/variants/obj-<name>/.
# -B: every call compiles everything, since make does not track flags (a name reused with other flags must not keep the old objects).
set -e
NAME=$1; shift
cd "$(dirname "$0")/../a-loam_amd/csrc"
make -B -j16 OUT=../lib/variants/lib$NAME.so OBJDIR=../lib/variants/obj-$NAME EXTRA_FLAGS="$*" >&2
echo a-loam_amd/lib/variants/lib$NAME.so
