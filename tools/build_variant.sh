#!/bin/bash
# Build a variant of libgsplat_hip.so with extra compiler flags into gpurun_ab/lib_<name>.so (A/B experiments).
# usage: tools/build_variant.sh <name> [extra hipcc flags...]
# The variant is built by the source tree's OWN csrc/Makefile, in a scratch copy of the sources: the object list, the headers and
# the set of files compiled with -ffp-contract=off are whatever that Makefile says.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${GS_VARIANT_SRC:-$ROOT/gaussiansplats3d_amd/csrc}     # (GS_VARIANT_SRC: another tree's csrc, e.g. a checkout of an older commit)
OUT=$ROOT/gpurun_ab; OBJ=/tmp/gsvar_$NAME
rm -rf $OBJ
mkdir -p $OUT $OBJ/gaussiansplats3d_amd/csrc $OBJ/include
cp $SRC/Makefile $SRC/*.hip $SRC/*.hpp $(ls $SRC/*.cpp 2>/dev/null) $OBJ/gaussiansplats3d_amd/csrc/     # (*.cpp: host-only sources, none in older trees)
cp $SRC/../../include/*.h $OBJ/include/
make -s -C $OBJ/gaussiansplats3d_amd/csrc -j${MAX_JOBS:-16} libgsplat_hip.so \
     CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function $*"
cp $OBJ/gaussiansplats3d_amd/csrc/libgsplat_hip.so $OUT/lib_$NAME.so
echo built $OUT/lib_$NAME.so
