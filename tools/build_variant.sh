#!/bin/bash
# Diagnostic: build build/variants/lib_<name>.so = the shipped library with the named sources recompiled with extra flags
#   tools/build_variant.sh <name> "<source.hip ...>" "<extra hipcc flags>"        (runs without a GPU)
# A macro that several units read takes all of them: SPLIT_SIGNED sits in gemm_common.h and is read by the units with
# split or bf16-mixed kernels (gemm.hip and gemm_exact.hip have none), so
#   tools/build_variant.sh nosign "gemm_split.hip gemm_amp_fwd.hip gemm_amp_wgrad.hip" "-DSPLIT_SIGNED=0"
# and the ADV_* knobs sit in advect_common.h, so an advection variant takes all four advect units:
#   tools/build_variant.sh halo12 "advect.hip advect_planes.hip advect_tilerow.hip advect_strips.hip" "-DADV_HALO_BWD=12"
# Likewise the DWCONV_* knobs sit in stencil_common.h, so a stencil variant takes all three stencil units:
#   tools/build_variant.sh notiles "stencil.hip stencil_planes.hip stencil_generic.hip" "-DDWCONV_TILES=0"
# A/B the variants on one box with PARADIS_HIP_LIB=build/variants/lib_<name>.so (tools/adv_trace*.sh, tools/ab_libs.sh).
set -e
NAME=$1; SRCS=$2; FLAGS=$3
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/build/variants; mkdir -p $OUT
OBJS=$(ls $R/build/obj/*.o)
for SRC in $SRCS; do
  BASE=$(basename $SRC .hip)
  EXTRA="-fno-slp-vectorize"
  case $BASE in advect*|feed) EXTRA="$EXTRA -ffp-contract=off";; esac
  /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -munsafe-fp-atomics $EXTRA $FLAGS \
      -c $R/paradis_model_amd/csrc/$BASE.hip -o $OUT/${BASE}_$NAME.o
  OBJS="$(echo "$OBJS" | grep -v "/$BASE.o") $OUT/${BASE}_$NAME.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/lib_$NAME.so $OBJS
echo "built $OUT/lib_$NAME.so"
