#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...]: an A/B build of the HIP library into ezrt_amd/lib/ab/libezrt_hip_NAME.so
# (EZRT_HIP_LIB selects it for a run; never loaded by default).  The sources are the Makefile's HIP_SRC.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p ezrt_amd/lib/ab
src=$(sed -n 's/^HIP_SRC *= *//p' Makefile)
[ -n "$src" ] || { echo "build_variant.sh: no HIP_SRC in the Makefile" >&2; exit 1; }
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero \
  -fno-slp-vectorize -Wall -Wno-unused-function -Iinclude -Iezrt_amd/csrc/hip "$@" -shared -o ezrt_amd/lib/ab/libezrt_hip_$name.so \
  $src -ldl -pthread
