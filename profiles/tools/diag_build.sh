#!/bin/bash
# Build diagnostic variants of the library (timing ablations of kirch_quad_kernel; results are NOT valid):
#   profiles/tools/diag_build.sh "NOLDS" "NOFMA -DKQ_DIAG_NOSTAGE" ...   ->  build/diag/lib_<name>.so
# Run one with IMPDAR_HIP_LIB=$PWD/build/diag/lib_<name>.so python bench.py --no-cpu
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p $R/build/diag
OBJS=""       # every other unit from the regular build (kirch_quad_kernel lives in kirch_ring32.hip)
for o in $R/impdar_amd/csrc/*.o; do [ $(basename $o .o) != kirch_ring32 ] && OBJS="$OBJS $o"; done
for v in "$@"; do
  n=$(echo $v | tr -d ' ' | sed 's/-DKQ_DIAG_/_/g; s/-D//g')
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wno-unused-function \
      -DKQ_DIAG_$v -c $R/impdar_amd/csrc/kirch_ring32.hip -o $R/build/diag/k_$n.o 2>&1 | grep -E "error" -A3
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $R/build/diag/k_$n.o -o $R/build/diag/lib_$n.so \
      -L/opt/rocm/lib -lrocfft -lrccl -Wl,-rpath,/opt/rocm/lib ) &
done
wait
ls $R/build/diag/*.so
