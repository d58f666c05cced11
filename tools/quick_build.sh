#!/bin/bash
# Tuning build: the v5 kernel header $1 (a copy of poms_amd/csrc/kron_v5_kernel.hpp being
# tuned) compiled with -DPOMS_V5_QUICK (p = 3 production kernels only) through the kron_v5*.hip
# units, linked with every other object of poms_amd/_obj into $2.
# (Every object: one left behind by a source that no longer exists has to be deleted.)
# Run with POMS_HIP_LIB=$2; never replaces poms_amd/libpoms_hip.so.
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$1; OUT=$2
T=$(mktemp -d)
cp "$ROOT"/poms_amd/csrc/*.hpp "$ROOT"/poms_amd/csrc/kron_v5*.hip $T/
cp "$SRC" $T/kron_v5_kernel.hpp
objs=""
for s in $T/kron_v5*.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -munsafe-fp-atomics \
      -DPOMS_V5_QUICK -I "$ROOT/include" -c $s -o $s.o
  objs="$objs $s.o"
done
for o in "$ROOT"/poms_amd/_obj/*.hip.o; do
  case "$(basename "$o")" in kron_v5*) ;; *) objs="$objs $o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $objs -L/opt/rocm/lib -lrccl
rm -rf $T
echo "built $OUT"
