#!/bin/bash
# Build libopeneat_hip.so for gfx950 in-tree (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
OUT=../lib
mkdir -p "$OUT" obj
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -ffp-contract=fast"
# rebuild an object when its source, any header here or the public header is newer
newer_header() {
  local h
  for h in *.h ../../include/openeat_hip.h; do [ "$h" -nt "$1" ] && return 0; done
  return 1
}
pids=()
objs=()                                     # the objects of the sources that exist: obj/ may hold those of deleted ones
for f in *.hip; do
  o=obj/${f%.hip}.o
  objs+=("$o")
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || newer_header "$o"; then
    echo "hipcc $f"
    $HIPCC $FLAGS -c "$f" -o "$o" &
    pids+=($!)
  fi
done
host_objs=()
for f in *.cpp; do
  o=obj/${f%.cpp}.o
  host_objs+=("$o")
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || newer_header "$o"; then
    echo "g++ $f"
    g++ -O2 -fPIC -std=c++17 -Wall -pthread -c "$f" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -pthread -o "$OUT/libopeneat_hip.so" "${objs[@]}" "${host_objs[@]}"
echo "built $OUT/libopeneat_hip.so"
# OE_DIAG=1: also build the stamped diagnostic variant (tools/gemm_stamps.py); never loaded by the product path
if [ "${OE_DIAG:-0}" = "1" ]; then
  mkdir -p obj_diag
  for f in *.hip; do $HIPCC $FLAGS -DOE_GEMM_STAMPS -c "$f" -o "obj_diag/${f%.hip}.o" & done
  wait
  $HIPCC --offload-arch=gfx950 -shared -fPIC -pthread -o "$OUT/libopeneat_hip_diag.so" "${objs[@]/#obj\//obj_diag/}" "${host_objs[@]}"
  echo "built $OUT/libopeneat_hip_diag.so"
fi
