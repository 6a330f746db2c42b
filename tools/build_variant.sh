#!/bin/bash
# tools/build_variant.sh NAME [-DMACRO=VALUE ...]: another build of the HIP library
# with compile-time switches, as ffn_amd/csrc/libffn_hip_NAME.so (select it with
# FFN_AMD_LIB=...: same-box A/B runs of kernel variants in one job).  Every
# ffn_*.hip is compiled, as _lib.load() wants the symbols of all of them.
# FFN_CSRC=DIR takes the sources from another csrc directory (another commit's,
# inside a tree with its include/ beside it) for an A/B of two source states.
set -e
name=$1; shift
cd "$(dirname "$0")/../ffn_amd/csrc"
out=$PWD
src=${FFN_CSRC:-$out}
mkdir -p build/$name
rm -f build/$name/ffn_*.o
pids=()
for f in "$src"/ffn_*.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c "$f" \
    -o build/$name/$(basename "$f" .hip).o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libffn_hip_$name.so build/$name/ffn_*.o
echo built libffn_hip_$name.so
