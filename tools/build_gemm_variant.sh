#!/bin/bash
# usage: tools/build_gemm_variant.sh <name> <extra hipcc flags...>  ->  inference-tools_amd/inference_amd/lib/libgpmi_<name>.so
# (like build_variant.sh, for flags that change gemm_tiles.h: every translation unit that includes it, directly or through
# potrf_colblock.h, is rebuilt; the others are taken from the last `make`)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
out=$ROOT/tools/variants; mkdir -p $out/obj_$name
cd $ROOT/inference-tools_amd/csrc
for src in $(sed -n 's/^SRCS *:= *//p' Makefile); do
  f=${src%.hip}
  if grep -q "gemm_tiles.h\|potrf_colblock.h" $f.hip || [ ! -f build/$f.o ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -I../../include -I. "$@" -c $f.hip -o $out/obj_$name/$f.o
  else
    cp build/$f.o $out/obj_$name/$f.o
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-z,defs -Wl,--version-script=gpmi.map -o $ROOT/inference-tools_amd/inference_amd/lib/libgpmi_$name.so $out/obj_$name/*.o -ldl
echo libgpmi_$name.so
