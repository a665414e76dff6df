#!/bin/bash
# Diagnostic builds of libzp with conv / wgrad ablations (ZP_ABL=1: no LDS-DMA in the loop, 2: no
# MFMA, 3: weights only, 4: strips only, 5: no epilogue (k_conv_quad); results are wrong): zebrapose_amd/libzp_abl<N>.so.  Only
# zp_conv.hip and zp_wgrad.hip are rebuilt; the other objects come from the product build (make first).
# Use with ZP_LIB=zebrapose_amd/libzp_abl<N>.so python tools/conv_ab.py ...
set -e
cd "$(dirname "$0")/../zebrapose_amd/csrc"
for n in "$@"; do
  mkdir -p build_abl$n
  for f in zp_conv zp_wgrad; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DZP_ABL=$n -c $f.hip -o build_abl$n/$f.o &
  done
done
wait
for n in "$@"; do
  objs=$(ls build/*.o | grep -v -e zp_conv.o -e zp_wgrad.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libzp_abl$n.so build_abl$n/zp_conv.o build_abl$n/zp_wgrad.o $objs
done
