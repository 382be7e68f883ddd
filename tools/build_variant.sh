#!/bin/bash
# Experiment builds of the conv kernels: build_variant.sh <name> <defines...>  ->  build/libvpt_<name>.so (bf16 library with the four
# vpt_conv3x3*.hip sources -- launch function, forward, dgrad, latency tiling -- compiled with the given -D flags).  Run with VPT_HIP_LIB=... (see _native.py).
# Forward-loop ablations (timing only): -DVPT_CONV_PROFILE -DVPT_CONV_FWD_ABLATE=1|2|4 (no weight DMA | no halo reloads | neither).
set -e
cd "$(dirname "$0")/../video-pre-training_amd"
name=$1; shift
mkdir -p build/var_$name
rm -f build/var_$name/vpt_conv3x3*.o
for src in csrc/vpt_conv3x3*.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-gpu-rdc -I../include "$@" -c $src -o build/var_$name/$(basename ${src%.hip}).o 2>/dev/null &
done
wait
objs=$(ls build/bf16/*.o | grep -v 'vpt_conv3x3[_a-z]*\.o')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/libvpt_$name.so $objs build/var_$name/vpt_conv3x3*.o
echo "built build/libvpt_$name.so"
