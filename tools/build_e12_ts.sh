#!/bin/bash
# libdreamer_hip with the conv1 + conv2 kernel's phase timestamps (DR_E12_TS):
# conv_split.hip recompiled, the other objects reused.  Builds the variant
# e12ts: the product schedule (k_enc12_split3_x8) with stamps.
# Read with tools/enc12_probe.py.
set -e
cd "$(dirname "$0")/.."
python -m dreamer_amd.build > /dev/null
FL="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-gpu-rdc -Wall -Wno-unused-function -Wno-unused-variable"
objs=$(ls dreamer_amd/_build/*.o | grep -v -e '/conv_split.o')
O=tools/variants/_build_e12ts
mkdir -p $O
/opt/rocm/bin/hipcc $FL -DDR_E12_TS=1 -c dreamer_amd/csrc/conv_split.hip -o $O/conv_split.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/variants/libdreamer_hip_e12ts.so $O/conv_split.o $objs
echo built tools/variants/libdreamer_hip_e12ts.so
