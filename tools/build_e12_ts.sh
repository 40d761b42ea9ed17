#!/bin/bash
# libdreamer_hip with the conv1 + conv2 kernel's phase timestamps (DR_E12_TS):
# conv_split.hip recompiled, the other objects reused.  Two variants:
#   e12ts     the product schedule (k_enc12_split3_x8) with stamps
#   e12ts_r3  the round-3 schedule (k_enc12_split3<8>) with stamps
# Read with tools/enc12_probe.py.
set -e
cd "$(dirname "$0")/.."
python -m dreamer_amd.build > /dev/null
FL="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-gpu-rdc -Wall -Wno-unused-function -Wno-unused-variable"
objs=$(ls dreamer_amd/_build/*.o | grep -v -e '/conv_split.o')
for V in "e12ts 1" "e12ts_r3 2"; do
  set -- $V
  O=tools/variants/_build_$1
  mkdir -p $O
  /opt/rocm/bin/hipcc $FL -DDR_E12_TS=$2 -c dreamer_amd/csrc/conv_split.hip -o $O/conv_split.o &
done
wait
for N in e12ts e12ts_r3; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/variants/libdreamer_hip_$N.so tools/variants/_build_$N/conv_split.o $objs
  echo built tools/variants/libdreamer_hip_$N.so
done
