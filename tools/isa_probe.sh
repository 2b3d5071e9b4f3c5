#!/bin/bash
# Compile only the weights-stationary conv kernels of conv_igemm.hip (seconds instead of minutes) and print ISA statistics.
# (the fp16, int8 and split-fp16 head pairs: conv_dual_ws<WsP3<T>, WsP4<T>>, instantiated for the probe at the end of conv_igemm.hip)
# usage: tools/isa_probe.sh [extra hipcc flags]; output: /tmp/probe/conv_igemm-hip-amdgcn-amd-amdhsa-gfx950.s
set -e
mkdir -p /tmp/probe
T=$(cd "$(dirname "$0")" && pwd); cd "$T/../unina-yolo-dla_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DUNINA_CONV_PROBE "$@" -c conv_igemm.hip -o /tmp/probe/conv_igemm.o -save-temps=obj
python3 "$T/isastat.py" /tmp/probe/conv_igemm-hip-amdgcn-amd-amdhsa-gfx950.s \
  _ZN5unina12conv_dual_wsINS_6WsTileIDF16_Li16ELi128ELi2ELi4EEENS1_IDF16_Li8ELi256ELi4ELi4EEELb0ELi0EEEvNS_10ConvParamsES4_i \
  _ZN5unina12conv_dual_wsINS_6WsTileIaLi16ELi128ELi2ELi4EEENS1_IaLi8ELi256ELi4ELi4EEELb0ELi0EEEvNS_10ConvParamsES4_i \
  _ZN5unina12conv_dual_wsINS_6WsTileINS_5s16_tELi16ELi128ELi4ELi4EEENS1_IS2_Li8ELi256ELi4ELi4EEELb0ELi0EEEvNS_10ConvParamsES5_i
