#!/bin/bash
# triage: ISA of one conv_p2 register tile (seconds): tools/dev/isa_p2.sh <MR> <NR> <out.s> [extra -D...]
# the plain bf16 instances (conv_p2.hip); UNIT=conv_p2_f8.hip (fp8 and fused-reduction variants) / conv_p2_group.hip (grouped kernel) for the others
M=$1; N=$2; OUT=$3; shift 3
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-strict-aliasing -I yolosharp_amd/csrc --cuda-device-only -S -DYS_P2_ONE -DYS_P2_ONE_M=$M -DYS_P2_ONE_N=$N "$@" yolosharp_amd/csrc/${UNIT:-conv_p2.hip} -o $OUT 2>&1 | grep -E "error" -A5 | head -20
