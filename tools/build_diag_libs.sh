#!/bin/bash
# Diagnostic builds of the library (never shipped): wave-time per phase (RT_PHASE_STAMPS), block
# execution counts (RT_BLOCK_COUNTS; with -DRT_COUNT_ROWS counters 1 and 6 count the large grid's footprint-row and list-emission trips instead of
# camera blocks and unit-sphere tries, with -DRT_COUNT_ENUM the enumeration's trips and the candidates it pushes: tools/build_variants.sh NAME "-DRT_BLOCK_COUNTS -DRT_COUNT_ENUM"),
# wave exit times (RT_EXIT_TIMES).  -> tools/lib_{stamps,counts,exit}.so
cd "$(dirname "$0")/.."
# (every translation unit of the library: the diagnostic macros live in the kernel they all instantiate)
SRCS=$(ls rtiow_amd/csrc/rt_*.hip rtiow_amd/csrc/wavefront/*.hip)
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -mllvm -amdgpu-mfma-vgpr-form -fPIC -shared -I include -I rtiow_amd/csrc"
hipcc $FLAGS -DRT_PHASE_STAMPS -o tools/lib_stamps.so $SRCS &
hipcc $FLAGS -DRT_BLOCK_COUNTS -o tools/lib_counts.so $SRCS &
# (the capped body: counter 1 = parked lanes, counter 6 = redraw blocks executed after the shared one; tools/dense_body_counts.py)
hipcc $FLAGS -DRT_BLOCK_COUNTS -DRT_COUNT_PARKS -o tools/lib_counts_parks.so $SRCS &
hipcc $FLAGS -DRT_EXIT_TIMES -o tools/lib_exit.so $SRCS &
hipcc $FLAGS -DRT_LDS_CONFLICTS -o tools/lib_ldsc.so $SRCS &
wait
ls -la tools/lib_stamps.so tools/lib_counts.so tools/lib_exit.so
