#!/bin/bash
# Builds the library as it was at a git revision (kernel sources only) for A/B timing: tools/build_at.sh REV NAME -> tools/var_NAME.so
set -e
cd "$(dirname "$0")/.."
REV=$1; NAME=$2
TMP=$(mktemp -d)
git archive $REV rtiow_amd/csrc include | tar -x -C $TMP
# every translation unit the revision has: the loader refuses a library that lacks a symbol it declares
SRCS=$(ls $TMP/rtiow_amd/csrc/rt_*.hip $TMP/rtiow_amd/csrc/wavefront/*.hip $TMP/rtiow_amd/csrc/denoise/*.hip 2>/dev/null || true)   # (an older revision lacks the folders)
hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -mllvm -amdgpu-mfma-vgpr-form \
  -fPIC -shared -I $TMP/include -I $TMP/rtiow_amd/csrc -o tools/var_$NAME.so $SRCS
rm -rf $TMP
ls -la tools/var_$NAME.so
