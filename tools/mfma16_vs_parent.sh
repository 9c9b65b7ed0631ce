#!/bin/bash
# DH_CONV_MFMA16=0 of this library against the PARENT commit's library, bit for bit, on the shapes of tests/helpers/conv_mfma_shapes.py.
# Builds the parent (default: HEAD~1) from git into a temporary worktree -- do that where no GPU time is spent -- and runs the test that compares.
# usage: bash tools/mfma16_vs_parent.sh [parent commit]        or, with a parent library already built:  DH_PARENT_LIB=<path> bash tools/mfma16_vs_parent.sh
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
if [ -z "$DH_PARENT_LIB" ]; then
  T=$(mktemp -d); trap 'git worktree remove --force $T/parent 2>/dev/null; rm -rf $T' EXIT
  git worktree add --detach $T/parent ${1:-HEAD~1} > /dev/null
  (cd $T/parent && python3 -m deephisto_amd.build > $T/build.log 2>&1) || { tail -20 $T/build.log; exit 1; }
  export DH_PARENT_LIB=$T/parent/deephisto_amd/libdeephisto_hip.so
fi
timeout -k 10 900 python3 -m pytest tests/test_gpu_conv_mfma_shape.py -q -k parent_library -rs
