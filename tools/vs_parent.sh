#!/bin/bash
# This library against the PARENT commit's library, bit for bit: runs the GPU tests that compare the two and skip without DH_PARENT_LIB.
# Builds the parent (default: HEAD~1) from git into a temporary worktree -- do that where no GPU time is spent -- and runs the pytest selection.
# usage: bash tools/vs_parent.sh [-p <parent commit>] [pytest selection ...]     or, with a parent library already built:  DH_PARENT_LIB=<path> bash tools/vs_parent.sh ...
# default selection: every such test --
#   tests/test_gpu_conv3_vs_parent.py                          every launch path of the 3x3 convolutions
#   tests/test_gpu_conv_mfma_shape.py -k parent_library        DH_CONV_MFMA16=0 on the shapes of tests/helpers/conv_mfma_shapes.py
#   tests/test_gpu_train_vs_parent.py                          training steps of the three engines, side stream on and off (tests/helpers/train_paths.py)
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
PARENT=HEAD~1
if [ "$1" = "-p" ]; then PARENT=$2; shift 2; fi
if [ -z "$DH_PARENT_LIB" ]; then
  T=$(mktemp -d); trap 'git worktree remove --force $T/parent 2>/dev/null; rm -rf $T' EXIT
  git worktree add --detach $T/parent $PARENT > /dev/null
  (cd $T/parent && python3 -m deephisto_amd.build > $T/build.log 2>&1) || { tail -20 $T/build.log; exit 1; }
  export DH_PARENT_LIB=$T/parent/deephisto_amd/libdeephisto_hip.so
fi
if [ $# -eq 0 ]; then set -- tests/test_gpu_conv3_vs_parent.py tests/test_gpu_train_vs_parent.py tests/test_gpu_conv_mfma_shape.py -k parent_library; fi
timeout -k 10 900 python3 -m pytest "$@" -q -rs
