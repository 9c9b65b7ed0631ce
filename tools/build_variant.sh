#!/bin/bash
# Build deephisto_amd/libdeephisto_hip_<name>.so with extra compiler flags (A/B experiments; tooling only): every
# deephisto_amd/csrc/*.hip with the flags of deephisto_amd/build.py plus the extra ones, at most 16 compiles at once.
# usage: tools/build_variant.sh <name> [extra hipcc flags...]
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
T=/tmp/dh_variant_$name; rm -rf "$T"; mkdir -p "$T"
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -ffp-contract=off"
export T
printf '%s\0' "$R"/deephisto_amd/csrc/*.hip |
  xargs -0 -P 16 -I{} sh -c 'src=$1; shift; hipcc "$@" -c "$src" -o "$T/$(basename "$src" .hip).o"' _ {} $F "$@"
hipcc -shared -fPIC --offload-arch=gfx950 "$T"/*.o -o "$R/deephisto_amd/libdeephisto_hip_$name.so"
echo built "$R/deephisto_amd/libdeephisto_hip_$name.so"
