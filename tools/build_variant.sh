#!/bin/bash
# Build a flag variant of librsp for A/B runs on the GPU (tools/ab_pc.sh VARIANTS=...):
#   tools/build_variant.sh NAME "-DFOO=1 -DBAR"   ->  radar-signal-process_amd/lib/ablate/librsp_NAME.so
# The flags reach every unit, kernels and host code (dev-only -D switches of either).
# KSRC=dir: take the sources (csrc/*.hip, *.cpp and the headers next to them) from dir instead
# of csrc (e.g. a `git archive` of an older commit for a bit-identity A/B).
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
name=$1; flags=${2:-}
make -s -j8 -C "$ROOT/radar-signal-process_amd" OBJ_DIR="build/ablate/$name" LIB="lib/ablate/librsp_$name.so" \
    EXTRA="$flags" ${KSRC:+SRC_DIR="$(cd "$KSRC" && pwd)"}
echo "built lib/ablate/librsp_$name.so ($flags)"
