#!/bin/bash
# tools/asm_funcs.sh <out dir> [git-ref|-] [extra hipcc flags] — the gfx950 assembly of every device source of the library, one .s per
# source under <out dir> (cross-compiles; no GPU), from the working tree ("-") or from a git ref, with the flags THAT tree's Makefile
# gives each file; mtr_kernels.hip also leaves its register / spill / scratch remarks in <out dir>/mtr_kernels.remarks.
# Compare two such directories function by function with tools/asm_diff.py.
set -e
out=$1; ref=${2:--}; shift; shift || true
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$out"; out=$(cd "$out" && pwd)
src="$root"
if [ "$ref" != "-" ]; then
  src=$(mktemp -d); (cd "$root" && git archive "$ref" mitransient_amd/csrc include | tar -x -C "$src")
fi
cd "$src/mitransient_amd/csrc"
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -munsafe-fp-atomics -Wno-unused-function"
KFLAGS=$(sed -n 's/^KFLAGS *= *//p' Makefile)
for f in $(sed -n 's/^SRCS *= *//p' Makefile | tr ' ' '\n' | grep '\.hip$'); do
  if [ "$f" = mtr_kernels.hip ]; then
    /opt/rocm/bin/hipcc $FL $KFLAGS "$@" -Rpass-analysis=kernel-resource-usage -S --cuda-device-only $f -o "$out/${f%.hip}.s" 2> "$out/mtr_kernels.remarks" &
  else
    /opt/rocm/bin/hipcc $FL "$@" -S --cuda-device-only $f -o "$out/${f%.hip}.s" &
  fi
done
wait
[ "$src" != "$root" ] && rm -rf "$src"
echo "assembly in $out"
