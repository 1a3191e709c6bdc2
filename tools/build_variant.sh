#!/bin/bash
# tools/build_variant.sh <name> [git-ref|-] [extra hipcc flags]
# Builds libmitransient_amd into ab/libs/lib_<name>.so (ab/ is git-ignored but travels to the GPU box), from the working
# tree ("-") or from a git ref (sources extracted to a temporary directory), for A/B runs with tools/ab.sh.
# With -DMTR_ONLY_C2 among the flags only mtr_kernels.hip is recompiled (one k_fused instantiation: the one config 2 runs) and
# linked against objects of the other sources cached under ab/obj/<source hash>/: a minute per variant.
set -e
name=$1; ref=${2:--}; shift; shift || true
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$root/ab/libs"
src="$root"
if [ "$ref" != "-" ]; then
  src=$(mktemp -d); (cd "$root" && git archive "$ref" mitransient_amd/csrc include | tar -x -C "$src")
fi
cd "$src/mitransient_amd/csrc"
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -munsafe-fp-atomics -Wno-unused-function"
KFLAGS=$(sed -n 's/^KFLAGS *= *//p' Makefile)      # the flags THAT tree's Makefile gives mtr_kernels.hip alone (none before round 8)
if [[ " $* " == *" -DMTR_ONLY_C2 "* ]]; then
  others=$(sed -n 's/^SRCS *= *//p' Makefile | tr ' ' '\n' | grep -v '^mtr_kernels.hip$')      # every other source of THAT tree's library
  h=$(cat $others *.h ../../include/mitransient_amd.h | sha256sum | cut -c1-16)
  od="$root/ab/obj/$h"; mkdir -p "$od"
  for f in $others; do
    [ -f "$od/$f.o" ] || /opt/rocm/bin/hipcc $FL -c $f -o "$od/$f.o" &
  done
  /opt/rocm/bin/hipcc $FL $KFLAGS "$@" -c mtr_kernels.hip -o "$od/kernels_$name.o" &
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o "$root/ab/libs/lib_$name.so" $(for f in $others; do echo "$od/$f.o"; done) "$od/kernels_$name.o"
else
  # every source, by that tree's own Makefile (its per-file flags included), with the extra flags on all of them — in a copy,
  # so that the working tree keeps its own library and objects
  if [ "$ref" = "-" ]; then
    src=$(mktemp -d); mkdir -p "$src/mitransient_amd" && cp -r "$root/mitransient_amd/csrc" "$src/mitransient_amd/" && cp -r "$root/include" "$src/"
    cd "$src/mitransient_amd/csrc" && rm -f libmitransient_amd.so *.o
  fi
  make CXXFLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -munsafe-fp-atomics -Wno-unused-function $*" libmitransient_amd.so
  cp libmitransient_amd.so "$root/ab/libs/lib_$name.so"
fi
[ "$src" != "$root" ] && rm -rf "$src"
echo "built ab/libs/lib_$name.so"
