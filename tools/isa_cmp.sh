#!/bin/bash
# Byte comparison of the device assembly of two source trees: every source in the Makefile's
# SRCS, compiled as the Makefile compiles it (the command line is read from `make -n`, so the
# per-file flags come along), plus the variant builds behind the ablation and profiling hooks.
# Nothing inside the assembly is inspected: `cmp` decides. -fuse-cuid=none takes out the one
# symbol (__hip_cuid_*) that differs between two compiles of the same source.
#   tools/isa_cmp.sh <tree A> <tree B> [work dir]        exit 0 iff every pair is identical
set -uo pipefail
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); WORK=${3:-$(mktemp -d)}
JOBS=${JOBS:-8}
mkdir -p "$WORK"
# variant builds: "<source> <name> <extra flags>"
VARIANTS="tr_spectral.hip skip1 -DTR_SPEC_SKIP=1
tr_spectral.hip prof -DTR_SPEC_PROFILE=1
tr_mnl.hip prof -DTR_MNL_PROFILE=1
tr_mnl_duo.hip skip2 -DTR_DUO_SKIP=2
tr_spectral_slice.hip trunc -DTR_SLICE_SPLITMODE=0 -DTR_SLICE_ACCUM=0"

emit() {  # the compile commands of one tree, one per line
  local tree=$1 out=$2 csrc=$1/tensor_regression_amd/csrc
  mkdir -p "$out"
  make -s -C "$csrc" build/tr_build_id.h || exit 2
  local srcs; srcs=$(make -s -C "$csrc" --eval 'print-srcs: ; @echo $(SRCS)' print-srcs)
  cmd_of() {  # the Makefile's compile line for $1, without dependency output, -c and -o
    make -n -C "$csrc" -W "$1" "build/${1%.hip}.o" | grep -m1 -- " -c $1" |
      sed -e 's/ -MMD -MP//' -e "s/ -c $1.*//"
  }
  for f in $srcs; do
    echo "cd $csrc && $(cmd_of "$f") --cuda-device-only -fuse-cuid=none -S $f -o $out/${f%.hip}.s"
  done
  while read -r f name extra; do
    echo "cd $csrc && $(cmd_of "$f") $extra --cuda-device-only -fuse-cuid=none -S $f -o $out/${f%.hip}.$name.s"
  done <<< "$VARIANTS"
}

{ emit "$A" "$WORK/a"; emit "$B" "$WORK/b"; } > "$WORK/cmds"
xargs -P "$JOBS" -d '\n' -n 1 bash -c < "$WORK/cmds" || { echo "a compile failed (see above)"; exit 2; }

rc=0
for s in "$WORK"/a/*.s; do
  n=$(basename "$s")
  if cmp -s "$s" "$WORK/b/$n"; then echo "identical  $n"; else echo "DIFFERENT  $n"; rc=1; fi
done
echo "outputs in $WORK"
exit $rc
