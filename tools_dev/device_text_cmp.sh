#!/bin/bash
# Compares the gfx950 device code of two builds, file by file: extracts the code object from each object file of
# scouter_amd/lib/obj and compares its .text bytes.  A host-only change leaves every file identical.
#   tools_dev/device_text_cmp.sh <objdir of the other build> [<objdir of this build>]
LL=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
A=$1; B=${2:-$(dirname "$0")/../scouter_amd/lib/obj}
T=$(mktemp -d)
for o in "$B"/*.o; do
  b=$(basename "$o" .o)
  for side in a b; do
    src=$A/$b.o; [ $side = b ] && src=$B/$b.o
    $LL/llvm-objcopy -O binary --only-section=.hip_fatbin "$src" $T/$b.$side.fatbin 2>/dev/null &&
      $LL/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/$b.$side.fatbin --output=$T/$b.$side.co 2>/dev/null &&
      $LL/llvm-objcopy -O binary --only-section=.text $T/$b.$side.co $T/$b.$side.text
  done
  if [ ! -s $T/$b.b.text ]; then echo "$b: no device code"
  elif cmp -s $T/$b.a.text $T/$b.b.text; then echo "$b: .text identical ($(stat -c %s $T/$b.b.text) bytes)"
  else echo "$b: .text DIFFERS"; fi
done
rm -rf $T
