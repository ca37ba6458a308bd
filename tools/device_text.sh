#!/bin/bash
# SHA-256 of the gfx950 device code of one source (no GPU needed):  tools/device_text.sh msm [flags]     (or a path to the source)
# Compiles the device side with the build's own flags, unbundles the code object and hashes the bytes of .text and .rodata.  A change
# that only moves text between files leaves both hashes as they were; symbol names and notes are not hashed.
set -e -o pipefail
src=$1; [ -f "$src" ] || src=dv-pari_amd/csrc/$1.hip; [ -f "$src" ] || src=dv-pari_amd/csrc/$1.cpp
llvm=/opt/rocm/llvm/bin; tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -c -x hip "$src" --cuda-device-only -o "$tmp/dev.bundle" \
  -Wno-pass-failed -Wno-int-to-pointer-cast $2
$llvm/clang-offload-bundler --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input="$tmp/dev.bundle" --output="$tmp/dev.co"
for sec in .text .rodata; do
  $llvm/llvm-objcopy -O binary --only-section=$sec "$tmp/dev.co" "$tmp/sec.bin"
  echo "$(basename "$src") $sec $(stat -c %s "$tmp/sec.bin") bytes sha256 $(sha256sum "$tmp/sec.bin" | cut -d' ' -f1)"
done
