#!/bin/bash
# sha256 of the gfx950 machine code (.text of the device code object) inside
# each decode object of a build directory (name, bytes, digest): two builds
# whose lines agree run the same default kernels.
#   tools/text_sha.sh ctc-beam-search-op_amd/csrc/build [gfx950]      (and .../build/st: the stream builds)
set -euo pipefail
dir=${1:?build directory}
arch=${2:-gfx950}
llvm=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for o in "$dir"/ctcx_decode.*.o "$dir"/ctcx_decode_gs.o "$dir"/ctcx_stable.o "$dir"/ctcx_stream_dense.o "$dir"/ctcx_times.o "$dir"/ctcx_skip.o "$dir"/ctcx_scores.o "$dir"/ctcx_stream_store.o; do
  [ -e "$o" ] || continue   # (build/st has the decode objects only; older builds lack the later units)
  n=$(basename "$o")
  "$llvm"/llvm-objcopy -O binary --only-section=.hip_fatbin "$o" "$tmp/fat.bin"
  # (an object without device code, such as build/st's dispatcher part 14, has no bundle)
  if ! "$llvm"/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--"$arch" \
    --input="$tmp/fat.bin" --output="$tmp/dev.co" --unbundle 2>/dev/null; then
    printf '%s - no-%s-code\n' "$n" "$arch"
    continue
  fi
  "$llvm"/llvm-objcopy -O binary --only-section=.text "$tmp/dev.co" "$tmp/text.bin"
  printf '%s %s %s\n' "$n" "$(stat -c %s "$tmp/text.bin")" "$(sha256sum "$tmp/text.bin" | cut -d" " -f1)"
done | sort -V
