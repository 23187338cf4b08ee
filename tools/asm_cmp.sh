#!/bin/bash
# Compare the gfx950 device assembly of every HIP source between two source trees (no GPU needed).
# tools/asm_cmp.sh TREE_A TREE_B [WORKDIR]
# Each csrc/*.hip of both trees is compiled device-only with the flags of parsy_bench_amd/build.py; lines that hold the
# source-text hash (__hip_cuid_), .file or .ident are dropped; per file it prints "identical" or the diff's first lines.
# The assembly carries the kernel descriptors and metadata notes too (VGPRs, AGPRs, LDS, scratch, argument layout).
# A source that one tree does not have counts as an empty one there (a file of host code alone compares equal to it).
# Exit status 0 only when every file is identical.
set -u
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); W=${3:-$(mktemp -d)}
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
FILES="chol_kernels trsv_kernels trsv_sub_kernels selinv_kernels refine_kernels grad_kernels cond_kernels apply_kernels updown_kernels rowmod_kernels eigs_kernels executor capi_exec capi_hostcalls mg"
mkdir -p "$W/a" "$W/b"
: > "$W/empty.hip"
asm() {  # tree, side, file
  local src=parsy_bench_amd/csrc/$3.hip
  [ -e "$1/$src" ] || { src="$W/empty.hip"; echo "$3.hip: not in $1" > "$W/$2/$3.absent"; }
  ( cd "$1" && "$HIPCC" --offload-arch=gfx950 -munsafe-fp-atomics -O3 -fPIC -std=c++17 -Wall -Wno-unused-function \
      -I include --cuda-device-only -S "$src" -o "$W/$2/$3.raw.s" 2> "$W/$2/$3.warn" ) || return 1
  grep -v -e '__hip_cuid_' -e '\.file' -e '\.ident' "$W/$2/$3.raw.s" > "$W/$2/$3.s"
}
for f in $FILES; do asm "$A" a $f & asm "$B" b $f & done
wait
rc=0
for f in $FILES; do
  if [ ! -s "$W/a/$f.s" ] || [ ! -s "$W/b/$f.s" ]; then echo "$f.hip: compile failed"; cat "$W/a/$f.warn" "$W/b/$f.warn" | head -20; rc=1; continue; fi
  if diff "$W/a/$f.s" "$W/b/$f.s" > "$W/$f.diff"; then
    echo "$f.hip: identical ($(wc -l < "$W/b/$f.s") lines of assembly, $(grep -c '^\s*\.amdhsa_kernel ' "$W/b/$f.s") kernels)"
  else
    echo "$f.hip: DIFFERENT ($(wc -l < "$W/$f.diff") diff lines)"; head -20 "$W/$f.diff"; rc=1
  fi
  cat "$W/a/$f.absent" "$W/b/$f.absent" 2>/dev/null | sed 's/^/  /'
  wa=$(grep -c 'warning:' "$W/a/$f.warn"); wb=$(grep -c 'warning:' "$W/b/$f.warn")
  echo "  warnings: $wa -> $wb"
done
exit $rc
