#!/bin/bash
# Compare the gfx950 device code of two source trees, kernel by kernel (no GPU needed).
# tools/asm_cmp.sh TREE_A TREE_B [WORKDIR]
# Every csrc/*.hip of both trees is compiled device-only with the flags of parsy_bench_amd/build.py (ASM_CMP_FLAGS adds
# more, e.g. a -D of a diagnostic build); tools/asm_cmp.py then compares, per kernel symbol and wherever the kernel lives in
# its tree, the function body, the kernel descriptor and the metadata note (VGPRs, AGPRs, LDS, scratch, argument layout),
# and lists the kernels only one tree has, those that differ (first diff lines) and the other device symbols of each tree.
# Exit status 0 only when every kernel of either tree is in both and identical and the other device symbols are the same.
set -u
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); W=${3:-$(mktemp -d)}
export HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
mkdir -p "$W"
exec python3 "$(dirname "$0")/asm_cmp.py" "$A" "$B" "$W"
