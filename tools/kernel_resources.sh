#!/bin/bash
# Register / scratch / spill figures of every kernel in object files built by the Makefile (default: every object of lib/obj).
# usage: tools/kernel_resources.sh [sparksmithwaterman_amd/lib/obj/swmi_tfused.o ...]
set -e
[ $# -gt 0 ] || set -- "$(dirname "$0")"/../sparksmithwaterman_amd/lib/obj/*.o
T=$(mktemp -d)
LLVM=/opt/rocm/lib/llvm/bin
echo "kernel scratch_bytes sgprs sgpr_spills vgprs vgpr_spills"
for OBJ in "$@"; do
    $LLVM/llvm-objcopy --dump-section .hip_fatbin=$T/fat.bin "$OBJ" 2>/dev/null || continue      # (an object without device code)
    $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/fat.bin --output=$T/k.co --unbundle
    $LLVM/llvm-readelf --notes $T/k.co | grep -E "\.name:|\.vgpr_count|\.sgpr_count|private_segment_fixed_size|spill_count" | paste - - - - - - | awk '{print $2, $4, $6, $8, $10, $12}'
done
rm -rf $T
