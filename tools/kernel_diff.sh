#!/bin/bash
# Compares the gfx950 kernels of two builds, kernel by kernel, whichever object each build put a kernel in: the check that a
# refactor which moves kernels between units left the device code alone.
# usage: tools/kernel_diff.sh OBJDIR_A OBJDIR_B        (two OBJ directories of the Makefile, e.g. lib/obj of two checkouts)
# Per kernel symbol found in either directory it prints `same` or `differs` (+ what: isa, meta, or the side that lacks it).
# Compared are the kernel's disassembly -- without addresses, raw bytes, `//` comments and the s_nop padding after its last
# instruction -- and its metadata note: VGPRs, SGPRs, both spill counts, scratch, static LDS and kernarg bytes.
# Exit status 1 if any kernel differs or is missing on one side.
set -e -o pipefail
[ $# -eq 2 ] || { echo "usage: $0 OBJDIR_A OBJDIR_B" >&2; exit 2; }
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT

# extract SIDE DIR: $T/SIDE/KERNEL.isa and $T/SIDE/KERNEL.meta for every kernel of every object of DIR
extract() {
    local side=$1 dir=$2 o b co name rest
    mkdir -p "$T/$side"
    for o in "$dir"/*.o; do
        [ -e "$o" ] || { echo "$0: no objects in $dir" >&2; exit 2; }
        b=$(basename "$o" .o)
        co=$T/$side/$b.co
        $LLVM/llvm-objcopy --dump-section .hip_fatbin="$T/$side/$b.fat" "$o" 2>/dev/null || continue      # (no device code)
        $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$T/$side/$b.fat" --output="$co" --unbundle
        [ -s "$co" ] || continue
        # the kernels of the metadata note: one line `name key=value ...` each (kernel-level keys only, not those of .args)
        $LLVM/llvm-readelf --notes "$co" | awk '
            function flush() { if (name != "") print name, "vgprs=" v[".vgpr_count"], "sgprs=" v[".sgpr_count"],
                                   "sgpr_spills=" v[".sgpr_spill_count"], "vgpr_spills=" v[".vgpr_spill_count"],
                                   "scratch=" v[".private_segment_fixed_size"], "lds=" v[".group_segment_fixed_size"],
                                   "kernarg=" v[".kernarg_segment_size"]; name = ""; delete v }
            /^ *amdhsa.kernels:/ { inside = 1; next }
            inside && /^ *amdhsa\./ { flush(); inside = 0 }
            inside && /^  - \./ { flush(); sub(/^  - /, "    ") }
            inside && /^    \.[a-z_]+: / { key = $1; sub(/:$/, "", key); if (key == ".name") name = $2; else v[key] = $2 }
            END { flush() }' > "$T/$side/$b.kernels"
        while read -r name rest; do
            echo "$rest" > "$T/$side/$name.meta"
            $LLVM/llvm-objdump -d --no-show-raw-insn --disassemble-symbols="$name" "$co" |
                sed -e 's|//.*$||' -e 's/[[:space:]]*$//' | grep -E '^[[:space:]]+[a-z]' |
                awk '{ l[NR] = $0 } END { n = NR; while (n > 0 && l[n] ~ /^[[:space:]]*(s_nop|s_code_end)/) n--; for (i = 1; i <= n; i++) print l[i] }' \
                > "$T/$side/$name.isa"
        done < "$T/$side/$b.kernels"
    done
}
extract a "$1"
extract b "$2"

status=0
for name in $( (cd "$T/a" && ls *.meta 2>/dev/null; cd "$T/b" && ls *.meta 2>/dev/null) | sed 's/\.meta$//' | sort -u); do
    what=
    if [ ! -e "$T/a/$name.meta" ]; then what="missing in $1"
    elif [ ! -e "$T/b/$name.meta" ]; then what="missing in $2"
    else
        [ -s "$T/a/$name.isa" ] && cmp -s "$T/a/$name.isa" "$T/b/$name.isa" || what="isa"
        cmp -s "$T/a/$name.meta" "$T/b/$name.meta" || what="${what:+$what, }meta: $(cat "$T/a/$name.meta") | $(cat "$T/b/$name.meta")"
    fi
    if [ -z "$what" ]; then echo "same     $name  ($(wc -l < "$T/a/$name.isa") instructions; $(cat "$T/a/$name.meta"))"
    else echo "differs  $name  ($what)"; status=1; fi
done
exit $status
