#!/bin/bash
# Instruction-level comparison of the device code of two builds of the library (CPU only): for every instantiation unit present in BOTH object
# directories, the gfx950 code object is taken out of the object's .hip_fatbin, disassembled with llvm-objdump -d, and the two listings are diffed
# with the address / encoding comments stripped (a unit's code can sit at another offset of its code object when its symbol table changed size).
# Kernel names are normalised for one kind of rename only: the backward kernels' trailing `bool VARLEN = false` and `bool LOCAL = false` template
# arguments (tfa_bwd_kernel.h, tfa_bwd_kv_kernel.h) add `Lb0E` to their mangled names — every trailing `Lb0E` of a backward kernel's name is dropped.  No output = every kernel of the old build compiles to the same instructions.
#   usage: tools/isa_diff.sh OLD_OBJDIR NEW_OBJDIR      (e.g. a build of the parent commit's tree and tiny-flash-attention_amd/build)
set -eu
old=$1 new=$2
B=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
dis() {   # object -> normalised listing of its gfx950 code object
  "$B/llvm-objcopy" --dump-section=.hip_fatbin="$tmp/f" "$1" /dev/null 2>/dev/null || return 0
  "$B/clang-offload-bundler" --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$tmp/f" --output="$tmp/d" --unbundle
  "$B/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$tmp/d" | tail -n +4 | sed -E 's@ *//.*@@; :a; s/(bwd_(kv_)?kernelI[^ >]*)Lb0E(EEvNS_5BArgsE)/\1\3/; ta'
}
for o in "$old"/*.o; do
  n=$(basename "$o")
  [ -f "$new/$n" ] || continue
  dis "$o" > "$tmp/a"
  dis "$new/$n" > "$tmp/b"
  diff "$tmp/a" "$tmp/b" | sed "s@^@$n: @" || true
done
