#!/bin/bash
# Instruction-level comparison of the device code of two builds of the library (CPU only): for every instantiation unit present in BOTH object
# directories, the gfx950 code object is taken out of the object's .hip_fatbin, disassembled with llvm-objdump -d, and the two listings are diffed
# with the address / encoding comments stripped (a unit's code can sit at another offset of its code object when its symbol table changed size).
# Behind the listing come the kernels' launch resources from the code object's notes (llvm-readelf --notes): .kernarg_segment_size, .vgpr_count,
# .sgpr_count, .agpr_count, the LDS size and the scratch size of every kernel, compared the same way.
# Kernel names are normalised for two renames only:
#   * the backward kernels' trailing `bool VARLEN = false` and `bool LOCAL = false` template arguments (tfa_bwd_kernel.h, tfa_bwd_kv_kernel.h) add `Lb0E`
#     to their mangled names — every trailing `Lb0E` of a backward kernel's name is dropped;
#   * the K/V-cache kernels' one entry point fwd_kernel_dma_kvc<T, D, CAUSAL, F32OUT, NT, Args> stands where fwd_kernel_dma_kvc / _kvc8 / _kvc_pack / _kvc8_pack /
#     _kvc_vq <T, D, CAUSAL, F32OUT, NT[, Args]> and _kvc_win / _kvc_tree <T, D, F32OUT, Args> (causal, no non-temporal twin) stood: every one of them is written
#     kvc<T,D,cCAUSAL,oF32OUT,nNT> — a unit holds the kernels of ONE argument struct, so that names each of its kernels.
# No output = every kernel of the old build compiles to the same instructions with the same resources.
#   usage: tools/isa_diff.sh OLD_OBJDIR NEW_OBJDIR      (e.g. a build of the parent commit's tree and tiny-flash-attention_amd/build)
set -eu
old=$1 new=$2
B=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
names() {  # the kernel-name normalisation
  sed -E 's@ *//.*@@; :a; s/(bwd_(kv_)?kernelI[^ >]*)Lb0E(EEvNS_5BArgsE)/\1\3/; ta
          s/_ZN3tfa[0-9]+fwd_kernel_dma_kvc(8|_pack|8_pack|_vq)?I(DF16b|DF16_)Li([0-9]+)ELb([01])ELb([01])ELb([01])E[A-Za-z0-9_]*/kvc<\2,\3,c\4,o\5,n\6>/g
          s/_ZN3tfa[0-9]+fwd_kernel_dma_kvc_(win|tree)I(DF16b|DF16_)Li([0-9]+)ELb([01])E[A-Za-z0-9_]*/kvc<\2,\3,c1,o\4,n0>/g'
}
dis() {   # object -> normalised listing of its gfx950 code object, then its kernels' resources
  "$B/llvm-objcopy" --dump-section=.hip_fatbin="$tmp/f" "$1" /dev/null 2>/dev/null || return 0
  "$B/clang-offload-bundler" --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$tmp/f" --output="$tmp/d" --unbundle
  "$B/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$tmp/d" | tail -n +4 | names
  "$B/llvm-readelf" --notes "$tmp/d" | grep -E '^ +(- )?\.(name|kernarg_segment_size|vgpr_count|sgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size):' | names
}
for o in "$old"/*.o; do
  n=$(basename "$o")
  [ -f "$new/$n" ] || continue
  dis "$o" > "$tmp/a"
  dis "$new/$n" > "$tmp/b"
  diff "$tmp/a" "$tmp/b" | sed "s@^@$n: @" || true
done
