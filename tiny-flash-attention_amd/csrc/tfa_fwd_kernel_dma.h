// tfa_fwd_kernel_dma.h — the forward tile loop with K/V tiles brought into LDS by LDS-DMA
// (`buffer_load_dwordx4 ... lds`, 1 KiB per wave-instruction) instead of global->VGPR->ds_write.
//
// Why: in the register-staged kernel (tfa_fwd_kernel.h) the staging costs ~13 % of the tile time
// (ablation: tools/ablate.py, NOSTAGE): 4 ds_write_b128 per thread per tile occupy the LDS store
// path and the single register set limits the global prefetch distance to one tile.  Here
//   * no staging VGPRs and no ds_write: the DMA writes LDS directly;
//   * three LDS tile buffers: tile j is computed while tile j+1 is landed/landing and tile j+2 is
//     in flight — two tiles of latency tolerance, waits are COUNTED (`s_waitcnt vmcnt(N)`, never a
//     drain while a younger tile is in flight) and barriers are raw `s_barrier`;
//   * an LDS-DMA piece lands lane-linear (wave-uniform base + lane*16), so the K chunk swizzle and
//     the V sub-tile order are applied to the per-lane SOURCE address; the LDS images are exactly
//     those of tfa_fwd_kernel.h (same fragment reads).
// Out-of-range rows still read as zeros (buffer descriptor bounds check), so ragged N is unchanged.
#pragma once
#include "tfa_fwd_kernel.h"
#include "tfa_acc_regs.h"
#include <type_traits>

namespace tfa {

// One LDS-DMA piece: every lane fetches 16 bytes at (descriptor base + voffset) and the wave's
// 1 KiB lands at LDS byte address lds_addr + lane*16 (M0 = wave-uniform LDS address).
// Inline asm on purpose: given the builtin, hipcc (ROCm 7.2) orders every later ds_read that may
// alias behind the DMA with `s_waitcnt vmcnt(0)`, which drains the two-tile-deep pipeline each
// tile.  Nothing here has a VGPR destination; completion is tracked by the counted vmcnt waits in
// the tile loop.  `s_nop 4` covers "SALU wrote an SGPR of the descriptor / M0 -> VMEM reads it".
static __device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %2, %3, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory");
}

// lds_dma16 with the non-temporal hint: K/V bytes no other workgroup will ask for (decode: one query block per K/V head)
static __device__ __forceinline__ void lds_dma16_nt(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %2, %3, 0 offen nt lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory");
}

// LDS-DMA without saving/restoring M0 around it (2 SALU less per piece in the hot loop).  Safe only because nothing else
// in the kernels that call it (fwd_kernel_il, bwd_kernel) uses M0 (hipcc emits no M0 user here: LDS instructions need none on gfx9+, SGPR spills use immediate
// lane indices); tests/test_abi.py disassembles the library and fails if that ever changes.
static __device__ __forceinline__ void lds_dma16_m0(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"                                     // SALU write of M0 -> LDS-DMA reads it: 1 wait state
      "buffer_load_dwordx4 %1, %2, 0 offen lds"
      :
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory", "m0");
}

// The 4-byte form: one dword per lane, 256 contiguous bytes of LDS per wave-instruction (the backward's per-tile row statistics)
static __device__ __forceinline__ void lds_dma4_m0(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "buffer_load_dword %1, %2, 0 offen lds"
      :
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory", "m0");
}

// The same with the non-temporal hint: K/V bytes nobody else will ask for (decode: one workgroup per K/V head)
static __device__ __forceinline__ void lds_dma16_m0_nt(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen nt lds"
      :
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory", "m0");
}

// LDS-DMA through a descriptor computed just before (per-tile windows): a VMEM instruction reading an SGPR that SALU code
// wrote needs 5 wait states, and nothing pads the inside of an asm.
static __device__ __forceinline__ void lds_dma16_m0_fresh(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voffset) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen lds"
      :
      : "s"(lds_addr), "v"(voffset), "s"(rs)
      : "memory", "m0");
}

constexpr int VF_PERSIST = 2048;   // launch one workgroup per CU and walk the work items (else one item per workgroup)
constexpr int VF_2BUF = 4096;      // two LDS tile buffers (64 KiB at D=128): two 4-wave workgroups fit one CU
constexpr int VF_LDSEPI = 16384;   // epilogue: transpose O through LDS and store whole rows (16-byte coalesced stores)
constexpr int VF_DMA_NT = 1 << 27;   // K/V tiles streamed with the non-temporal hint (decode over a K/V cache larger than the memory-side cache)
constexpr int VF_PRIO = 1024;   // s_setprio(1) around the MFMA clusters (experiment, tests/tools/ab.py)
constexpr int VF_KVCACHE = 1 << 28;  // attention over a K/V cache (tfa_fwd_kvcache): every sequence's length is read on the device, the key chunks are cut from it,
                                     // K/V tiles may come through a block table (fwd_kernel_dma_kvc below; its arguments: KvcArgs)

// Arguments of the KV-cache form: KArgs as tfa_fwd_splitkv fills them, plus what only this form reads.  A struct of its own — KArgs has no room for two pointers, a
// stride and a page size, and it keeps its size and layout (asserted in tfa_fwd_kernel.h), so no existing kernel's argument block moves.
// In this form Nk is unused (the length comes from seqlens), ks_b / vs_b are the PAGE strides when block_table is set, and nsplit / chunk: nsplit only.
struct KvcArgs : KArgs {
  const int* seqlens;       // device int32, B entries: sequence b holds seqlens[b] + n_new keys, clamped into [0, capacity] by every work item
  const int* block_table;   // device int32 (B, max_blocks) by bt_stride, or nullptr: contiguous cache
  long long bt_stride;
  int n_new;                // keys appended in front of this launch (tfa_kvcache_append)
  int capacity;             // keys a sequence can hold
  int num_pages;            // paged: block-table entries are clamped into [0, num_pages)
  int nq_pos;               // query rows per sequence for the causal shift len_b - nq_pos (Nq of the caller's problem)
  FastDiv fd_nsplit;        // len / nsplit
  FastDiv fd_tpp;           // tile / (page_size / 64)
  int tpp;                  // 64-key tiles per page
  int pad_;
};

// The e4m3 form of the KV-cache form (tfa_fwd_kvcache_fp8): k_cache / v_cache hold OCP e4m3fn bytes with one fp32 descale per (sequence, K/V head).  The tile loop is
// the 16-bit one: a tile's LDS-DMA is replaced by register staging — every lane loads the 8 source bytes behind the 16 LDS bytes its DMA piece would have filled
// (same descriptors, same extents, now in bytes of 1-byte elements: rows behind the length still arrive as zeros, and 0x00 decodes to +0), decodes them to T (exact:
// every finite e4m3 value is a bf16 and an f16) and writes them to that LDS address.  K swizzle, V layout, fragment reads, MFMAs, softmax and epilogue see what they see
// in the 16-bit form; each cache element is decoded once.  k_descale is folded into the score scale, v_descale multiplied into O in fp32 in the epilogue.
constexpr int VF_KV_E4M3 = 1 << 29;
struct Kvc8Args : KvcArgs {
  const float* k_descale;   // device fp32 by (kd_b, kd_h) elements, or nullptr = 1.0; indexed by (sequence, K/V head), paged or not
  const float* v_descale;
  long long kd_b, kd_h, vd_b, vd_h;
};
template <bool KV8>
struct Kvc8View {
  template <typename A> static __device__ __forceinline__ const Kvc8Args& of(const A& a) { return a; }
};
// The packed form of the KV-cache form (tfa_fwd_kvcache_pack, TFA_PACK_GQA_ON with Nq > 1): the Nq * G rows (position t, head g) of the G = H / Hk query heads that share
// K/V head hk are rows of ONE problem over sequence b's keys, position-major — row = t * G + g — so that the last visible key still grows with the row index and the
// causal tile bounds of the body (kv_end, wave_last_tile, need_mask, the heavy / light pairing) hold with t = row / G in the place of the row.  In such a launch KArgs
// describes the PACKED problem: H = Hk, Nq = Nq * G rows, nmb / nwork / nbh from them, qs_h / os_h the stride of a whole group of G heads, q_bytes / o_bytes the extent
// of a group's rows; KvcArgs::nq_pos stays the caller's Nq.  Q rows are addressed by two strides (t * qs_n + g * q_hs), O and LSE are written to the caller's
// (b, h, t) addresses, rows at or beyond Nq * G are pointed at TFA_OOB.  The arguments ride BEHIND the form's struct, not inside KvcArgs: Kvc8Args derives from
// it, and a KvcArgs that grows moves the descales' kernel-argument offsets — the unpacked e4m3 kernels would no longer compile to the instructions they had.
template <typename Base>
struct KvcPacked : Base {
  int pk_g;                 // G = H / Hk, 2..128
  FastDiv pk_fd_g;          // row / G
  int pk_pad_;
  long long q_hs, o_hs;     // ELEMENTS between consecutive query heads of q / out (out: of the fp32 partials when split)
};
template <typename A> struct KvcPack { static constexpr bool value = false; };
template <typename B> struct KvcPack<const KvcPacked<B>> { static constexpr bool value = true; };
template <bool PACK>
struct KvcPackView {
  template <typename A> static __device__ __forceinline__ const A& of(const A& a) { return a; }
};
// The varlen-q form of the KV-cache form (tfa_fwd_kvcache_varlen; FlashAttention-3's cu_seqlens_q / max_seqlen_q): q is packed (total_q, H, D) and sequence b owns the
// query rows [q0_b, q0_b + nq_b) — q0_b = clamp(cu[b], 0, total_q), nq_b = clamp(cu[b + 1] - cu[b], 0, min(max_q, total_q - q0_b)) — read and clamped by every work
// item itself, as scalar loads, the way it reads the sequence's length.  The launch carries nmb = ceil(max_q * G' / 128) query blocks per (sequence, head) (G' = G packed,
// 1 unpacked; KArgs::Nq = max_q * G' sizes it and is not read by this form's statements); a block with no row of its sequence (mb * 128 >= nq_b * G') issues no Q, K or V
// request and no store.  Everything that reads the launch-uniform Nq / nq_pos elsewhere takes nq_b here: the causal shift len_b - nq_b, the packed block's last valid
// row, row validity.  The Q descriptor starts at row q0_b and ends at the sequence's last row; O, LSE and the fp32 partials go to (h, q0_b + t) of (H, total_q, .)
// buffers — qs_b / os_b are 0, os_h / the LSE's head stride total_q rows — so tfa_merge runs unchanged over H * total_q rows.  The grid is sized by max_q, so
// one long prefill chunk in a batch of decode rows makes most work items empty; each empty item costs its scalar loads and an exit (KvcSched below removes them).
// The arguments ride BEHIND the form's struct (KvcArgs, Kvc8Args or their KvcPacked<>), for KvcPacked's reason: no existing kernel's argument block moves.
// G = 1 (MHA) is served by the unpacked instantiations (KvcPacked::pk_g is 2..128): that is why both exist.
template <typename Base>
struct KvcVarlenQ : Base {
  using vq_base = Base;
  const int* vq_cu;         // device int32, B + 1 entries
  int vq_max_q;             // max_seqlen_q: the most rows a sequence brings
  int vq_total_q;           // rows of q / out / lse
};
template <typename B> struct KvcPack<const KvcVarlenQ<B>> : KvcPack<const B> {};
template <typename A> struct KvcVq { static constexpr bool value = false; };
template <typename B> struct KvcVq<const KvcVarlenQ<B>> { static constexpr bool value = true; };
template <bool VQ>
struct KvcVqView {
  template <typename A> static __device__ __forceinline__ const A& of(const A& a) { return a; }
};
// The scheduled form of the varlen-q form (tfa_fwd_kvcache_varlen_sched; FlashAttention-3's scheduler_metadata): the launch carries heads * bound work items instead of
// B * heads * ceil(max_q * G' / 128) — bound = the host's upper limit of the batch's non-empty items — and work item `si` of a head takes its (sequence, item of that
// sequence) from row si of a list that tfa_kvcache_varlen_schedule built on the device: int32 metadata, SCHED_HDR header words (n_items first), then n_items rows
// (b, wi), 8 bytes each, one scalar load.  KArgs::nbh = heads and nwork = bound feed the item decomposition (the per-XCD head grouping included) unchanged.
// The list is a HINT, verified against what the kernel already trusts: n_items is clamped into [0, bound], b into [0, B), nq_b / the block count nb_b are
// recomputed from cu_seqlens_q as in the varlen-q form, and a wi outside the sequence's own items is an empty item — so stale, foreign or random metadata
// misplaces or drops work, it never moves an access outside the tensors.  A causal item is the heavy / light pair (nb_b - 1 - wi, wi) of the SEQUENCE's blocks
// (the varlen-q form pairs on the launch-level count).  An index at or beyond n_items exits in front of its first request.
// The arguments ride BEHIND KvcVarlenQ<>, for KvcPacked's reason: no existing kernel's argument block moves.
constexpr int SCHED_HDR = 8;     // header words of the metadata: n_items, B, G', causal, max_seqlen_q, total_q, bound, 0
template <typename Base>
struct KvcSched : Base {
  const int* sc_meta;       // device int32, SCHED_HDR + 2 * sc_bound entries, 8-byte aligned
  int sc_bound;             // item rows the buffer holds = KArgs::nwork
  int sc_pad_;
};
template <typename B> struct KvcPack<const KvcSched<B>> : KvcPack<const B> {};
template <typename B> struct KvcVq<const KvcSched<B>> : KvcVq<const B> {};
template <typename A> struct KvcSc { static constexpr bool value = false; };
template <typename B> struct KvcSc<const KvcSched<B>> { static constexpr bool value = true; };
template <bool SCHED>
struct KvcScView {
  template <typename A> static __device__ __forceinline__ const A& of(const A& a) { return a; }
};
// The windowed form of the KV-cache form (tfa_fwd_kvcache_window; the model configs' sliding_window, FlashAttention's window_size = (left, 0)): on the causal template,
// key j is visible to the row at position t of sequence b iff t + shift_b - left <= j <= t + shift_b (and 0 <= j < len_b), shift_b = len_b - nq_b.  With
// lo_b = max(0, shift_b - left) the first key the sequence's first row sees and lo64_b = lo_b & ~63, the range cut into chunks is [lo64_b, len_b): no work item loads a
// block-table entry of a page that ends at or before lo64_b, or a K/V byte in front of it.  A query block starts at the first 64-key tile some row of it sees — its
// chunk is narrowed to start there in decode(), so the prefetch, the tile loop and the buffer rotation count from it — and a wave skips the tiles in front of its
// first row's window as it skips those behind its last row's diagonal.  Keys of a visited tile left of a row's window are masked to -inf (they must be finite:
// P = 0 times a NaN V row is NaN).  The one argument rides BEHIND the form's struct — any of the twelve above — for KvcPacked's reason.
template <typename Base>
struct KvcWindow : Base {
  using win_base = Base;
  int win_left;             // keys a row sees in front of its own: w - 1 >= 0 (the host clamps it to the capacity)
  int win_pad_;
};
template <typename B> struct KvcPack<const KvcWindow<B>> : KvcPack<const B> {};
template <typename B> struct KvcVq<const KvcWindow<B>> : KvcVq<const B> {};
template <typename B> struct KvcSc<const KvcWindow<B>> : KvcSc<const B> {};
template <typename A> struct KvcWin { static constexpr bool value = false; };
template <typename B> struct KvcWin<const KvcWindow<B>> { static constexpr bool value = true; };
template <bool WIN>
struct KvcWinView {
  template <typename A> static __device__ __forceinline__ const A& of(const A& a) { return a; }
};
// The tree form of the KV-cache form (tfa_fwd_kvcache_tree; the verification step of a speculative token tree): on the causal template, with s = j - shift_b the
// index of key j among the step's new keys, key j is visible to the row at position t iff the causal rule admits it and (s < 0 or s >= 64 or bit s of the row's
// 64-bit word is set).  The word of row t is tree[b * tree_bs + t * tree_rs] (varlen-q: tree[(q0_b + t) * tree_rs]), loaded once per query block by the lane that
// owns the row (packed: t = row / G) — two dwords, kept in two VGPRs; a row outside the sequence takes all ones and loads nothing.  In the body's coordinates
// shift_b is Blk::shift, which decode() has already reduced by the chunk's first key: the new keys are [shift, shift + 64) in every chunk of every split, and
// nothing is carried across a chunk seam.  The mask removes no tile: chunks, tile bounds, grid and workspace are the underlying form's.  Only the (at most two)
// tiles that meet [shift, shift + 64) take the masked body on the mask's account.  Masked new keys are multiplied by P = 0, so they must be finite.  The
// arguments ride BEHIND the form's struct — any of the twelve above — for KvcPacked's reason.
template <typename Base>
struct KvcTree : Base {
  using tree_base = Base;
  const unsigned long long* tree;   // device, 8-byte words: bit s of a row's word = the row sees the s-th new key of its sequence
  long long tree_bs, tree_rs;       // words between sequences (unused in the varlen-q form) and between rows
};
template <typename B> struct KvcPack<const KvcTree<B>> : KvcPack<const B> {};
template <typename B> struct KvcVq<const KvcTree<B>> : KvcVq<const B> {};
template <typename B> struct KvcSc<const KvcTree<B>> : KvcSc<const B> {};
template <typename A> struct KvcTr { static constexpr bool value = false; };
template <typename B> struct KvcTr<const KvcTree<B>> { static constexpr bool value = true; };
template <bool TREE>
struct KvcTreeView {
  template <typename A> static __device__ __forceinline__ const A& of(const A& a) { return a; }
};
template <bool KV8, typename T> struct KvElem { using type = T; };
template <typename T> struct KvElem<true, T> { using type = unsigned char; };

// 8 e4m3 bytes of a K/V row (NT: with the non-temporal hint)
template <bool NT>
static __device__ __forceinline__ u32x2 kv8_load(__amdgpu_buffer_rsrc_t rs, int voffset) {
  return __builtin_amdgcn_raw_buffer_load_b64(rs, voffset, 0, NT ? 2 : 0);
}
// 8 e4m3 bytes -> 8 T (v_cvt_pk_f32_fp8: OCP e4m3fn on gfx950; the fp32 -> T conversion of an e4m3 value is exact)
template <typename T>
static __device__ __forceinline__ u32x4 kv8_decode(u32x2 s) {
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  typedef __attribute__((ext_vector_type(8))) T t8;
  t8 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)s[h], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)s[h], true);
    r[4 * h + 0] = (T)lo[0]; r[4 * h + 1] = (T)lo[1]; r[4 * h + 2] = (T)hi[0]; r[4 * h + 3] = (T)hi[1];
  }
  return __builtin_bit_cast(u32x4, r);
}

// The kernel walks a STREAM of query blocks: workgroup g takes work items g, g+G, g+2G, ... (G =
// gridDim.x; a causal work item is the pair {heavy block nmb-1-i, light block i}, so every item costs
// the same).  With G = number of CUs the launch is persistent: no workgroup turn-around between
// blocks (measured ~5.2k cycles each), and the next block's first two K/V tiles and its Q fragments are
// requested BEFORE the current block's epilogue, so its prologue latency hides behind the O stores.
// With G = number of items the same code degenerates to one item per workgroup.
// The kernel's body is tfa_fwd_kernel_dma_body.inc, included by its two entry points: fwd_kernel_dma (KArgs: every launch up to tfa_fwd_splitkv) and the KV-cache form
// fwd_kernel_dma_kvc (KvcArgs and the structs behind it, VF_KVCACHE) at the end of this file.  The KV-cache statements of the body sit in `if constexpr (KVC)` and read their arguments through
// KvcView<KVC>::of(p) — a dependent expression in fwd_kernel_dma, never instantiated there: its instantiations compile to the instructions they had before the form existed.
template <bool KVC>
struct KvcView {
  template <typename A> static __device__ __forceinline__ const KvcArgs& of(const A& a) { return a; }
};

template <typename T, int D, int NW, bool CAUSAL, bool F32OUT, int VF, int AB = 0>
// D = 256 (WIDE): the partial pass of tfa_fwd_splitkv at head dims above 128 — a K/V streaming kernel for decode-like shapes.  One wave
// per SIMD with the whole register file; O lives in the hand-owned AccVGPRs a[0:127] and Q is read from AccVGPRs (tfa_acc_regs.h:
// left to hipcc's own AccVGPR plan this instantiation spills 252 registers and streams 8-9 GB/s per workgroup); LDS fragments are
// read a group ahead of the asm MFMAs.
__global__ __launch_bounds__(NW * 64, D > 128 ? 1 : 2) void fwd_kernel_dma(const KArgs p) {
#include "tfa_fwd_kernel_dma_body.inc"
}

// The KV-cache form (tfa_fwd_kvcache and every entry point behind it): the split-KV instantiation's tile loop — four waves, two LDS buffers — with the lengths, the
// chunks and the pages formed on the device.  ONE entry point for every form: Args is any of the argument structs above (tfa_launch.h: TFA_KVC_FORMS names them) and
// the body reads what the form adds through the traits beside each struct; the e4m3 cache side is the Args' own (Kvc8Args among its bases; T is then the type of q,
// out and of the decoded tiles).  NT: K/V streamed with the non-temporal hint (caches beyond the memory-side cache, every byte read by one workgroup — the host
// decides).  The windowed and tree forms are instantiated causal and without the hint only (tfa_kvc_inst.inc)
template <typename T, int D, bool CAUSAL, bool F32OUT, bool NT, typename Args>
__global__ __launch_bounds__(256, 2) void fwd_kernel_dma_kvc(const Args p) {
  constexpr int NW = 4, AB = 0, VF = VF_PAIR | VF_2BUF | VF_KVCACHE | (std::is_base_of<Kvc8Args, Args>::value ? VF_KV_E4M3 : 0) | (NT ? VF_DMA_NT : 0);
#include "tfa_fwd_kernel_dma_body.inc"
}

}  // namespace tfa
