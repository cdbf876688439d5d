/*
 * tfa.h — C ABI of the MI355X (gfx950) FlashAttention-2 forward path.
 *
 * This is the drop-in boundary for the ONE hot path of 66RING/tiny-flash-attention:
 * the fused  S = scale * Q K^T  ->  online softmax  ->  O = P V  forward tile loop.
 * Everything here is `extern "C"`, plain pointers and sizes; no torch types.
 * Pointers are DEVICE pointers (HBM) unless stated otherwise.  The library never
 * allocates or frees device memory and keeps no state between calls except the
 * PER-THREAD debug knobs tfa_set_variant() / tfa_debug_set_trace() (thread-local: a thread
 * that forces a variant does not change what other threads' calls run).
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *
 *   tfa_fwd_bhnd      <- flash_attention_v2_cutlass(q,k,v,is_causal,softmax_scale) -> {out, lse}
 *                        flash_attention_cutlass/csrc/flash_attention.cu:741-772
 *                        (declared flash_attention_cutlass/include/attention_api.h:10-11,
 *                         bound   flash_attention_cutlass/csrc/attention_api.cpp:6-10)
 *                     <- flash_attention_v2_cuda(q,k,v) -> out      [scale=1/sqrt(D), non causal]
 *                        flash_attention_cuda/csrc/flash_attention.cu:375-424
 *                     <- _kernels.flash_attn(q,k,v,is_causal,softmax_scale) -> out   [CPU sibling]
 *                        flash_attention_c/csrc/attn.cpp:237-262
 *   tfa_fwd           <- set_params_fprop + run_flash_attn_cutlass (strided / GQA / Nq!=Nk general form)
 *                        flash_attention_cutlass/csrc/flash_attention.cu:320-361, 731-739
 *                        flash_attention_cutlass/csrc/flash.h:6-59   (Flash_fwd_params)
 *                        flash_attention_c/csrc/attn.cpp:171-203     (strided params, causal offset)
 *   tfa_strerror      <- CUDA_ERROR_CHECK / TORCH_CHECK text
 *                        flash_attention_cutlass/include/attention_api.cuh:12-29
 *   tfa_merge, tfa_fwd_splitkv (partial results over key chunks + merge)
 *                     <- the v1 block-merge rule  flash_attention_py/tiny_flash_attn.py:63-68, README_zh.md:104-125
 *   tfa_bwd           <- no reference entry: the reference only SAVES softmax_lse for a backward
 *                        flash_attention_cutlass/csrc/flash_attention.cu:353-354, 614-623
 *
 * Semantics (identical to the reference; see oracle/ for the CPU restatement):
 *   S[i,j]  = softmax_scale * sum_d q[i,d] k[j,d]            (16-bit products, fp32 accumulate)
 *   causal:   S[i,j] = -inf for j > i + (Nk - Nq)            (attn.cpp:122-124)
 *   m_i = max_j S ; P = exp(S - m_i) ; l_i = sum_j P         (fp32)
 *   O[i,:]  = (sum_j round16(P[i,j]) v[j,:]) / l_i           (P rounded to the input dtype before PV,
 *                                                             flash_attention.cu:601; l sums unrounded P)
 *   O -> rounded to the input dtype (RNE), or left fp32 when out_dtype == TFA_F32
 *   LSE_i   = m_i + ln(l_i)   (natural log, scale included)  (flash_attention.cu:623)
 *   empty row (no visible key): O = 0, LSE = +inf            (flash_attention.cu:620-623)
 * Rounding points (which row reference m' stands in P = exp(S - m') when P is rounded to 16 bits; O and LSE are the same numbers mathematically
 * under every rule, and every rule holds the reference's atol 1e-2 and the rigorous bound |O - O_fp64| <= 2^-8 * A (bf16) / 2^-11 * A (fp16),
 * A[i,d] = sum_j P[i,j] |v[j,d]| / l_i — tfa_fwd_rounding_rule says which one a call runs):
 *   TFA_RULE_EXACT_MAX   the exact running maximum, the reference's own rule (flash_attention.cu:263-316, main_torch_only.py:240-260): the flag
 *                        TFA_FWD_EXACT_MAX (element-wise rtol 1e-3 against the reference's tile loop), the split-KV kernel, fp32 tensors
 *   TFA_RULE_LAZY        a per-row reference that trails the running maximum by at most 2^8 (P <= 2^8; a wave of 32 rows re-bases together when
 *                        one of them outgrows it): fp16 on the default kernels, every special-case instantiation, head dims above 128
 *   TFA_RULE_FIRST_TILE  bf16 on the default kernels' main instantiations (round 6): m' = the row's maximum over its FIRST 64-key tile, kept for
 *                        the whole row — bf16 has fp32's exponent range, so no running maximum is needed for range, and the kernel forms none
 *                        (it tests the row SUMS instead: beyond 2^40 a wave re-bases by an exact power of two, which moves no result bit; a
 *                        single tile that lifts a row sum beyond 2^64 makes the workgroup redo that query block with TFA_RULE_LAZY).
 *                        Stated domain: |v| * Nk < 2^63 (beyond it P*v could overflow fp32 before a re-base; the lazy rule's own limit is 2^119).
 *
 * Error convention: every entry point returns 0 on success, a negative tfa_status on a
 * rejected argument (nothing was launched), or a positive hipError_t when the HIP runtime
 * reported an error on launch.  No entry point synchronises the device or calls exit()
 * (the reference does both, flash_attention.cu:767-769; callers already synchronise).
 */
#ifndef TFA_H_
#define TFA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFA_VERSION 111 /* 0.1.11 (still): + a device-built work list for the packed-q K/V-cache call — tfa_kvcache_varlen_schedule / _schedule_size / _schedule_plan build it from cu_seqlens_q in one launch, tfa_fwd_kvcache_varlen_sched / _sched_plan run heads * bound work items from it instead of B * heads * ceil(max_seqlen_q * G' / 128) (FlashAttention-3's get_scheduler_metadata / scheduler_metadata=; the scheduled form of the KV-cache kernel); new entry points and kernels only: every existing entry point, struct, kernel and result bit unchanged.  0.1.11 (still): + the packed append into an e4m3 cache and / or with q rotated in place in the same launch — tfa_kvcache_append_varlen_ex / _plan (struct tfa_append_q; tfa_kvcache_fp8 as in tfa_fwd_kvcache_fp8); new struct, entry points and kernels only: every existing entry point, struct, kernel and result bit unchanged.  0.1.11 (still): + packed ragged query rows over a K/V cache — tfa_fwd_kvcache_varlen and its _workspace / _plan / _suggest_splits companions (struct tfa_kvcache_varlen_q: cu_seqlens_q in device memory, max_seqlen_q, total_q; q packed (total_q, H, D), every sequence's rows read and clamped on the device: the varlen-q form of the KV-cache kernel, packed GQA rows by default); new struct, entry points and kernels only: every existing entry point, struct, kernel and result bit unchanged.  0.1.11 (still): + the GQA packing of the K/V-cache calls chosen by the caller — tfa_fwd_kvcache_pack and its _workspace / _plan / _suggest_splits companions (TFA_PACK_GQA_AUTO / ON / OFF; ON packs the query heads of a K/V head as position-major rows at any Nq: the packed form of the KV-cache kernel); new entry points and kernels only: every existing entry point, struct, kernel and result bit unchanged.  0.1.11 (still): + the serving step's parts around attention — tfa_rotary / tfa_rotary_plan (rotary embedding at device-side positions, one or two tensors a launch) and tfa_kvcache_append_varlen / _plan (packed new K/V rows into a paged or contiguous cache, K optionally rotated on the way in); new structs and kernels only: every existing entry point, struct, kernel and result bit unchanged.  0.1.11 (still): + a dense additive bias / mask — tfa_fwd_bias / tfa_bwd_bias and their _plan / _variant / _rounding_rule companions (struct tfa_attn_bias: a (B|1, H|1, Nq, Nk) tensor of q's dtype or fp32 in device memory, read by the kernels inside the tile loop; a third form of the fixed-length local kernels on the ALiBi hook); every existing entry point, kernel and result bit unchanged.  0.1.11 (still): + attention over a K/V cache — tfa_fwd_kvcache, its _workspace / _plan / _suggest_splits companions and tfa_kvcache_append (device-side cache_seqlens, paged K/V through a block table, in-place append; the KV-cache form of the LDS-DMA kernel); every existing entry point, kernel and result bit unchanged.  0.1.11 (still): + soft-capping — tfa_fwd_softcap / tfa_bwd_softcap, their varlen forms and _plan / _variant / _rounding_rule companions (softcap: a host float, tanh capping of the scaled scores in front of the ALiBi bias and the mask; slopes optional; a second form of the local kernels on the ALiBi hook); every existing entry point, kernel and result bit unchanged.  0.1.11 (still): + ALiBi — tfa_fwd_alibi / tfa_bwd_alibi, their varlen forms and _plan / _variant / _rounding_rule companions (alibi_slopes in device memory, a form of the local kernels); every existing entry point, kernel and result bit unchanged.  0.1.11: tfa_bwd at head dims up to 128 runs hand-scheduled tile loops in both launches; the dQ launch accumulates dP from -delta (gradient bits differ from 0.1.10, inside the same bounds); no interface change.  0.1.10: bf16 on the default kernels rounds P against the first key tile's row maximum (max-free tile loop; tfa_fwd_rounding_rule says which rule a call runs), the tile bodies behind the hand-scheduled loop are generated too, tfa_debug_mfma_ceiling returns TFA_ERR_SHAPE for bad sizes; 0.1.9: (b,h) slices of 2 GiB and more at head dims above 128 (windowed instantiations of the 256-wide forward and backward kernels; TFA_ERR_STRIDE before), tfa_debug_mfma_ceiling; 0.1.8: TFA_FWD_EXACT_MAX runs the il8 kernel's exact-max instantiation (variant 38) on grids that fill the chip; 0.1.7: tfa_bwd computes delta inside its dQ launch (tfa_debug_bwd_split bit 3 restores the separate launch), tfa_debug_set_trace is served by traced twins of the main kernels; 0.1.6: + fp32 q,k,v (TFA_F32 input: the correctness path behind the reference's fp32 fixtures), variant numbers are ids (tfa_variant_available), tfa_bwd_workspace_bytes is 0 wherever the workspace would be ignored; 0.1.5: + tfa_fwd_params::flags (TFA_FWD_EXACT_MAX), split-KV for head dims up to 256; 0.1.4: + tfa_fwd_suggest_splits, key-split kernels for small grids, split-KV / backward head dims multiples of 8; 0.1.3: forward head dims = every multiple of 8 up to 256; tfa_debug_set_flags; 0.1.2: + tfa_variant_available; debug knobs are per thread; 0.1.1: split-KV, tfa_merge, tfa_bwd */

/* element types */
enum tfa_dtype { TFA_F16 = 0, TFA_BF16 = 1,
                 TFA_F32 = 2 /* outputs of the 16-bit kernels; as the dtype of q,k,v: the fp32 correctness path (below) */ };

enum tfa_status {
  TFA_OK = 0,
  TFA_ERR_NULL = -1,          /* a required pointer is NULL */
  TFA_ERR_DTYPE = -2,         /* dtype not in {F16,BF16}; out_dtype not in {dtype,F32} */
  TFA_ERR_HEAD_DIM = -3,      /* forward, split-KV, backward: D not a multiple of 8 in [8,256]; merge: not a multiple of 4 in [4,256];
                               * TFA_FWD_EXACT_MAX: not a multiple of 8 in [8,128] */
  TFA_ERR_SHAPE = -4,         /* B,H,Hk,Nq,Nk <= 0 or H % Hk != 0 */
  TFA_ERR_STRIDE = -5,        /* a stride is negative, not 16-byte aligned, rows overlap, or 768 rows of a (b,h) slice span 2 GiB
                               * (tfa_fwd and tfa_bwd switch to per-block / per-tile descriptor windows when a slice is larger, ~6 % / ~3 %
                               * slower — at every head dim since 0.1.9; tfa_fwd_splitkv then runs one windowed launch per key chunk) */
  TFA_ERR_ALIGN = -6,         /* a base pointer is not 16-byte aligned */
  TFA_ERR_VARIANT = -7,       /* unknown kernel variant */
  TFA_ERR_SCALE = -8          /* softmax_scale is not finite or is <= 0; the _softcap entry points: softcap is not finite or is <= 0 */
};

/*
 * General problem descriptor.  Tensors are 4-D logical (B, H, N, D) with arbitrary
 * batch/head/row strides (in ELEMENTS) and unit stride along D, so both the reference's
 * contiguous (B,H,N,D) layout and the (B,N,H,D) layout of flash_attn_func are expressible.
 * K and V have Hk heads (Hk divides H; Hk == H for plain MHA; query head h reads kv head
 * h / (H/Hk), the grouping of flash_attention_c/csrc/archive_)/attn.cpp:61).
 */
typedef struct tfa_fwd_params {
  const void* q;  /* (B,H ,Nq,D) */
  const void* k;  /* (B,Hk,Nk,D) */
  const void* v;  /* (B,Hk,Nk,D) */
  void* out;      /* (B,H ,Nq,D) of out_dtype */
  float* lse;     /* (B,H,Nq) fp32 contiguous, or NULL to skip */
  int32_t B, H, Hk, Nq, Nk, D;
  int64_t q_stride[3];   /* batch, head, row (elements) */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];   /* in elements of out_dtype */
  float softmax_scale;
  int32_t is_causal;     /* bottom-right aligned when Nq != Nk */
  int32_t dtype;         /* tfa_dtype of q,k,v: TFA_F16 or TFA_BF16 (the MFMA kernels: everything this header describes), or TFA_F32 — fp32
                          * tensors, the dtype of the reference's own CPU fixtures (flash_attention_c/test.py:35-48) and of the float arm of
                          * flash_attention_cuda/csrc/flash_attention.cu:411: served by a correctness kernel with fp32 arithmetic end to end
                          * (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 rate; csrc/tfa_fwd_f32.hip), out_dtype must be TFA_F32, head dims =
                          * multiples of 4 up to 256, rows 16-byte aligned, flags 0; tfa_fwd only (no split-KV, no backward).  Meets the
                          * reference's fp32 results to 1e-5 (tests/test_f32_gpu.py). */
  int32_t out_dtype;     /* == dtype, or TFA_F32 (debug/parity: unrounded fp32 O; also the partial results of split-KV) */
  /* split-KV (SURVEY section 8(f) row 4): when k, v are the chunk [kv_offset, kv_offset + Nk) of a longer key
   * sequence of nk_total keys, the causal mask is taken against GLOBAL key positions: key kv_offset + j is
   * visible to row i iff kv_offset + j <= i + (nk_total - Nq).  out / lse are then PARTIAL results (rows that
   * see no key of the chunk: out = 0, lse = +inf) to be combined with tfa_merge.  Both 0 = the whole sequence. */
  int64_t kv_offset;
  int64_t nk_total;      /* 0 means kv_offset + Nk */
  int32_t flags;         /* TFA_FWD_* bits, 0 = default */
  int32_t reserved_;     /* must be 0 */
} tfa_fwd_params;

/* tfa_fwd_params::flags
 * TFA_FWD_EXACT_MAX: round P to 16 bits at the REFERENCE's points — every KV tile is exponentiated against the exact running
 *   row maximum, as flash_attention_cutlass/csrc/flash_attention.cu:263-316 and flash_attention_py/main_torch_only.py:240-260
 *   do — instead of the default kernels' own row reference (TFA_RULE_LAZY / TFA_RULE_FIRST_TILE above: same mathematics, O and LSE agree to
 *   the P-rounding bound, but the 16-bit roundings of P fall elsewhere).  Head dims up to 128, (b,h) slices below 2 GiB, no GQA row packing.  Where the
 *   default would run the il8 kernel (grids that fill the chip: the BASELINE configs 3, 4, 5) the flag runs that kernel's exact-max
 *   instantiation ("exact-il8", variant 38, round 5: the same issue-interleaved tile body; a tile in which some row of a wave saw a new
 *   maximum also multiplies O by exp2(old - new) behind its QK^T MFMAs) — 8-10 % slower than the default: bench.py quotes the pair in one line,
 *   `value` and `value_at_reference_rounding_points`; everywhere else the burst-structured LDS-DMA kernel (variant 17; 10-15 % slower than the default).  For callers
 *   that compare against the reference element by element (rtol 1e-3 with fp32 output).
 *
 * WHICH TOLERANCE EACH PATH GUARANTEES (stated and asserted in tests/test_parity_gpu.py; A[i,d] = sum_j P_ij |v_jd| is the
 * non-cancelling magnitude of an output element, eps16 = 2^-8 for bf16, 2^-11 for fp16):
 *   every path, 16-bit output vs the exact (fp64) result:      |d| <= 1e-2                 — the reference's own bar (test.py:87)
 *   every path, fp32 output vs the exact result:               |d| <= eps16 * A + 1e-6     — the rigorous bound of rounding P to 16 bits
 *   every path, LSE:                                           |d| <= 1e-4, +inf exactly where a row sees no key
 *   the KV-cache family (tfa_fwd_kvcache and its _fp8 / _pack / _varlen / _varlen_sched forms, any split count, behind either append),
 *   16-bit output vs the exact result:                         |d| <= eps16 * A + 1e-6 + half an ulp16 of the result — the fp32-output bound plus the ONE
 *                                                              rounding of O (partials and tfa_merge are fp32); A = v_descale * sum_j P_ij |dec v_jd|
 *   the KV-cache family, LSE (u = 2^-24, T = max_j scale * k_descale * sum_d |q_d| |dec k_jd|, n keys):
 *                                                              |d| <= u * ((D + 15) * T + 4 * ceil(n / 64) + 13) + 2^-22 * |lse|, merged over s parts
 *                                                              + u * (5 * s + 4) + u * |lse| — derived term by term from the kernel body and tfa_merge
 *                                                              (tests/kvcache_ref.py: lse_bound); both asserted element by element in
 *                                                              tests/test_kvcache_fwd_bounds_gpu.py, proved to fit and to bite in tests/test_kvcache_bounds_cpu.py
 *   the prefill forward family (tfa_fwd by kernel variant, its _local / _alibi / _softcap / _bias forms, tfa_fwd_varlen and its forms, tfa_fwd_varlen_paged,
 *   tfa_fwd_splitkv with any split count), 16-bit output vs the exact result:
 *                                                              |d| <= eps16 * A + 1e-6 + half an ulp16 of the result — the fp32-output bound plus the ONE
 *                                                              rounding of O (partials and tfa_merge are fp32), on EVERY element; the fp32 output: the
 *                                                              bound above, on every element.  It holds on rows whose dominant key lies outside their
 *                                                              first 64-key tile under TFA_RULE_FIRST_TILE too, with and without the 2^40 re-base: asserted on
 *                                                              the main instantiations of variants 30, 32, 36 and 37 (there the kernels use all of it:
 *                                                              0.96-0.995 measured and emulated, against 0.5 under the other rules)
 *   the prefill forward family, LSE (u = 2^-24, T = max_j scale * sum_d |q_d| |k_jd| + slope * |i + shift - j| + |bias_ij|, n keys,
 *   R = 1 + floor(T / (20 ln 2))):
 *                                                              |d| <= u * ((D + 15 + 2 [slopes] + 2 [bias]) * T + R * (T + ln n) + 11 * ceil(n / 64)
 *                                                              + 3 ln n + 13 + 16 * softcap) + 2^-22 * |lse|, merged over s parts + u * (5 * s + 4) + u * |lse|
 *                                                              — derived term by term from the il / x4 tile loops and their epilogue, the LDS-DMA body and
 *                                                              tfa_merge (tests/fwd_ref.py: lse_bound); a worst-case sum: 0.04-0.9 of 1e-4 up to D = 136,
 *                                                              looser at D = 256 and where T is large (steep slopes, saturated caps, peaked rows), so the
 *                                                              1e-4 bar stays asserted next to it.  All asserted element by element
 *                                                              in tests/test_fwd_bounds_gpu.py on inputs that put weight on the keys where indexing goes
 *                                                              wrong, proved to fit and to bite in tests/test_fwd_bounds_cpu.py
 *   default kernels (TFA_RULE_LAZY / TFA_RULE_FIRST_TILE), fp32 output vs the reference's tile loop restated with THEIR rounding points:
 *                                                              |d| <= 1e-3 * |ref| + 1e-4 * A  (<= 1e-4 of the elements may flip one rounding of P)
 *   TFA_FWD_EXACT_MAX, fp32 output vs the reference's own tile loop (main_torch_only.py:160-270), element by element:
 *                                                              |d| <= 1e-3 * |ref|  on the elements with |ref| > 0.05 * A (config 4: 0.01 * A) — an element
 *                                                              whose value is a cancelling sum has no meaningful relative error —, 1e-4 of those
 *                                                              elements exempt: this is how BASELINE.json's rtol = 1e-3 is read and asserted
 *                                                              (tests/test_parity_gpu.py::test_exact_running_max_flag_at_baseline_sizes, whole heads of
 *                                                              BASELINE configs 3 and 4); measured cost: 0.517-0.529 vs 0.468-0.479 ms on the headline
 *                                                              shape (profiles/r06_bench_driver_protocol*.json). */
#define TFA_FWD_EXACT_MAX 1

/* Library version (TFA_VERSION of the build). */
int tfa_version(void);

/* Human-readable text for a return code of any entry point (static storage). */
const char* tfa_strerror(int status);

/* Launch the forward pass described by *p on HIP stream `stream` (NULL = default stream).
 * Asynchronous: returns after enqueueing.  Never allocates.  The kernel is chosen from the problem's size (256-row blocks,
 * 128-row blocks, keys split inside the workgroup for grids smaller than the chip, the 256-wide kernel for D > 128); with
 * Hk < H and one query row per head (batched decode) the H/Hk query heads of a K/V head are run as rows of one problem, so
 * K and V stream once per K/V head.  Results do not depend on those choices beyond the rounding of P to 16 bits. */
int tfa_fwd(const tfa_fwd_params* p, void* stream);

/* Convenience form for the reference's layout: q,k,v,out contiguous (B,H,N,D), Nq == Nk == N,
 * Hk == H, out dtype == input dtype.  This is exactly the argument list of
 * flash_attention_v2_cutlass (flash_attention.cu:741-742) plus explicit sizes. */
int tfa_fwd_bhnd(const void* q, const void* k, const void* v, void* out, float* lse,
                 int B, int H, int N, int D, float softmax_scale, int is_causal,
                 int dtype, void* stream);

/* Same, but O is written as fp32 (no final rounding) — the debug path used to check the
 * rtol=1e-3 parity target below one bf16 ulp (precedent: FPC_O=float,
 * flash_attention_cutlass/standalone_src/flash_attention_cutlass_standalone.cu:18-23). */
int tfa_fwd_bhnd_f32out(const void* q, const void* k, const void* v, float* out, float* lse,
                        int B, int H, int N, int D, float softmax_scale, int is_causal,
                        int dtype, void* stream);

/* Validate *p without launching; on success optionally reports the launch geometry. */
int tfa_fwd_plan(const tfa_fwd_params* p, int* grid, int* block, int* lds_bytes);

/* The kernel variant tfa_fwd would run for *p (>= 0; the forced one if tfa_set_variant is active), or a
 * negative TFA_ERR_* code.  The parity tests use it to pick the matching same-rounding-points emulation:
 * variants named "il..." keep a lazily re-based row reference instead of the exact running max
 * (oracle/oracle.py: tiled_emulation_lazy), all others follow main_torch_only.py:240-257 exactly. */
int tfa_fwd_variant(const tfa_fwd_params* p);

/* The row reference tfa_fwd would round P against for *p (the header's "Rounding points"): TFA_RULE_*, or a negative TFA_ERR_* code.  Decided
 * by the same predicates as the launch (kernel variant, dtype, which instantiation of the variant the sizes select); the parity tests pick
 * their same-rounding-points emulation with it (oracle/oracle.py: tiled_emulation, tiled_emulation_lazy, tiled_emulation_first_tile). */
#define TFA_RULE_EXACT_MAX 0
#define TFA_RULE_LAZY 1
#define TFA_RULE_FIRST_TILE 2
int tfa_fwd_rounding_rule(const tfa_fwd_params* p);

/* Time `iters` back-to-back launches of *p with HIP events recorded on `stream`
 * (after `warmup` untimed launches).  Writes the average milliseconds per launch.
 * Synchronises `stream`.  Used by bench.py for the roofline numbers. */
int tfa_fwd_time(const tfa_fwd_params* p, int warmup, int iters, void* stream, float* avg_ms);

/* ---- split-KV merge (SURVEY section 8(f) row 4) ---------------------------------------------------------
 * Combines `nparts` partial attention results over disjoint key chunks of the same queries — the online-softmax
 * merge rule the reference states for its v1 form (flash_attention_py/tiny_flash_attn.py:63-68, README_zh.md:104-125):
 *   lse = log sum_p exp(lse_p),   out = sum_p exp(lse_p - lse) * out_p      (parts with lse_p = +inf are empty).
 * o_parts: nparts x rows x D fp32 (part stride o_part_stride elements, rows contiguous, rows = B*H*Nq);
 * lse_parts: nparts x rows fp32 (part stride lse_part_stride).  out: rows x D of out_dtype (F16/BF16/F32),
 * lse_out: rows fp32 or NULL.  A row whose parts are all empty gives out = 0, lse = +inf. */
int tfa_merge(const float* o_parts, const float* lse_parts, int nparts, int64_t rows, int D,
              int64_t o_part_stride, int64_t lse_part_stride, void* out, int out_dtype, float* lse_out, void* stream);

/* Split-KV on one GPU in ONE launch (decode-like shapes: few query rows, long K/V, too few workgroups to fill the
 * chip): the key sequence is cut into `splits` chunks (multiples of 64 keys), the grid carries one copy of the work per
 * chunk (LDS-DMA kernel, 64 / 128 / 256 wide), partials go to `workspace`, tfa_merge writes *p's out (contiguous (B,H,Nq,D)) and lse.
 * (b,h) slices of 2 GiB and more: one launch of tfa_fwd's windowed kernel per chunk instead; when such a launch leaves
 * the chip mostly idle the launches are forked over four side streams owned by the calling thread and joined into `stream` before the
 * merge (event fork / join: legal inside a stream capture — the streams and events are created on the thread's first such call, so make
 * one call outside a capture first).  Everything the call enqueues is ordered before later work on `stream`.
 * workspace: tfa_fwd_splitkv_workspace(p, splits) floats (16-byte aligned); negative return = TFA_ERR_*. */
long long tfa_fwd_splitkv_workspace(const tfa_fwd_params* p, int splits);
int tfa_fwd_splitkv(const tfa_fwd_params* p, int splits, float* workspace, void* stream);
/* The split count a host that can provide a workspace should use for *p: 1 = call tfa_fwd (the grid fills the chip, or the
 * keys are too few to be worth a merge), >= 2 = call tfa_fwd_splitkv with that many chunks (decode-like shapes: B*H*ceil(Nq/128)
 * workgroups on half of the CUs or fewer, at least 4096 keys, causal only when Nq <= Nk/4; measured 3-9x on B1 H32 Nq1
 * Nk16k..64k, B1 H8 Nq16 Nk32k, 1.7-2x on short non-causal / chunked-prefill problems with one to four heads, 1.4-1.6x when a quarter to a half of the CUs had work; head dims above 128:
 * 4-11x, K/V at 3.6-5.5 TB/s; at most 4 for the one-launch-per-chunk route of slices beyond 2 GiB: 1.4-1.8x).
 * The reference-named bindings (attention_cutlass / attention_cuda / _kernels and their Python mirrors) follow it. */
int tfa_fwd_suggest_splits(const tfa_fwd_params* p);

/* ---- backward (SURVEY section 8(f) row 3) ------------------------------------------------------------
 * The reference has no backward pass; it saves softmax_lse for one ("LogSumExp save for backward",
 * flash_attention_cutlass/csrc/flash_attention.cu:353-354, :614-623; tiny_flash_attn_triton.py:27-29).
 * tfa_bwd consumes exactly what tfa_fwd produced: out and lse of the same q,k,v, and the upstream
 * gradient dout (same shape/dtype as out), and writes dq (shape of q), dk, dv (shape of k, v; for
 * grouped-query attention summed over the query heads of each kv head).  Same layout rules as tfa_fwd
 * (strides in elements, unit stride along D, 16-byte aligned rows); grads are written in the input
 * dtype, or in fp32 when grad_dtype == TFA_F32 (debug path for tolerance checks below one 16-bit ulp).
 * `delta` is caller-provided scratch of B*H*Nq floats (rowsum(dout o out), filled by the call). */
typedef struct tfa_bwd_params {
  const void* q;
  const void* k;
  const void* v;
  const void* out;
  const void* dout;
  const float* lse;      /* (B,H,Nq) contiguous, natural log, as written by tfa_fwd */
  void* dq;
  void* dk;
  void* dv;
  float* delta;          /* scratch, B*H*Nq floats */
  int B, H, Hk, Nq, Nk, D;
  int64_t q_stride[3];   /* batch, head, row (elements) */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];
  int64_t do_stride[3];
  int64_t dq_stride[3];
  int64_t dk_stride[3];
  int64_t dv_stride[3];
  float softmax_scale;
  int is_causal;
  int dtype;             /* TFA_F16 / TFA_BF16: q,k,v,out,dout */
  int grad_dtype;        /* == dtype, or TFA_F32 */
  /* Optional: a scratch buffer of at least tfa_bwd_workspace_bytes(p) bytes (16-byte aligned), or NULL.  With it the dK/dV launch
   * keeps dS = P o (dP - delta) (16 bit, B*H*Nk*Nq elements) and dQ becomes ONE GEMM over it instead of a recomputation of S and
   * dP: 5 GEMM units in all instead of 7, at the price of O(Nq*Nk) scratch memory.  Same results (the same 16-bit dS feeds dQ
   * either way, up to P having been rounded to 16 bit first), still deterministic.  NULL / too small: the O(N)-memory path. */
  void* workspace;
  int64_t workspace_bytes;
} tfa_bwd_params;

/* Launch the backward on `stream` (asynchronous): dQ (S, dP, dQ: 3 GEMM units; the launch also computes delta = rowsum(dO o O) for its rows
 * and writes it to tfa_bwd_params::delta), then dK and dV in ONE launch that computes S and dP once each (4 units; tfa_bwd_kv_kernel.h);
 * with tfa_bwd_params::workspace: delta (a launch of its own), dK/dV (which also writes dS), dQ = dS.K (1 unit).
 * Head dims 136..256: three single-gradient launches (dQ, dK, dV) of the 256-wide kernel, one wave per SIMD.
 * Deterministic: no atomics, fixed summation order. */
int tfa_bwd(const tfa_bwd_params* p, void* stream);
/* Debug / A-B (per thread): bit 0 makes tfa_bwd run dK and dV as two single-gradient launches (S computed twice: the form of
 * versions <= 0.1.4); bit 1 forces the windowed instantiations (the ones slices of 2 GiB and more get) on any problem; bit 3 (value 8)
 * computes delta by a launch of its own in front of the dQ launch (the form up to version 0.1.6) instead of inside it. */
int tfa_debug_bwd_split(int on);
/* Validate *p without launching (no GPU needed). */
int tfa_bwd_plan(const tfa_bwd_params* p);
/* Bytes of tfa_bwd_params::workspace that switch tfa_bwd to its 5-GEMM form for *p (B*H * roundup(Nk,128) * roundup(Nq,256) * 2),
 * 0 when tfa_bwd would not use a workspace for *p (head dims above 128, (b,h) slices of 2 GiB and more, a head's slab reaching
 * 2 GiB, the two-launch debug form), negative = TFA_ERR_*. */
long long tfa_bwd_workspace_bytes(const tfa_bwd_params* p);
/* Algorithmic work of one call: flops = 2.5 x the forward's (5 GEMMs of 2*Nq*Nk*D each per head, halved
 * when causal), bytes = q,k,v,out,dout read once + dq,dk,dv written once + lse. */
int tfa_bwd_work(const tfa_bwd_params* p, double* flops, double* bytes);
/* Time `iters` back-to-back tfa_bwd calls with HIP events on `stream` (after `warmup` untimed ones). */
int tfa_bwd_time(const tfa_bwd_params* p, int warmup, int iters, void* stream, float* avg_ms);

/* Kernel-variant selector for A/B measurement and bring-up (state of the CALLING THREAD).  -1 = automatic (default).
 * Variant numbers live in [0, tfa_num_variants()); tfa_variant_available(i) says whether THIS build carries number i (the product
 * build: the six dispatched kernels 17, 30, 32, 34, 36, 37), tfa_variant_name(i) describes it. */
int tfa_set_variant(int variant);
int tfa_get_variant(void);
int tfa_num_variants(void);
const char* tfa_variant_name(int variant);
/* 1 if variant i is compiled into this build, else 0.  The product build carries the dispatched kernels only; the
 * other entries of the table are A/B arms built with -DTFA_EXPERIMENTAL (make EXPERIMENTAL=1) and are rejected
 * with TFA_ERR_VARIANT otherwise. */
int tfa_variant_available(int variant);

/* Debug/profiling: when dev_buf != NULL every workgroup of subsequent launches writes 8 x uint64
 * {t_start, t_after_prologue, t_after_loop, t_end (shader cycles, s_memtime), n_kv_tiles (low 32 bits),
 * XCC_ID | HW_ID << 32, the workgroup's life in 100 MHz s_memrealtime ticks, (bh<<32)|query_block}
 * at dev_buf[8*workgroup_id ...]; the buffer must hold 64 B per workgroup (tfa_fwd_plan reports the
 * grid).  (t_end - t_start) / ticks * 100 MHz is the shader clock the workgroup actually ran at:
 * bench.py reports its median as the sustained clock next to the nominal 2.4 GHz.  NULL (default)
 * disables it.  The stamps are written by a traced TWIN of the kernel (the kernels the library dispatches are compiled without the
 * stamp code: its scalar state costs every workgroup ~130 register-lane moves): the main 16-bit-output instantiation of the il kernels
 * (variants 30, 32, 36, 37), and the dma / x4 kernels; the special-case instantiations (windowed slices, decode-like idle waves, head
 * dims below the kernel's width, fp32 output) leave the buffer untouched. */
int tfa_debug_set_trace(void* dev_buf);
/* Kernel bring-up flags of the calling thread (0 = normal).  128: the trace stamps describe a causal workgroup's SECOND
 * pass (the light block) instead of the first; 256: launch the windowed-descriptor instantiation (the one slices of
 * 2 GiB and more get) whatever the slice size — tests compare its bits with the default; 8192: tfa_fwd_splitkv takes its one-launch-per-chunk
 * route (the one (b,h) slices of 2 GiB and more take) on any problem; 16384: that route launches its chunks in
 * line on the caller's stream instead of forking them over the thread's side streams; the low bits insert fences / force the burst path in the x4 kernel
 * (tfa_fwd_kernel_x4.h) and are only meaningful to tools/. */
int tfa_debug_set_flags(int flags);
/* Host-side check of the kernels' work-item decode (no GPU needed): decodes workgroup `id` of a launch with the given batch, query
 * heads, K/V heads and work items per head exactly as the il kernels do on the device — the host-computed magic-number divisions
 * (tfa_launch.h: fill_decode, tfa_fwd_kernel.h: FastDiv) applied in the kernels' branch-free form — and writes {b, h, hk, wi} to
 * out[0..3].  tests/test_abi.py compares it with the plain divisions of the three dispatch orders. */
int tfa_debug_decode(int B, int H, int Hk, int nwork, int id, int* out);

/* Measurement aid (bench.py): the rate in TFLOP/s that a stream of nothing but v_mfma_f32_32x32x16_bf16 sustains on this GPU with operand values
 * taken from the first 16 MiB of `operands` (device memory, `bytes` >= 16 MiB of bf16 data — bench.py passes its q tensor), launched on `stream` for about `seconds`
 * (<= 30); synchronises the stream.  On the reference's normal(0, 0.5) inputs the board's power cap holds that stream to ~0.68 of the nominal
 * 2.5 PFLOP/s and boxes differ by +-5 %: the figure belongs next to `roofline.frac`, measured in the same run, not hard-coded.
 * It SYNCHRONISES `stream` between its groups of launches and allocates / frees device memory: it cannot be called inside a stream capture.
 * *tflops is 0 on every error return (bad sizes: TFA_ERR_SHAPE; no timed group completed: hipErrorNotReady). */
int tfa_debug_mfma_ceiling(const void* operands, unsigned long long bytes, double seconds, void* stream, double* tflops);

/* Algorithmic work of *p: flops = 4*B*H*Nq*Nk*D (x1/2 when causal, the reference's
 * convention) and bytes = Q+K+V read once + O written once (+LSE). */
int tfa_fwd_work(const tfa_fwd_params* p, double* flops, double* bytes);

/* ---- packed variable-length batches (the cu_seqlens form of FlashAttention-2's flash_attn_varlen_func) --------------------------------
 * B sequences of different lengths packed along the rows: q is (total_q, H, D), k and v are (total_k, Hk, D), out is shaped like q; sequence b is
 * rows [cu_seqlens_q[b], cu_seqlens_q[b+1]) of q / out and [cu_seqlens_k[b], cu_seqlens_k[b+1]) of k / v.  cu_seqlens_q / _k are DEVICE int32
 * arrays of B + 1 entries (cu[0] = 0, non-decreasing) that the library never reads on the host: no copy, no synchronisation — a call is asynchronous
 * and can be captured in a graph.  Each work item of the kernels reads its sequence's four bounds itself (scalar loads) and clamps them into
 * [0, total_q] / [0, total_k] and the lengths to max_seqlen_q / _k, so a bad cu_seqlens can misplace results but never address outside the tensors.
 *   - every sequence has at most max_seqlen_q query rows and max_seqlen_k keys (host integers: they size the grids);
 *   - causal masking per sequence, bottom-right aligned as in tfa_fwd: key j is visible to row i iff j <= i + (Nk_b - Nq_b); rows that see no key —
 *     every row of a sequence with Nk_b = 0 — get out = 0, lse = +inf; sequences with Nq_b = 0 are allowed;
 *   - lse: fp32 (H, total_q), contiguous, natural log (FlashAttention-2's varlen layout); delta (backward scratch) the same;
 *   - GQA / MQA as in tfa_fwd (Hk divides H): dk / dv are summed over the query heads of each K/V head, within each sequence;
 *   - rows outside every sequence (cu_q[B] <= r < total_q, and the same for keys) are never read into a result and never written.
 * Strides are (head, row) pairs in elements, unit stride along D, every row 16-byte aligned; head dims = multiples of 8 up to 128; 16-bit q, k, v.
 * Kernels: the forward runs the varlen form of the kernel tfa_fwd would pick for the fixed-length problem (B, H, Hk, max_seqlen_q, max_seqlen_k, D)
 * — il8 (variant 30) or il4 (32); the key-split choices (36, 37) map to il4.  Only the MAIN instantiation of each exists in varlen form (full width,
 * for bf16 the first-tile rule): with equal lengths and a head dim that reaches the kernel's last 32 columns (D = 40..64 or 104..128) the call runs
 * the very kernel tfa_fwd runs, with the same bits.  Head dims that leave the kernel's last 32 columns empty (D <= 32, 72..96) run the full-width kernel with
 * those columns read as zeros: tfa_fwd runs a narrow instantiation there (fewer MFMAs — a third fewer at D = 96 — and, for bf16, TFA_RULE_LAZY), so the two
 * agree within the bounds of "Rounding points" but not in bits.  The backward's varlen launches are full-width too (tfa_bwd's dQ and dK/dV launches have
 * narrow twins at those head dims).
 * The backward runs its dQ launch (which also forms delta) and its fused dK/dV launch in varlen form.
 * Out of scope (refused): head dims above 128 (TFA_ERR_HEAD_DIM), fp32 inputs (TFA_ERR_DTYPE), TFA_FWD_EXACT_MAX and any other flag (flags must be 0:
 * TFA_ERR_SHAPE), split-KV, GQA decode row packing, the backward's dS-workspace form, dropout (sliding windows: tfa_fwd_varlen_local below), and sequences whose
 * max_seqlen rows would not fit one buffer descriptor (TFA_ERR_STRIDE: no windowed varlen form).  Paged K/V — the keys in a page pool behind a block table — is
 * tfa_fwd_varlen_paged below.  A NULL cu_seqlens is TFA_ERR_NULL;
 * B, H, Hk, max_seqlen or total <= 0 or H % Hk != 0 is TFA_ERR_SHAPE.
 * Measured: profiles/varlen_bench.txt (tools/bench_varlen.py; equal lengths at the speed of tfa_fwd / tfa_bwd, mixed lengths against padding and
 * against one call per sequence), quoted in INTEGRATION.md. */
typedef struct tfa_varlen_fwd_params {
  const void* q;               /* (total_q, H,  D) */
  const void* k;               /* (total_k, Hk, D) */
  const void* v;               /* (total_k, Hk, D) */
  void* out;                   /* (total_q, H,  D) of out_dtype */
  float* lse;                  /* (H, total_q) fp32 contiguous, or NULL to skip */
  const int32_t* cu_seqlens_q; /* device, B + 1 entries */
  const int32_t* cu_seqlens_k; /* device, B + 1 entries */
  int32_t B, H, Hk, D;
  int32_t max_seqlen_q, max_seqlen_k;
  int32_t total_q, total_k;    /* rows of q / out and of k / v */
  int64_t q_stride[2];         /* head, row (elements) */
  int64_t k_stride[2];
  int64_t v_stride[2];
  int64_t o_stride[2];         /* in elements of out_dtype */
  float softmax_scale;
  int32_t is_causal;
  int32_t dtype;               /* TFA_F16 or TFA_BF16 */
  int32_t out_dtype;           /* == dtype, or TFA_F32 */
  int32_t flags;               /* must be 0 */
  int32_t reserved_;           /* must be 0 */
} tfa_varlen_fwd_params;

typedef struct tfa_varlen_bwd_params {
  const void* q;
  const void* k;
  const void* v;
  const void* out;
  const void* dout;            /* shaped like out, input dtype */
  const float* lse;            /* (H, total_q), as written by tfa_fwd_varlen */
  void* dq;                    /* shaped like q, grad_dtype */
  void* dk;                    /* shaped like k */
  void* dv;                    /* shaped like v */
  float* delta;                /* scratch, H * total_q floats (4-byte aligned) */
  const int32_t* cu_seqlens_q;
  const int32_t* cu_seqlens_k;
  int32_t B, H, Hk, D;
  int32_t max_seqlen_q, max_seqlen_k;
  int32_t total_q, total_k;
  int64_t q_stride[2];         /* head, row (elements) */
  int64_t k_stride[2];
  int64_t v_stride[2];
  int64_t o_stride[2];
  int64_t do_stride[2];
  int64_t dq_stride[2];        /* in elements of grad_dtype */
  int64_t dk_stride[2];
  int64_t dv_stride[2];
  float softmax_scale;
  int32_t is_causal;
  int32_t dtype;               /* TFA_F16 / TFA_BF16 */
  int32_t grad_dtype;          /* == dtype, or TFA_F32 */
  int32_t flags;               /* must be 0 */
  int32_t reserved_;           /* must be 0 */
} tfa_varlen_bwd_params;

/* Launch the packed forward on `stream` (asynchronous, never allocates, never reads cu_seqlens on the host). */
int tfa_fwd_varlen(const tfa_varlen_fwd_params* p, void* stream);
/* Validate *p without launching (no GPU needed); on success optionally reports the launch geometry. */
int tfa_fwd_varlen_plan(const tfa_varlen_fwd_params* p, int* grid, int* block, int* lds_bytes);
/* The kernel variant tfa_fwd_varlen runs for *p (30 or 32; the forced one if tfa_set_variant forces 30 or 32), or a negative TFA_ERR_* code. */
int tfa_fwd_varlen_variant(const tfa_varlen_fwd_params* p);
/* The row reference P is rounded against (TFA_RULE_*, the header's "Rounding points"): TFA_RULE_FIRST_TILE for bf16, TFA_RULE_LAZY for fp16. */
int tfa_fwd_varlen_rounding_rule(const tfa_varlen_fwd_params* p);
/* Launch the packed backward on `stream` (asynchronous): the dQ launch (it writes delta), then the fused dK/dV launch.  Deterministic. */
int tfa_bwd_varlen(const tfa_varlen_bwd_params* p, void* stream);

/* ---- paged K/V for packed variable-length batches (FlashAttention-2's flash_attn_varlen_func(..., block_table=...): chunked prefill) ------------
 * tfa_fwd_varlen with the keys in a page pool: q / out / lse / cu_seqlens_q as in tfa_fwd_varlen; p->k / p->v point at the pool (num_pages, page_size, Hk, D)
 * with p->k_stride / v_stride = {head, row} as before and the page strides in *pg; p->total_k is ignored.  Sequence b has Nk_b = cu_seqlens_k[b+1] -
 * cu_seqlens_k[b] keys (only the difference is used), clamped on the device into [0, min(max_seqlen_k, max_blocks * page_size)]; key j is row j % page_size
 * of page block_table[b, j / page_size], the entry clamped into [0, num_pages) before use — a bad entry or length can misplace a read but never leaves the
 * pool.  Nothing is read on the host: no copy, no synchronisation, capturable in a graph and replayable after lengths and table were overwritten in place.
 * Causal masking per sequence, bottom-right aligned (shift = Nk_b - Nq_b): new tokens see the whole prefix and each other causally; rows that see no key get
 * out = 0, lse = +inf; Nq_b = 0 and Nk_b = 0 are legal.  Whatever lies behind a sequence's length — the tail of its last page, unreferenced pages, stale keys,
 * NaN — arrives as zeros: every 64-key tile has a descriptor of its own whose extent ends at the sequence's last key and at the valid head dim.
 * Strides in elements, unit stride along D, 16-byte aligned rows and pages; page_size a positive multiple of 64 (the kernels' key tile); the pool may be of any
 * size (2 GiB, 4 GiB and more: page bases are 64-bit pointer arithmetic), only 64 rows at the row stride must fit one descriptor (TFA_ERR_STRIDE otherwise).
 * Kernels: the paged form of the kernel tfa_fwd_varlen would run (_variant: 30 or 32, the same answer; _plan: the same geometry), 128- or 256-row query blocks —
 * built for prefill; decode-shaped batches (one row per sequence) are correct but waste the block: tfa_fwd_kvcache is the call for them.  Per-tile descriptors
 * mean the compiler-scheduled tile bodies (as for slices beyond 2 GiB in tfa_fwd) and so TFA_RULE_LAZY for both types (_rounding_rule) — tfa_fwd_varlen on
 * the same keys rounds bf16 by TFA_RULE_FIRST_TILE: the two agree within the bounds of "Rounding points", not in bits.
 * Refused: a NULL pg or block_table (TFA_ERR_NULL); page_size not a positive multiple of 64, max_blocks or num_pages <= 0 (TFA_ERR_SHAPE); flags != 0
 * (TFA_ERR_SHAPE); a table that is not 4-byte aligned (TFA_ERR_ALIGN); negative or misaligned table / page strides (TFA_ERR_STRIDE); and what tfa_fwd_varlen
 * refuses (D > 128, fp32 inputs, a variant other than 30 / 32).
 * Out of scope: a backward; paged K/V combined with windows, softcap or ALiBi; fp8 page pools; seqused_k; a hand-scheduled paged tile loop; D > 128.
 * (The append for packed new rows is tfa_kvcache_append_varlen, below; tfa_kvcache_append serves one row count per batch.)
 * Measured: profiles/varlen_paged_bench.txt (tools/bench_varlen_paged.py), quoted in README.md and DESIGN.md 8g. */
typedef struct tfa_paged_kv {
  const int32_t* block_table;  /* device int32 (B, max_blocks), unit stride along max_blocks */
  int64_t table_stride;        /* elements between the rows of block_table */
  int32_t max_blocks;          /* entries per row */
  int32_t page_size;           /* keys per page, a positive multiple of 64 */
  int32_t num_pages;           /* pages in the pool */
  int32_t reserved_;           /* must be 0 */
  int64_t k_page_stride;       /* elements between the pages of k */
  int64_t v_page_stride;
} tfa_paged_kv;
int tfa_fwd_varlen_paged(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg, void* stream);
int tfa_fwd_varlen_paged_plan(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg, int* grid, int* block, int* lds_bytes);
/* The kernel variant (30 or 32: tfa_fwd_varlen_variant's answer for *p) / the rounding rule (TFA_RULE_LAZY) of the paged call, or a negative TFA_ERR_* code. */
int tfa_fwd_varlen_paged_variant(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg);
int tfa_fwd_varlen_paged_rounding_rule(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg);

/* ---- local (sliding-window) attention (FlashAttention-2's window_size = (left, right)) ---------------------------------------------------
 * The same params structs as tfa_fwd / tfa_bwd / tfa_fwd_varlen / tfa_bwd_varlen plus the window: with shift = Nk - Nq per sequence (bottom-right
 * aligned, as is_causal), key j is visible to query row i iff  i + shift - window_left <= j <= i + shift + window_right.  -1 = unbounded on that side;
 * is_causal = 1 forces window_right = 0.  A side that reaches every key of every row is unbounded (left >= Nk - 1, right >= Nq - 1; max_seqlen for
 * varlen).  (-1, -1) and (-1, 0) then run exactly what tfa_fwd / tfa_bwd (and the varlen forms) run with is_causal = 0 / 1: same kernels, same bits.
 * Rows that see no key get out = 0 and lse = +inf; dk / dv of keys that no row sees are 0; GQA sums as in tfa_bwd.
 * Any other window runs the LOCAL instantiations: the il8 (variant 30) or il4 (32) forward — il8 where tfa_fwd would pick it, il4 for everything else
 * (split-KV, decode row packing and the key-split kernels have no local form) — without causal pairing, visiting only the key tiles that meet its rows'
 * windows; rounding rule TFA_RULE_LAZY (bf16 included).  Full width only: head dims below the kernel's width read the missing columns as zeros.  The
 * backward runs its dQ launch (which forms delta) and its fused dK/dV launch, each visiting only the tiles inside the window, deterministic; never the
 * dS-workspace form (tfa_bwd_params::workspace is ignored).
 * Refused for a true window: head dims above 128 (TFA_ERR_HEAD_DIM), fp32 inputs (TFA_ERR_DTYPE), any flag — TFA_FWD_EXACT_MAX included — (TFA_ERR_SHAPE),
 * a side below -1 (TFA_ERR_SHAPE, for every window), kv_offset / nk_total != 0 (TFA_ERR_SHAPE), Nq + Nk >= 2^28 (TFA_ERR_SHAPE), slices that need
 * per-tile descriptors (TFA_ERR_STRIDE), a forced variant other than 30 / 32 (TFA_ERR_VARIANT).
 * Measured: profiles/window_bench.txt (tools/bench_window.py), quoted in README.md and INTEGRATION.md. */
int tfa_fwd_local(const tfa_fwd_params* p, int window_left, int window_right, void* stream);
int tfa_fwd_local_plan(const tfa_fwd_params* p, int window_left, int window_right, int* grid, int* block, int* lds_bytes);
/* The kernel variant tfa_fwd_local runs for *p (tfa_fwd_variant's answer for (-1, -1) / (-1, 0)), or a negative TFA_ERR_* code. */
int tfa_fwd_local_variant(const tfa_fwd_params* p, int window_left, int window_right);
/* The row reference P is rounded against (TFA_RULE_*): TFA_RULE_LAZY for a true window, tfa_fwd_rounding_rule's answer otherwise. */
int tfa_fwd_local_rounding_rule(const tfa_fwd_params* p, int window_left, int window_right);
int tfa_fwd_varlen_local(const tfa_varlen_fwd_params* p, int window_left, int window_right, void* stream);
int tfa_fwd_varlen_local_plan(const tfa_varlen_fwd_params* p, int window_left, int window_right, int* grid, int* block, int* lds_bytes);
int tfa_fwd_varlen_local_variant(const tfa_varlen_fwd_params* p, int window_left, int window_right);
int tfa_fwd_varlen_local_rounding_rule(const tfa_varlen_fwd_params* p, int window_left, int window_right);
/* The backward of a local forward (same window, same params as tfa_bwd / tfa_bwd_varlen); _plan validates without launching. */
int tfa_bwd_local(const tfa_bwd_params* p, int window_left, int window_right, void* stream);
int tfa_bwd_local_plan(const tfa_bwd_params* p, int window_left, int window_right);
int tfa_bwd_varlen_local(const tfa_varlen_bwd_params* p, int window_left, int window_right, void* stream);
int tfa_bwd_varlen_local_plan(const tfa_varlen_bwd_params* p, int window_left, int window_right);

/* ---- ALiBi (FlashAttention-2's alibi_slopes) -----------------------------------------------------------------------------------------------
 * The same params structs as tfa_fwd / tfa_bwd / tfa_fwd_varlen / tfa_bwd_varlen plus the slopes and a window.  With shift = Nk - Nq per sequence
 * (bottom-right aligned, as is_causal and the window):
 *     S[i,j] = softmax_scale * q_i . k_j  -  alibi_slopes[b * slopes_batch_stride + h] * | i + shift - j |
 * then the mask (is_causal / the window, exactly as the _local entry points read them; (-1, -1) = none), the softmax and P V.  Everything downstream is
 * defined on these biased scores: lse is the true logsumexp_j S[i,j] INCLUDING the bias, causal or not (tfa_bwd_alibi and tfa_merge consume it); rows that
 * see no key get out = 0 and lse = +inf; the backward recomputes P from the biased scores and returns dq, dk, dv — the slopes get no gradient.
 * alibi_slopes: fp32 in DEVICE memory, one slope per QUERY head h (GQA: the H / Hk query heads of a K/V head have their own) of batch entry / sequence b;
 * slopes_batch_stride = 0: one row of H slopes shared by the batch, = H: a (B, H) array.  The library never reads the array on the host — no copy, no
 * synchronisation, a call can be captured in a graph and replayed after the values were changed in place.  Any finite value is legal (zero and negative
 * included); non-finite slopes give unspecified results; nothing is validated on the host.  (Without slopes call the existing entry points: there is no
 * "NULL = no bias" here.)
 * Every call runs the ALiBi form of the LOCAL instantiations, whatever the window — full and causal attention carry unbounded sides: the il8 (variant 30)
 * or il4 (32) forward as tfa_fwd_local chooses, one query block per work item, every tile through the compiler-scheduled bodies (the bias is added to the
 * raw scores in front of the row maximum); rounding rule TFA_RULE_LAZY for both dtypes.  The backward runs the dQ launch (which forms delta) and the fused
 * dK/dV launch of that form, deterministic; never the dS-workspace form (tfa_bwd_params::workspace is ignored).
 * Refused, nothing launched: alibi_slopes NULL (TFA_ERR_NULL) or not 4-byte aligned (TFA_ERR_ALIGN), slopes_batch_stride other than 0 or H
 * (TFA_ERR_STRIDE), and what the local form refuses, with its codes: head dims above 128 (TFA_ERR_HEAD_DIM), fp32 inputs (TFA_ERR_DTYPE), any flag —
 * TFA_FWD_EXACT_MAX included — (TFA_ERR_SHAPE), a window side below -1 (TFA_ERR_SHAPE), kv_offset / nk_total != 0 (TFA_ERR_SHAPE), Nq + Nk >= 2^28
 * (TFA_ERR_SHAPE), slices that need per-tile descriptors (TFA_ERR_STRIDE), a forced variant other than 30 / 32 (TFA_ERR_VARIANT).
 * The kernels form the distance i + shift - j exactly in int32 and convert it to fp32 in front of |.|: beyond 2^24 positions (Nq + Nk < 2^28 is admitted) it
 * carries fp32's relative rounding, the same order as the rounding of slope * |distance| itself.
 * Tolerances: the header's "which tolerance each path guarantees", with the LSE bar relative to its size — |d| <= 1e-4 * max(1, |lse|): with Nq > Nk and no
 * causal mask every key of the first rows is Nq - Nk positions away and the LSE itself is of the order of slope * (Nq - Nk).
 * Measured: profiles/alibi_bench.txt (tools/bench_alibi.py), quoted in README.md. */
int tfa_fwd_alibi(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream);
/* Validate and report the launch geometry of tfa_fwd_alibi without launching (no GPU needed). */
int tfa_fwd_alibi_plan(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, int* grid,
                       int* block, int* lds_bytes);
/* The kernel variant tfa_fwd_alibi runs for *p (30 or 32), or a negative TFA_ERR_* code. */
int tfa_fwd_alibi_variant(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
/* The row reference P is rounded against: TFA_RULE_LAZY (bf16 and fp16), or a negative TFA_ERR_* code. */
int tfa_fwd_alibi_rounding_rule(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
/* Packed variable-length batches: b indexes the sequence (slopes_batch_stride = H: one row of slopes per sequence), the distance is taken per sequence. */
int tfa_fwd_varlen_alibi(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                         void* stream);
int tfa_fwd_varlen_alibi_plan(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                              int* grid, int* block, int* lds_bytes);
int tfa_fwd_varlen_alibi_variant(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
int tfa_fwd_varlen_alibi_rounding_rule(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                       int window_right);
/* The backward of an ALiBi forward (same slopes, same window, same params as tfa_bwd / tfa_bwd_varlen); _plan validates without launching. */
int tfa_bwd_alibi(const tfa_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream);
int tfa_bwd_alibi_plan(const tfa_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
int tfa_bwd_varlen_alibi(const tfa_varlen_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                         void* stream);
int tfa_bwd_varlen_alibi_plan(const tfa_varlen_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);

/* ---- Soft-capping (FlashAttention-2's softcap: tanh logit capping, Gemma-2 / Grok style) -----------------------------------------------------
 * The ALiBi entry points' arguments with `softcap` in front; alibi_slopes may be NULL here (no bias).  With x[i,j] = softmax_scale * q_i . k_j, c = softcap > 0
 * and shift = Nk - Nq per sequence:
 *     S[i,j] = c * tanh(x[i,j] / c)  -  alibi_slopes[b * slopes_batch_stride + h] * | i + shift - j |        (second term only with slopes)
 * then the mask (is_causal / the window, as the _alibi entry points read them; (-1, -1) = none), the softmax and P V.  The ORDER is FlashAttention-2's: the cap
 * on the scaled scores first, then the bias, then the mask.  Everything downstream is defined on S: lse is the true logsumexp_j S[i,j] (capped, biased,
 * masked; tfa_bwd_softcap and tfa_merge consume it unchanged); rows that see no key get out = 0 and lse = +inf.  The backward recomputes P from the same S,
 * forms dS = P o (dP - delta) and passes dS * (1 - tanh^2(x / c)) on to dq and dk (the chain rule through the cap); dv and delta are as without a cap.
 * softcap is a host float: no gradient, nothing is read from the device, nothing synchronises, a call can be captured in a graph.  Zero slopes give the bits
 * of NULL slopes.
 * Every call runs the soft-capping form of the LOCAL instantiations, whatever the window and with or without slopes (one kernel per dtype, width and fixed /
 * varlen; the slopes are a launch-uniform branch in it): il8 (variant 30) or il4 (32) as tfa_fwd_alibi chooses, every tile through the compiler-scheduled
 * bodies, rounding rule TFA_RULE_LAZY for both dtypes; the backward is the dQ launch (which forms delta) and the fused dK/dV launch of that form,
 * deterministic, never the dS-workspace form.  tfa_fwd_suggest_splits / split-KV have no soft-capping form.
 * tanh: the GPU has no such instruction; the kernels form 1 - tanh(x / c) = 1 / (0.5 + exp2(2 log2(e) x / c - 1)) from one hardware exponential and one
 * hardware reciprocal (1 ulp each).  It saturates to -c / +c when the exponential underflows / overflows, never NaN for finite scores.  Accuracy: a capped
 * score is within 2^-20 * c (absolute, scaled-score domain) of the exact c * tanh(x / c) — 5e-5 at c = 50 — which is also the bound on what the cap adds
 * to the LSE's error; the derivative 1 - tanh^2 is formed as q (2 - q), q = 1 - tanh, without cancellation.
 * Refused, nothing launched: softcap <= 0 (0 included: without a cap call the other entry points), NaN or infinite (TFA_ERR_SCALE); with slopes, what
 * tfa_fwd_alibi refuses for them (TFA_ERR_ALIGN, TFA_ERR_STRIDE); and what the local form refuses, with its codes: head dims above 128 (TFA_ERR_HEAD_DIM),
 * fp32 inputs (TFA_ERR_DTYPE), any flag — TFA_FWD_EXACT_MAX included — (TFA_ERR_SHAPE), a window side below -1 (TFA_ERR_SHAPE), kv_offset / nk_total != 0
 * (TFA_ERR_SHAPE), Nq + Nk >= 2^28 (TFA_ERR_SHAPE), slices that need per-tile descriptors (TFA_ERR_STRIDE), a forced variant other than 30 / 32
 * (TFA_ERR_VARIANT).
 * Tolerances: the header's "which tolerance each path guarantees", LSE |d| <= 1e-4 * max(1, |lse|) as for ALiBi.
 * Rates: tools/bench_softcap.py measures them against the same masks without a cap (README.md, "Soft-capping"; DESIGN.md 8d). */
int tfa_fwd_softcap(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                    void* stream);
/* Validate and report the launch geometry of tfa_fwd_softcap without launching (no GPU needed). */
int tfa_fwd_softcap_plan(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                         int* grid, int* block, int* lds_bytes);
/* The kernel variant tfa_fwd_softcap runs for *p (30 or 32), or a negative TFA_ERR_* code. */
int tfa_fwd_softcap_variant(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
/* The row reference P is rounded against: TFA_RULE_LAZY (bf16 and fp16), or a negative TFA_ERR_* code. */
int tfa_fwd_softcap_rounding_rule(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                  int window_right);
/* Packed variable-length batches: b indexes the sequence, the bias distance is taken per sequence. */
int tfa_fwd_varlen_softcap(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                           int window_right, void* stream);
int tfa_fwd_varlen_softcap_plan(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                int window_right, int* grid, int* block, int* lds_bytes);
int tfa_fwd_varlen_softcap_variant(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                   int window_right);
int tfa_fwd_varlen_softcap_rounding_rule(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride,
                                         int window_left, int window_right);
/* The backward of a soft-capped forward (same softcap, slopes, window and params as tfa_bwd / tfa_bwd_varlen); _plan validates without launching. */
int tfa_bwd_softcap(const tfa_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                    void* stream);
int tfa_bwd_softcap_plan(const tfa_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right);
int tfa_bwd_varlen_softcap(const tfa_varlen_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                           int window_right, void* stream);
int tfa_bwd_varlen_softcap_plan(const tfa_varlen_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                int window_right);

/* ---- Dense additive bias and masks (scaled_dot_product_attention's attn_mask; FlashAttention-2 has no such argument) ------------------------
 * The same params structs as tfa_fwd / tfa_bwd plus a bias tensor and a window.  With bias broadcast to (B, H, Nq, Nk):
 *     S[i,j] = softmax_scale * q_i . k_j  +  bias[b, h, i, j]
 * then the mask (is_causal / the window, exactly as the _local entry points read them; (-1, -1) = none), the softmax and P V.  h is the QUERY head (GQA: the
 * H / Hk query heads of a K/V head have their own slices).  Everything downstream is defined on these biased scores: lse is the true logsumexp_j S[i,j]
 * INCLUDING the bias (tfa_bwd_bias and tfa_merge consume it); an entry of -inf masks its (i, j); a row without a finite score gets out = 0 and lse = +inf,
 * as everywhere else.  +inf and NaN in the bias are undefined (unspecified results, never an access outside the tensors).  The backward recomputes P from
 * the same biased scores and returns dq, dk, dv; the bias gets NO gradient.
 * tfa_attn_bias: `bias` points at element [0, 0, 0, 0] in DEVICE memory, dtype TFA_F32 or the dtype of q; stride[] counts ELEMENTS between batch entries,
 * query heads and query rows, 0 = that dimension is broadcast; the keys of a row are contiguous (unit stride).  The kernels' work items read the tensor
 * themselves — 8-byte (16-bit bias) or 16-byte (fp32) loads of four consecutive keys through one buffer descriptor per (b, h) slice whose extent is
 * ((Nq - 1) * stride[2] + Nk) * esize bytes: rows behind the last read as zeros, nothing outside the tensor is touched, elements between Nk and stride[2]
 * of a row are read and ignored.  The library never reads the tensor on the host: no copy, no synchronisation, a call can be captured in a graph and
 * replayed after the bias was overwritten in place.
 * Every call runs the bias form of the fixed-length LOCAL instantiations, whatever the window (full and causal attention carry unbounded sides): il8
 * (variant 30) or il4 (32) as tfa_fwd_alibi chooses for the same problem, same grid; every tile through the compiler-scheduled bodies, the tile's bias
 * requested at the top of the body ahead of the QK^T MFMAs and added to the raw scores (bias / softmax_scale) in front of the mask and the row maximum;
 * rounding rule TFA_RULE_LAZY for both dtypes.  Every tile the mask admits is visited: tiles that the bias masks completely are not skipped.  The backward
 * is the dQ launch (which forms delta) and the fused dK/dV launch of that form, deterministic; never the dS-workspace form.
 * Refused, nothing launched: a NULL struct or bias pointer (TFA_ERR_NULL); a dtype that is neither TFA_F32 nor q's (TFA_ERR_DTYPE); reserved_ != 0
 * (TFA_ERR_SHAPE); a base that is not 16-byte aligned (TFA_ERR_ALIGN); a negative stride, a non-zero stride that is not a multiple of 8 elements, a row
 * stride below Nk, or a (b, h) slice of 2 GiB or more (TFA_ERR_STRIDE); and what the ALiBi form refuses, with its codes: head dims above 128
 * (TFA_ERR_HEAD_DIM), fp32 q (TFA_ERR_DTYPE), any flag — TFA_FWD_EXACT_MAX included — (TFA_ERR_SHAPE), a window side below -1, kv_offset / nk_total != 0,
 * Nq + Nk >= 2^28 (TFA_ERR_SHAPE), q / k / v / out slices that need per-tile descriptors (TFA_ERR_STRIDE), a forced variant other than 30 / 32
 * (TFA_ERR_VARIANT).  Out of scope: a gradient for the bias; a bias with packed variable-length, KV-cache or paged calls, with alibi_slopes or softcap, with
 * split-KV; bool or 8-bit masks read by the kernel (convert them to 0 / -inf); skipping fully masked tiles.
 * Tolerances: the header's "which tolerance each path guarantees", LSE |d| <= 1e-4 * max(1, |lse|) as for ALiBi.
 * Cost: a full-shape bias is B * H * Nq * Nk * esize bytes that come from HBM once per forward and twice per backward; tools/bench_bias.py prints that
 * floor beside each measured time (README.md, "Attention bias"). */
typedef struct tfa_attn_bias {
  const void* bias;
  int32_t dtype;       /* TFA_F16 / TFA_BF16 (q's) / TFA_F32 */
  int32_t reserved_;   /* 0 */
  int64_t stride[3];   /* batch, head, row in elements; 0 = broadcast */
} tfa_attn_bias;
int tfa_fwd_bias(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, void* stream);
/* Validate and report the launch geometry of tfa_fwd_bias without launching (no GPU needed): tfa_fwd_alibi_plan's for the same problem. */
int tfa_fwd_bias_plan(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, int* grid, int* block, int* lds_bytes);
/* The kernel variant tfa_fwd_bias runs for *p (30 or 32), or a negative TFA_ERR_* code. */
int tfa_fwd_bias_variant(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right);
/* The row reference P is rounded against: TFA_RULE_LAZY (bf16 and fp16), or a negative TFA_ERR_* code. */
int tfa_fwd_bias_rounding_rule(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right);
/* The backward of a biased forward (same bias, window and params as tfa_bwd); _plan validates without launching. */
int tfa_bwd_bias(const tfa_bwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, void* stream);
int tfa_bwd_bias_plan(const tfa_bwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right);

/* ---- attention over a K/V cache (FlashAttention-2's flash_attn_with_kvcache: cache_seqlens, paged KV, in-place append) ------------------------
 * The inference step of a serving loop: B sequences, each with its own number of cached keys, the lengths in DEVICE memory.
 *   cache_seqlens: int32, B entries, never read on the host — no copy, no synchronisation; a call can be captured in a graph and replayed after the
 *     lengths were advanced in place.  Every work item reads its sequence's length itself (a scalar load): len_b = cache_seqlens[b] + n_new, clamped
 *     into [0, capacity].  Sequence b attends keys [0, len_b); a sequence with len_b = 0 gets out = 0, lse = +inf.
 *   contiguous cache (block_table NULL): k_cache / v_cache are (B, capacity, Hk, D) by strides {batch, head, row} in elements, unit stride along D.
 *   paged cache (block_table != NULL): k_cache / v_cache are (num_pages, page_size, Hk, D) by strides {page, head, row}; key j of sequence b is row
 *     j % page_size of page block_table[b * block_table_stride + j / page_size]; capacity = max_blocks * page_size (the caller states it); page_size is a
 *     positive multiple of 64, so a 64-key tile never straddles pages.  Entries are clamped into [0, num_pages) for reading; the append drops a row whose
 *     entry lies outside.
 *   is_causal: bottom-right aligned per sequence — key j is visible to query row i iff j <= i + (len_b - Nq); rows that see no key (len_b < Nq): out = 0,
 *     lse = +inf.
 *   k_new / v_new (both or neither; n_new rows per sequence, (B, n_new, Hk, D) by strides {batch, head, row}): copied into the cache at key positions
 *     cache_seqlens[b] + t first (a launch of its own on `stream`, 16-byte loads and stores), then attended.  A row at or beyond the capacity is not
 *     written — and not attended, as the length is clamped.  Nothing is stored outside the cache tensors.  cache_seqlens itself is not modified: the
 *     caller advances it, as in FlashAttention-2.
 * Whatever the cache holds behind len_b — the tail of the last page, stale keys of an earlier request, NaN — is never read into a result: every K/V buffer
 * descriptor ends at the last valid key, so those rows arrive as zeros (a masked P = 0 times a non-finite V would be NaN).
 * Kernel: the KV-cache form of the LDS-DMA kernel behind tfa_fwd_splitkv (variant 17; exact running max: TFA_RULE_EXACT_MAX), 64 or 128 wide.  The key range
 * of EVERY sequence is cut into `splits` chunks from its own length on the device — chunk_b = round_up(ceil(len_b / splits), 64) — so ragged batches stay
 * balanced; chunks behind a sequence's end give empty partials, which tfa_merge skips.  splits == 1 writes out / lse directly (any out strides, no workspace);
 * splits >= 2 writes fp32 partials to `workspace` and tfa_merge writes out, which must then be contiguous (B, H, Nq, D).  lse: (B, H, Nq) fp32 or NULL.
 * GQA / MQA decode (Nq == 1, Hk < H, H / Hk <= 128): the H / Hk query heads of a K/V head run as rows of one problem, K and V stream once per K/V head.
 * Nq > 1 runs unpacked here — K and V are streamed once per QUERY head — and packed on request: tfa_fwd_kvcache_pack(…, TFA_PACK_GQA_ON, …) below.
 * Everything is enqueued on `stream` alone — append, attention, merge, in that order; no side streams, no events: a captured step is a straight line.
 * Refused, nothing launched: a NULL params / q / out / k_cache / v_cache / cache_seqlens, one of k_new / v_new without the other or with n_new <= 0
 * (TFA_ERR_NULL / TFA_ERR_SHAPE); dtype other than TFA_F16 / TFA_BF16 (TFA_ERR_DTYPE); D not a multiple of 8 in [8, 128] (TFA_ERR_HEAD_DIM); B, H, Hk, Nq,
 * capacity <= 0, H % Hk != 0, n_new < 0, splits < 1 (TFA_ERR_SHAPE); paged: page_size not a positive multiple of 64, capacity not a multiple of page_size,
 * num_pages <= 0 (TFA_ERR_SHAPE), block_table_stride < capacity / page_size (TFA_ERR_STRIDE); strides negative, not 16-byte aligned or overlapping rows, a
 * contiguous (b, h) slice — or a page — that does not fit one 2 GiB descriptor, out not contiguous (B, H, Nq, D) with splits >= 2 (TFA_ERR_STRIDE); base
 * pointers not 16-byte aligned, block_table / cache_seqlens / lse not 4-byte aligned, a misaligned workspace (TFA_ERR_ALIGN); a NULL workspace with
 * splits >= 2 (TFA_ERR_NULL); softmax_scale not finite or <= 0 (TFA_ERR_SCALE).
 * Out of scope: rotary embedding inside the call (done by composition: tfa_rotary on q and k_new with seqlen_offsets = cache_seqlens, then this call), cache_batch_idx,
 * cache_leftpad, windows, softcap, ALiBi, head dims above 128, fp32 inputs, TFA_FWD_EXACT_MAX, a backward.
 * Tolerances: the header's "which tolerance each path guarantees".  Measured: profiles/kvcache_bench.txt (tools/bench_kvcache.py), quoted in README.md. */
typedef struct tfa_kvcache_params {
  const void* q;                 /* (B, H, Nq, D) by q_stride */
  void* out;                     /* (B, H, Nq, D) by o_stride, input dtype */
  float* lse;                    /* (B, H, Nq) fp32 contiguous, or NULL to skip */
  void* k_cache;                 /* written only by the append */
  void* v_cache;
  const int32_t* block_table;    /* device (B, max_blocks) int32, or NULL: contiguous cache */
  const int32_t* cache_seqlens;  /* device, B entries */
  const void* k_new;             /* (B, n_new, Hk, D), or NULL */
  const void* v_new;
  int32_t B, H, Hk, Nq, D;
  int32_t capacity;              /* keys a sequence can hold: Nk_max, or max_blocks * page_size */
  int32_t n_new;                 /* rows of k_new / v_new per sequence; 0 without them */
  int32_t page_size;             /* paged: keys per page, a positive multiple of 64; contiguous: ignored */
  int32_t num_pages;             /* paged: pages in k_cache / v_cache; contiguous: ignored */
  int32_t reserved_;             /* must be 0 */
  int64_t q_stride[3];           /* batch, head, row (elements) */
  int64_t o_stride[3];
  int64_t k_stride[3];           /* batch (contiguous) or page (paged), head, row */
  int64_t v_stride[3];
  int64_t knew_stride[3];        /* batch, head, row */
  int64_t vnew_stride[3];
  int64_t block_table_stride;    /* elements between the rows of block_table */
  float softmax_scale;
  int32_t is_causal;
  int32_t dtype;                 /* TFA_F16 or TFA_BF16: q, caches, k_new / v_new, out */
  int32_t reserved2_;            /* must be 0 */
} tfa_kvcache_params;

/* Append (when k_new / v_new are given), attend, merge — on `stream`, asynchronous, never allocates, never reads device memory on the host.
 * workspace: tfa_fwd_kvcache_workspace(p, splits) floats, 16-byte aligned; may be NULL when that is 0 (splits == 1). */
int tfa_fwd_kvcache(const tfa_kvcache_params* p, int splits, float* workspace, void* stream);
/* Floats of workspace the call uses: 0 for one chunk, else chunks * B * H * Nq * (D + 1) — chunks = min(splits, ceil(capacity / 64)); negative = TFA_ERR_*. */
long long tfa_fwd_kvcache_workspace(const tfa_kvcache_params* p, int splits);
/* Validate *p and `splits` without launching (no GPU needed); on success optionally reports the attention launch's geometry. */
int tfa_fwd_kvcache_plan(const tfa_kvcache_params* p, int splits, int* grid, int* block, int* lds_bytes);
/* The split count to use for *p, from host-known sizes only: the capacity stands in for the lengths, the CU count comes from the library.  1 when the
 * grid already fills the chip (B * heads * ceil(rows / 128) workgroups on more than half of the CUs — heads = Hk and rows = H / Hk for packed GQA decode),
 * the capacity is below 4096 keys, or causal with Nq > capacity / 4; else one chunk per idle CU (two per CU from a quarter of the CUs on), at most
 * capacity / 1024 and at most 32: tfa_fwd_suggest_splits' rule. */
int tfa_fwd_kvcache_suggest_splits(const tfa_kvcache_params* p);
/* The append alone (k_new / v_new required): q, out, lse, Nq, H, softmax_scale and is_causal are not looked at. */
int tfa_kvcache_append(const tfa_kvcache_params* p, void* stream);

/* ---- an fp8 (OCP e4m3fn) K/V cache behind the same calls ---------------------------------------------------------------------------------------
 * k_cache / v_cache hold e4m3fn bytes (torch.float8_e4m3fn: 254 finite codes, 0x7f / 0xff NaN, no infinities) with one fp32 descale per (sequence, K/V head);
 * q, out and the new rows k_new / v_new keep the 16-bit dtype p->dtype.  The calls take tfa_kvcache_params as above plus this struct; in them k_stride /
 * v_stride count cache ELEMENTS, which are bytes, and everything said above about lengths, chunks, pages, empty rows, packing, splits, the single stream and graph
 * capture holds unchanged.
 *   Definition: attention over the exactly decoded cache.  e4m3fn -> bf16 / f16 is exact for every finite code, so
 *     S[i,j] = softmax_scale * k_descale[b,hk] * q_i . dec(k8_j),  causal mask,  softmax,  out = v_descale[b,hk] * P . dec(v8),  lse = logsumexp(S).
 *   Q and P are not quantised and no fp8 MFMA is used: with descales of 1.0 (or NULL) out and lse are BIT-IDENTICAL to tfa_fwd_kvcache over the caches converted to
 *   p->dtype, for the same `splits`.  k_descale is folded into the score scale of the work item, v_descale multiplied into O in fp32 in front of its one rounding
 *   (splits >= 2: into the fp32 partials; tfa_merge is unchanged).
 *   k_descale / v_descale: device fp32, element (b, hk) at b * stride[0] + hk * stride[1] (elements; 0 allowed: a broadcast per-tensor scale), or NULL = 1.0.  With a
 *     paged cache they are still indexed by the sequence b, not by the page.  Read by the kernels only (a scalar load per work item) — never on the host, so a captured
 *     step sees values overwritten in place.  Precondition: finite and > 0; other values give unspecified results but no access out of bounds.
 *   Zero fill: the descriptor extents end at the last valid key, now in bytes of 1-byte elements; the byte 0x00 decodes to +0, so NaN codes behind len_b never reach a result.
 *   Append (k_new / v_new, 16-bit): quantised on the device and stored in place, byte = rne_e4m3fn(clamp(float(x) / descale[b,hk], -448, 448)) — a true fp32 division,
 *     the clamp in front of the (non-saturating) conversion, NaN stays NaN; capacity and page checks as in tfa_kvcache_append; the rows are then attended as quantised.
 *   D: a multiple of 16 in [16, 128] — 16-byte rows of 1-byte elements, and no 16-byte chunk reaches into the next head's bytes.
 * Kernel: the e4m3 form of the KV-cache kernel.  A tile's LDS-DMA becomes register staging: 8 bytes per lane and piece through the same descriptors, decoded once
 * (v_cvt_pk_f32_fp8, then the exact conversion to p->dtype) and written to the LDS bytes the DMA would have filled, so the tile loop, the LDS layout and the LDS size —
 * 4 * 64 * W * 2 bytes, W = 64 or 128 the kernel width: 32 / 64 KiB, two workgroups per CU — are the 16-bit form's.  Grid and block equal tfa_fwd_kvcache_plan's.
 * Refused, nothing launched — everything tfa_fwd_kvcache refuses (p->dtype: TFA_F16 / TFA_BF16 only), and: a NULL tfa_kvcache_fp8 (TFA_ERR_NULL); format other than
 * TFA_KV_E4M3 (TFA_ERR_DTYPE); reserved_ != 0 (TFA_ERR_SHAPE); D not a multiple of 16 in [16, 128] (TFA_ERR_HEAD_DIM); cache strides not multiples of 16 bytes, a
 * negative descale stride (TFA_ERR_STRIDE); a descale pointer not 4-byte aligned (TFA_ERR_ALIGN).
 * tfa_fwd_kvcache_suggest_splits serves both cache types (it reads sizes only).
 * Out of scope: e5m2 and e4m3fnuz caches, per-token or per-page scales, an fp8 q or out, fp8 in tfa_fwd / varlen / the backward, D > 128, and what tfa_fwd_kvcache leaves out.
 * The 2 GiB bound on a contiguous (b, h) slice is still counted as for 2-byte elements (TFA_ERR_STRIDE as in tfa_fwd_kvcache for the same strides): an fp8 cache
 * halves the bytes streamed and stored, it does not double the rows one contiguous slice may span; pages are not affected.
 * Not measured yet (tools/bench_kvcache_fp8.py). */
#define TFA_KV_E4M3 1
typedef struct tfa_kvcache_fp8 {
  const float* k_descale;        /* device, or NULL = 1.0 */
  const float* v_descale;
  int64_t k_descale_stride[2];   /* batch, K/V head (elements; 0 allowed) */
  int64_t v_descale_stride[2];
  int32_t format;                /* TFA_KV_E4M3 */
  int32_t reserved_;             /* must be 0 */
} tfa_kvcache_fp8;
int tfa_fwd_kvcache_fp8(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits, float* workspace, void* stream);
long long tfa_fwd_kvcache_fp8_workspace(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits);
int tfa_fwd_kvcache_fp8_plan(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits, int* grid, int* block, int* lds_bytes);
int tfa_kvcache_append_fp8(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, void* stream);

/* ---- the same calls with the GQA packing chosen by the caller (FlashAttention-3's pack_gqa) ------------------------------------------------------
 * pack_gqa is a scheduling choice: it never changes the definition of out or lse, the append, the refusals, the alignment rules or the workspace size.
 *   TFA_PACK_GQA_AUTO  what tfa_fwd_kvcache / tfa_fwd_kvcache_fp8 run — the same launches, the same bits: packed iff Nq == 1 (Hk < H, H / Hk <= 128).
 *   TFA_PACK_GQA_OFF   unpacked, also at Nq == 1: K and V stream once per query head (the A/B arm).
 *   TFA_PACK_GQA_ON    packed whenever Hk < H and G = H / Hk <= 128.  Nq == 1: AUTO's packed call, the same bits.  Nq > 1: the packed form of the KV-cache
 *     kernel — the Nq * G rows (position t, head g) of K/V head hk run as rows of one problem over sequence b's keys in POSITION-MAJOR order, row = t * G + g, so
 *     head hk * G + g at position t = row / G.  Causal visibility stays per position — key j is visible iff j <= t + (len_b - Nq) — and, the last visible key still
 *     growing with the row index, so do the kernel's causal tile bounds (one magic division per row).  Q rows are loaded by two strides (t * row stride + g * head
 *     stride, any q strides the unpacked call takes), out / lse / the fp32 partials are written to their unpacked (b, h, t) places: workspace layout, tfa_merge and
 *     every tensor layout are the unpacked call's.  K and V stream once per K/V head while Nq * G <= 128; beyond, ceil(Nq * G / 128) query blocks per (b, hk)
 *     (causal: paired heavy / light on the packed block index) — still fewer passes than unpacked.  With H == Hk, or G > 128, or a head group of q / out whose rows
 *     do not fit the 32-bit byte offsets of one 2 GiB descriptor, ON runs the unpacked call: packing is an optimisation, never a requirement and never an error.
 *   any other value: TFA_ERR_SHAPE.
 * q8 == NULL: the 16-bit cache (tfa_fwd_kvcache's); else the e4m3 cache (tfa_fwd_kvcache_fp8's).  Lengths on the device, per-sequence chunks, paged caches, descales,
 * empty rows (out = 0, lse = +inf), descriptors that end at the last valid key, launches on `stream` alone, graph capture: as in the unpacked calls.
 * _workspace: the same number of floats whatever pack_gqa.  _plan: the attention launch's geometry — packed, B * Hk * work items * chunks workgroups, work items =
 * query blocks nmb = ceil(Nq * G / 128), or ceil(nmb / 2) causal.  _suggest_splits: tfa_fwd_kvcache_suggest_splits' rule with the workgroups counted from the
 * geometry the mode runs (packed: B * Hk * ceil(Nq * G / 128)); AUTO equals tfa_fwd_kvcache_suggest_splits.
 * Kernels: csrc/tfa_fwd_kernel_dma.h (KvcPacked; fwd_kernel_dma_kvc over it) — instantiations of their own, so every other kernel keeps its instructions
 * (profiles/kvcache_packgqa_isa_unchanged.txt).  Measured: profiles/kvcache_packgqa_bench.txt (tools/bench_kvcache_packgqa.py), quoted in README.md. */
#define TFA_PACK_GQA_AUTO 0
#define TFA_PACK_GQA_ON   1
#define TFA_PACK_GQA_OFF  2
int tfa_fwd_kvcache_pack(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8 /* NULL: 16-bit cache */, int pack_gqa, int splits, float* workspace, void* stream);
long long tfa_fwd_kvcache_pack_workspace(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack_gqa, int splits);
int tfa_fwd_kvcache_pack_plan(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block, int* lds_bytes);
int tfa_fwd_kvcache_pack_suggest_splits(const tfa_kvcache_params* p, int pack_gqa);

/* ---- the same attention for PACKED RAGGED query rows (FlashAttention-3's flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=), the interface this mirrors) ------------
 * One call for a unified batch — decode rows, chunked-prefill rows, any mix — whose row counts live on the device.  q is packed (total_q, H, D); sequence b owns the
 * query rows [q0_b, q0_b + nq_b), q0_b = clamp(cu_seqlens_q[b], 0, total_q), nq_b = clamp(cu_seqlens_q[b + 1] - cu_seqlens_q[b], 0, min(max_seqlen_q, total_q - q0_b)):
 * every work item reads and clamps them itself, as it reads cache_seqlens; nothing is read on the host, a captured launch follows in-place updates of all three arrays.
 * Sequence b attends keys [0, len_b), len_b = clamp(cache_seqlens[b], 0, capacity) — the length INCLUDING the rows appended for this step (tfa_kvcache_append_varlen
 * is the append for packed rows; k_new / v_new must be NULL and n_new 0 here: TFA_ERR_SHAPE).  Causal: bottom-right aligned per sequence, key j visible to row t of
 * sequence b iff j <= t + (len_b - nq_b).  A row that sees no key (len_b == 0, or len_b < nq_b under causal) gives out = 0, lse = +inf; nq_b == 0 is legal.  Rows of
 * out / lse that belong to no sequence are not written; nothing outside the tensors is read or written whatever the three device arrays hold.
 * In *p: B = the sequences (cu_seqlens_q has B + 1 entries; the batch of a contiguous cache, the rows of block_table, cache_seqlens and the descales); Nq is not looked
 * at; q_stride / o_stride are {ignored, head, row}; lse is (H, total_q) fp32 contiguous or NULL.  splits == 1: out by any o_stride; splits >= 2: out must be the
 * contiguous (H, total_q, D) (TFA_ERR_STRIDE) and tfa_merge runs unchanged over H * total_q rows.  Paged and contiguous caches, q8 (NULL: 16-bit cache; else e4m3 with
 * descales by sequence), per-sequence chunks, zero fill behind the lengths, launches on `stream` alone: as in tfa_fwd_kvcache_pack.
 * pack_gqa: TFA_PACK_GQA_AUTO = ON here — packed (position-major rows t * G + g of a K/V head) whenever Hk < H and G = H / Hk <= 128 — or OFF; H == Hk and G > 128 run
 * unpacked (KvcPacked serves G = 2..128; MHA is why the unpacked varlen-q instantiations exist).  A scheduling choice: it never changes the result's definition.
 * Geometry: work item = (sequence, K/V head or head, query block, chunk); the launch carries nmb = ceil(max_seqlen_q * G' / 128) blocks per (sequence, head), G' = G
 * packed, 1 unpacked; causal blocks pair heavy / light on that launch-level index; _plan's grid = B * heads * work items * chunks.  A block with no row of its sequence
 * issues no Q, K or V request and no store.  The grid is sized by max_seqlen_q — one 2048-row prefill chunk in a batch of decode rows makes most work items empty,
 * each costing its scalar loads and an exit: tfa_fwd_kvcache_varlen_sched below runs the same blocks from a device-built work list that holds the non-empty items only.
 * _workspace: 0 for one chunk, else chunks * H * total_q * (D + 1) floats.  _suggest_splits: tfa_fwd_kvcache_pack_suggest_splits' rule with the workgroups counted as
 * heads * min(B * nmb, ceil(total_q * G' / 128) + B) — the second term bounds the non-empty blocks from what the host knows.
 * Refused, nothing launched: a NULL vq or cu_seqlens_q (TFA_ERR_NULL); max_seqlen_q <= 0, total_q <= 0, a nonzero reserved field (TFA_ERR_SHAPE); a cu_seqlens_q that
 * is not 4-byte aligned (TFA_ERR_ALIGN); everything tfa_fwd_kvcache_pack refuses.
 * Kernels: csrc/tfa_fwd_kernel_dma.h (KvcVarlenQ; fwd_kernel_dma_kvc over it) — instantiations and units of their own, so every other kernel keeps its instructions
 * (profiles/kvcache_varlenq_isa_unchanged.txt). */
typedef struct tfa_kvcache_varlen_q {
  const int32_t* cu_seqlens_q;   /* device, B + 1 entries */
  int32_t max_seqlen_q, total_q;
  int32_t reserved_[2];          /* must be 0 */
} tfa_kvcache_varlen_q;
int tfa_fwd_kvcache_varlen(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8 /* NULL: 16-bit cache */, int pack_gqa, int splits, float* workspace, void* stream);
long long tfa_fwd_kvcache_varlen_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits);
int tfa_fwd_kvcache_varlen_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block, int* lds_bytes);
int tfa_fwd_kvcache_varlen_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa);

/* ---- the SCHEDULED form of the packed-q call (FlashAttention-3's get_scheduler_metadata(...) / scheduler_metadata=, the interface this mirrors) -----------------------
 * tfa_fwd_kvcache_varlen launches B * heads * ceil(max_seqlen_q * G' / 128) query blocks per chunk whatever the row counts are.  Here a serving step builds a work list
 * once — tfa_kvcache_varlen_schedule: ONE launch of one workgroup on `stream`, nothing read on the host, nothing allocated — and every layer's attention call
 * (tfa_fwd_kvcache_varlen_sched) launches heads * bound * chunks workgroups that take their (sequence, item) from it.  Both launches capture into a graph; a replay
 * follows in-place updates of cu_seqlens_q and cache_seqlens as long as B, max_seqlen_q, total_q, the packing and is_causal stay what the list was sized for.
 * metadata: int32 in device memory, 8-byte aligned, tfa_kvcache_varlen_schedule_size elements = 8 + 2 * bound:
 *   [0..8)       header: n_items, B, G', causal, max_seqlen_q, total_q, bound, 0          (n_items is read by the kernel; the rest is for debugging and tests)
 *   [8 + 2 i ..) item i: (b, wi), i < n_items — ascending b, then ascending wi; a sequence without rows contributes nothing.  (Longest-first is not done.)
 *   (q0_b, nq_b) are clamped as tfa_fwd_kvcache_varlen's work items clamp them; nb_b = ceil(nq_b * G' / 128) blocks.  Not causal: nb_b items, wi = the block.  Causal:
 *   ceil(nb_b / 2) items, wi = the heavy / light pair of blocks (nb_b - 1 - wi, wi) of the SEQUENCE's own count (the middle block alone when nb_b is odd).
 * bound, the item rows the buffer holds and the per-head grid, is what the host knows: with nmb = ceil(max_seqlen_q * G' / 128) and F = ceil(total_q * G' / 128),
 *   not causal:  min(B * nmb, F + B)                        — a sequence of n rows fills at most n * G' / 128 + 1 blocks, and the rows sum to at most total_q;
 *   causal:      min(B * ceil(nmb / 2), floor((F + 2 B) / 2)) — ceil(nb / 2) <= (nb + 1) / 2 for every sequence, summed over the blocks bounded above.
 *   A cu_seqlens_q that is not monotonic can describe more items; the list then ends at `bound` (n_items is clamped, nothing is written behind the buffer) and the
 *   rows of the dropped items are not written.
 * The list is a hint to the attention kernel, never trusted: n_items is clamped into [0, bound], b into [0, B), nq_b and nb_b are recomputed from cu_seqlens_q, a wi
 * outside the sequence's own items is an empty item.  Stale, foreign or random metadata gives unspecified or unwritten rows; nothing outside the tensors is read or
 * written — the guarantee the call gives for cu_seqlens_q, cache_seqlens and block_table.  With the list of this batch, out and lse equal tfa_fwd_kvcache_varlen's bit
 * for bit: a block's arithmetic does not depend on the work item that runs it.
 * tfa_kvcache_varlen_schedule* read of *p only B, H, Hk; is_causal is their own argument (the attention call takes p->is_causal: the two must agree).  pack_gqa as above.
 *   _schedule_size: the int32 elements, or a negative tfa_status.  _schedule_plan: grid 1, block 256, the scan's LDS bytes; validates without a GPU.
 *   Refused, nothing launched: NULL p / vq / cu_seqlens_q / metadata (TFA_ERR_NULL); B, H, Hk <= 0, H % Hk != 0, a bad pack_gqa, max_seqlen_q <= 0, total_q <= 0, a nonzero
 *   reserved field (TFA_ERR_SHAPE); cu_seqlens_q not 4-byte or metadata not 8-byte aligned (TFA_ERR_ALIGN).
 * tfa_fwd_kvcache_varlen_sched: tfa_fwd_kvcache_varlen with the list; _workspace and _suggest_splits are tfa_fwd_kvcache_varlen's, unchanged.  _sched_plan's grid =
 *   heads * bound * chunks.  Refused: a NULL metadata (TFA_ERR_NULL), one not 8-byte aligned (TFA_ERR_ALIGN), everything tfa_fwd_kvcache_varlen_plan refuses, and a
 *   packing that tfa_fwd_kvcache_varlen would silently drop (a head group's rows beyond one descriptor: TFA_ERR_STRIDE — the list was sized for the packing named).
 * Kernels: csrc/tfa_kvcache_schedule.hip; csrc/tfa_fwd_kernel_dma.h (KvcSched, behind KvcVarlenQ) — instantiations and units of their own, so every other kernel
 * keeps its instructions (profiles/kvcache_sched_isa_unchanged.txt). */
long long tfa_kvcache_varlen_schedule_size(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal);
int tfa_kvcache_varlen_schedule(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal, int32_t* metadata, void* stream);
int tfa_kvcache_varlen_schedule_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal, int* grid, int* block, int* lds_bytes);
int tfa_fwd_kvcache_varlen_sched(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8 /* NULL: 16-bit cache */, int pack_gqa, int splits, const int32_t* metadata, float* workspace, void* stream);
int tfa_fwd_kvcache_varlen_sched_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block, int* lds_bytes);

/* ---- a SLIDING WINDOW over the K/V cache (the model configs' sliding_window; FlashAttention's window_size = (window_left, 0)) -------------------------------
 * One entry point for every form above: vq == NULL is the 4-D call (tfa_fwd_kvcache_pack's arguments, k_new / v_new appended first), vq != NULL the packed-q call
 * (tfa_fwd_kvcache_varlen's), metadata != NULL its scheduled form (tfa_fwd_kvcache_varlen_sched's; needs vq); q8 != NULL an e4m3 cache.  p->is_causal must be set.
 * Definition: key j is visible to row t of sequence b iff  t + shift_b - window_left <= j <= t + shift_b  and  0 <= j < len_b,  shift_b = len_b - nq_b, with len_b and
 *   nq_b clamped exactly as the underlying form clamps them (Nq in the 4-D form, the clamped cu_seqlens_q difference in the packed form): a row sees its own key and
 *   the window_left keys in front of it.  A row that sees no key gives out = 0, lse = +inf.  window_left >= capacity reaches every key a row can see.
 * Chunks: with lo_b = max(0, shift_b - window_left) the first key the sequence's first row sees and lo64_b = lo_b & ~63, the range cut into the call's chunks is
 *   [lo64_b, len_b), not [0, len_b): chunk_b = round_up(ceil((len_b - lo64_b) / chunks), 64), chunk s covers [lo64_b + s * chunk_b, min(len_b, lo64_b + (s + 1) *
 *   chunk_b)).  Chunk starts stay multiples of 64 (a tile never straddles a page); trailing empty chunks give the empty partials tfa_merge skips.  The chunk count, the
 *   workspace size and the merge are the underlying form's.
 * What is touched (the promise to an engine that frees the pages behind the window): no work item of sequence b loads a block-table entry of a page that ends at or
 *   before lo64_b, and none loads a K/V byte in front of key lo64_b.  Those table entries may hold anything, those pages may hold NaN.  Inside a query block the tile
 *   loop starts at the first 64-key tile some row of the block sees (packed rows: per position t = row / G), and a wave skips the tiles in front of its own first
 *   row's window.  Behind len_b the descriptors end as they do in every form.
 * Finite keys: the keys of a VISITED tile that lie left of a row's window are masked to -inf — they are the sequence's own older keys, at or behind lo64_b, and the
 *   caller keeps them finite: P = 0 times a NaN V row is NaN.
 * GQA at Nq == 1 (vq == NULL): TFA_PACK_GQA_AUTO and _ON run the G heads of a K/V head as position-major packed rows (t = row / G = 0, the causal bounds hold), so K/V
 *   streams once per K/V head; at Nq > 1 the packing follows tfa_fwd_kvcache_pack (ON packs, AUTO does not).  Packed-q calls pack as tfa_fwd_kvcache_varlen does.
 * _window_suggest_splits: the underlying form's rule with min(capacity, round_up(window_left + rows, 64) + 64) standing in for the lengths, rows = Nq or max_seqlen_q.
 * _window_plan: the underlying form's grid, block and LDS bytes (the window changes no launch geometry); validates without a GPU.  A plan has no list: `scheduled`
 *   != 0 asks for the scheduled form's geometry (tfa_fwd_kvcache_varlen_sched_plan's; needs vq), 0 for the unscheduled one's.
 * Refused, nothing launched: window_left < 0, p->is_causal == 0, metadata without vq (TFA_ERR_SHAPE); everything the underlying form refuses, with its codes.
 * Kernels: csrc/tfa_fwd_kernel_dma.h (KvcWindow, behind the form's struct; fwd_kernel_dma_kvc over it) — the causal template, the 16-bit direct output and the fp32 partials,
 * units of their own (tfa_kvc_inst_win_*, tfa_kvc8_inst_win_*), so every other kernel keeps its instructions (profiles/kvcache_window_isa_unchanged.txt). */
int tfa_fwd_kvcache_window(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq /* NULL: 4-D */, const tfa_kvcache_fp8* q8 /* NULL: 16-bit cache */, int pack_gqa, int window_left, int splits, const int32_t* metadata /* NULL: unscheduled; needs vq */, float* workspace, void* stream);
int tfa_fwd_kvcache_window_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int window_left, int splits, int scheduled, int* grid, int* block, int* lds_bytes);
long long tfa_fwd_kvcache_window_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int window_left, int splits);
int tfa_fwd_kvcache_window_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int window_left);

/* ---- a TREE MASK over the step's new keys (the verification step of a speculative token tree: EAGLE, Medusa, SpecInfer-style drafts) ---------------------------------
 * One entry point for every form above, as tfa_fwd_kvcache_window: vq == NULL is the 4-D call (k_new / v_new appended first), vq != NULL the packed-q call, metadata !=
 * NULL its scheduled form (needs vq); q8 != NULL an e4m3 cache.  p->is_causal must be set.
 * Definition, for row t of sequence b, with len_b and nq_b clamped exactly as the underlying form clamps them and base_b = len_b - nq_b (its shift_b): key j is visible iff
 *   (1) 0 <= j < len_b,  (2) j <= t + base_b — the causal rule as it stands; trees are stored parents-first —  and  (3) with s = j - base_b:  s < 0, or s >= 64, or
 *   bit s of the row's 64-bit word is set.  The mask only removes keys from what causal admits, and only among the first 64 new keys of a sequence: the committed
 *   prefix is always seen, and so is a new key from the 64th on (sequences that bring more than 64 rows; all-ones words make such a sequence plain causal — a
 *   chunked-prefill sequence beside tree-verify sequences in one batch).  Any sub-causal pattern is legal: it need not be closed under ancestry, and a row whose own
 *   bit is clear is legal.  A row that sees no key gives out = 0, lse = +inf.  An all-ones word gives the plain causal call's bits for that row.
 * The words: row t of sequence b reads mask[b * batch_stride + t * row_stride] in the 4-D form, mask[(q0_b + t) * row_stride] in the packed form (q0_b the
 *   sequence's clamped first packed row; batch_stride is not read), strides in 8-byte elements, >= 0.  Read on the device only, by the lane that owns the row, two dwords once
 *   per query block, through an index inside the rows the form itself trusts: no access outside B x Nq (total_q) words whatever the lengths hold.  No synchronisation;
 *   a captured launch replayed after the words were overwritten in place computes with the new words.
 * Finite keys: a masked new key is multiplied by P = 0, so the new keys must be finite (they were just appended).
 * The mask removes no tile: chunks, tile bounds, grid, workspace and the split suggestion are the underlying form's (_tree_plan, _tree_workspace, _tree_suggest_splits
 *   mirror the _window family argument for argument and return the form's numbers).  At most the two 64-key tiles per chunk that hold the new keys take the masked tile body
 *   on the mask's account.
 * GQA at Nq == 1 (vq == NULL): as tfa_fwd_kvcache_window — TFA_PACK_GQA_AUTO and _ON run position-major packed rows.
 * Refused, nothing launched: a NULL tree or mask (TFA_ERR_NULL), a mask that is not 8-byte aligned (TFA_ERR_ALIGN), a negative stride (TFA_ERR_STRIDE), p->is_causal == 0,
 *   metadata without vq (TFA_ERR_SHAPE); everything the underlying form refuses, with its codes.  No window: a tree mask with a sliding window is not implemented.
 * Kernels: csrc/tfa_fwd_kernel_dma.h (KvcTree, behind the form's struct; fwd_kernel_dma_kvc over it) — the causal template, the 16-bit direct output and the fp32 partials,
 * units of their own (tfa_kvc_inst_tree_*, tfa_kvc8_inst_tree_*), so every other kernel keeps its instructions (profiles/kvcache_tree_isa_unchanged.txt). */
typedef struct tfa_kvcache_tree {
  const void* mask;              /* device, 8-byte words (int64): bit s of a row's word = the row sees the s-th new key of its sequence */
  int64_t batch_stride;          /* words between sequences (4-D form; not read in the packed form) */
  int64_t row_stride;            /* words between rows (packed form: between packed rows) */
} tfa_kvcache_tree;
int tfa_fwd_kvcache_tree(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq /* NULL: 4-D */, const tfa_kvcache_fp8* q8 /* NULL: 16-bit cache */, int pack_gqa, const tfa_kvcache_tree* tree, int splits, const int32_t* metadata /* NULL: unscheduled; needs vq */, float* workspace, void* stream);
int tfa_fwd_kvcache_tree_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, const tfa_kvcache_tree* tree, int splits, int scheduled, int* grid, int* block, int* lds_bytes);
long long tfa_fwd_kvcache_tree_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, const tfa_kvcache_tree* tree, int splits);
int tfa_fwd_kvcache_tree_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, const tfa_kvcache_tree* tree);

/* ---- SHARED-PREFIX (cascade) attention over a paged cache: the keys a group of sequences shares are streamed once per group (n-way sampling, beam search, one system
 * prompt behind many requests) ----------------------------------------------------------------------------------------------------------------------------------------
 * Two levels over ONE paged 16-bit pool, both in the packed-q layout of tfa_fwd_kvcache_varlen:
 *   level 1 — *p and *vq as tfa_fwd_kvcache_varlen takes them, over each sequence's OWN keys only: sequence b owns the packed rows [q0_b, q0_b + nq_b) (clamped as
 *     there) and attends its keys [0, ulen_b), ulen_b = clamp(cache_seqlens[b], 0, capacity), through block_table[b]; p->is_causal: own key j is visible to row t iff
 *     j <= t + (ulen_b - nq_b).  cache_seqlens counts own keys only and includes this step's rows.  p->k_new must be NULL, p->block_table must not be.
 *   level 0 — *cs: group g owns the packed rows [pcu[g], pcu[g+1]) of the same q (clamped by the same rule with prefix_max_seqlen_q in max_seqlen_q's place; a group is a
 *     run of consecutive sequences) and EVERY row of it sees EVERY shared key [0, plen_g), plen_g = clamp(prefix_seqlens[g], 0, prefix_max_blocks * page_size), through
 *     prefix_block_table[g] into the same pool.  p->is_causal does not act on level 0 (the caller's contract: the shared keys precede all of the step's rows); plen_g
 *     need not be a multiple of the page size.
 * A row's result is softmax attention over the disjoint union of its group's shared keys and its sequence's visible own keys, lse the logsumexp over that union.  A row in
 *   no group takes no shared keys, a row in no sequence no own keys; a row that sees no key at all gives out = 0, lse = +inf — every row of out (H, total_q, D) and lse
 *   (H, total_q) is written.  Overlapping groups, or anything else the six device arrays may hold, give unspecified values in the rows concerned and never an access
 *   outside the tensors.  Nothing is read on the host; bytes behind a length read as zeros; a captured call replayed after the arrays were overwritten in place computes
 *   with the new values.
 * What runs, all on `stream`: a fill of the workspace's LSE words with +inf; the packed-q kernel over level 0 (non-causal, the groups as its sequences, prefix_splits
 *   chunks) writing fp32 partials into parts [0, ns0) of the workspace; the same kernel over level 1 (splits chunks) into parts [ns0, ns0 + ns1) — fp32 also when
 *   ns1 == 1 —; ONE merge over the ns0 + ns1 parts (csrc/tfa_merge.hip: merge_skip_kernel), which SKIPS a part whose LSE is +inf whatever its O words hold: rows no
 *   group or no sequence owns are never written by a level.  O is rounded to 16 bits once.  ns0 / ns1: the chunk counts after the clamp every call applies
 *   (min(splits, ceil(capacity / 64)) per level).
 * metadata / prefix_metadata (NULL: unscheduled): the lists tfa_kvcache_varlen_schedule built for level 1 (from *p, *vq, p->is_causal) and for level 0 (from the level-0
 *   batch — B = num_groups, prefix_cu_seqlens_q, prefix_max_seqlen_q — with is_causal = 0); each level then runs its scheduled form.  Results are bit for bit those without.
 * _workspace: (ns0 + ns1) * H * total_q * (D + 1) floats — never 0: this call always merges.  _plan: the launch of one level (level 0 | 1; scheduled / prefix_scheduled
 *   != 0 ask for that level's scheduled geometry) — equal to the plan of the packed-q call the level stands for.  _suggest_splits: tfa_fwd_kvcache_varlen_suggest_splits
 *   per level, with each level's geometry.  _plan, _workspace and _suggest_splits need no GPU.
 * Refused, nothing launched: NULL cs or a NULL member of it, a NULL p->block_table (TFA_ERR_NULL); num_groups, prefix_max_blocks or prefix_max_seqlen_q <= 0, a non-zero
 *   reserved_, prefix_splits < 1, a level other than 0 / 1 (TFA_ERR_SHAPE); a misaligned index array (TFA_ERR_ALIGN); prefix_block_table_stride < prefix_max_blocks, an
 *   out that is not dense (H, total_q, D) (TFA_ERR_STRIDE: always checked — this call always merges); everything tfa_fwd_kvcache_varlen refuses, with its codes.
 * Not here: e4m3 pools, contiguous caches, the 4-D layout, a window or a tree on either level, more than two levels, an append. */
typedef struct tfa_kvcache_cascade {
  const int32_t* prefix_cu_seqlens_q;   /* device, num_groups + 1 */
  const int32_t* prefix_seqlens;        /* device, num_groups */
  const int32_t* prefix_block_table;    /* device, num_groups x prefix_max_blocks, row stride below */
  int64_t prefix_block_table_stride;
  int32_t num_groups, prefix_max_blocks, prefix_max_seqlen_q, reserved_;
} tfa_kvcache_cascade;
int tfa_fwd_kvcache_cascade(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits, int prefix_splits, const int32_t* metadata /* NULL: unscheduled */, const int32_t* prefix_metadata /* NULL: unscheduled */, float* workspace, void* stream);
long long tfa_fwd_kvcache_cascade_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits, int prefix_splits);
int tfa_fwd_kvcache_cascade_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits, int prefix_splits, int scheduled, int prefix_scheduled, int level /* 0 | 1 */, int* grid, int* block, int* lds_bytes);
int tfa_fwd_kvcache_cascade_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int* splits, int* prefix_splits);

/* ---- rotary position embedding (FlashAttention-2's apply_rotary_emb; its ROCm build runs a Triton kernel, this one is HIP) ----------------------------
 * Rotates x (B, N, H, D) — or packed (total, H, D) with cu_seqlens — into out; optionally a second tensor x2 -> out2 of H2 heads with strides of its own in the
 * same launch (q and k of one step).  16-bit elements, any batch / head / row strides (elements), unit stride along D: a slice of a packed QKV projection works.
 *   Position: row t of sequence b has pos = seqlen_offsets[b] + t (device int32, B entries — cache_seqlens is the intended argument) or seqlen_offset + t when
 *     seqlen_offsets is NULL.  Packed: t = row - cu_seqlens[b], b found on the device by a binary search of cu_seqlens (B + 1 entries) whose answer is verified.
 *     Nothing is read on the host: no copy, no synchronisation, capturable in a graph and replayable after the offsets were overwritten in place.
 *   Definition, in fp32, every output element rounded once (to nearest even): with (x1, x2) = elements (i, i + rotary_dim / 2) (interleaved = 0, GPT-NeoX) or
 *     (2i, 2i + 1) (interleaved = 1, GPT-J), c = cos[pos, i], s = sin[pos, i] (s = -sin[pos, i] with conjugate = 1: the backward of the rotation):
 *       o1 = x1 * c - x2 * s,   o2 = x1 * s + x2 * c      computed as fma(x1, c, -(x2 * s)) and fma(x1, s, x2 * c);
 *     elements [rotary_dim, D) are copied.  Copied bit for bit as well: a row whose pos lies outside [0, seqlen_ro); a packed row outside every sequence (rows behind
 *     cu_seqlens[B]); a row whose search fails because cu_seqlens is not monotonic.  No value of cu_seqlens or seqlen_offsets causes an access outside x, out, cos, sin.
 *   cos / sin: (seqlen_ro, rotary_dim / 2) of x's dtype or fp32 (cs_dtype), rows cos_stride / sin_stride elements apart, 16-byte aligned rows and bases.
 *   In place (out == x with the same strides; likewise out2 == x2): the thread that stores a chunk loaded it, so there is nothing to order; the chunks behind
 *     rotary_dim and the unrotated rows are then not touched.  x and out must otherwise not overlap.
 * Kernel (csrc/tfa_rotary.hip): one work item per (row, head, pair of 16-byte chunks) — two loads and two stores (GPT-NeoX), one each (GPT-J) —, 256 threads a block,
 * items of one row adjacent so its heads share the cos / sin reads; no LDS, no trigonometry.  _plan reports ceil(rows * (H + H2) * items / 256) blocks, items =
 * rotary_dim / 16 + (D - rotary_dim) / 8 (GPT-NeoX) or D / 8 (GPT-J).  The pair arithmetic is csrc/tfa_rotary.h's, shared with tfa_kvcache_append_varlen.
 * Refused, nothing launched: a NULL params / x / out / cos / sin, one of x2 / out2 without the other (TFA_ERR_NULL); dtype not TFA_F16 / TFA_BF16, cs_dtype neither
 * dtype nor TFA_F32 (TFA_ERR_DTYPE); D not a positive multiple of 8, rotary_dim not a multiple of 16 in [16, D] (TFA_ERR_HEAD_DIM); B, N, H, seqlen_ro <= 0, H2 < 0, H2 > 0
 * without x2 or x2 with H2 = 0, interleaved / conjugate not 0 or 1, a grid of 2^31 blocks or more (TFA_ERR_SHAPE); a stride negative or not a multiple of 16 bytes,
 * a table row stride below rotary_dim / 2, out == x with other strides (TFA_ERR_STRIDE); a tensor or table base not 16-byte aligned, seqlen_offsets / cu_seqlens not
 * 4-byte aligned (TFA_ERR_ALIGN).
 * Out of scope: fp32 / fp8 x, rotary_dim not a multiple of 16, gradients of cos / sin, trigonometry on the device, a rotation fused into an attention kernel.
 * Tolerance (tests/test_rotary_gpu.py): |out - exact| <= ulp(exact) / 2 + 2^-21 * (|x1| + |x2|).  Measured: profiles/rotary_append_bench.txt (tools/bench_rotary_append.py), quoted in README.md. */
typedef struct tfa_rotary_params {
  const void* x;                  /* (B, N, H, D) by x_stride, or packed (N, H, D) with cu_seqlens: N = total rows, x_stride[0] ignored */
  void* out;                      /* same shape by o_stride; may be x */
  const void* x2;                 /* optional second tensor, H2 heads, or NULL */
  void* out2;
  const void* cos;                /* (seqlen_ro, rotary_dim / 2) of cs_dtype */
  const void* sin;
  const int32_t* seqlen_offsets;  /* device, B entries, or NULL: seqlen_offset for every sequence */
  const int32_t* cu_seqlens;      /* device, B + 1 entries, or NULL */
  int32_t B;
  int32_t N;                      /* rows per sequence; packed: rows in all */
  int32_t H, H2, D, rotary_dim, seqlen_ro;
  int32_t seqlen_offset;          /* host offset, used when seqlen_offsets is NULL */
  int64_t x_stride[3];            /* batch, head, row (elements) */
  int64_t o_stride[3];
  int64_t x2_stride[3];
  int64_t o2_stride[3];
  int64_t cos_stride;             /* elements between the rows of cos */
  int64_t sin_stride;
  int32_t dtype;                  /* TFA_F16 or TFA_BF16: x, out, x2, out2 */
  int32_t cs_dtype;               /* dtype, or TFA_F32 */
  int32_t interleaved;            /* 0: GPT-NeoX pairs (i, i + rotary_dim / 2); 1: GPT-J pairs (2i, 2i + 1) */
  int32_t conjugate;              /* 1: rotate by -angle (sin negated) */
} tfa_rotary_params;
/* On `stream`, asynchronous, never allocates, never reads device memory on the host. */
int tfa_rotary(const tfa_rotary_params* p, void* stream);
/* Validate *p without launching (no GPU needed); on success optionally reports the launch's geometry. */
int tfa_rotary_plan(const tfa_rotary_params* p, int* grid, int* block);

/* ---- packed new K/V rows into a paged or contiguous cache (the append of a unified batch: chunked prefill and decode rows in one call) ---------------
 * k / v: (total_new, Hk, D) packed, strides {head, row} in elements, unit stride along D; sequence b owns rows [cu_seqlens[b], cu_seqlens[b+1]); row t of
 * sequence b goes to key position pos = cache_seqlens[b] + t of the cache — paged (num_pages, page_size, Hk, D) through block_table, or contiguous
 * (B, capacity, Hk, D) with block_table NULL; cache strides {page or batch, head, row} as in tfa_kvcache_params, capacity = max_blocks * page_size when paged.
 * cu_seqlens (B + 1), cache_seqlens (B) and block_table are device int32 and read on the device only: no copy, no synchronisation, capturable in a graph.
 * The row's sequence is found by a binary search of cu_seqlens whose answer is verified.  Dropped, exactly as tfa_kvcache_append drops: a position below 0 or at /
 * beyond the capacity; a block-table entry outside [0, num_pages); and a packed row outside every sequence (padding behind cu_seqlens[B], a cu_seqlens that is not
 * monotonic).  Nothing is ever stored outside the cache tensors, whatever the three arrays hold.  cache_seqlens is not advanced.  Two rows that map to one slot
 * leave either one there.  k / v must not overlap the caches.
 * rotary_cos / rotary_sin (both or neither; tfa_rotary's tables, cs_dtype, strides, rotary_dim, seqlen_ro, rotary_interleaved): K is rotated at its key position pos
 * on the way in — FlashAttention-2's rule for the cache — by the device functions tfa_rotary runs, V is copied: the cache holds the bits that tfa_rotary(k,
 * cu_seqlens, seqlen_offsets = cache_seqlens) followed by the plain append leaves (a pos at or beyond seqlen_ro: stored unrotated).
 * Kernel (csrc/tfa_kvcache_append_varlen.hip): one thread per (row, K/V head, 16-byte chunk), one K and one V store; a thread of K's rotated part loads its
 * partner chunk too.  _plan reports ceil(total_new * Hk * D / 8 / 256) blocks of 256 threads.
 * Refused, nothing launched — tfa_kvcache_append's codes: a NULL params / k / v / cache / cu_seqlens / cache_seqlens, one rotary table without the other
 * (TFA_ERR_NULL); dtype not TFA_F16 / TFA_BF16, cs_dtype neither dtype nor TFA_F32 (TFA_ERR_DTYPE); D not a multiple of 8 in [8, 128], rotary_dim not a multiple of
 * 16 in [16, D] (TFA_ERR_HEAD_DIM); B, total_new, Hk, capacity <= 0, paged: page_size not a positive multiple of 64, capacity not a multiple of it, num_pages <= 0,
 * with tables seqlen_ro <= 0, rotary_interleaved not 0 or 1, reserved_ != 0 (TFA_ERR_SHAPE); strides negative or not multiples of 16 bytes, row strides below D,
 * block_table_stride < capacity / page_size, a table row stride below rotary_dim / 2 (TFA_ERR_STRIDE); bases not 16-byte aligned, the int32 arrays not 4-byte aligned
 * (TFA_ERR_ALIGN).
 * e4m3 caches and the step's q rotated in the same launch: tfa_kvcache_append_varlen_ex, below (this entry point serves 16-bit caches and rotates K only).
 * Out of scope: advancing cache_seqlens.
 * Measured: profiles/rotary_append_bench.txt (tools/bench_rotary_append.py), quoted in README.md. */
typedef struct tfa_kvcache_append_varlen_params {
  const void* k;                  /* (total_new, Hk, D) by k_stride */
  const void* v;
  void* k_cache;
  void* v_cache;
  const int32_t* cu_seqlens;      /* device, B + 1 entries */
  const int32_t* cache_seqlens;   /* device, B entries */
  const int32_t* block_table;     /* device (B, max_blocks) int32, or NULL: contiguous cache */
  const void* rotary_cos;         /* (seqlen_ro, rotary_dim / 2) of cs_dtype, or NULL */
  const void* rotary_sin;
  int32_t B, total_new, Hk, D;
  int32_t capacity;               /* keys a sequence can hold: the contiguous cache's rows, or max_blocks * page_size */
  int32_t page_size;              /* paged: keys per page, a positive multiple of 64; contiguous: ignored */
  int32_t num_pages;              /* paged: pages in the caches; contiguous: ignored */
  int32_t rotary_dim, seqlen_ro;  /* with tables only */
  int32_t rotary_interleaved;
  int32_t dtype;                  /* TFA_F16 or TFA_BF16: k, v, caches (tfa_kvcache_append_varlen_ex with q8: k, v and q; the caches hold e4m3) */
  int32_t cs_dtype;               /* with tables: dtype, or TFA_F32 */
  int64_t k_stride[2];            /* head, row (elements) */
  int64_t v_stride[2];
  int64_t kc_stride[3];           /* batch (contiguous) or page (paged), head, row */
  int64_t vc_stride[3];
  int64_t block_table_stride;     /* elements between the rows of block_table */
  int64_t cos_stride;             /* elements between the rows of rotary_cos */
  int64_t sin_stride;
  int64_t reserved_;              /* must be 0 */
} tfa_kvcache_append_varlen_params;
int tfa_kvcache_append_varlen(const tfa_kvcache_append_varlen_params* p, void* stream);
int tfa_kvcache_append_varlen_plan(const tfa_kvcache_append_varlen_params* p, int* grid, int* block);

/* ---- the packed append into an e4m3 cache, and / or with the step's q rotated in place in the same launch ------------------------------------------------
 * tfa_kvcache_append_varlen with two optional companions; with both NULL the call IS tfa_kvcache_append_varlen's launch (the same kernel, the same bits).
 * q8 (tfa_kvcache_fp8, as in tfa_fwd_kvcache_fp8): k_cache / v_cache hold e4m3fn bytes, paged or contiguous.  k / v stay 16-bit: p->dtype is THEIR dtype, and
 *   kc_stride / vc_stride count cache elements, which are bytes.  Sequence, position, page lookup and every drop rule are the 16-bit packed append's.  Stored
 *   byte = rne_e4m3fn(clamp(float(x) / descale[b, hk], -448, 448)) — a true fp32 division, NaN stays NaN: the rule, the device function (csrc/tfa_quantise8.h)
 *   and the bits of tfa_kvcache_append_fp8.  The descales are indexed by the sequence b, not by the page, element (b, hk) at b * stride[0] + hk * stride[1]
 *   (0 allowed: a broadcast per-tensor scale; NULL = 1.0), and read on the device only.  With rotary tables K is first rotated and rounded once to p->dtype —
 *   the bits tfa_rotary leaves — and then quantised; V is only quantised: the caches hold the bytes of tfa_rotary(k, cu_seqlens, seqlen_offsets = cache_seqlens)
 *   followed by the plain e4m3 append (a pos at or beyond seqlen_ro: stored unrotated).  D: a multiple of 16 in [16, 128]; cache strides: multiples of 16 bytes.
 * rq (tfa_append_q): q, packed (total_new, H, D) of p->dtype with strides {head, row} in elements, unit stride along D, 16-byte aligned rows and base — a slice
 *   of a packed QKV projection works — is rotated IN PLACE at the positions K is rotated at: row t of sequence b at cache_seqlens[b] + t.  It leaves the bits
 *   of tfa_rotary(q, out = q, cu_seqlens, seqlen_offsets = cache_seqlens).  Untouched bit for bit: elements behind rotary_dim, rows outside every sequence,
 *   rows whose position lies outside [0, seqlen_ro).  q has no capacity: a row whose K is dropped (beyond the capacity, a bad table entry) still has its q
 *   rotated.  Requires the tables; no relation between H and Hk is needed.  PRECONDITION: q must not overlap k, v or the caches (k / v are read by other
 *   threads of the launch than the ones that write q).
 * Kernel (csrc/tfa_kvcache_append_varlen_ex.hip): the append's threads — one per (row, K/V head, 16-byte chunk of the 16-bit source); e4m3: 8-byte stores,
 * neighbouring lanes neighbouring pieces of a row — followed by q's: one per (row, head, item of the rotated part), an item a pair of chunks (GPT-NeoX: the
 * thread that stores a chunk loaded it, nothing to order in place) or one chunk (GPT-J).  _plan reports
 *   ceil((total_new * Hk * D / 8 + total_new * H * items) / 256) blocks of 256 threads, items = rotary_dim / 16 (GPT-NeoX) or rotary_dim / 8 (GPT-J), 0 without rq;
 * with q8 and rq both NULL, tfa_kvcache_append_varlen_plan's answer.
 * Refused, nothing launched: everything tfa_kvcache_append_varlen refuses (with q8 the cache strides are checked as bytes); from q8 what tfa_kvcache_append_fp8
 * refuses — format other than TFA_KV_E4M3 (TFA_ERR_DTYPE), reserved_ != 0 (TFA_ERR_SHAPE), D not a multiple of 16 in [16, 128] (TFA_ERR_HEAD_DIM), cache strides not
 * multiples of 16 bytes, a negative descale stride (TFA_ERR_STRIDE), a descale pointer not 4-byte aligned (TFA_ERR_ALIGN); from rq — a NULL q, missing tables
 * (TFA_ERR_NULL), H <= 0, reserved_ != 0 (TFA_ERR_SHAPE), strides negative or not multiples of 16 bytes, a row stride below D (TFA_ERR_STRIDE), a base not 16-byte
 * aligned (TFA_ERR_ALIGN).
 * Out of scope: an out-of-place q, per-token or per-page scales, scales computed on the device, e5m2 / e4m3fnuz caches, D > 128, advancing cache_seqlens.
 * Measured: profiles/append_varlen_ex_bench.txt (tools/bench_rotary_append.py), quoted in README.md. */
typedef struct tfa_append_q {
  void* q;                        /* (total_new, H, D) by q_stride, of p->dtype; rotated in place */
  int32_t H;
  int32_t reserved_;              /* must be 0 */
  int64_t q_stride[2];            /* head, row (elements) */
} tfa_append_q;
int tfa_kvcache_append_varlen_ex(const tfa_kvcache_append_varlen_params* p, const tfa_kvcache_fp8* q8 /* NULL: 16-bit caches */, const tfa_append_q* rq /* NULL: no q */,
                                 void* stream);
int tfa_kvcache_append_varlen_ex_plan(const tfa_kvcache_append_varlen_params* p, const tfa_kvcache_fp8* q8, const tfa_append_q* rq, int* grid, int* block);

#ifdef __cplusplus
}
#endif
#endif /* TFA_H_ */
