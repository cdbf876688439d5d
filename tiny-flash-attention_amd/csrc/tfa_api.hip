// tfa_api.hip — the extern "C" boundary declared in include/tfa.h.
// Validates a problem descriptor, fills the kernel arguments, picks a kernel variant and
// launches on the caller's stream.  Mirrors what the reference host entry does
// (flash_attention_cutlass/csrc/flash_attention.cu:320-361 set_params_fprop, :731-739 dispatch,
//  :741-772 entry) minus allocation (the caller owns all buffers) and minus the device sync.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tfa.h"
#include "tfa_launch.h"
#include "tfa_kvcache.h"

namespace tfa {
// fp32 tensors (the reference's fp32 fixtures: a correctness path on v_mfma_f32_32x32x2_f32): tfa_fwd_f32.hip
hipError_t launch_f32(const KArgs& a, bool causal, hipStream_t stream, int* grid_out, bool dry);
template <> hipError_t launch_splitkv_wide<__bf16>(const KArgs&, bool, hipStream_t, LaunchGeom*, bool);
template <> hipError_t launch_splitkv_wide<_Float16>(const KArgs&, bool, hipStream_t, LaunchGeom*, bool);
// tfa_merge.hip, the merge of tfa_fwd_kvcache_cascade: tfa_merge's arguments and checks; a part whose LSE is +inf contributes nothing whatever its O words hold
int merge_skip(const float* o_parts, const float* lse_parts, int nparts, int64_t rows, int D, int64_t o_part_stride, int64_t lse_part_stride, void* out, int out_dtype,
               float* lse_out, void* stream);
}  // namespace tfa

namespace {

// Debug knobs (tfa_set_variant, tfa_debug_set_trace) are PER THREAD: a thread that forces a variant or a trace buffer
// for an A/B measurement does not change what any other thread's calls run.  Nothing else in the library is mutable.
thread_local int g_variant = -1;   // -1 = automatic
thread_local unsigned long long* g_trace = nullptr;
thread_local int g_dbg_flags = 0;                    // kernel bring-up flags (tfa_debug_set_flags): KArgs::dbg   // per-workgroup cycle stamps (tfa_debug_set_trace)

int num_cus() { return tfa::num_cus_current_device(); }

// every (b,h) slice of q, k, v and out fits ONE buffer descriptor (< 2 GiB including the rows a ragged block may reach past the
// end): what the key-split, split-KV, backward and x4 kernels need; larger slices run the windowed il4 / il8 instantiations
bool one_descriptor(const tfa_fwd_params* p) {
  const auto small = [&](int64_t n, const int64_t* st, int es) { return tfa::span_bytes(n + 512, st[2], p->D, es) < (int64_t)0x7fffffff; };
  return small(p->Nq, p->q_stride, 2) && small(p->Nk, p->k_stride, 2) && small(p->Nk, p->v_stride, 2) && small(p->Nq, p->o_stride, 4);
}

// An OUTPUT whose (b,h) slices share memory — a broadcast batch or head stride, or slices that interleave — would be written by several
// workgroups at once (inputs may broadcast freely: they are only read).  Row overlap inside a slice is the callers' `stride[2] < D` test.
bool out_aliases_itself(const tfa_fwd_params* p) {
  // the dims that have more than one index, by ascending stride: each stride must clear the span of everything below it (rows of D elements
  // at the bottom).  Sufficient, and every layout a tensor library hands out — (B,H,N,D), (B,N,H,D), slices and views of them — passes
  int64_t st[3] = {p->o_stride[0], p->o_stride[1], p->o_stride[2]};
  int64_t ext[3] = {p->B, p->H, p->Nq};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (st[j] < st[i]) { const int64_t t = st[i]; st[i] = st[j]; st[j] = t; const int64_t e = ext[i]; ext[i] = ext[j]; ext[j] = e; }
  int64_t span = p->D;
  for (int i = 0; i < 3; ++i) {
    if (ext[i] <= 1) continue;
    if (st[i] < span) return true;
    span = tfa::span_bytes(ext[i] - 1, st[i], span, 1);      // (INT64_MAX when it leaves 64 bit: every stride above it then aliases)
  }
  return false;
}

// NOTE on tfa_set_variant (a per-thread debug knob): a forced variant means "run exactly that kernel on the problem as given" —
// GQA row packing (pack_gqa_rows) and tfa_fwd_suggest_splits are both switched off while one is set, and head dims above 128
// always run kX4D256Variant (the only kernel that wide).  Tools that force a variant reset it to -1 in a finally block.
int pick_variant(const tfa_fwd_params* p) {
  if (p && p->D > 128) return tfa::kX4D256Variant;   // one kernel serves 136..256 (a forced variant does not apply)
  if (g_variant >= 0) return g_variant;
  if (!p) return tfa::kDefaultVariant;
  if (p->flags & TFA_FWD_EXACT_MAX) {
    // the exact running max (validate: D <= 128): where the default would run il8 — grids that fill the chip, whole 256-row blocks' worth of
    // rows, slices below 2 GiB — its exact-max instantiation (round 5); everywhere else the burst-structured LDS-DMA kernel
    tfa_fwd_params d = *p;
    d.flags &= ~TFA_FWD_EXACT_MAX;
    // (variant 38 has the main instantiation only: the same rule the launch switch applies to variant 30 — tfa_launch.h: il_instantiation; packed rows never get here)
    const bool main30 = pick_variant(&d) == tfa::kDefaultVariant &&
                        tfa::il_instantiation(tfa::kDefaultVariant, !one_descriptor(p), p->Nq, 0, 128, 128) == tfa::IL_MAIN;
    return main30 ? tfa::kExactVariant : tfa::kSplitVariant;
  }
  // Measured on MI355X (tests/tools/ab.py, profiles/): 256-row query blocks (8 waves) are fastest when there
  // are enough of them to fill 256 CUs and no causal diagonal; 128-row blocks (two 4-wave workgroups per
  // CU) waste less of the causal diagonal and fill the chip on small problems (BASELINE config 2:
  // B4 H8 N1024 has only 128 blocks of 256 rows).
  // The issue-interleaved kernel (tfa_fwd_kernel_il.h) wins wherever the grid fills the chip (+5..11% at D=128).
  if (p->B <= 0 || p->H <= 0 || p->Nq <= 0) return tfa::kDefaultVariant;   // (validate refuses these: any answer serves)
  const long long blocks256 = tfa::sat_mul((long long)p->B * p->H, ((long long)p->Nq + 255) / 256);
  const long long blocks128 = tfa::sat_mul((long long)p->B * p->H, ((long long)p->Nq + 127) / 128);
  const int cus = num_cus();
  // (partial passes — kv_offset / nk_total — reach the kernels as a causal shift only: every rule below applies to them too)
  // Grids of at most one 128-row block per CU: the 4-wave kernel would run one wave per SIMD (causal: paired, on half the CUs) —
  // split the keys inside the workgroup instead (il8-ksplit: 8 waves on one block, unpaired).  Causal it always pays (B1 H8 N4096 +15 %,
  // B1 H16 N2048 +19 %, B1 H64 N512 +27 %, B4 H8 N1024 D64 +31 % over il4).  Non-causal the 4-wave kernel with the hand-scheduled tile loop
  // (round 5: +8..19 % on these grids; the key-split waves see half the tiles each and gain 0..3 %) is ahead up to 2048 keys (BASELINE config 2:
  // 611 vs 542 TF, B4 H8 N1024 D128 816 vs 762, B1 H16 N2048 955 vs 931) and level at 4096 (1043 vs 1056): key split from 4096 keys on
  // (profiles/r05_ksplit_retune.txt; rounds 2-4 had it from 1024: profiles/r02_ksplit_ab.txt).
  const bool one_desc = one_descriptor(p);   // (slices of 2 GiB and more: the windowed il4 / il8 instantiations)
  if (one_desc && blocks128 <= cus && p->Nk >= (p->is_causal ? 512 : 4096)) return tfa::kKSplitVariant;
  // causal, up to two 128-row blocks per CU, long sequences: the same kernel with the blocks paired heavy+light (one round of
  // equal workgroups, two waves per SIMD): B1 H16 N4096 +4 %, B1 H8 N8192 +7 %, B1 H4 N16384 +11 % over il4; N=2048: -2..+5 %
  if (one_desc && p->is_causal && blocks128 <= 2 * cus && p->Nk >= 4096) return tfa::kKSplitPairVariant;
  // at most 128 query rows (decode, cross-attention onto few queries): a 256-row block would be half idle; 128-row blocks put two
  // workgroups on a CU and keep twice the K/V bytes in flight (B32 H32 Nq1 Nk16384 D64: K/V at 6.1 vs 5.0 TB/s, D128: 6.1 vs 6.0)
  if (p->Nq <= 128) return tfa::kSmallGridVariant;
  // non-causal, at least one 256-row block per CU: the 8-wave kernel already has two waves per SIMD everywhere
  // (B1 H16 N4096: 1160 vs 1091 TF for il4, B1 H32 N2048: 1098 vs 1038)
  if (!p->is_causal && blocks256 >= cus) return tfa::kDefaultVariant;
  // small grids: 128-row blocks, two 4-wave workgroups per CU, issue-interleaved, O through the idle tile buffers
  // (D=128: +8..15 % over the burst kernel on B1 H8 N2048 / B2 H16 N1024 / B1 H32 N4096; D=64, BASELINE config 2: +2 %)
  if (blocks256 < 512) return tfa::kSmallGridVariant;
  // (with O leaving through LDS the 8-wave il kernel also wins on short sequences: N=512..2048, causal or not, it beats
  //  the 4-wave one by 3-5 %, tests/tools/ab.py n512/n1k/n2k configs)
  return tfa::kDefaultVariant;
}

// extent in bytes of one (b,h) slice: rows 0..N-1 at row stride, D contiguous elements each.  Kernels with one descriptor
// per slice need every byte offset they form (up to one block past the end) inside int32; the il / x4 kernels address the
// slice through per-block / per-tile windows (rsrc_at), so only a WINDOW (a 256-row query block or a 64-row tile plus the
// rows a ragged tail may reach past it) has to fit 2 GiB — long (B,N,H,D) tensors whose head slices span more are fine.
bool slice_bytes(int64_t n, int64_t row_stride, int d, int esize, bool windowed, unsigned long long* out, int* big) {
  const int64_t bytes = tfa::span_bytes(n - 1, row_stride, d, esize);
  const int64_t whole = tfa::span_bytes(n + 512, row_stride, d, esize);       // one descriptor per slice
  const int64_t window = tfa::span_bytes(768, row_stride, d, esize);          // one per query block / tile
  if (bytes <= 0) return false;
  if (whole >= (int64_t)0x7fffffff) {
    if (!windowed || window >= (int64_t)0x7fffffff) return false;
    *big = 1;
  }
  *out = (unsigned long long)bytes;
  return true;
}

int validate(const tfa_fwd_params* p, tfa::KArgs* a, int variant, int row_mod = 0, bool wide_split = false) {
  if (!p) return TFA_ERR_NULL;
  if (!p->q || !p->k || !p->v || !p->out) return TFA_ERR_NULL;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (p->out_dtype != p->dtype && p->out_dtype != TFA_F32) return TFA_ERR_DTYPE;
  if (p->D < 8 || p->D > 256 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->Nq <= 0 || p->Nk <= 0) return TFA_ERR_SHAPE;
  if (p->H % p->Hk != 0) return TFA_ERR_SHAPE;
  if (!(p->softmax_scale > 0.f) || !isfinite(p->softmax_scale)) return TFA_ERR_SCALE;
  if ((p->flags & ~TFA_FWD_EXACT_MAX) != 0 || p->reserved_ != 0) return TFA_ERR_SHAPE;
  if ((p->flags & TFA_FWD_EXACT_MAX) && p->D > 128) return TFA_ERR_HEAD_DIM;          // no exact-max kernel that wide
  const bool ablate = (variant >= 100 && variant < 100 + 512) || (variant >= 700 && variant < 716) || (variant >= 1000 && variant < 2256) || (variant >= 3000 && variant < 3256);   // timing-only ablations (debug)
  if (!ablate && !tfa::variant_built(variant)) return TFA_ERR_VARIANT;
  if (p->D != 64 && p->D != 128 && (ablate || !tfa::supports_padded_d(variant))) return TFA_ERR_HEAD_DIM;   // (A/B arms: 64 / 128 only)
  // (wide_split: tfa_fwd_splitkv's partial pass — the LDS-DMA kernel exists 256 wide for that purpose only)
  if (p->D > 128 ? !(variant == tfa::kX4D256Variant || (wide_split && variant == tfa::kSplitVariant)) : variant == tfa::kX4D256Variant) return TFA_ERR_HEAD_DIM;
  const int esz = 2, osz = (p->out_dtype == TFA_F32) ? 4 : 2;
  const int64_t* st[4] = {p->q_stride, p->k_stride, p->v_stride, p->o_stride};
  for (int t = 0; t < 4; ++t) {
    const int es = (t == 3) ? osz : esz;
    for (int i = 0; i < 3; ++i) {
      if (st[t][i] < 0) return TFA_ERR_STRIDE;
      if (st[t][i] % (16 / es) != 0) return TFA_ERR_STRIDE;   // 16-byte vector access on every row
    }
    if (st[t][2] < p->D) return TFA_ERR_STRIDE;               // rows must not overlap
  }
  if (out_aliases_itself(p)) return TFA_ERR_STRIDE;
  if (((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & 15) return TFA_ERR_ALIGN;
  if (p->lse && ((uintptr_t)p->lse & 3)) return TFA_ERR_ALIGN;

  memset(a, 0, sizeof(*a));
  a->q = p->q; a->k = p->k; a->v = p->v; a->o = p->out; a->lse = p->lse;
  a->B = p->B; a->H = p->H; a->Hk = p->Hk; a->Nq = p->Nq; a->Nk = p->Nk;
  {
    if (p->kv_offset < 0 || p->nk_total < 0 || p->kv_offset >= (int64_t)0x3fffffff) return TFA_ERR_SHAPE;   // (kv_offset + Nk <= total < 2^30 below)
    const int64_t total = p->nk_total ? p->nk_total : (p->kv_offset + p->Nk);
    if (p->kv_offset + p->Nk > total || total - p->Nq - p->kv_offset < -(int64_t)0x3fffffff || total >= (int64_t)0x3fffffff) return TFA_ERR_SHAPE;
    a->shift = (int)(total - p->Nq - p->kv_offset);
  }
  a->qs_b = p->q_stride[0]; a->qs_h = p->q_stride[1]; a->qs_n = p->q_stride[2];
  a->ks_b = p->k_stride[0]; a->ks_h = p->k_stride[1]; a->ks_n = p->k_stride[2];
  a->vs_b = p->v_stride[0]; a->vs_h = p->v_stride[1]; a->vs_n = p->v_stride[2];
  a->os_b = p->o_stride[0]; a->os_h = p->o_stride[1]; a->os_n = p->o_stride[2];
  const bool win = !ablate && tfa::windowed_slices(variant);
  if (!slice_bytes(p->Nq, a->qs_n, p->D, esz, win, &a->q_bytes, &a->big)) return TFA_ERR_STRIDE;
  if (!slice_bytes(p->Nk, a->ks_n, p->D, esz, win, &a->k_bytes, &a->big)) return TFA_ERR_STRIDE;
  if (!slice_bytes(p->Nk, a->vs_n, p->D, esz, win, &a->v_bytes, &a->big)) return TFA_ERR_STRIDE;
  if (!slice_bytes(p->Nq, a->os_n, p->D, osz, win, &a->o_bytes, &a->big)) return TFA_ERR_STRIDE;
  if ((g_dbg_flags & 256) && win) a->big = 1;   // tests: run the windowed instantiation on a small problem
  a->scale = p->softmax_scale;
  // (trace and grid share their bytes with the ALiBi slopes: run_form calls set_alibi AFTER validate(), and it must stay the last writer of them)
  a->trace = g_trace;
  a->grid = num_cus();
  if (g_dbg_flags & 512) a->grid = 8;            // tests: persistent kernels with 8 workgroups, so that small problems walk several work items each
  a->scale_log2 = p->softmax_scale * 1.4426950408889634f;
  const int bm = ablate ? 256 : tfa::block_m_of(variant);
  a->nmb = (p->Nq + bm - 1) / bm;
  a->nwork = (p->is_causal && (ablate || tfa::pairs_causal(variant))) ? (a->nmb + 1) / 2 : a->nmb;
  const int64_t nbh = (int64_t)p->B * p->H;
  if (nbh * a->nwork >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
  a->nbh = (int)nbh;
  a->dbg = g_dbg_flags;
  // K and V together beyond 768 MiB: the cache will not survive in the memory-side cache until the next call -> decode kernels may
  // stream it with the non-temporal hint (tfa_fwd_kernel_il.h / tfa_fwd_kernel_dma.h: kv_private, VF_DMA_NT)
  a->kv_stream = (tfa::sat_mul((long long)p->B * p->Hk, (long long)p->Nk * p->D * 4) >= (768ll << 20)) ? 1 : 0;
  a->row_mod = row_mod;
  a->dv = p->D;
  return TFA_OK;
}

// GQA / MQA with few query rows (decode): the G = H/Hk query heads that share a K/V head are G x Nq ROWS of one problem over
// that head's keys — the same bytes described differently (head stride G times larger, rows one head apart), so K and V are
// streamed once per K/V head instead of once per query head and the grid shrinks G-fold.  One query row: any strides, and
// a causal mask hides nothing from it (its position is the last key), so the packed problem is non-causal.  More rows: only
// non-causal and with the heads of q / out adjacent in memory (rows of consecutive heads are then equidistant).  The LSE layout
// (B,H,Nq) is the packed problem's (B,Hk,G*Nq) as it stands.  Causal with several rows (speculative decoding, the tail of a
// chunked prefill): row r of the packed block is query position r % Nq, which the decode instantiations of the il kernels
// understand (KArgs::row_mod, *row_mod here; causal_rows says whether the caller's kernel is one of them); nk_total carries
// the causal shift of the ORIGINAL problem (Nk - Nq) past the larger row count.  Returns false when *p is not such a problem.
bool pack_gqa_rows(const tfa_fwd_params* p, tfa_fwd_params* o, int* row_mod = nullptr, bool causal_rows = false) {
  if (row_mod) *row_mod = 0;
  if (!p || p->Hk <= 0 || p->H <= p->Hk || p->H % p->Hk != 0 || p->Nq <= 0 || p->Nk <= 0) return false;
  if (p->kv_offset != 0 || p->nk_total != 0) return false;
  const int G = p->H / p->Hk;
  const bool one_row = p->Nq == 1;
  if ((long long)G * p->Nq > 128) return false;          // beyond one query block nothing is shared any more
  int64_t q_rows = 0, o_rows = 0, q_head = 0, o_head = 0;   // (strides near INT64_MAX / 2 are refused by validate, not packed: every product checked)
  if (__builtin_mul_overflow((int64_t)p->Nq, p->q_stride[2], &q_rows) || __builtin_mul_overflow((int64_t)p->Nq, p->o_stride[2], &o_rows) ||
      __builtin_mul_overflow((int64_t)G, p->q_stride[1], &q_head) || __builtin_mul_overflow((int64_t)G, p->o_stride[1], &o_head)) return false;
  const bool adjacent = p->q_stride[1] == q_rows && p->o_stride[1] == o_rows;
  const bool with_positions = !one_row && p->is_causal;
  if (!one_row && !adjacent) return false;
  if (with_positions && !(causal_rows && row_mod && p->D <= 128 && p->Nk >= p->Nq)) return false;
  *o = *p;
  o->H = p->Hk;
  o->Nq = G * p->Nq;
  if (one_row) {
    o->q_stride[2] = p->q_stride[1];
    o->o_stride[2] = p->o_stride[1];
    o->is_causal = 0;
  }
  if (with_positions) {
    *row_mod = p->Nq;
    o->nk_total = (int64_t)p->Nk + (int64_t)(G - 1) * p->Nq;   // shift = nk_total - G*Nq = Nk - Nq
  }
  o->q_stride[1] = q_head;
  o->o_stride[1] = o_head;
  return true;
}

// the row reference P is rounded against (include/tfa.h) for a 16-bit problem of head dim D that runs `variant`: the il kernels' lazily re-based reference,
// except — bf16, the main instantiation (the one that carries the hand-scheduled statement: tfa_fwd_kernel_il.h MAXFREE) — the first key tile's maximum;
// the 256-wide kernel re-bases lazily too; the LDS-DMA kernel and the exact-max il8 keep the exact running maximum
int rounding_rule(int variant, int dtype, int D, bool main_inst) {
  if (D > 128) return TFA_RULE_LAZY;
  const tfa::Variant* vi = tfa::variant_info(variant);
  if (!vi || !(vi->vf & tfa::VF_IL) || variant == tfa::kExactVariant) return TFA_RULE_EXACT_MAX;
  return (dtype == TFA_BF16 && main_inst && TFA_IL_USE_MAXFREE) ? TFA_RULE_FIRST_TILE : TFA_RULE_LAZY;
}

// fp32 q, k, v (tfa_fwd_params::dtype == TFA_F32): the correctness path behind the reference's fp32 fixtures (tfa_fwd_f32.hip).  fp32 output
// only; any strides with 16-byte aligned rows; head dims = multiples of 4 up to 256; GQA, Nq != Nk, kv_offset / nk_total as for the 16-bit types.
int run_f32(const tfa_fwd_params* p, void* stream, tfa::LaunchGeom* geom, bool dry) {
  if (!p->q || !p->k || !p->v || !p->out) return TFA_ERR_NULL;
  if (p->out_dtype != TFA_F32) return TFA_ERR_DTYPE;
  if (p->D < 4 || p->D > 256 || (p->D % 4) != 0) return TFA_ERR_HEAD_DIM;
  if (p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->Nq <= 0 || p->Nk <= 0 || p->H % p->Hk != 0) return TFA_ERR_SHAPE;
  if (!(p->softmax_scale > 0.f) || !isfinite(p->softmax_scale)) return TFA_ERR_SCALE;
  if (p->flags != 0 || p->reserved_ != 0) return TFA_ERR_SHAPE;          // (TFA_FWD_EXACT_MAX is about 16-bit rounding points: this path has none)
  const int64_t* st[4] = {p->q_stride, p->k_stride, p->v_stride, p->o_stride};
  for (int t = 0; t < 4; ++t) {
    for (int i = 0; i < 3; ++i)
      if (st[t][i] < 0 || st[t][i] % 4 != 0) return TFA_ERR_STRIDE;
    if (st[t][2] < p->D) return TFA_ERR_STRIDE;
  }
  if (out_aliases_itself(p)) return TFA_ERR_STRIDE;
  if (p->Nq >= 0x3fffffff) return TFA_ERR_SHAPE;                          // (the kernel forms row + 32 + shift in 32-bit arithmetic)
  if (((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & 15) return TFA_ERR_ALIGN;
  if (p->lse && ((uintptr_t)p->lse & 3)) return TFA_ERR_ALIGN;
  tfa::KArgs a;
  memset(&a, 0, sizeof(a));
  a.q = p->q; a.k = p->k; a.v = p->v; a.o = p->out; a.lse = p->lse;
  a.B = p->B; a.H = p->H; a.Hk = p->Hk; a.Nq = p->Nq; a.Nk = p->Nk;
  if (p->kv_offset < 0 || p->nk_total < 0 || p->kv_offset >= (int64_t)0x3fffffff) return TFA_ERR_SHAPE;
  const int64_t total = p->nk_total ? p->nk_total : (p->kv_offset + p->Nk);
  if (p->kv_offset + p->Nk > total || total - p->Nq - p->kv_offset < -(int64_t)0x3fffffff || total >= (int64_t)0x3fffffff) return TFA_ERR_SHAPE;
  a.shift = (int)(total - p->Nq - p->kv_offset);
  a.qs_b = p->q_stride[0]; a.qs_h = p->q_stride[1]; a.qs_n = p->q_stride[2];
  a.ks_b = p->k_stride[0]; a.ks_h = p->k_stride[1]; a.ks_n = p->k_stride[2];
  a.vs_b = p->v_stride[0]; a.vs_h = p->v_stride[1]; a.vs_n = p->v_stride[2];
  a.os_b = p->o_stride[0]; a.os_h = p->o_stride[1]; a.os_n = p->o_stride[2];
  a.scale = p->softmax_scale;
  a.scale_log2 = p->softmax_scale * 1.4426950408889634f;
  const int64_t nbh = (int64_t)p->B * p->H;
  if (nbh * ((p->Nq + 31) / 32) >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
  a.nbh = (int)nbh;
  a.dv = p->D;
  int grid = 0;
  const hipError_t e = tfa::launch_f32(a, p->is_causal != 0, reinterpret_cast<hipStream_t>(stream), &grid, dry);
  if (geom) { geom->grid = grid; geom->block = 256; geom->lds = 0; }
  return (int)e;
}

int run(const tfa_fwd_params* p_in, void* stream, tfa::LaunchGeom* geom, bool dry, int* variant_out = nullptr, int* rule_out = nullptr) {
  if (p_in && p_in->dtype == TFA_F32) {
    if (variant_out) *variant_out = -1;
    if (rule_out) *rule_out = TFA_RULE_EXACT_MAX;
    return run_f32(p_in, stream, geom, dry);
  }
  tfa_fwd_params packed;
  int row_mod = 0;
  const bool may_pack = g_variant < 0 && !(g_dbg_flags & 4096) && p_in && !(p_in->flags & TFA_FWD_EXACT_MAX);
  const tfa_fwd_params* p = (may_pack && pack_gqa_rows(p_in, &packed, &row_mod, true)) ? &packed : p_in;
  int variant = pick_variant(p);
  tfa::KArgs a;
  int st = validate(p, &a, variant, row_mod);
  // The packed description is an optimisation, never a requirement: whenever it does not validate (packing moves the head
  // stride into the row-stride slot, so e.g. a q broadcast over heads — head stride 0 — fails the "rows do not overlap" test)
  // or needs the windowed instantiations (which know nothing of packed positions), the problem runs as the caller gave it.
  if (p != p_in && (st != TFA_OK || (a.big && row_mod))) {
    p = p_in;
    row_mod = 0;
    variant = pick_variant(p);
    st = validate(p, &a, variant);
  }
  if (st != TFA_OK) return st;
  if (variant_out) *variant_out = variant;
  if (rule_out) {
    const bool main_inst = tfa::is_il_variant(variant) && tfa::il_instantiation(variant, a.big != 0, a.Nq, a.row_mod, a.dv, p->D > 64 ? 128 : 64) == tfa::IL_MAIN;
    *rule_out = rounding_rule(variant, p->dtype, p->D, main_inst);
  }
  const bool causal = p->is_causal != 0;
  const bool f32out = p->out_dtype == TFA_F32;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // kernel width: 64 serves D <= 64, 128 serves 64 < D <= 128, 256 (the x4 kernel) the rest (KArgs::dv = the valid part)
  return (int)tfa::by_dtype_width<64, 128, 256>(p->dtype, p->D, [&](auto k) {
    using T = typename decltype(k)::T;
    if constexpr (decltype(k)::W == 256) return tfa::launch_x4_unit<T, 256>(a, causal, f32out, 0, s, geom, dry);
    else return tfa::launch_fwd<T, decltype(k)::W>(a, causal, f32out, variant, s, geom, dry);
  });
}

void fill_bhnd(tfa_fwd_params* p, const void* q, const void* k, const void* v, void* out, float* lse,
               int B, int H, int N, int D, float scale, int causal, int dtype, int out_dtype) {
  memset(p, 0, sizeof(*p));
  p->q = q; p->k = k; p->v = v; p->out = out; p->lse = lse;
  p->B = B; p->H = H; p->Hk = H; p->Nq = N; p->Nk = N; p->D = D;
  const int64_t sb = (int64_t)H * N * D, sh = (int64_t)N * D, sn = D;
  int64_t* st[4] = {p->q_stride, p->k_stride, p->v_stride, p->o_stride};
  for (int t = 0; t < 4; ++t) { st[t][0] = sb; st[t][1] = sh; st[t][2] = sn; }
  p->softmax_scale = scale; p->is_causal = causal; p->dtype = dtype; p->out_dtype = out_dtype;
}

// The varlen and local forms (VF_IL_VARLEN / VF_IL_LOCAL instantiations of il8 and il4: tfa_fwd_form_inst.inc) of a problem that passed its form's own checks.
//   f:   the fixed-length problem the kernels see — varlen: ONE sequence of max_seqlen_q x max_seqlen_k rows (batch stride 0); validate() checks dtypes, scale,
//        strides, alignment and that such a slice fits one descriptor, and fills the kernel arguments;
//   eq:  the problem whose kernel choice the form takes over (pick_variant) — the caller's for fixed-length windows, (B, H, Hk, max_seqlen_q, max_seqlen_k, D)
//        for varlen;
//   vl:  the varlen call, or nullptr: B sequences run as the grid's batch and each work item reads its bounds from cu_seqlens on the device
//        (tfa_fwd_kernel.h: varlen_seq) — the host never reads them;
//   win: the normalised {left, right} of a true window (window_form: WIN_LOCAL), or nullptr;
//   al:  the ALiBi slopes (checked by the caller), or nullptr: with them the ALiBi form of the local kernels runs whatever the window is — win is then always given,
//        its unbounded sides as -1 (set_window).  al->capped: the soft-capping form instead (tfa_fwd_softcap; al->slopes may then be null).
// Kernel: il8 (30) where tfa_fwd would pick it, il4 (32) for everything else (the key-split kernels, split-KV and decode row packing have no such form); a
// variant forced by tfa_set_variant must be one of the two.
//   pg:  the page pool and block table of tfa_fwd_varlen_paged (checked by run_varlen), or nullptr: the paged form of the plain varlen kernels (vl set, no win, no al).
//        f.Nk is then one tile's rows — what one descriptor has to hold — and the kernels' key limit is set here: the smaller of max_seqlen_k and a table row's capacity
int run_form(const tfa_fwd_params& f_in, const tfa_fwd_params& eq, const tfa_varlen_fwd_params* vl, const int* win, const tfa::AlibiArg* al, void* stream,
             tfa::LaunchGeom* geom, bool dry, int* variant_out, int* rule_out, const tfa_paged_kv* pg = nullptr) {
  tfa_fwd_params f = f_in;
  int variant;
  if (win) {
    if ((int64_t)f.Nq + f.Nk >= (1 << 28)) return TFA_ERR_SHAPE;   // (the kernels' window arithmetic in int32 with room to spare)
    if (g_variant >= 0 && g_variant != tfa::kDefaultVariant && g_variant != tfa::kSmallGridVariant) return TFA_ERR_VARIANT;
    variant = pick_variant(&eq) == tfa::kDefaultVariant ? tfa::kDefaultVariant : tfa::kSmallGridVariant;
    f.is_causal = 0;                                 // (validate: one query block per work item — no causal pairs)
  } else {
    variant = pick_variant(&eq);                     // (a variant forced by tfa_set_variant: taken when it is 30 or 32)
    if (variant == tfa::kKSplitVariant || variant == tfa::kKSplitPairVariant) variant = tfa::kSmallGridVariant;
    if (variant != tfa::kDefaultVariant && variant != tfa::kSmallGridVariant) return TFA_ERR_VARIANT;
  }
  tfa::KArgs a;
  const int st = validate(&f, &a, variant);
  if (st != TFA_OK) return st;
  if (a.big) return TFA_ERR_STRIDE;                  // a slice beyond one descriptor: no windowed varlen / local form
  if (vl) {
    const int64_t nbh = (int64_t)vl->B * vl->H;
    if (nbh * a.nwork >= (int64_t)0x7fffffff || (int64_t)vl->H * vl->total_q >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
    a.B = vl->B;
    a.nbh = (int)nbh;
    a.kv_stream = 0;
    a.cu_q = vl->cu_seqlens_q; a.cu_k = vl->cu_seqlens_k;   // (KArgs: in the bytes of the split-KV fields, which the il kernels never read)
    a.total_q = vl->total_q; a.total_k = vl->total_k;       // (Nq / Nk = max_seqlen_q / _k, from validate())
  }
  if (pg) {
    // (KArgs: the paged arguments lie in bytes no varlen launch reads — tfa_fwd_kernel.h; behind validate(), which wrote k_bytes, v_bytes, big, grid and trace there)
    const int64_t cap = (int64_t)pg->max_blocks * pg->page_size;
    a.Nk = (int)(eq.Nk < cap ? eq.Nk : cap);
    a.shift = 0;                                     // (per sequence on the device)
    a.total_k = 0x7fffffff;                          // (varlen_seq: of cu_seqlens_k only the differences count, clamped into [0, Nk])
    a.ks_b = pg->k_page_stride; a.vs_b = pg->v_page_stride;
    a.pg_table_stride = pg->table_stride;
    a.pg_tpp = pg->page_size / 64;
    a.pg_fd_tpp = tfa::fastdiv_of((unsigned)a.pg_tpp);
    a.pg_num_pages = pg->num_pages;
    a.pg_max_blocks = pg->max_blocks;
    a.block_table = pg->block_table;
  }
  if (win) tfa::set_window(&a, win[0], win[1], f.Nq, f.Nk);   // (after the last read of a.big: the window shares its bytes)
  if (al && al->biased) tfa::set_bias(&a, *al->bias, f.Nq, f.Nk);   // (the bias shares the bytes of the slopes and more: the last writer too)
  else if (al) tfa::set_alibi(&a, *al);
  if (variant_out) *variant_out = variant;
  if (rule_out) *rule_out = rounding_rule(variant, f.dtype, f.D, !win && !pg);   // (the local and paged forms are not the main instantiation)
  const bool causal = f.is_causal != 0, f32out = f.out_dtype == TFA_F32;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return (int)tfa::by_dtype_width<64, 128>(f.dtype, f.D, [&](auto k) {
    using T = typename decltype(k)::T;
    constexpr int W = decltype(k)::W;
    if (pg) return tfa::launch_fwd_form<T, W, tfa::FORM_VARLEN | tfa::FORM_PAGED>(a, causal, f32out, variant, s, geom, dry);
    return tfa::by_form(vl != nullptr, win != nullptr, al != nullptr, al && al->capped, al && al->biased, [&](auto form) {
      return tfa::launch_fwd_form<T, W, decltype(form)::FORM>(a, causal, f32out, variant, s, geom, dry);
    });
  });
}

// tfa_fwd_local: FULL and CAUSAL windows are tfa_fwd's own problems; a true window covers the whole key sequence (no partial passes)
// tfa_fwd_alibi (al): every window, FULL and CAUSAL included, is the local form's problem — the ALiBi kernels are instantiations of it
// tfa_fwd_bias (al->biased): the same, with the dense bias in the slopes' place
int run_local(const tfa_fwd_params* p, const int* w, const tfa::AlibiArg* al, void* stream, tfa::LaunchGeom* geom, bool dry, int* variant_out, int* rule_out) {
  if (!p) return TFA_ERR_NULL;
  int win[2] = {w[0], w[1]};
  const int form = tfa::window_form(&win[0], &win[1], p->is_causal != 0, p->Nq, p->Nk);
  if (form < 0) return form;
  if (form != tfa::WIN_LOCAL && !al) {
    tfa_fwd_params f = *p;
    f.is_causal = form == tfa::WIN_CAUSAL;
    return run(&f, stream, geom, dry, variant_out, rule_out);
  }
  if (p->kv_offset != 0 || p->nk_total != 0) return TFA_ERR_SHAPE;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (p->D < 8 || p->D > 128 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->flags != 0) return TFA_ERR_SHAPE;
  if (al) {
    if (p->H <= 0) return TFA_ERR_SHAPE;
    const int st = al->biased ? tfa::check_bias(al->bias, p->dtype, p->Nq, p->Nk) : tfa::check_alibi(*al, p->H, p->softmax_scale);
    if (st != TFA_OK) return st;
  }
  return run_form(*p, *p, nullptr, win, al, stream, geom, dry, variant_out, rule_out);
}

// Packed variable-length batches (include/tfa.h: tfa_fwd_varlen, tfa_fwd_varlen_local — w: the window, or nullptr).  The host knows the sequences' bounds only
// as max_seqlen_q / _k; run_form runs the fixed-length problem of one sequence of that size B times.
// pg: tfa_fwd_varlen_paged's page pool (no window, no slopes): k / v are the pool, total_k is ignored, and K / V are checked as ONE 64-key tile — all a descriptor
// ever holds of them — so the pool may be of any size.
int run_varlen(const tfa_varlen_fwd_params* p, const int* w, const tfa::AlibiArg* al, void* stream, tfa::LaunchGeom* geom, bool dry, int* variant_out,
               int* rule_out, const tfa_paged_kv* pg = nullptr, bool paged = false) {
  if (!p) return TFA_ERR_NULL;
  if (paged && (!pg || !pg->block_table)) return TFA_ERR_NULL;
  if (!p->q || !p->k || !p->v || !p->out || !p->cu_seqlens_q || !p->cu_seqlens_k) return TFA_ERR_NULL;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;             // (fp32 inputs: no varlen form)
  if (p->D < 8 || p->D > 128 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;           // (the 256-wide kernel has no varlen form)
  if (p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->max_seqlen_q <= 0 || p->max_seqlen_k <= 0 || p->total_q <= 0 || (!pg && p->total_k <= 0)) return TFA_ERR_SHAPE;
  if (p->H % p->Hk != 0) return TFA_ERR_SHAPE;
  if (p->flags != 0 || p->reserved_ != 0) return TFA_ERR_SHAPE;                        // (TFA_FWD_EXACT_MAX: no varlen form)
  if (pg) {
    if (pg->page_size <= 0 || (pg->page_size % 64) != 0 || pg->max_blocks <= 0 || pg->num_pages <= 0 || pg->reserved_ != 0) return TFA_ERR_SHAPE;
    if ((uintptr_t)pg->block_table & 3) return TFA_ERR_ALIGN;
    if (pg->table_stride < 0 || pg->k_page_stride < 0 || pg->v_page_stride < 0 || (pg->k_page_stride * 2) % 16 != 0 || (pg->v_page_stride * 2) % 16 != 0) return TFA_ERR_STRIDE;
  }
  int win[2] = {-1, -1}, form = p->is_causal ? tfa::WIN_CAUSAL : tfa::WIN_FULL;
  if (w) {
    win[0] = w[0];
    win[1] = w[1];
    form = tfa::window_form(&win[0], &win[1], p->is_causal != 0, p->max_seqlen_q, p->max_seqlen_k);
    if (form < 0) return form;
  }
  if (al) {
    const int st = tfa::check_alibi(*al, p->H, p->softmax_scale);
    if (st != TFA_OK) return st;
  }
  tfa_fwd_params f;
  memset(&f, 0, sizeof(f));
  f.q = p->q; f.k = p->k; f.v = p->v; f.out = p->out; f.lse = p->lse;
  f.B = 1; f.H = p->H; f.Hk = p->Hk; f.Nq = p->max_seqlen_q; f.Nk = pg ? 64 : p->max_seqlen_k; f.D = p->D;
  const int64_t* src[4] = {p->q_stride, p->k_stride, p->v_stride, p->o_stride};
  int64_t* dst[4] = {f.q_stride, f.k_stride, f.v_stride, f.o_stride};
  for (int t = 0; t < 4; ++t) { dst[t][0] = 0; dst[t][1] = src[t][0]; dst[t][2] = src[t][1]; }
  f.softmax_scale = p->softmax_scale; f.is_causal = form == tfa::WIN_CAUSAL; f.dtype = p->dtype; f.out_dtype = p->out_dtype;
  tfa_fwd_params eq = f;
  eq.B = p->B;
  eq.Nk = p->max_seqlen_k;
  return run_form(f, eq, p, (form == tfa::WIN_LOCAL || al) ? win : nullptr, al, stream, geom, dry, variant_out, rule_out, pg);
}

// One forward call as an entry point names it: fixed-length (p) or packed variable-length (vp), with the {left, right} window of the _local entry points or
// without (win == nullptr), with the ALiBi slopes of the _alibi entry points (which always carry a window) or without — and the route that runs it.  The _plan, _variant and _rounding_rule entry points are dry runs of that route (no GPU needed).
struct FwdCall {
  const tfa_fwd_params* p;
  const tfa_varlen_fwd_params* vp;
  const int* win;
  const tfa::AlibiArg* alibi = nullptr;
  const tfa_paged_kv* paged = nullptr;   // tfa_fwd_varlen_paged (is_paged: the entry point was a paged one — a NULL struct is then an error, not "not paged")
  bool is_paged = false;
};
int route(const FwdCall& c, void* stream, tfa::LaunchGeom* geom = nullptr, bool dry = false, int* variant_out = nullptr, int* rule_out = nullptr) {
  if (c.vp || c.is_paged) return run_varlen(c.vp, c.win, c.alibi, stream, geom, dry, variant_out, rule_out, c.paged, c.is_paged);
  if (c.win) return run_local(c.p, c.win, c.alibi, stream, geom, dry, variant_out, rule_out);
  return run(c.p, stream, geom, dry, variant_out, rule_out);
}
int plan(const FwdCall& c, int* grid, int* block, int* lds_bytes) {
  tfa::LaunchGeom g{0, 0, 0};
  const int st = route(c, nullptr, &g, true);
  if (st != TFA_OK) return st;
  if (grid) *grid = g.grid;
  if (block) *block = g.block;
  if (lds_bytes) *lds_bytes = g.lds;
  return TFA_OK;
}
// the kernel variant (rule == false) or rounding rule (true) of a call, or its TFA_ERR_*.  A dry run reports a HIP error (a positive status) only where a
// launcher refuses a variant: tfa_set_variant's timing-only ablation numbers, which a product build accepts but carries no kernel for; they read as TFA_ERR_SHAPE
// here.  (The varlen routes never get there: they refuse every variant but 30 and 32 first.)
int variant_or_rule(const FwdCall& c, bool rule) {
  tfa::LaunchGeom g{0, 0, 0};
  int v = -1, r = -1;
  const int st = route(c, nullptr, &g, true, &v, &r);
  if (st != TFA_OK) return st > 0 ? TFA_ERR_SHAPE : st;
  return rule ? r : v;
}

// every field any form's kernel reads: the host fills this once, a launch takes the struct of its form out of it (kvc_typed)
using KvcAll = tfa::KvcTree<tfa::KvcWindow<tfa::KvcSched<tfa::KvcVarlenQ<tfa::KvcPacked<tfa::Kvc8Args>>>>>;
template <typename A>
A kvc_typed(const KvcAll& ka) {
  A v;
  memset(&v, 0, sizeof(v));
  static_cast<tfa::KvcArgs&>(v) = ka;
  if constexpr (std::is_base_of<tfa::Kvc8Args, A>::value) static_cast<tfa::Kvc8Args&>(v) = ka;
  if constexpr (tfa::KvcPack<const A>::value) { v.pk_g = ka.pk_g; v.pk_fd_g = ka.pk_fd_g; v.q_hs = ka.q_hs; v.o_hs = ka.o_hs; }
  if constexpr (tfa::KvcVq<const A>::value) { v.vq_cu = ka.vq_cu; v.vq_max_q = ka.vq_max_q; v.vq_total_q = ka.vq_total_q; }
  if constexpr (tfa::KvcSc<const A>::value) { v.sc_meta = ka.sc_meta; v.sc_bound = ka.sc_bound; }
  if constexpr (tfa::KvcWin<const A>::value) v.win_left = ka.win_left;
  if constexpr (tfa::KvcTr<const A>::value) { v.tree = ka.tree; v.tree_bs = ka.tree_bs; v.tree_rs = ka.tree_rs; }
  return v;
}

}  // namespace

extern "C" {

int tfa_version(void) { return TFA_VERSION; }

const char* tfa_strerror(int status) {
  switch (status) {
    case TFA_OK: return "success";
    case TFA_ERR_NULL: return "tfa: a required pointer is NULL";
    case TFA_ERR_DTYPE: return "tfa: unsupported dtype (q/k/v must be fp16 or bf16, out matching or fp32; or q/k/v fp32 with fp32 out: the correctness path)";
    case TFA_ERR_HEAD_DIM: return "tfa: unsupported head dim (forward, split-KV and backward: multiples of 8 up to 256; TFA_FWD_EXACT_MAX: multiples of 8 up to 128; merge: multiples of 4 up to 256)";
    case TFA_ERR_SHAPE: return "tfa: bad shape (sizes must be positive and H % Hk == 0)";
    case TFA_ERR_STRIDE: return "tfa: bad stride (must be >=0, rows 16-byte aligned and non-overlapping; 768 rows of a (b,h) slice must span < 2 GiB, the whole slice for split-KV / backward)";
    case TFA_ERR_ALIGN: return "tfa: base pointers must be 16-byte aligned";
    case TFA_ERR_VARIANT: return "tfa: unknown kernel variant";
    case TFA_ERR_SCALE: return "tfa: softmax_scale must be finite and > 0";
    default: break;
  }
  if (status > 0) return hipGetErrorString((hipError_t)status);
  return "tfa: unknown status";
}

int tfa_fwd(const tfa_fwd_params* p, void* stream) { return run(p, stream, nullptr, false); }

int tfa_fwd_bhnd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int H, int N,
                 int D, float softmax_scale, int is_causal, int dtype, void* stream) {
  tfa_fwd_params p;
  fill_bhnd(&p, q, k, v, out, lse, B, H, N, D, softmax_scale, is_causal, dtype, dtype);
  return run(&p, stream, nullptr, false);
}

int tfa_fwd_bhnd_f32out(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H,
                        int N, int D, float softmax_scale, int is_causal, int dtype, void* stream) {
  tfa_fwd_params p;
  fill_bhnd(&p, q, k, v, out, lse, B, H, N, D, softmax_scale, is_causal, dtype, TFA_F32);
  return run(&p, stream, nullptr, false);
}

int tfa_fwd_plan(const tfa_fwd_params* p, int* grid, int* block, int* lds_bytes) { return plan({p, nullptr, nullptr}, grid, block, lds_bytes); }

// ---- side streams for the one-launch-per-chunk route of tfa_fwd_splitkv ----------------------------------------------------
// The chunk launches of one call are independent; on ONE stream they run one after the other and a decode-like problem (few
// workgroups per launch) fills the chip no better than tfa_fwd.  They are therefore forked over a few side streams and joined
// back into the caller's stream before the merge (event fork / join: legal inside a stream capture too).  The streams and events
// belong to the calling thread and the current device; they are created on first use and live as long as the thread.
constexpr int kSideStreams = 4;
struct SideStreams {
  int device = -1;
  hipStream_t s[kSideStreams] = {};
  hipEvent_t fork = nullptr, join[kSideStreams] = {};
  bool ok = false;
};
SideStreams* side_streams() {
  thread_local SideStreams pools[8];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  SideStreams* sp = nullptr;
  for (auto& q : pools)
    if (q.device == dev) { sp = &q; break; }
  if (!sp)
    for (auto& q : pools)
      if (q.device < 0) { sp = &q; break; }
  if (!sp) return nullptr;                                   // (more than eight devices driven by one thread: run the chunks in line)
  if (sp->device == dev) return sp->ok ? sp : nullptr;
  sp->device = dev;
  bool ok = hipEventCreateWithFlags(&sp->fork, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; i < kSideStreams && ok; ++i)
    ok = hipStreamCreateWithFlags(&sp->s[i], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&sp->join[i], hipEventDisableTiming) == hipSuccess;
  sp->ok = ok;
  if (!ok) (void)hipGetLastError();
  return ok ? sp : nullptr;
}

// ---- split-KV in one launch ------------------------------------------------------------------------------------------
static int splitkv_geometry(const tfa_fwd_params* p, int splits, int* nsplit, int* chunk) {
  if (!p || splits < 1) return TFA_ERR_SHAPE;
  if (p->dtype == TFA_F32) return TFA_ERR_DTYPE;                             // fp32 q, k, v: tfa_fwd only (tfa.h) — whichever route the call would take
  if (p->kv_offset != 0 || p->nk_total != 0) return TFA_ERR_SHAPE;          // the call splits the WHOLE key sequence
  if (p->B <= 0 || p->H <= 0 || p->Nq <= 0 || p->Nk <= 0 || p->D <= 0) return TFA_ERR_SHAPE;   // (no key: the chunk below would be 0 and divide; the others size the workspace)
  long long c = (((long long)p->Nk + splits - 1) / splits + 63) / 64 * 64;   // 64 bit: Nk + splits - 1 leaves int for splits near INT32_MAX
  if (c > INT32_MAX / 64 * 64) c = INT32_MAX / 64 * 64;                       // (Nk within 63 of INT32_MAX: the largest chunk an int holds, two of them)
  *chunk = (int)c;
  *nsplit = (int)((p->Nk + c - 1) / c);
  return TFA_OK;
}

long long tfa_fwd_splitkv_workspace(const tfa_fwd_params* p, int splits) {
  int ns = 0, ch = 0;
  const int st = splitkv_geometry(p, splits, &ns, &ch);
  if (st != TFA_OK) return st;
  return tfa::size_product({ns, p->B, p->H, p->Nq, (long long)p->D + 1});
}

int tfa_fwd_splitkv(const tfa_fwd_params* p, int splits, float* workspace, void* stream) {
  int ns = 0, ch = 0;
  int st = splitkv_geometry(p, splits, &ns, &ch);
  if (st != TFA_OK) return st;
  if (p->D < 8 || p->D > 256 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->flags & TFA_FWD_EXACT_MAX) return TFA_ERR_SHAPE;                    // (the merge moves the rounding points: see tfa.h)
  if (!workspace || ((uintptr_t)workspace & 15)) return workspace ? TFA_ERR_ALIGN : TFA_ERR_NULL;
  // the merge writes contiguous rows: out must be a contiguous (B,H,Nq,D) tensor
  if (p->o_stride[2] != p->D || p->o_stride[1] != (int64_t)p->Nq * p->D || p->o_stride[0] != (int64_t)p->H * p->Nq * p->D) return TFA_ERR_STRIDE;
  const long long rows = (long long)p->B * p->H * p->Nq;
  float* ws_o = workspace;
  float* ws_l = workspace + (long long)ns * rows * p->D;
  tfa_fwd_params q = *p;                                  // the partial pass: fp32 O and LSE of every chunk into the workspace
  q.out = ws_o;
  q.lse = ws_l;
  q.out_dtype = TFA_F32;
  q.o_stride[0] = (int64_t)p->H * p->Nq * p->D; q.o_stride[1] = (int64_t)p->Nq * p->D; q.o_stride[2] = p->D;
  if (!one_descriptor(p) || (g_dbg_flags & 8192)) {
    // (b,h) slices of 2 GiB and more (long strided K/V caches): the LDS-DMA kernel below addresses a slice through ONE descriptor,
    // tfa_fwd's kernels through windows — the partial passes are `ns` launches of tfa_fwd over key chunks (kv_offset / nk_total:
    // the causal mask stays against global key positions), one launch per chunk instead of one in all, same partials, same
    // merge.  (Debug flag 8192 forces this route: tests compare it with the one-launch form.)
    const int64_t rs_k = p->k_stride[2], rs_v = p->v_stride[2];
    hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
    // chunks that leave the chip mostly idle run side by side on the thread's side streams (debug flag 16384: in line)
    const long long blocks = (long long)p->B * p->H * ((p->Nq + 127) / 128);
    SideStreams* const pool = (ns >= 2 && blocks * 2 <= num_cus() && !(g_dbg_flags & 16384)) ? side_streams() : nullptr;
    SideStreams* ss = pool;
    // fork: every side stream waits for the caller's stream.  A stream that has been forked MUST be joined back before this function
    // returns, whatever happens in between (inside a stream capture an unjoined fork invalidates the capture): `forked` counts them,
    // and a failure half way through the fork simply runs the chunks in line on the caller's stream.
    int forked = 0;
    if (ss) {
      if (hipEventRecord(ss->fork, caller) == hipSuccess) {
        for (; forked < kSideStreams; ++forked)
          if (hipStreamWaitEvent(ss->s[forked], ss->fork, 0) != hipSuccess) break;
      }
      if (forked < kSideStreams) { (void)hipGetLastError(); ss = nullptr; }   // partial fork: joined below, chunks in line
    }
    int st_chunks = TFA_OK;
    for (int c = 0; c < ns && st_chunks == TFA_OK; ++c) {
      tfa_fwd_params qc = q;
      const int64_t k0 = (int64_t)c * ch;
      qc.k = reinterpret_cast<const char*>(p->k) + k0 * rs_k * 2;
      qc.v = reinterpret_cast<const char*>(p->v) + k0 * rs_v * 2;
      qc.Nk = (int)((p->Nk - k0) < ch ? (p->Nk - k0) : ch);
      qc.kv_offset = k0;
      qc.nk_total = p->Nk;
      qc.out = ws_o + (long long)c * rows * p->D;
      qc.lse = ws_l + (long long)c * rows;
      st_chunks = run(&qc, ss ? (void*)ss->s[c % kSideStreams] : stream, nullptr, false);
    }
    // join — every forked stream, also after a failed launch or a partial fork: the caller's stream must not lose the fork
    int st_join = TFA_OK;
    if (forked > 0) {
      for (int i = 0; i < forked; ++i) {                   // (`pool`, not `ss`: a partial fork dropped ss above)
        hipError_t e = hipEventRecord(pool->join[i], pool->s[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(caller, pool->join[i], 0);
        if (e != hipSuccess && st_join == TFA_OK) { st_join = (int)e; (void)hipGetLastError(); }   // keep joining the others
      }
    }
    if (st_chunks != TFA_OK) return st_chunks;
    if (st_join != TFA_OK) return st_join;                 // (HIP errors are reported as positive status codes: tfa_strerror)
    return tfa_merge(ws_o, ws_l, ns, rows, p->D, rows * p->D, rows, p->out, p->out_dtype, p->lse, stream);
  }
  const int variant = tfa::kSplitVariant;                 // the LDS-DMA kernel carries the chunk dimension in its grid
  tfa::KArgs a;
  {
    // GQA decode: one stream of K/V per K/V head (the workspace rows keep their order).  As in run(): the packed description is an
    // optimisation, never a requirement — when it does not validate (a q broadcast over heads: head stride 0; a row stride that
    // pushes (G + 512) rows past 2 GiB) the problem runs as the caller gave it.
    tfa_fwd_params qp;
    st = TFA_ERR_SHAPE;
    if (!(g_dbg_flags & 4096) && pack_gqa_rows(&q, &qp)) {
      st = validate(&qp, &a, variant, 0, true);
      if (st == TFA_OK) q = qp;
    }
    if (st != TFA_OK) st = validate(&q, &a, variant, 0, true);
  }
  if (st != TFA_OK) return st;
  a.nsplit = ns;
  a.chunk = ch;

  a.o_part_stride = rows * p->D;
  a.lse_part_stride = rows;
  if ((long long)a.nbh * a.nwork * ns >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool causal = q.is_causal != 0;                   // (the packed one-row problem is non-causal)
  // head dims 136..256: the same kernel 256 wide (one wave per SIMD, hand-owned accumulators)
  const hipError_t e = tfa::by_dtype_width<64, 128, 256>(p->dtype, p->D, [&](auto k) {
    using T = typename decltype(k)::T;
    if constexpr (decltype(k)::W == 256) return tfa::launch_splitkv_wide<T>(a, causal, s, nullptr, false);
    else return tfa::launch_fwd<T, decltype(k)::W>(a, causal, true, variant, s, nullptr, false);
  });
  if (e != hipSuccess) return (int)e;
  return tfa_merge(ws_o, ws_l, ns, rows, p->D, rows * p->D, rows, p->out, p->out_dtype, p->lse, stream);
}

// THE split-suggestion rule, on what its caller knows of the problem: `blocks` workgroups of 128 query rows (> 0), `keys` keys per sequence, causal_prefill —
// a causal problem whose late chunks would serve few rows (measured 0.93-1.06x).
// Up to a quarter of the CUs: one chunk per idle CU (measured 3-9x).  Between a quarter and a half: the split kernel fits two workgroups per CU, fill those
// (blocks 96: 226 -> 141 us with 4 chunks, 128: 230-240 -> 165-175 us; at 160-192 blocks a split no longer pays: profiles/r03_decode_nt_ab.txt)
static int suggest_splits_for(long long blocks, long long keys, bool causal_prefill) {
  const int cus = num_cus();
  if (blocks > cus / 2 || keys < 4096) return 1;          // (blocks * 2 > cus, without the product)
  if (causal_prefill) return 1;
  long long s = blocks * 4 > cus ? 2 * cus / blocks : cus / blocks;
  if (s > keys / 1024) s = keys / 1024;
  if (s > 32) s = 32;
  return s >= 2 ? (int)s : 1;
}

int tfa_fwd_suggest_splits(const tfa_fwd_params* p_in) {
  if (!p_in || g_variant >= 0) return 1;                  // a forced kernel variant means: run exactly that
  if (p_in->dtype == TFA_F32) return 1;                   // (the fp32 correctness path is one pass)
  if (p_in->flags & TFA_FWD_EXACT_MAX) return 1;          // (the merge of partial passes moves the rounding points as well)
  tfa_fwd_params packed;
  const tfa_fwd_params* p = pack_gqa_rows(p_in, &packed) ? &packed : p_in;
  // ((b,h) slices of 2 GiB and more take tfa_fwd_splitkv's one-launch-per-chunk route, the launches spread over side streams: a
  //  small chunk count, below)
  if (p->kv_offset != 0 || p->nk_total != 0 || p->B <= 0 || p->H <= 0 || p->Nq <= 0) return 1;
  const long long blocks = tfa::sat_mul((long long)p->B * p->H, ((long long)p->Nq + 127) / 128);
  const int s = suggest_splits_for(blocks, p->Nk, p->is_causal && (long long)p->Nq * 4 > p->Nk);
  // one launch per chunk (slices of 2 GiB and more): every chunk costs a launch on the host and the four side
  // streams overlap about two launches' worth — measured 1.4-1.8x over one pass at four chunks, less at eight or sixteen
  // (tools/bench_decode_wide.py, profiles/r03_decode_wide.txt)
  return (s > 4 && !one_descriptor(p_in)) ? 4 : s;        // (the caller's strides, as tfa_fwd_splitkv tests them — not the packed ones)
}

// ---- attention over a K/V cache (tfa.h: tfa_fwd_kvcache) ----------------------------------------------------------------------------------
// What the append and the attention both need of *p: the cache side.  Nothing here (or anywhere on this path) reads device memory.
// q8 != nullptr: the cache holds e4m3 bytes (tfa_fwd_kvcache_fp8) — its strides count bytes, its rows are 16-byte chunks of 16 elements; q, out and the new rows stay 16-bit
static int kvcache_check_cache(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8 = nullptr) {
  if (!p) return TFA_ERR_NULL;
  const int ces = q8 ? 1 : 2;                                     // bytes per cache element
  if (q8) {
    if (q8->format != TFA_KV_E4M3) return TFA_ERR_DTYPE;
    if (q8->reserved_ != 0) return TFA_ERR_SHAPE;
    if (p->D < 16 || p->D > 128 || (p->D % 16) != 0) return TFA_ERR_HEAD_DIM;
    for (int i = 0; i < 2; ++i)
      if (q8->k_descale_stride[i] < 0 || q8->v_descale_stride[i] < 0) return TFA_ERR_STRIDE;
    if (((uintptr_t)q8->k_descale | (uintptr_t)q8->v_descale) & 3) return TFA_ERR_ALIGN;
  }
  if (!p->k_cache || !p->v_cache || !p->cache_seqlens) return TFA_ERR_NULL;
  if ((p->k_new == nullptr) != (p->v_new == nullptr)) return TFA_ERR_NULL;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (p->D < 8 || p->D > 128 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->B <= 0 || p->Hk <= 0 || p->capacity <= 0 || p->n_new < 0 || p->reserved_ != 0 || p->reserved2_ != 0) return TFA_ERR_SHAPE;
  if (p->k_new ? p->n_new <= 0 : p->n_new != 0) return TFA_ERR_SHAPE;
  const bool paged = p->block_table != nullptr;
  if (paged) {
    if (p->page_size <= 0 || (p->page_size % 64) != 0 || (p->capacity % p->page_size) != 0 || p->num_pages <= 0) return TFA_ERR_SHAPE;
    if (p->block_table_stride < p->capacity / p->page_size) return TFA_ERR_STRIDE;
  }
  const int64_t span = paged ? p->page_size : p->capacity;       // rows one buffer descriptor has to reach: a page, or a sequence's slice
  const int64_t* st[4] = {p->k_stride, p->v_stride, p->knew_stride, p->vnew_stride};
  for (int t = 0; t < (p->k_new ? 4 : 2); ++t) {
    const int es = t < 2 ? ces : 2;
    for (int i = 0; i < 3; ++i)
      if (st[t][i] < 0 || (st[t][i] * es) % 16 != 0) return TFA_ERR_STRIDE;
    if (st[t][2] < p->D) return TFA_ERR_STRIDE;
    if (t < 2 && ((span + 512) * st[t][2] + p->D) * es >= (int64_t)0x7fffffff) return TFA_ERR_STRIDE;   // (one_descriptor's bound)
  }
  if (((uintptr_t)p->k_cache | (uintptr_t)p->v_cache | (uintptr_t)p->k_new | (uintptr_t)p->v_new) & 15) return TFA_ERR_ALIGN;
  if (((uintptr_t)p->cache_seqlens | (uintptr_t)p->block_table) & 3) return TFA_ERR_ALIGN;
  return TFA_OK;
}

// the chunk count a call runs: every chunk of a full sequence holds at least one 64-key tile
static int kvcache_chunks(const tfa_kvcache_params* p, int splits) {
  const int tiles = (p->capacity + 63) / 64;
  return splits < tiles ? splits : tiles;
}

// GQA / MQA decode runs packed (pack_gqa_rows: one query row per head, the H / Hk heads of a K/V head as rows of one non-causal problem)
static bool kvcache_packs(const tfa_kvcache_params* p) { return p->Nq == 1 && p->Hk > 0 && p->H > p->Hk && p->H % p->Hk == 0 && p->H / p->Hk <= 128; }
// ... and, asked for (tfa_fwd_kvcache_pack: TFA_PACK_GQA_ON), so do several rows per sequence — the Nq * G rows (position t, head g) of a K/V head as position-major
// rows of one problem, by the packed form of the kernel (tfa_fwd_kernel_dma.h: KvcPacked).  More than 128 heads per K/V head run unpacked, as at Nq == 1
static bool kvcache_packs_positions(const tfa_kvcache_params* p, int pack) {
  return pack == TFA_PACK_GQA_ON && p->Nq > 1 && p->Hk > 0 && p->H > p->Hk && p->H % p->Hk == 0 && p->H / p->Hk <= 128;
}
// The packed description of a validated launch: *a (the caller's problem, validate()) becomes the problem of B * Hk head groups of Nq * G rows; *pk receives what only
// the packed kernels read.  False — *a untouched, the call runs unpacked — when a group's rows do not fit the 32-bit byte offsets of one descriptor
// (o_esize: 4 for the fp32 partials of a split call, else 2)
static bool kvcache_pack_args(const tfa_kvcache_params* p, bool causal, int o_esize, tfa::KArgs* a, tfa::KvcPacked<tfa::Kvc8Args>* pk) {
  const int G = p->H / p->Hk;
  const long long rows = (long long)p->Nq * G;
  const long long q_hs = a->qs_h, o_hs = a->os_h;
  const long long q_ext = ((long long)(p->Nq - 1) * a->qs_n + (long long)(G - 1) * q_hs + p->D) * 2;
  const long long o_ext = ((long long)(p->Nq - 1) * a->os_n + (long long)(G - 1) * o_hs + p->D) * o_esize;
  if (rows >= 0x3fffffffll || q_ext >= 0x7fffffffll || o_ext >= 0x7fffffffll) return false;
  const int bm = tfa::block_m_of(tfa::kSplitVariant);
  const long long nmb = (rows + bm - 1) / bm;
  const long long nwork = (causal && tfa::pairs_causal(tfa::kSplitVariant)) ? (nmb + 1) / 2 : nmb;
  if ((long long)p->B * p->Hk * nwork >= 0x7fffffffll) return false;
  a->H = p->Hk;
  a->Nq = (int)rows;
  a->qs_h = G * q_hs;
  a->os_h = G * o_hs;
  a->q_bytes = (unsigned long long)q_ext;
  a->o_bytes = (unsigned long long)o_ext;
  a->nmb = (int)nmb;
  a->nwork = (int)nwork;
  a->nbh = p->B * p->Hk;
  pk->pk_g = G;
  pk->pk_fd_g = tfa::fastdiv_of((unsigned)G);
  pk->pk_pad_ = 0;
  pk->q_hs = q_hs;
  pk->o_hs = o_hs;
  return true;
}

static int kvcache_append_run(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, void* stream);

// the packed-q layout (tfa_fwd_kvcache_varlen) packs iff asked (AUTO = ON) and the heads group: Hk < H, G <= 128.  G = 1 and G > 128 run the unpacked instantiations
static bool kvcache_vq_packs(const tfa_kvcache_params* p, int pack) { return pack != TFA_PACK_GQA_OFF && p->Hk > 0 && p->H > p->Hk && p->H % p->Hk == 0 && p->H / p->Hk <= 128; }

// the launch geometry of max_q rows of gp heads each per (sequence, K/V head or head): query blocks, work items (causal blocks pair heavy / light on the launch-level index)
static void kvcache_vq_blocks(int max_q, int gp, bool causal, long long* nmb, long long* nwork) {
  const int bm = tfa::block_m_of(tfa::kSplitVariant);
  *nmb = ((long long)max_q * gp + bm - 1) / bm;
  *nwork = (causal && tfa::pairs_causal(tfa::kSplitVariant)) ? (*nmb + 1) / 2 : *nmb;
}

// the scheduled form's host-known upper bound of the batch's work items per head (= the item rows of the metadata and the `nwork` of its launch).  A sequence of n rows
// fills nb = ceil(n * G' / 128) <= n * G' / 128 + 1 blocks and never more than nmb, so with sum n <= total_q (a monotonic cu_seqlens_q) the blocks number at most
// S = min(B * nmb, ceil(total_q * G' / 128) + B): the non-causal bound.  Causal items are pairs, ceil(nb / 2) <= (nb + 1) / 2 each, so they number at most
// min(B * ceil(nmb / 2), floor((ceil(total_q * G' / 128) + 2 B) / 2)).  (tests/test_kvcache_sched_abi.py enumerates small batches against both.)
static long long kvcache_sched_bound(int B, int max_q, int total_q, int gp, bool causal) {
  long long nmb, nwork;
  kvcache_vq_blocks(max_q, gp, causal, &nmb, &nwork);
  const long long filled = ((long long)total_q * gp + 127) / 128;
  const long long launched = (long long)B * nwork, rows = nwork < nmb ? (filled + 2ll * B) / 2 : filled + B;
  return launched < rows ? launched : rows;
}
static_assert(tfa::SCHED_HDR == tfa::SCHEDULE_HDR, "one header size for the kernel that writes the list and the one that reads it");

// One K/V-cache call as an entry point names it — the K/V-cache counterpart of FwdCall — and the one host path that runs it: the 16-bit cache (q8 == nullptr) or
// the e4m3 one, q 4-D or packed (vq: tfa_fwd_kvcache_varlen and, sched, its scheduled form over the list `meta`), with a rider (a window of win_left keys, a tree)
// or without.  The _plan and _workspace entry points are dry runs of it (no GPU needed).
struct KvcCall {
  const tfa_kvcache_params* p = nullptr;
  const tfa_kvcache_varlen_q* vq = nullptr;
  const tfa_kvcache_fp8* q8 = nullptr;
  int pack = TFA_PACK_GQA_AUTO;         // AUTO: what tfa_fwd_kvcache runs (packed q: ON); ON / OFF: the caller's choice
  int splits = 1;
  const int32_t* meta = nullptr;        // the list tfa_kvcache_varlen_schedule built (NULL allowed in a dry run)
  bool sched = false;
  int win_left = -1;
  const tfa_kvcache_tree* tree = nullptr;
  int rider = tfa::KVC_NONE;            // the entry point's: KVC_WIN wants win_left >= 0, KVC_TREE a tree — their absence is then an error, not "no rider"
  bool packed_q = false;                // the entry point takes a packed q: a NULL vq is then an error, not "4-D"
  // one level of tfa_fwd_kvcache_cascade (parts > 0): the call is a partial pass only — fp32 O and LSE at every chunk count, one included, into parts
  // [part0, part0 + chunks) of a workspace of `parts` parts; the merge over all parts is the caller's.  A base-pointer offset: the kernels do not learn of it
  int part0 = 0, parts = 0;
};
static KvcCall kvc_call(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack, int splits) {
  KvcCall c;
  c.p = p; c.q8 = q8; c.pack = pack; c.splits = splits;
  return c;
}
static KvcCall kvc_varlen_call(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack, int splits, const int32_t* meta, bool sched) {
  KvcCall c = kvc_call(p, q8, pack, splits);
  c.vq = vq; c.packed_q = true; c.meta = meta; c.sched = sched;
  return c;
}
// the rider entry points take either layout: a vq makes the call a packed-q one
static KvcCall kvc_window_call(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack, int left, int splits, const int32_t* meta,
                               bool sched) {
  KvcCall c = kvc_varlen_call(p, vq, q8, pack, splits, meta, sched);
  c.packed_q = vq != nullptr; c.rider = tfa::KVC_WIN; c.win_left = left;
  return c;
}
static KvcCall kvc_tree_call(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack, const tfa_kvcache_tree* tree, int splits,
                             const int32_t* meta, bool sched) {
  KvcCall c = kvc_varlen_call(p, vq, q8, pack, splits, meta, sched);
  c.packed_q = vq != nullptr; c.rider = tfa::KVC_TREE; c.tree = tree;
  return c;
}

// the rows of out and lse: (B, H, Nq) or, packed q, (H, total_q)
static long long kvcache_rows(const KvcCall& c) { return c.vq ? (long long)c.p->H * c.vq->total_q : (long long)c.p->B * c.p->H * c.p->Nq; }

// The geometry and packing of the 4-D layout: *f is validated into *a.  One row per sequence packs heads-as-rows (pack_gqa_rows: a non-causal problem, run by the
// unpacked kernels) — as in tfa_fwd_splitkv the packed description is an optimisation, never a requirement: when it does not validate the problem runs as the caller
// gave it.  Several rows per sequence, asked for, pack position-major (*packed: the KvcPacked<> kernels): the validated problem is the caller's own — its packed
// description replaces the geometry only.  With a rider, one row per sequence packs position-major too: heads-as-rows is a non-causal problem, which has no rider —
// the position-major one serves it, t = row / G = 0.
static int kvcache_geom_4d(const KvcCall& c, int ns, tfa_fwd_params* f, tfa::KArgs* a, KvcAll* ka, bool* packed) {
  const tfa_kvcache_params* p = c.p;
  const bool rider = c.rider != tfa::KVC_NONE;
  tfa_fwd_params fp;
  int st = TFA_ERR_SHAPE;
  if (!rider && c.pack != TFA_PACK_GQA_OFF && kvcache_packs(p) && pack_gqa_rows(f, &fp)) {
    st = validate(&fp, a, tfa::kSplitVariant);
    if (st == TFA_OK) *f = fp;
  }
  if (st != TFA_OK) st = validate(f, a, tfa::kSplitVariant);
  if (st != TFA_OK) return st;
  const bool pack_pos = kvcache_packs_positions(p, c.pack) || (rider && c.pack != TFA_PACK_GQA_OFF && kvcache_packs(p));
  *packed = pack_pos && kvcache_pack_args(p, f->is_causal != 0, ns > 1 ? 4 : 2, a, ka);
  return TFA_OK;
}

// The geometry and packing of the packed-q layout: *f — one sequence of min(max_seqlen_q, total_q) rows — is validated into *a, which then takes the launch's
// geometry: max_seqlen_q * G' rows per (sequence, head) or, scheduled, heads * bound work items
static int kvcache_geom_vq(const KvcCall& c, int ns, const tfa_fwd_params* f, tfa::KArgs* a, KvcAll* ka, bool* packed_out) {
  const tfa_kvcache_params* p = c.p;
  const tfa_kvcache_varlen_q* vq = c.vq;
  const int st = validate(f, a, tfa::kSplitVariant);
  if (st != TFA_OK) return st;
  const bool causal = f->is_causal != 0;
  const int G = p->H / p->Hk, mq = f->Nq;
  const int osz = (ns > 1 || c.parts > 0) ? 4 : 2;
  bool packed = kvcache_vq_packs(p, c.pack);
  if (packed) {      // a head group's rows must fit the 32-bit byte offsets of one descriptor; else unpacked — packing is an optimisation, never a requirement
    const long long q_ext = ((long long)(mq - 1) * a->qs_n + (long long)(G - 1) * a->qs_h + p->D) * 2;
    const long long o_ext = ((long long)(mq - 1) * a->os_n + (long long)(G - 1) * a->os_h + p->D) * osz;
    if ((long long)vq->max_seqlen_q * G >= 0x3fffffffll || q_ext >= 0x7fffffffll || o_ext >= 0x7fffffffll) packed = false;
    if (c.sched && !packed) return TFA_ERR_STRIDE;       // the list was sized and built for the packing the caller named (tfa_kvcache_varlen_schedule_size): no silent change of it
  }
  const int gp = packed ? G : 1, heads = packed ? p->Hk : p->H;
  if ((long long)vq->max_seqlen_q * gp >= 0x3fffffffll) return TFA_ERR_SHAPE;
  long long nmb, nwork;
  kvcache_vq_blocks(vq->max_seqlen_q, gp, causal, &nmb, &nwork);
  const long long bound = c.sched ? kvcache_sched_bound(p->B, vq->max_seqlen_q, vq->total_q, gp, causal) : 0;
  if ((long long)p->B * heads * nwork * ns >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  if (c.sched && (long long)heads * bound * ns >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  if (packed) {
    ka->pk_g = G;
    ka->pk_fd_g = tfa::fastdiv_of((unsigned)G);
    ka->q_hs = a->qs_h;
    ka->o_hs = a->os_h;
    a->qs_h *= G;
    a->os_h *= G;
    a->H = p->Hk;
  }
  a->B = p->B;
  a->Nq = (int)((long long)vq->max_seqlen_q * gp);          // sizes the grid; the kernels take every sequence's own row count
  a->nmb = (int)nmb;
  a->nwork = (int)nwork;
  a->nbh = p->B * heads;
  if (c.sched) {                                             // heads * bound work items: the item decomposition runs over (head, row of the list)
    a->nbh = heads;
    a->nwork = (int)bound;
  }
  ka->vq_cu = vq->cu_seqlens_q;
  ka->vq_max_q = vq->max_seqlen_q;
  ka->vq_total_q = vq->total_q;
  ka->sc_meta = c.meta;
  ka->sc_bound = (int)bound;
  *packed_out = packed;
  return TFA_OK;
}

static int kvcache_run(const KvcCall& c, float* workspace, void* stream, tfa::LaunchGeom* geom, bool dry) {
  const tfa_kvcache_params* p = c.p;
  const tfa_kvcache_varlen_q* vq = c.vq;
  const tfa_kvcache_fp8* q8 = c.q8;
  // the rider's own checks: both are forms of the causal template, over any layout
  if (c.rider != tfa::KVC_NONE) {
    if (!p || (c.rider == tfa::KVC_TREE && (!c.tree || !c.tree->mask))) return TFA_ERR_NULL;
    if ((c.rider == tfa::KVC_WIN && c.win_left < 0) || !p->is_causal || (c.sched && !vq)) return TFA_ERR_SHAPE;
    if (c.rider == tfa::KVC_TREE) {
      if ((uintptr_t)c.tree->mask & 7) return TFA_ERR_ALIGN;
      if (c.tree->row_stride < 0 || (!vq && c.tree->batch_stride < 0)) return TFA_ERR_STRIDE;
    }
  }
  if (c.packed_q) {
    if (!p || !vq || !vq->cu_seqlens_q) return TFA_ERR_NULL;
    if (c.sched && !dry) {
      if (!c.meta) return TFA_ERR_NULL;
      if ((uintptr_t)c.meta & 7) return TFA_ERR_ALIGN;
    }
  }
  int st = kvcache_check_cache(p, q8);
  if (st != TFA_OK) return st;
  if (!p->q || !p->out) return TFA_ERR_NULL;
  if (p->H <= 0 || (!vq && p->Nq <= 0) || p->H % p->Hk != 0 || c.splits < 1) return TFA_ERR_SHAPE;
  if (c.pack != TFA_PACK_GQA_AUTO && c.pack != TFA_PACK_GQA_ON && c.pack != TFA_PACK_GQA_OFF) return TFA_ERR_SHAPE;
  if (vq) {
    if (vq->max_seqlen_q <= 0 || vq->total_q <= 0 || vq->reserved_[0] != 0 || vq->reserved_[1] != 0) return TFA_ERR_SHAPE;
    if (p->k_new || p->v_new || p->n_new != 0) return TFA_ERR_SHAPE;      // the append for packed rows is tfa_kvcache_append_varlen
    if ((uintptr_t)vq->cu_seqlens_q & 3) return TFA_ERR_ALIGN;
  }
  const bool paged = p->block_table != nullptr;
  const int ns = kvcache_chunks(p, c.splits);
  const long long rows = kvcache_rows(c);
  // the problem validate() sees (strides, alignment, the 2 GiB bounds of the q / out descriptors): the caller's or, packed q, ONE sequence of the most rows a
  // sequence can own after the device's clamp — its descriptors start at the sequence's first row
  tfa_fwd_params f;
  memset(&f, 0, sizeof(f));
  f.q = p->q; f.k = p->k_cache; f.v = p->v_cache; f.out = p->out; f.lse = p->lse;
  f.B = vq ? 1 : p->B; f.H = p->H; f.Hk = p->Hk; f.D = p->D;
  f.Nq = !vq ? p->Nq : vq->max_seqlen_q < vq->total_q ? vq->max_seqlen_q : vq->total_q;
  f.Nk = paged ? p->page_size : p->capacity;              // the rows one K/V descriptor spans (validate: slice_bytes)
  for (int i = 0; i < 3; ++i) { f.q_stride[i] = p->q_stride[i]; f.k_stride[i] = p->k_stride[i]; f.v_stride[i] = p->v_stride[i]; f.o_stride[i] = p->o_stride[i]; }
  if (vq) f.q_stride[0] = f.o_stride[0] = 0;              // {ignored, head, row}
  f.softmax_scale = p->softmax_scale;
  f.is_causal = p->is_causal ? 1 : 0;
  f.dtype = f.out_dtype = p->dtype;
  const bool partial = c.parts > 0;                        // a level of the cascade call: its parts of a larger workspace, no merge here
  if (partial && (!vq || c.part0 < 0 || c.part0 + ns > c.parts)) return TFA_ERR_SHAPE;
  const bool f32 = ns > 1 || partial;
  const long long nparts = partial ? c.parts : ns;         // the parts of the workspace: all O parts, then all LSE parts (part0 is 0 unless partial)
  float* ws_o = workspace ? workspace + (long long)c.part0 * rows * p->D : nullptr;
  float* ws_l = workspace ? workspace + nparts * rows * p->D + (long long)c.part0 * rows : nullptr;
  if (f32) {
    // the merge writes contiguous rows: out must be a contiguous (B,H,Nq,D) or (H,total_q,D) tensor; the partial pass writes fp32 O and LSE of every chunk into the workspace
    const int64_t head_rows = vq ? vq->total_q : p->Nq;
    if (p->o_stride[2] != p->D || p->o_stride[1] != head_rows * p->D || (!vq && p->o_stride[0] != (int64_t)p->H * p->Nq * p->D)) return TFA_ERR_STRIDE;
    if (((uintptr_t)p->out & 15)) return TFA_ERR_ALIGN;
    if (p->lse && ((uintptr_t)p->lse & 3)) return TFA_ERR_ALIGN;
    if (!dry) {
      if (!workspace) return TFA_ERR_NULL;
      if ((uintptr_t)workspace & 15) return TFA_ERR_ALIGN;
    }
    f.out = dry ? (void*)p->out : (void*)ws_o;            // (a plan has no workspace: any aligned address stands in)
    f.lse = dry ? nullptr : ws_l;
    f.out_dtype = TFA_F32;
  }
  tfa::KArgs a;
  KvcAll ka;
  memset(&ka, 0, sizeof(ka));
  bool packed = false;                                     // the KvcPacked<> kernels run
  st = vq ? kvcache_geom_vq(c, ns, &f, &a, &ka, &packed) : kvcache_geom_4d(c, ns, &f, &a, &ka, &packed);
  if (st != TFA_OK) return st;
  static_cast<tfa::KArgs&>(ka) = a;
  ka.nsplit = ns;
  ka.chunk = 0;                                            // (formed per sequence on the device)
  ka.o_part_stride = ns > 1 ? rows * p->D : 0;
  ka.lse_part_stride = ns > 1 ? rows : 0;
  ka.trace = nullptr;
  ka.seqlens = p->cache_seqlens;
  ka.block_table = p->block_table;
  ka.bt_stride = p->block_table_stride;
  ka.n_new = p->n_new;
  ka.capacity = p->capacity;
  ka.num_pages = paged ? p->num_pages : 1;
  ka.nq_pos = vq ? vq->max_seqlen_q : p->Nq;               // (packed q: not read — the shift is len_b - nq_b)
  ka.tpp = paged ? p->page_size / 64 : 1;
  ka.fd_nsplit = tfa::fastdiv_of((unsigned)ns);
  ka.fd_tpp = tfa::fastdiv_of((unsigned)ka.tpp);
  ka.kv_stream = ((long long)p->B * p->Hk * p->capacity * p->D * (q8 ? 2 : 4) >= (768ll << 20)) ? 1 : 0;
  if ((long long)ka.nbh * ka.nwork * ns >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  const bool causal = f.is_causal != 0;                    // (the packed one-row problem is non-causal)
  // tfa_fwd_splitkv's rule for the non-temporal hint; a rider's range is small: no such twin
  const bool nt = c.rider == tfa::KVC_NONE && ns > 1 && ka.kv_stream && ka.nmb == 1 && ka.H == ka.Hk;
  if (!dry && p->k_new) {                                  // this step's keys first, on the same stream
    st = kvcache_append_run(p, q8, stream);
    if (st != TFA_OK) return st;
  }
  if (q8) {
    ka.k_descale = q8->k_descale; ka.v_descale = q8->v_descale;
    ka.kd_b = q8->k_descale_stride[0]; ka.kd_h = q8->k_descale_stride[1];
    ka.vd_b = q8->v_descale_stride[0]; ka.vd_h = q8->v_descale_stride[1];
  }
  if (c.rider == tfa::KVC_WIN) ka.win_left = c.win_left < p->capacity ? c.win_left : p->capacity;
  if (c.rider == tfa::KVC_TREE) {
    ka.tree = static_cast<const unsigned long long*>(c.tree->mask);
    ka.tree_bs = vq ? 0 : c.tree->batch_stride;
    ka.tree_rs = c.tree->row_stride;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int layout = !vq ? tfa::KVC_PLAIN : c.sched ? tfa::KVC_SCHED : tfa::KVC_VQ;
  const hipError_t e = tfa::by_dtype_width<64, 128>(p->dtype, p->D, [&](auto k) {
    return tfa::by_kvc_form(q8 != nullptr, packed, layout, c.rider, [&](auto form) {
      using A = typename decltype(form)::Args;
      return tfa::launch_kvc<typename decltype(k)::T, decltype(k)::W, A>(kvc_typed<A>(ka), causal, f32, nt, s, geom, dry);
    });
  });
  if (e != hipSuccess) return (int)e;
  if (dry || partial || ns == 1) return TFA_OK;
  return tfa_merge(ws_o, ws_l, ns, rows, p->D, rows * p->D, rows, p->out, p->dtype, p->lse, stream);
}

static int kvcache_plan(const KvcCall& c, int* grid, int* block, int* lds_bytes) {
  tfa::LaunchGeom g{0, 0, 0};
  const int st = kvcache_run(c, nullptr, nullptr, &g, true);
  if (st != TFA_OK) return st;
  if (grid) *grid = g.grid;
  if (block) *block = g.block;
  if (lds_bytes) *lds_bytes = g.lds;
  return TFA_OK;
}

// fp32 words: every chunk's partial O rows and LSEs
static long long kvcache_workspace(const KvcCall& c) {
  const int st = kvcache_run(c, nullptr, nullptr, nullptr, true);
  if (st != TFA_OK) return st;
  const int ns = kvcache_chunks(c.p, c.splits);
  return ns > 1 ? ns * kvcache_rows(c) * (c.p->D + 1) : 0;
}

int tfa_fwd_kvcache(const tfa_kvcache_params* p, int splits, float* workspace, void* stream) {
  return kvcache_run(kvc_call(p, nullptr, TFA_PACK_GQA_AUTO, splits), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_plan(const tfa_kvcache_params* p, int splits, int* grid, int* block, int* lds_bytes) {
  return kvcache_plan(kvc_call(p, nullptr, TFA_PACK_GQA_AUTO, splits), grid, block, lds_bytes);
}
long long tfa_fwd_kvcache_workspace(const tfa_kvcache_params* p, int splits) { return kvcache_workspace(kvc_call(p, nullptr, TFA_PACK_GQA_AUTO, splits)); }

// the e4m3 cache: the second struct is required (its NULL descale pointers mean 1.0)
int tfa_fwd_kvcache_fp8(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits, float* workspace, void* stream) {
  return q8 ? kvcache_run(kvc_call(p, q8, TFA_PACK_GQA_AUTO, splits), workspace, stream, nullptr, false) : TFA_ERR_NULL;
}
int tfa_fwd_kvcache_fp8_plan(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits, int* grid, int* block, int* lds_bytes) {
  return q8 ? kvcache_plan(kvc_call(p, q8, TFA_PACK_GQA_AUTO, splits), grid, block, lds_bytes) : TFA_ERR_NULL;
}
long long tfa_fwd_kvcache_fp8_workspace(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int splits) {
  return q8 ? kvcache_workspace(kvc_call(p, q8, TFA_PACK_GQA_AUTO, splits)) : (long long)TFA_ERR_NULL;
}

// the same calls with the GQA packing chosen by the caller (q8 == NULL: the 16-bit cache)
int tfa_fwd_kvcache_pack(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, float* workspace, void* stream) {
  return kvcache_run(kvc_call(p, q8, pack_gqa, splits), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_pack_plan(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block, int* lds_bytes) {
  return kvcache_plan(kvc_call(p, q8, pack_gqa, splits), grid, block, lds_bytes);
}
long long tfa_fwd_kvcache_pack_workspace(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, int pack_gqa, int splits) {
  return kvcache_workspace(kvc_call(p, q8, pack_gqa, splits));
}

static int kvcache_suggest_splits(const tfa_kvcache_params* p, int pack) {
  if (!p || p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->Nq <= 0 || p->capacity <= 0 || p->H % p->Hk != 0) return 1;
  if (pack != TFA_PACK_GQA_AUTO && pack != TFA_PACK_GQA_ON && pack != TFA_PACK_GQA_OFF) return 1;
  // tfa_fwd_suggest_splits' rule on host-known sizes: the capacity stands in for the lengths (which live on the device)
  const bool packed = pack != TFA_PACK_GQA_OFF && kvcache_packs(p);     // one row per sequence: a non-causal problem
  const bool packed_rows = kvcache_packs_positions(p, pack);            // several: workgroups counted from the packed geometry
  const long long blocks = (packed || packed_rows) ? tfa::sat_mul((long long)p->B * p->Hk, ((long long)p->Nq * (p->H / p->Hk) + 127) / 128)
                                                   : tfa::sat_mul((long long)p->B * p->H, ((long long)p->Nq + 127) / 128);
  return suggest_splits_for(blocks, p->capacity, p->is_causal && !packed && (long long)p->Nq * 4 > p->capacity);
}
int tfa_fwd_kvcache_suggest_splits(const tfa_kvcache_params* p) { return kvcache_suggest_splits(p, TFA_PACK_GQA_AUTO); }
int tfa_fwd_kvcache_pack_suggest_splits(const tfa_kvcache_params* p, int pack_gqa) { return kvcache_suggest_splits(p, pack_gqa); }

// ---- the varlen-q form (tfa.h: tfa_fwd_kvcache_varlen): q packed (total_q, H, D), sequence b's rows read from cu_seqlens_q on the device ----------------------------
int tfa_fwd_kvcache_varlen(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, float* workspace, void* stream) {
  return kvcache_run(kvc_varlen_call(p, vq, q8, pack_gqa, splits, nullptr, false), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_varlen_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block, int* lds_bytes) {
  return kvcache_plan(kvc_varlen_call(p, vq, q8, pack_gqa, splits, nullptr, false), grid, block, lds_bytes);
}
long long tfa_fwd_kvcache_varlen_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits) {
  return kvcache_workspace(kvc_varlen_call(p, vq, q8, pack_gqa, splits, nullptr, false));
}
int tfa_fwd_kvcache_varlen_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa) {
  if (!p || !vq || p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->capacity <= 0 || p->H % p->Hk != 0 || vq->max_seqlen_q <= 0 || vq->total_q <= 0) return 1;
  if (pack_gqa != TFA_PACK_GQA_AUTO && pack_gqa != TFA_PACK_GQA_ON && pack_gqa != TFA_PACK_GQA_OFF) return 1;
  // tfa_fwd_kvcache_pack_suggest_splits' rule; the workgroups that have rows are bounded from what the host knows: a sequence of n rows fills at most
  // n * G' / 128 + 1 blocks, so the batch at most total_q * G' / 128 + B — and never more than the launch carries
  const bool packed = kvcache_vq_packs(p, pack_gqa);
  const int gp = packed ? p->H / p->Hk : 1;
  const long long nmb = ((long long)vq->max_seqlen_q * gp + 127) / 128;
  const long long launched = (long long)p->B * nmb, filled = ((long long)vq->total_q * gp + 127) / 128 + p->B;
  const long long blocks = tfa::sat_mul(packed ? p->Hk : p->H, launched < filled ? launched : filled);
  return suggest_splits_for(blocks, p->capacity, p->is_causal && vq->max_seqlen_q > 1 && (long long)vq->max_seqlen_q * 4 > p->capacity);
}

// ---- the scheduled form (tfa.h: tfa_kvcache_varlen_schedule, tfa_fwd_kvcache_varlen_sched): the work items of a list built on the device ---------------------------
// what the list depends on, checked: of *p only B, H, Hk are read.  *gp_out: G' of the packing named; *bound_out: the item rows
static int kvcache_sched_check(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack, int* gp_out, long long* bound_out, int is_causal) {
  if (!p || !vq) return TFA_ERR_NULL;
  if (p->B <= 0 || p->H <= 0 || p->Hk <= 0 || p->H % p->Hk != 0) return TFA_ERR_SHAPE;
  if (pack != TFA_PACK_GQA_AUTO && pack != TFA_PACK_GQA_ON && pack != TFA_PACK_GQA_OFF) return TFA_ERR_SHAPE;
  if (vq->max_seqlen_q <= 0 || vq->total_q <= 0 || vq->reserved_[0] != 0 || vq->reserved_[1] != 0) return TFA_ERR_SHAPE;
  const int gp = kvcache_vq_packs(p, pack) ? p->H / p->Hk : 1;
  if ((long long)vq->max_seqlen_q * gp >= 0x3fffffffll) return TFA_ERR_SHAPE;
  const long long bound = kvcache_sched_bound(p->B, vq->max_seqlen_q, vq->total_q, gp, is_causal != 0);
  if (bound >= 0x3fffffffll) return TFA_ERR_SHAPE;
  *gp_out = gp;
  *bound_out = bound;
  return TFA_OK;
}
long long tfa_kvcache_varlen_schedule_size(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal) {
  int gp;
  long long bound;
  const int st = kvcache_sched_check(p, vq, pack_gqa, &gp, &bound, is_causal);
  return st != TFA_OK ? st : tfa::SCHEDULE_HDR + 2 * bound;
}
static int kvcache_schedule_run(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack, int is_causal, int32_t* meta, void* stream, bool dry) {
  int gp;
  long long bound;
  const int st = kvcache_sched_check(p, vq, pack, &gp, &bound, is_causal);
  if (st != TFA_OK) return st;
  if (!vq->cu_seqlens_q || (!dry && !meta)) return TFA_ERR_NULL;
  if (((uintptr_t)vq->cu_seqlens_q & 3) || ((uintptr_t)meta & 7)) return TFA_ERR_ALIGN;
  if (dry) return TFA_OK;
  tfa::ScheduleArgs a;
  a.cu = vq->cu_seqlens_q;
  a.meta = meta;
  a.B = p->B; a.gp = gp; a.causal = is_causal ? 1 : 0;
  a.max_q = vq->max_seqlen_q; a.total_q = vq->total_q;
  a.bound = (int)bound;
  return (int)tfa::launch_kvcache_schedule(a, reinterpret_cast<hipStream_t>(stream));
}
int tfa_kvcache_varlen_schedule(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal, int32_t* metadata, void* stream) {
  return kvcache_schedule_run(p, vq, pack_gqa, is_causal, metadata, stream, false);
}
int tfa_kvcache_varlen_schedule_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int is_causal, int* grid, int* block, int* lds_bytes) {
  const int st = kvcache_schedule_run(p, vq, pack_gqa, is_causal, nullptr, nullptr, true);
  if (st != TFA_OK) return st;
  if (grid) *grid = 1;
  if (block) *block = 256;
  if (lds_bytes) *lds_bytes = 256 * 8;
  return TFA_OK;
}
int tfa_fwd_kvcache_varlen_sched(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, const int32_t* metadata,
                                 float* workspace, void* stream) {
  return kvcache_run(kvc_varlen_call(p, vq, q8, pack_gqa, splits, metadata, true), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_varlen_sched_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int splits, int* grid, int* block,
                                      int* lds_bytes) {
  return kvcache_plan(kvc_varlen_call(p, vq, q8, pack_gqa, splits, nullptr, true), grid, block, lds_bytes);
}

// ---- the windowed form (tfa.h: tfa_fwd_kvcache_window): one entry point over the 4-D, packed-q and scheduled layouts ------------------------------------------------
int tfa_fwd_kvcache_window(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int window_left, int splits, const int32_t* metadata,
                           float* workspace, void* stream) {
  return kvcache_run(kvc_window_call(p, vq, q8, pack_gqa, window_left, splits, metadata, metadata != nullptr), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_window_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int window_left, int splits, int scheduled,
                                int* grid, int* block, int* lds_bytes) {
  return kvcache_plan(kvc_window_call(p, vq, q8, pack_gqa, window_left, splits, nullptr, scheduled != 0), grid, block, lds_bytes);
}
long long tfa_fwd_kvcache_window_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, int window_left, int splits) {
  return kvcache_workspace(kvc_window_call(p, vq, q8, pack_gqa, window_left, splits, nullptr, false));
}
int tfa_fwd_kvcache_window_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, int window_left) {
  if (!p || window_left < 0 || p->capacity <= 0) return 1;
  // the underlying form's rule; the keys a row streams, min(capacity, round_up(window_left + rows, 64) + 64), stand in for the lengths
  const long long rows = vq ? vq->max_seqlen_q : p->Nq;
  const long long reach = ((window_left + (rows > 0 ? rows : 0) + 63) & ~63ll) + 64;
  tfa_kvcache_params w = *p;
  if (reach < w.capacity) w.capacity = (int)reach;
  return vq ? tfa_fwd_kvcache_varlen_suggest_splits(&w, vq, pack_gqa) : kvcache_suggest_splits(&w, pack_gqa);
}

// ---- the tree form (tfa.h: tfa_fwd_kvcache_tree): one entry point over the same three layouts; the mask removes no tile, so everything but the kernel is the form's --------
int tfa_fwd_kvcache_tree(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, const tfa_kvcache_tree* tree, int splits,
                         const int32_t* metadata, float* workspace, void* stream) {
  return kvcache_run(kvc_tree_call(p, vq, q8, pack_gqa, tree, splits, metadata, metadata != nullptr), workspace, stream, nullptr, false);
}
int tfa_fwd_kvcache_tree_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, const tfa_kvcache_tree* tree, int splits,
                              int scheduled, int* grid, int* block, int* lds_bytes) {
  return kvcache_plan(kvc_tree_call(p, vq, q8, pack_gqa, tree, splits, nullptr, scheduled != 0), grid, block, lds_bytes);
}
long long tfa_fwd_kvcache_tree_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_fp8* q8, int pack_gqa, const tfa_kvcache_tree* tree,
                                         int splits) {
  return kvcache_workspace(kvc_tree_call(p, vq, q8, pack_gqa, tree, splits, nullptr, false));
}
int tfa_fwd_kvcache_tree_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, int pack_gqa, const tfa_kvcache_tree* tree) {
  (void)tree;                                              // the underlying form's rule: the mask removes no tile
  if (!p) return 1;
  return vq ? tfa_fwd_kvcache_varlen_suggest_splits(p, vq, pack_gqa) : kvcache_suggest_splits(p, pack_gqa);
}

// ---- the cascade form (tfa.h: tfa_fwd_kvcache_cascade): two packed-q calls over one pool — the groups' shared keys, the sequences' own — as partial passes into one
// workspace, and one merge over all their parts.  Both levels are KvcCalls through kvcache_run; what is new on the device is the merge that skips empty parts
// (tfa_merge.hip: tfa::merge_skip)
// level 0 as a packed-q call of its own: the groups as its sequences, non-causal, over the same q, out and pool
struct KvcCascade {
  tfa_kvcache_params p0;
  tfa_kvcache_varlen_q vq0;
};
static int kvcache_cascade_levels(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, KvcCascade* lv) {
  if (!p || !vq || !cs || !cs->prefix_cu_seqlens_q || !cs->prefix_seqlens || !cs->prefix_block_table || !p->block_table) return TFA_ERR_NULL;
  if (cs->num_groups <= 0 || cs->prefix_max_blocks <= 0 || cs->prefix_max_seqlen_q <= 0 || cs->reserved_ != 0) return TFA_ERR_SHAPE;
  if (p->page_size <= 0 || (long long)cs->prefix_max_blocks * p->page_size > 0x7fffffffll) return TFA_ERR_SHAPE;
  if (((uintptr_t)cs->prefix_cu_seqlens_q | (uintptr_t)cs->prefix_seqlens | (uintptr_t)cs->prefix_block_table) & 3) return TFA_ERR_ALIGN;
  lv->p0 = *p;
  lv->p0.B = cs->num_groups;
  lv->p0.cache_seqlens = cs->prefix_seqlens;
  lv->p0.block_table = cs->prefix_block_table;
  lv->p0.block_table_stride = cs->prefix_block_table_stride;
  lv->p0.capacity = cs->prefix_max_blocks * p->page_size;
  lv->p0.is_causal = 0;
  lv->vq0 = *vq;
  lv->vq0.cu_seqlens_q = cs->prefix_cu_seqlens_q;
  lv->vq0.max_seqlen_q = cs->prefix_max_seqlen_q;
  return TFA_OK;
}
// the two levels as calls: dry runs of both validate everything before anything is launched.  *ns0 / *ns1: the chunk counts each level runs
static int kvcache_cascade_calls(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack, int splits, int prefix_splits,
                                 const int32_t* meta, const int32_t* prefix_meta, bool sched, bool prefix_sched, KvcCascade* lv, KvcCall* c0, KvcCall* c1, int* ns0,
                                 int* ns1) {
  int st = kvcache_cascade_levels(p, vq, cs, lv);
  if (st != TFA_OK) return st;
  if (splits < 1 || prefix_splits < 1) return TFA_ERR_SHAPE;
  *c0 = kvc_varlen_call(&lv->p0, &lv->vq0, nullptr, pack, prefix_splits, prefix_meta, prefix_sched);
  *c1 = kvc_varlen_call(p, vq, nullptr, pack, splits, meta, sched);
  if (p->capacity <= 0) return TFA_ERR_SHAPE;
  *ns0 = kvcache_chunks(&lv->p0, prefix_splits);
  *ns1 = kvcache_chunks(p, splits);
  c0->part0 = 0; c1->part0 = *ns0;
  c0->parts = c1->parts = *ns0 + *ns1;
  st = kvcache_run(*c1, nullptr, nullptr, nullptr, true);
  return st != TFA_OK ? st : kvcache_run(*c0, nullptr, nullptr, nullptr, true);
}

int tfa_fwd_kvcache_cascade(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits, int prefix_splits,
                            const int32_t* metadata, const int32_t* prefix_metadata, float* workspace, void* stream) {
  KvcCascade lv;
  KvcCall c0, c1;
  int ns0 = 0, ns1 = 0;
  int st = kvcache_cascade_calls(p, vq, cs, pack_gqa, splits, prefix_splits, metadata, prefix_metadata, metadata != nullptr, prefix_metadata != nullptr, &lv, &c0, &c1,
                                 &ns0, &ns1);
  if (st != TFA_OK) return st;
  if (!workspace) return TFA_ERR_NULL;
  if (((uintptr_t)workspace & 15) || (((uintptr_t)metadata | (uintptr_t)prefix_metadata) & 7)) return TFA_ERR_ALIGN;
  const int parts = ns0 + ns1;
  const long long rows = kvcache_rows(c1);
  float* ws_l = workspace + (long long)parts * rows * p->D;
  // every part starts empty (+inf, 0x7f800000): the rows no group owns, the rows no sequence owns and the blocks without rows are written by no level
  const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws_l), 0x7f800000, (size_t)((long long)parts * rows), reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return (int)e;
  st = kvcache_run(c0, workspace, stream, nullptr, false);
  if (st != TFA_OK) return st;
  st = kvcache_run(c1, workspace, stream, nullptr, false);
  if (st != TFA_OK) return st;
  return tfa::merge_skip(workspace, ws_l, parts, rows, p->D, rows * p->D, rows, p->out, p->dtype, p->lse, stream);
}
long long tfa_fwd_kvcache_cascade_workspace(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits,
                                            int prefix_splits) {
  KvcCascade lv;
  KvcCall c0, c1;
  int ns0 = 0, ns1 = 0;
  const int st = kvcache_cascade_calls(p, vq, cs, pack_gqa, splits, prefix_splits, nullptr, nullptr, false, false, &lv, &c0, &c1, &ns0, &ns1);
  if (st != TFA_OK) return st;
  return (long long)(ns0 + ns1) * kvcache_rows(c1) * (p->D + 1);
}
int tfa_fwd_kvcache_cascade_plan(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int splits, int prefix_splits,
                                 int scheduled, int prefix_scheduled, int level, int* grid, int* block, int* lds_bytes) {
  KvcCascade lv;
  KvcCall c0, c1;
  int ns0 = 0, ns1 = 0;
  const int st = kvcache_cascade_calls(p, vq, cs, pack_gqa, splits, prefix_splits, nullptr, nullptr, scheduled != 0, prefix_scheduled != 0, &lv, &c0, &c1, &ns0, &ns1);
  if (st != TFA_OK) return st;
  if (level != 0 && level != 1) return TFA_ERR_SHAPE;
  return kvcache_plan(level == 0 ? c0 : c1, grid, block, lds_bytes);
}
int tfa_fwd_kvcache_cascade_suggest_splits(const tfa_kvcache_params* p, const tfa_kvcache_varlen_q* vq, const tfa_kvcache_cascade* cs, int pack_gqa, int* splits,
                                           int* prefix_splits) {
  KvcCascade lv;
  if (!splits || !prefix_splits) return TFA_ERR_NULL;
  const int st = kvcache_cascade_levels(p, vq, cs, &lv);
  if (st != TFA_OK) return st;
  *splits = tfa_fwd_kvcache_varlen_suggest_splits(p, vq, pack_gqa);
  *prefix_splits = tfa_fwd_kvcache_varlen_suggest_splits(&lv.p0, &lv.vq0, pack_gqa);
  return TFA_OK;
}

static int kvcache_append_run(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, void* stream) {
  const int st = kvcache_check_cache(p, q8);
  if (st != TFA_OK) return st;
  if (!p->k_new) return TFA_ERR_NULL;
  tfa::Append8Args a;                                      // (the 16-bit launch takes its AppendArgs base)
  memset(&a, 0, sizeof(a));
  a.k_new = p->k_new; a.v_new = p->v_new; a.k_cache = p->k_cache; a.v_cache = p->v_cache;
  a.seqlens = p->cache_seqlens;
  a.block_table = p->block_table;
  a.bt_stride = p->block_table_stride;
  a.ks_b = p->k_stride[0]; a.ks_h = p->k_stride[1]; a.ks_n = p->k_stride[2];
  a.vs_b = p->v_stride[0]; a.vs_h = p->v_stride[1]; a.vs_n = p->v_stride[2];
  a.kn_b = p->knew_stride[0]; a.kn_h = p->knew_stride[1]; a.kn_n = p->knew_stride[2];
  a.vn_b = p->vnew_stride[0]; a.vn_h = p->vnew_stride[1]; a.vn_n = p->vnew_stride[2];
  a.n_new = p->n_new; a.Hk = p->Hk; a.cpr = p->D / 8;
  a.total = (long long)p->B * p->n_new * p->Hk * a.cpr;
  a.capacity = p->capacity;
  a.page_size = p->block_table ? p->page_size : 1;
  a.num_pages = p->block_table ? p->num_pages : 1;
  if (!q8) return (int)tfa::launch_kvcache_append(a, reinterpret_cast<hipStream_t>(stream));
  a.k_descale = q8->k_descale; a.v_descale = q8->v_descale;
  a.kd_b = q8->k_descale_stride[0]; a.kd_h = q8->k_descale_stride[1];
  a.vd_b = q8->v_descale_stride[0]; a.vd_h = q8->v_descale_stride[1];
  a.bf16 = p->dtype == TFA_BF16 ? 1 : 0;
  return (int)tfa::launch_kvcache_append_fp8(a, reinterpret_cast<hipStream_t>(stream));
}

int tfa_kvcache_append(const tfa_kvcache_params* p, void* stream) { return kvcache_append_run(p, nullptr, stream); }
int tfa_kvcache_append_fp8(const tfa_kvcache_params* p, const tfa_kvcache_fp8* q8, void* stream) { return q8 ? kvcache_append_run(p, q8, stream) : TFA_ERR_NULL; }

int tfa_fwd_varlen(const tfa_varlen_fwd_params* p, void* stream) { return route({nullptr, p, nullptr}, stream); }
int tfa_fwd_varlen_plan(const tfa_varlen_fwd_params* p, int* grid, int* block, int* lds_bytes) { return plan({nullptr, p, nullptr}, grid, block, lds_bytes); }
int tfa_fwd_varlen_variant(const tfa_varlen_fwd_params* p) { return variant_or_rule({nullptr, p, nullptr}, false); }
int tfa_fwd_varlen_rounding_rule(const tfa_varlen_fwd_params* p) { return variant_or_rule({nullptr, p, nullptr}, true); }

int tfa_fwd_varlen_paged(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg, void* stream) { return route({nullptr, p, nullptr, nullptr, pg, true}, stream); }
int tfa_fwd_varlen_paged_plan(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg, int* grid, int* block, int* lds_bytes) {
  return plan({nullptr, p, nullptr, nullptr, pg, true}, grid, block, lds_bytes);
}
int tfa_fwd_varlen_paged_variant(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg) { return variant_or_rule({nullptr, p, nullptr, nullptr, pg, true}, false); }
int tfa_fwd_varlen_paged_rounding_rule(const tfa_varlen_fwd_params* p, const tfa_paged_kv* pg) { return variant_or_rule({nullptr, p, nullptr, nullptr, pg, true}, true); }

int tfa_fwd_local(const tfa_fwd_params* p, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  return route({p, nullptr, w}, stream);
}
int tfa_fwd_local_plan(const tfa_fwd_params* p, int window_left, int window_right, int* grid, int* block, int* lds_bytes) {
  const int w[2] = {window_left, window_right};
  return plan({p, nullptr, w}, grid, block, lds_bytes);
}
int tfa_fwd_local_variant(const tfa_fwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return variant_or_rule({p, nullptr, w}, false);
}
int tfa_fwd_local_rounding_rule(const tfa_fwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return variant_or_rule({p, nullptr, w}, true);
}
int tfa_fwd_varlen_local(const tfa_varlen_fwd_params* p, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  return route({nullptr, p, w}, stream);
}
int tfa_fwd_varlen_local_plan(const tfa_varlen_fwd_params* p, int window_left, int window_right, int* grid, int* block, int* lds_bytes) {
  const int w[2] = {window_left, window_right};
  return plan({nullptr, p, w}, grid, block, lds_bytes);
}
int tfa_fwd_varlen_local_variant(const tfa_varlen_fwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return variant_or_rule({nullptr, p, w}, false);
}
int tfa_fwd_varlen_local_rounding_rule(const tfa_varlen_fwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return variant_or_rule({nullptr, p, w}, true);
}

// ALiBi: the fixed-length (p) or varlen (vp) call with its slopes and window
#define TFA_ALIBI_CALL(p, vp)                                   \
  const int w[2] = {window_left, window_right};                 \
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride};    \
  const FwdCall call{p, vp, w, &al}
int tfa_fwd_alibi(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream) {
  TFA_ALIBI_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return route(call, stream);
}
int tfa_fwd_alibi_plan(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, int* grid, int* block,
                       int* lds_bytes) {
  TFA_ALIBI_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return plan(call, grid, block, lds_bytes);
}
int tfa_fwd_alibi_variant(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  TFA_ALIBI_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, false);
}
int tfa_fwd_alibi_rounding_rule(const tfa_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  TFA_ALIBI_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, true);
}
int tfa_fwd_varlen_alibi(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream) {
  TFA_ALIBI_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return route(call, stream);
}
int tfa_fwd_varlen_alibi_plan(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, int* grid,
                              int* block, int* lds_bytes) {
  TFA_ALIBI_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return plan(call, grid, block, lds_bytes);
}
int tfa_fwd_varlen_alibi_variant(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  TFA_ALIBI_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, false);
}
int tfa_fwd_varlen_alibi_rounding_rule(const tfa_varlen_fwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  TFA_ALIBI_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, true);
}
#undef TFA_ALIBI_CALL

// Soft-capping: the ALiBi call with the cap in front; the slopes may be NULL
#define TFA_SOFTCAP_CALL(p, vp)                                                 \
  const int w[2] = {window_left, window_right};                                 \
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride, true, softcap};     \
  const FwdCall call{p, vp, w, &al}
int tfa_fwd_softcap(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                    void* stream) {
  TFA_SOFTCAP_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return route(call, stream);
}
int tfa_fwd_softcap_plan(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                         int* grid, int* block, int* lds_bytes) {
  TFA_SOFTCAP_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return plan(call, grid, block, lds_bytes);
}
int tfa_fwd_softcap_variant(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  TFA_SOFTCAP_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, false);
}
int tfa_fwd_softcap_rounding_rule(const tfa_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                  int window_right) {
  TFA_SOFTCAP_CALL(p, nullptr);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, true);
}
int tfa_fwd_varlen_softcap(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                           int window_right, void* stream) {
  TFA_SOFTCAP_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return route(call, stream);
}
int tfa_fwd_varlen_softcap_plan(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                int window_right, int* grid, int* block, int* lds_bytes) {
  TFA_SOFTCAP_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return plan(call, grid, block, lds_bytes);
}
int tfa_fwd_varlen_softcap_variant(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                   int window_right) {
  TFA_SOFTCAP_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, false);
}
int tfa_fwd_varlen_softcap_rounding_rule(const tfa_varlen_fwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride,
                                         int window_left, int window_right) {
  TFA_SOFTCAP_CALL(nullptr, p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, true);
}
#undef TFA_SOFTCAP_CALL

// Dense bias: the fixed-length ALiBi call with the bias tensor in the slopes' place (a NULL struct is refused by check_bias)
#define TFA_BIAS_CALL(p)                                        \
  const int w[2] = {window_left, window_right};                 \
  tfa::AlibiArg al{};                                           \
  al.bias = bias;                                               \
  al.biased = true;                                             \
  const FwdCall call{p, nullptr, w, &al}
int tfa_fwd_bias(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, void* stream) {
  TFA_BIAS_CALL(p);
  if (!p) return TFA_ERR_NULL;
  return route(call, stream);
}
int tfa_fwd_bias_plan(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, int* grid, int* block, int* lds_bytes) {
  TFA_BIAS_CALL(p);
  if (!p) return TFA_ERR_NULL;
  return plan(call, grid, block, lds_bytes);
}
int tfa_fwd_bias_variant(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right) {
  TFA_BIAS_CALL(p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, false);
}
int tfa_fwd_bias_rounding_rule(const tfa_fwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right) {
  TFA_BIAS_CALL(p);
  if (!p) return TFA_ERR_NULL;
  return variant_or_rule(call, true);
}
#undef TFA_BIAS_CALL

int tfa_fwd_variant(const tfa_fwd_params* p) { return variant_or_rule({p, nullptr, nullptr}, false); }   // (run()'s final choice, after GQA packing and its fall-back)
int tfa_fwd_rounding_rule(const tfa_fwd_params* p) { return variant_or_rule({p, nullptr, nullptr}, true); }

int tfa_fwd_time(const tfa_fwd_params* p, int warmup, int iters, void* stream, float* avg_ms) {
  if (!avg_ms || iters <= 0 || warmup < 0) return TFA_ERR_NULL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int i = 0; i < warmup; ++i) {
    const int st = run(p, stream, nullptr, false);
    if (st != 0) return st;
  }
  hipEvent_t e0, e1;
  hipError_t e = hipEventCreate(&e0);
  if (e != hipSuccess) return (int)e;
  e = hipEventCreate(&e1);
  if (e != hipSuccess) { (void)hipEventDestroy(e0); return (int)e; }
  int st = 0;
  (void)hipEventRecord(e0, s);
  for (int i = 0; i < iters && st == 0; ++i) st = run(p, stream, nullptr, false);
  (void)hipEventRecord(e1, s);
  e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != 0) return st;
  if (e != hipSuccess) return (int)e;
  *avg_ms = ms / (float)iters;
  return TFA_OK;
}

int tfa_set_variant(int variant) {
  // dispatchable numbers: -1 (automatic), the kVariants table, and the timing-only ablation ranges of the EXPERIMENTAL build
  const bool in_table = variant >= 0 && variant < tfa::kNumVariants;
  const bool ablation = (variant >= 100 && variant < 612) || (variant >= 700 && variant < 716) || (variant >= 1000 && variant < 2256) ||
                        (variant >= 3000 && variant < 3256);
  if (variant != -1 && !in_table && !ablation) return TFA_ERR_VARIANT;
  if (in_table && !tfa::variant_built(variant)) return TFA_ERR_VARIANT;
  g_variant = variant;
  return TFA_OK;
}
int tfa_get_variant(void) { return g_variant; }
int tfa_debug_set_flags(int flags) { g_dbg_flags = flags; return TFA_OK; }
int tfa_debug_decode(int B, int H, int Hk, int nwork, int id, int* out) {
  if (!out || B < 1 || H < 1 || Hk < 1 || nwork < 1 || id < 0 || H % Hk) return TFA_ERR_SHAPE;
  tfa::KArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.Hk = Hk; a.nwork = nwork; a.nbh = B * H;
  tfa::fill_decode(&a);
  // the device code of tfa_fwd_kernel_il.h, on the host (fd_div is a device function: its formula here)
  auto div = [](int n, tfa::FastDiv f) { return (int)(((unsigned)(((unsigned long long)(unsigned)n * f.m) >> 32) + (unsigned)n) >> f.l); };
  const int x = a.rr ? (id & 7) : 0, s = a.rr ? (id >> 3) : id;
  const int sq = div(s, a.fd_wa), r = s - sq * a.wa;
  const int kg = a.rr ? x + 8 * sq : sq;
  const int rq = div(r, a.fd_nwork);
  out[3] = r - rq * a.nwork;
  out[0] = div(kg, a.fd_wd);
  out[1] = (kg - out[0] * a.wd) * a.wg + rq;
  out[2] = div(out[1], a.fd_g);
  return TFA_OK;
}
int tfa_debug_set_trace(void* dev_buf) { g_trace = reinterpret_cast<unsigned long long*>(dev_buf); return TFA_OK; }
int tfa_num_variants(void) { return tfa::kNumVariants; }
int tfa_variant_available(int variant) { return tfa::variant_built(variant) ? 1 : 0; }
const char* tfa_variant_name(int variant) {
  if (variant < 0 || variant >= tfa::kNumVariants) return "auto";
  const tfa::Variant* v = tfa::variant_info(variant);
  return v ? v->name : "(an A/B arm: not in this build, make EXPERIMENTAL=1)";
}

int tfa_fwd_work(const tfa_fwd_params* p, double* flops, double* bytes) {
  if (!p) return TFA_ERR_NULL;
  const double bh = (double)p->B * p->H;
  double pairs;   // visible (query,key) pairs per (b,h)
  if (p->is_causal) {
    // row i sees min(Nk, max(0, i + 1 + Nk - Nq)) keys
    pairs = 0;
    const long long shift = (long long)p->Nk - p->Nq;
    if (shift >= 0) {
      pairs = (double)p->Nq * (double)(shift) + 0.5 * (double)p->Nq * ((double)p->Nq + 1.0);
    } else {
      const double n = (double)p->Nk;   // only the last Nk rows see anything
      pairs = 0.5 * n * (n + 1.0);
    }
    // the reference's convention is exactly half of the full square when Nq == Nk
    if (p->Nq == p->Nk) pairs = 0.5 * (double)p->Nq * (double)p->Nk;
  } else {
    pairs = (double)p->Nq * (double)p->Nk;
  }
  if (flops) *flops = 4.0 * bh * pairs * p->D;
  if (bytes) {
    const double osz = (p->out_dtype == TFA_F32) ? 4.0 : 2.0;
    const double bkv = (double)p->B * p->Hk;
    const double isz = (p->dtype == TFA_F32) ? 4.0 : 2.0;
    *bytes = bh * p->Nq * p->D * isz + 2.0 * bkv * p->Nk * p->D * isz + bh * p->Nq * p->D * osz +
             (p->lse ? bh * p->Nq * 4.0 : 0.0);
  }
  return TFA_OK;
}

}  // extern "C"
