// tfa_kvcache.h — host-side declarations of the K/V-cache path (include/tfa.h: tfa_fwd_kvcache, tfa_kvcache_append): the append kernel's
// arguments, beside the launcher of the KV-cache form of the LDS-DMA kernel (tfa_launch.h: launch_kvc over TFA_KVC_FORMS; tfa_fwd_kernel_dma.h: VF_KVCACHE,
// KvcArgs), one translation unit per (form, dtype, width) — tfa_kvc_inst.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfa {

// tfa_kvcache_append.hip (strides in ELEMENTS; 16-bit elements, 16-byte chunks)
struct AppendArgs {
  const void* k_new;          // (B, n_new, Hk, D) by strides kn_* / vn_*
  const void* v_new;
  void* k_cache;
  void* v_cache;
  const int* seqlens;         // device, B entries: row t of sequence b goes to key position seqlens[b] + t
  const int* block_table;     // device (B, max_blocks) by bt_stride, or nullptr: contiguous cache
  long long bt_stride;
  long long ks_b, ks_h, ks_n; // cache strides: batch (contiguous) or page (paged), head, row
  long long vs_b, vs_h, vs_n;
  long long kn_b, kn_h, kn_n; // k_new strides: batch, head, row
  long long vn_b, vn_h, vn_n;
  long long total;            // threads with work: B * n_new * Hk * cpr
  int n_new, Hk, cpr;         // cpr = D / 8: 16-byte chunks per row
  int capacity;               // keys a sequence can hold: Nk_max, or max_blocks * page_size
  int page_size, num_pages;
};
hipError_t launch_kvcache_append(const AppendArgs& a, hipStream_t stream);

// tfa_kvcache_append_fp8.hip: the same append into an e4m3 cache — the new rows are 16-bit (bf16: the k_new / v_new dtype), the cache strides count bytes, every thread
// turns 8 elements into 8 bytes: byte = rne_e4m3fn(clamp(float(x) / descale[b, hk], -448, 448)), NaN stays NaN
struct Append8Args : AppendArgs {
  const float* k_descale;     // device fp32 by (kd_b, kd_h) elements, or nullptr = 1.0
  const float* v_descale;
  long long kd_b, kd_h, vd_b, vd_h;
  int bf16;                   // the new rows' dtype: 1 = bf16, 0 = f16
};
hipError_t launch_kvcache_append_fp8(const Append8Args& a, hipStream_t stream);

// tfa_kvcache_schedule.hip: the work list of tfa_fwd_kvcache_varlen_sched, built on the device from cu_seqlens_q (one workgroup of 256 threads)
constexpr int SCHEDULE_HDR = 8;   // header words (tfa_fwd_kernel_dma.h: SCHED_HDR — the same number, asserted in tfa_api.hip)
struct ScheduleArgs {
  const int* cu;              // device int32, B + 1 entries
  int* meta;                  // device int32, SCHEDULE_HDR + 2 * bound entries, 8-byte aligned
  int B, gp, causal;          // gp = G' (G packed, 1 unpacked)
  int max_q, total_q;
  int bound;                  // item rows the buffer holds
};
hipError_t launch_kvcache_schedule(const ScheduleArgs& a, hipStream_t stream);

}  // namespace tfa
