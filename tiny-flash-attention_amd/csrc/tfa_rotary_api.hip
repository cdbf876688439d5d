// tfa_rotary_api.hip — the C entry points of the serving step's parts around attention (include/tfa.h): tfa_rotary / tfa_rotary_plan and
// tfa_kvcache_append_varlen / _plan and tfa_kvcache_append_varlen_ex / _plan.  Validation on host-known values only (nothing here reads device memory), then one launch on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tfa.h"
#include "tfa_rotary.h"

namespace {

bool bad_stride(int64_t s) { return s < 0 || s % 8 != 0; }         // 16-bit elements: every row, head and batch a whole number of 16-byte chunks on
bool bad_stride8(int64_t s) { return s < 0 || s % 16 != 0; }          // the strides of an e4m3 cache: bytes

// the tables of both entry points: (seqlen_ro, rotary_dim / 2) of cs_dtype, 16-byte aligned rows
int check_tables(const void* cos, const void* sin, int dtype, int cs_dtype, int D, int rotary_dim, int seqlen_ro, int64_t cos_stride, int64_t sin_stride, int interleaved) {
  if (cs_dtype != dtype && cs_dtype != TFA_F32) return TFA_ERR_DTYPE;
  if (rotary_dim < 16 || rotary_dim > D || (rotary_dim % 16) != 0) return TFA_ERR_HEAD_DIM;
  if (seqlen_ro <= 0 || (interleaved != 0 && interleaved != 1)) return TFA_ERR_SHAPE;
  const int es = cs_dtype == TFA_F32 ? 4 : 2;
  if (cos_stride < rotary_dim / 2 || sin_stride < rotary_dim / 2 || cos_stride % (16 / es) != 0 || sin_stride % (16 / es) != 0) return TFA_ERR_STRIDE;
  if (((uintptr_t)cos | (uintptr_t)sin) & 15) return TFA_ERR_ALIGN;
  return TFA_OK;
}

int rotary_run(const tfa_rotary_params* p, void* stream, int* grid, int* block, bool dry) {
  if (!p) return TFA_ERR_NULL;
  if (!p->x || !p->out || !p->cos || !p->sin) return TFA_ERR_NULL;
  if ((p->x2 == nullptr) != (p->out2 == nullptr)) return TFA_ERR_NULL;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (p->cs_dtype != p->dtype && p->cs_dtype != TFA_F32) return TFA_ERR_DTYPE;
  if (p->D < 8 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->rotary_dim < 16 || p->rotary_dim > p->D || (p->rotary_dim % 16) != 0) return TFA_ERR_HEAD_DIM;
  if (p->B <= 0 || p->N <= 0 || p->H <= 0 || p->H2 < 0 || (p->H2 > 0) != (p->x2 != nullptr)) return TFA_ERR_SHAPE;
  if (p->conjugate != 0 && p->conjugate != 1) return TFA_ERR_SHAPE;
  const bool packed = p->cu_seqlens != nullptr;
  const int64_t* st[4] = {p->x_stride, p->o_stride, p->x2_stride, p->o2_stride};
  for (int t = 0; t < (p->x2 ? 4 : 2); ++t)
    for (int i = packed ? 1 : 0; i < 3; ++i)
      if (bad_stride(st[t][i])) return TFA_ERR_STRIDE;
  for (int t = 0; t < (p->x2 ? 2 : 1); ++t) {              // in place: the same rows, not a shifted or re-strided view of them
    const void* x = t ? p->x2 : p->x;
    const void* o = t ? p->out2 : p->out;
    if (x == o)
      for (int i = packed ? 1 : 0; i < 3; ++i)
        if (st[2 * t][i] != st[2 * t + 1][i]) return TFA_ERR_STRIDE;
  }
  const int tb = check_tables(p->cos, p->sin, p->dtype, p->cs_dtype, p->D, p->rotary_dim, p->seqlen_ro, p->cos_stride, p->sin_stride, p->interleaved);
  if (tb != TFA_OK) return tb;
  if (((uintptr_t)p->x | (uintptr_t)p->out | (uintptr_t)p->x2 | (uintptr_t)p->out2) & 15) return TFA_ERR_ALIGN;
  if (((uintptr_t)p->seqlen_offsets | (uintptr_t)p->cu_seqlens) & 3) return TFA_ERR_ALIGN;

  tfa::RotaryArgs a;
  memset(&a, 0, sizeof(a));
  a.t[0].x = p->x; a.t[0].out = p->out;
  a.t[0].xs_b = packed ? 0 : p->x_stride[0]; a.t[0].xs_h = p->x_stride[1]; a.t[0].xs_n = p->x_stride[2];
  a.t[0].os_b = packed ? 0 : p->o_stride[0]; a.t[0].os_h = p->o_stride[1]; a.t[0].os_n = p->o_stride[2];
  if (p->x2) {
    a.t[1].x = p->x2; a.t[1].out = p->out2;
    a.t[1].xs_b = packed ? 0 : p->x2_stride[0]; a.t[1].xs_h = p->x2_stride[1]; a.t[1].xs_n = p->x2_stride[2];
    a.t[1].os_b = packed ? 0 : p->o2_stride[0]; a.t[1].os_h = p->o2_stride[1]; a.t[1].os_n = p->o2_stride[2];
  }
  a.cos = p->cos; a.sin = p->sin;
  a.cos_stride = p->cos_stride; a.sin_stride = p->sin_stride;
  a.offsets = p->seqlen_offsets; a.offset = p->seqlen_offset;
  a.cu = p->cu_seqlens;
  a.B = p->B; a.N = p->N; a.H = p->H; a.H2 = p->H2;
  a.rows = packed ? (long long)p->N : (long long)p->B * p->N;
  a.rd8 = p->rotary_dim / 8;
  a.ipr = p->interleaved ? p->D / 8 : p->rotary_dim / 16 + (p->D - p->rotary_dim) / 8;
  // (checked products: B * N * (H + H2) * items leaves 64 bit for sizes near INT32_MAX — a grid of 2^31 blocks or more either way)
  if (__builtin_mul_overflow(a.rows, (long long)p->H + p->H2, &a.total) || __builtin_mul_overflow(a.total, (long long)a.ipr, &a.total)) return TFA_ERR_SHAPE;
  if (a.total > 0x7ffffffell * 256) return TFA_ERR_SHAPE;                     // the grid stays below 2^31 blocks
  a.seqlen_ro = p->seqlen_ro;
  a.interleaved = p->interleaved; a.conjugate = p->conjugate;
  a.bf16 = p->dtype == TFA_BF16 ? 1 : 0;
  a.cos_f32 = p->cs_dtype == TFA_F32 ? 1 : 0;
  return (int)tfa::launch_rotary(a, reinterpret_cast<hipStream_t>(stream), grid, block, dry);
}

// q8 != nullptr: the caches hold e4m3 bytes — their strides count bytes, D is a multiple of 16 (tfa_fwd_kvcache_fp8's rules: the attention kernels read these caches);
// rq != nullptr: q is rotated in place in the same launch.  Both nullptr: tfa_kvcache_append_varlen's launch.
int append_varlen_run(const tfa_kvcache_append_varlen_params* p, const tfa_kvcache_fp8* q8, const tfa_append_q* rq, void* stream, int* grid, int* block, bool dry) {
  if (!p) return TFA_ERR_NULL;
  if (q8) {
    if (q8->format != TFA_KV_E4M3) return TFA_ERR_DTYPE;
    if (q8->reserved_ != 0) return TFA_ERR_SHAPE;
    if (p->D < 16 || p->D > 128 || (p->D % 16) != 0) return TFA_ERR_HEAD_DIM;
    for (int i = 0; i < 2; ++i)
      if (q8->k_descale_stride[i] < 0 || q8->v_descale_stride[i] < 0) return TFA_ERR_STRIDE;
    if (((uintptr_t)q8->k_descale | (uintptr_t)q8->v_descale) & 3) return TFA_ERR_ALIGN;
  }
  if (rq && (!rq->q || !p->rotary_cos || !p->rotary_sin)) return TFA_ERR_NULL;
  if (!p->k || !p->v || !p->k_cache || !p->v_cache || !p->cu_seqlens || !p->cache_seqlens) return TFA_ERR_NULL;
  if ((p->rotary_cos == nullptr) != (p->rotary_sin == nullptr)) return TFA_ERR_NULL;
  if (p->dtype != TFA_F16 && p->dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (p->D < 8 || p->D > 128 || (p->D % 8) != 0) return TFA_ERR_HEAD_DIM;
  if (p->B <= 0 || p->total_new <= 0 || p->Hk <= 0 || p->capacity <= 0 || p->reserved_ != 0) return TFA_ERR_SHAPE;
  const bool paged = p->block_table != nullptr;
  if (paged) {
    if (p->page_size <= 0 || (p->page_size % 64) != 0 || (p->capacity % p->page_size) != 0 || p->num_pages <= 0) return TFA_ERR_SHAPE;
    if (p->block_table_stride < p->capacity / p->page_size) return TFA_ERR_STRIDE;
  }
  for (int i = 0; i < 2; ++i)
    if (bad_stride(p->k_stride[i]) || bad_stride(p->v_stride[i])) return TFA_ERR_STRIDE;
  for (int i = 0; i < 3; ++i) {
    if (q8 ? bad_stride8(p->kc_stride[i]) || bad_stride8(p->vc_stride[i]) : bad_stride(p->kc_stride[i]) || bad_stride(p->vc_stride[i])) return TFA_ERR_STRIDE;
  }
  if (p->k_stride[1] < p->D || p->v_stride[1] < p->D || p->kc_stride[2] < p->D || p->vc_stride[2] < p->D) return TFA_ERR_STRIDE;
  if (p->rotary_cos) {
    const int tb = check_tables(p->rotary_cos, p->rotary_sin, p->dtype, p->cs_dtype, p->D, p->rotary_dim, p->seqlen_ro, p->cos_stride, p->sin_stride,
                                p->rotary_interleaved);
    if (tb != TFA_OK) return tb;
  }
  if (((uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->k_cache | (uintptr_t)p->v_cache) & 15) return TFA_ERR_ALIGN;
  if (((uintptr_t)p->cu_seqlens | (uintptr_t)p->cache_seqlens | (uintptr_t)p->block_table) & 3) return TFA_ERR_ALIGN;
  if (rq) {
    if (rq->H <= 0 || rq->reserved_ != 0) return TFA_ERR_SHAPE;
    if (bad_stride(rq->q_stride[0]) || bad_stride(rq->q_stride[1]) || rq->q_stride[1] < p->D) return TFA_ERR_STRIDE;
    if ((uintptr_t)rq->q & 15) return TFA_ERR_ALIGN;
  }

  tfa::AppendVarlenExArgs a;
  memset(&a, 0, sizeof(a));
  a.k = p->k; a.v = p->v; a.k_cache = p->k_cache; a.v_cache = p->v_cache;
  a.cu = p->cu_seqlens; a.seqlens = p->cache_seqlens; a.block_table = p->block_table;
  a.bt_stride = p->block_table_stride;
  a.ks_b = p->kc_stride[0]; a.ks_h = p->kc_stride[1]; a.ks_n = p->kc_stride[2];
  a.vs_b = p->vc_stride[0]; a.vs_h = p->vc_stride[1]; a.vs_n = p->vc_stride[2];
  a.kn_h = p->k_stride[0]; a.kn_n = p->k_stride[1];
  a.vn_h = p->v_stride[0]; a.vn_n = p->v_stride[1];
  a.B = p->B; a.Hk = p->Hk; a.cpr = p->D / 8;
  if (__builtin_mul_overflow((long long)p->total_new * p->Hk, (long long)a.cpr, &a.total) || a.total > 0x7ffffffell * 256) return TFA_ERR_SHAPE;   // (2^31 blocks or more)
  a.capacity = p->capacity;
  a.page_size = paged ? p->page_size : 1;
  a.num_pages = paged ? p->num_pages : 1;
  if (p->rotary_cos) {
    a.cos = p->rotary_cos; a.sin = p->rotary_sin;
    a.cos_stride = p->cos_stride; a.sin_stride = p->sin_stride;
    a.rd8 = p->rotary_dim / 8;
    a.seqlen_ro = p->seqlen_ro;
    a.interleaved = p->rotary_interleaved;
    a.cos_f32 = p->cs_dtype == TFA_F32 ? 1 : 0;
  }
  a.bf16 = p->dtype == TFA_BF16 ? 1 : 0;
  if ((a.total + 255) / 256 >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  if (!q8 && !rq) return (int)tfa::launch_kvcache_append_varlen(a, reinterpret_cast<hipStream_t>(stream), grid, block, dry);
  if (q8) {
    a.fp8 = 1;
    a.k_descale = q8->k_descale; a.v_descale = q8->v_descale;
    a.kd_b = q8->k_descale_stride[0]; a.kd_h = q8->k_descale_stride[1];
    a.vd_b = q8->v_descale_stride[0]; a.vd_h = q8->v_descale_stride[1];
  }
  if (rq) {
    a.q = rq->q; a.H = rq->H;
    a.q_h = rq->q_stride[0]; a.q_n = rq->q_stride[1];
    a.q_ipr = p->rotary_interleaved ? a.rd8 : a.rd8 / 2;
    if (__builtin_mul_overflow((long long)p->total_new * rq->H, (long long)a.q_ipr, &a.q_total) || a.q_total > 0x7ffffffell * 256) return TFA_ERR_SHAPE;
  }
  if ((a.total + a.q_total + 255) / 256 >= (long long)0x7fffffff) return TFA_ERR_SHAPE;
  return (int)tfa::launch_kvcache_append_varlen_ex(a, reinterpret_cast<hipStream_t>(stream), grid, block, dry);
}

}  // namespace

extern "C" {

int tfa_rotary(const tfa_rotary_params* p, void* stream) { return rotary_run(p, stream, nullptr, nullptr, false); }
int tfa_rotary_plan(const tfa_rotary_params* p, int* grid, int* block) { return rotary_run(p, nullptr, grid, block, true); }

int tfa_kvcache_append_varlen(const tfa_kvcache_append_varlen_params* p, void* stream) { return append_varlen_run(p, nullptr, nullptr, stream, nullptr, nullptr, false); }
int tfa_kvcache_append_varlen_plan(const tfa_kvcache_append_varlen_params* p, int* grid, int* block) {
  return append_varlen_run(p, nullptr, nullptr, nullptr, grid, block, true);
}

int tfa_kvcache_append_varlen_ex(const tfa_kvcache_append_varlen_params* p, const tfa_kvcache_fp8* q8, const tfa_append_q* rq, void* stream) {
  return append_varlen_run(p, q8, rq, stream, nullptr, nullptr, false);
}
int tfa_kvcache_append_varlen_ex_plan(const tfa_kvcache_append_varlen_params* p, const tfa_kvcache_fp8* q8, const tfa_append_q* rq, int* grid, int* block) {
  return append_varlen_run(p, q8, rq, nullptr, grid, block, true);
}

}  // extern "C"
