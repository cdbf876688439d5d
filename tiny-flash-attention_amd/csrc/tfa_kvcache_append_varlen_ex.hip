// tfa_kvcache_append_varlen_ex.hip — the packed append (tfa_kvcache_append_varlen.hip) with a quantisation behind it and / or the step's q rotated in the same
// launch (include/tfa.h: tfa_kvcache_append_varlen_ex).  The first `total` threads are the append's: one per (row, K/V head, 16-byte chunk of the 16-bit source),
// the same search of cu_seqlens, the same position, page lookup and drop rules.  FP8: the chunk — K's after its rotation and its one rounding to the 16-bit type,
// the bits tfa_rotary leaves — is divided by the (sequence, K/V head)'s descale, clamped and converted by tfa_quantise8.h's function (tfa_kvcache_append_fp8's
// bytes) and stored as 8 bytes; the lanes of a row store neighbouring 8-byte pieces.  The K side keeps the "load the partner chunk, keep my half" form: its source
// and destination differ.  The q_total threads behind them rotate q IN PLACE at K's positions, cache_seqlens[b] + t: there one thread owns a whole pair of chunks
// (GPT-NeoX) or one chunk of four pairs (GPT-J) — tfa_rotary.hip's form, the thread that stores a chunk loaded it, so there is nothing to order — and only the
// rotated part has threads: elements behind rotary_dim, rows outside every sequence and rows whose position lies outside [0, seqlen_ro) are never touched.
// q has no capacity: a row whose K is dropped still has its q rotated.  q must not overlap k, v or the caches.  No LDS; ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_quantise8.h"
#include "tfa_rotary.h"

namespace tfa {

// ROT: 0 = no tables, 1 = GPT-NeoX halves, 2 = GPT-J interleaved
template <typename T, bool CF32, int ROT, bool FP8>
__global__ __launch_bounds__(256) void kvcache_append_varlen_ex_kernel(const AppendVarlenExArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) {
    if constexpr (ROT != 0) {
      // ---- q: qid = (row * H + h) * q_ipr + item
      const long long qid = gid - a.total;
      if (qid >= a.q_total) return;
      const int item = (int)(qid % a.q_ipr);
      const long long r = qid / a.q_ipr;
      const int h = (int)(r % a.H);
      const long long row = r / a.H;
      const int b = rot_find_sequence(a.cu, a.B, row);
      if (b < 0) return;                                        // a row outside every sequence: untouched
      const long long pos = (long long)a.seqlens[b] + (row - (long long)a.cu[b]);
      if (pos < 0 || pos >= a.seqlen_ro) return;                // no table row: untouched
      unsigned short* qp = reinterpret_cast<unsigned short*>(a.q) + row * a.q_n + (long long)h * a.q_h;
      const void* cosr = (const char*)a.cos + pos * a.cos_stride * (CF32 ? 4 : 2);
      const void* sinr = (const char*)a.sin + pos * a.sin_stride * (CF32 ? 4 : 2);
      if constexpr (ROT == 2) {
        const rot_u32x4 xa = *reinterpret_cast<const rot_u32x4*>(qp + item * 8);
        rot_u32x4 oa;
        rotary_chunk_interleaved<T, CF32>(xa, cosr, sinr, item * 4, 1.f, oa);
        *reinterpret_cast<rot_u32x4*>(qp + item * 8) = oa;
      } else {
        const int half = a.rd8 * 4;                             // rotary_dim / 2 elements
        const rot_u32x4 xa = *reinterpret_cast<const rot_u32x4*>(qp + item * 8);
        const rot_u32x4 xb = *reinterpret_cast<const rot_u32x4*>(qp + half + item * 8);
        rot_u32x4 oa, ob;
        rotary_chunks_halves<T, CF32>(xa, xb, cosr, sinr, item * 8, 1.f, oa, ob);
        *reinterpret_cast<rot_u32x4*>(qp + item * 8) = oa;
        *reinterpret_cast<rot_u32x4*>(qp + half + item * 8) = ob;
      }
    }
    return;
  }
  // ---- K / V: gid = (row * Hk + hk) * cpr + c
  const int c = (int)(gid % a.cpr);
  long long r = gid / a.cpr;
  const int hk = (int)(r % a.Hk);
  const long long row = r / a.Hk;
  const int b = rot_find_sequence(a.cu, a.B, row);
  if (b < 0) return;                                          // a row outside every sequence
  const long long pos = (long long)a.seqlens[b] + (row - (long long)a.cu[b]);
  if (pos < 0 || pos >= a.capacity) return;                   // at or beyond the capacity: not written
  long long koff, voff;
  if (a.block_table) {
    const int pidx = (int)(pos / a.page_size);
    const int page = a.block_table[(long long)b * a.bt_stride + pidx];
    if (page < 0 || page >= a.num_pages) return;              // not a page of this cache
    const long long prow = pos - (long long)pidx * a.page_size;
    koff = (long long)page * a.ks_b + prow * a.ks_n;
    voff = (long long)page * a.vs_b + prow * a.vs_n;
  } else {
    koff = (long long)b * a.ks_b + pos * a.ks_n;
    voff = (long long)b * a.vs_b + pos * a.vs_n;
  }
  koff += (long long)hk * a.ks_h + c * 8;                     // cache strides and offsets: elements of the cache (FP8: bytes)
  voff += (long long)hk * a.vs_h + c * 8;
  const unsigned short* kp = reinterpret_cast<const unsigned short*>(a.k) + row * a.kn_n + (long long)hk * a.kn_h;
  const unsigned short* vp = reinterpret_cast<const unsigned short*>(a.v) + row * a.vn_n + (long long)hk * a.vn_h;
  rot_u32x4 kx = *reinterpret_cast<const rot_u32x4*>(kp + c * 8);
  const rot_u32x4 vx = *reinterpret_cast<const rot_u32x4*>(vp + c * 8);
  if constexpr (ROT != 0) {
    if (c < a.rd8 && pos < a.seqlen_ro) {                     // (pos >= 0 holds); a position behind the tables is stored unrotated, as tfa_rotary leaves it
      const void* cosr = (const char*)a.cos + pos * a.cos_stride * (CF32 ? 4 : 2);
      const void* sinr = (const char*)a.sin + pos * a.sin_stride * (CF32 ? 4 : 2);
      if constexpr (ROT == 2) {
        rot_u32x4 o;
        rotary_chunk_interleaved<T, CF32>(kx, cosr, sinr, c * 4, 1.f, o);
        kx = o;
      } else {
        const int hc = a.rd8 / 2;                             // chunks per half
        const bool first = c < hc;
        const int j = first ? c : c - hc;
        const rot_u32x4 partner = *reinterpret_cast<const rot_u32x4*>(kp + (first ? c + hc : j) * 8);
        rot_u32x4 oa, ob;
        rotary_chunks_halves<T, CF32>(first ? kx : partner, first ? partner : kx, cosr, sinr, j * 8, 1.f, oa, ob);
        kx = first ? oa : ob;
      }
    }
  }
  if constexpr (FP8) {
    typedef typename q8_vec<T>::type t8;
    const float kd = a.k_descale ? a.k_descale[(long long)b * a.kd_b + (long long)hk * a.kd_h] : 1.f;
    const float vd = a.v_descale ? a.v_descale[(long long)b * a.vd_b + (long long)hk * a.vd_h] : 1.f;
    *reinterpret_cast<q8_u32x2*>(reinterpret_cast<unsigned char*>(a.k_cache) + koff) = quantise8_bytes<T>(__builtin_bit_cast(t8, kx), kd);
    *reinterpret_cast<q8_u32x2*>(reinterpret_cast<unsigned char*>(a.v_cache) + voff) = quantise8_bytes<T>(__builtin_bit_cast(t8, vx), vd);
  } else {
    *reinterpret_cast<rot_u32x4*>(reinterpret_cast<unsigned short*>(a.k_cache) + koff) = kx;
    *reinterpret_cast<rot_u32x4*>(reinterpret_cast<unsigned short*>(a.v_cache) + voff) = vx;
  }
}

template <typename T, bool CF32, bool FP8>
static void launch_rot(const AppendVarlenExArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.interleaved) hipLaunchKernelGGL((kvcache_append_varlen_ex_kernel<T, CF32, 2, FP8>), dim3(blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((kvcache_append_varlen_ex_kernel<T, CF32, 1, FP8>), dim3(blocks), dim3(256), 0, stream, a);
}

template <typename T>
static void launch_t(const AppendVarlenExArgs& a, unsigned blocks, hipStream_t stream) {
  if (!a.cos) {                                               // no tables: no q either; without fp8 the plain launch serves (the caller's branch)
    hipLaunchKernelGGL((kvcache_append_varlen_ex_kernel<T, false, 0, true>), dim3(blocks), dim3(256), 0, stream, a);
  } else if (a.fp8) {
    if (a.cos_f32) launch_rot<T, true, true>(a, blocks, stream);
    else launch_rot<T, false, true>(a, blocks, stream);
  } else {
    if (a.cos_f32) launch_rot<T, true, false>(a, blocks, stream);
    else launch_rot<T, false, false>(a, blocks, stream);
  }
}

hipError_t launch_kvcache_append_varlen_ex(const AppendVarlenExArgs& a, hipStream_t stream, int* grid, int* block, bool dry) {
  if (!a.fp8 && !a.q) return launch_kvcache_append_varlen(a, stream, grid, block, dry);
  if (a.q && !a.cos) return hipErrorInvalidValue;
  const long long blocks = (a.total + a.q_total + 255) / 256;
  if (blocks <= 0 || blocks >= (long long)0x7fffffff) return hipErrorInvalidValue;
  if (grid) *grid = (int)blocks;
  if (block) *block = 256;
  if (dry) return hipSuccess;
  (void)hipGetLastError();
  if (a.bf16) launch_t<__bf16>(a, (unsigned)blocks, stream);
  else launch_t<_Float16>(a, (unsigned)blocks, stream);
  return hipGetLastError();
}

}  // namespace tfa
