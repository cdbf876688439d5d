// tfa_kvcache_append_varlen.hip — a unified batch's new K/V rows into a paged or contiguous cache (include/tfa.h: tfa_kvcache_append_varlen).  k / v are packed
// (total_new, Hk, D); sequence b owns rows [cu_seqlens[b], cu_seqlens[b+1]) and its row t goes to key position cache_seqlens[b] + t, through the block table when
// the cache is paged.  One thread per (row, K/V head, 16-byte chunk): one K store and one V store.  The row's sequence is found by a binary search of cu_seqlens on
// the device (tfa_rotary.h: rot_find_sequence — verified, so a broken cu_seqlens drops rows, never misplaces them outside the checks below); the drop rules are
// tfa_kvcache_append's: a position below 0 or at / beyond the capacity, a block-table entry that is not a page of the cache.  Nothing is stored outside the caches.
// With cos / sin, K is rotated at its key position on the way in by tfa_rotary.h's device functions — the bits tfa_rotary leaves: a thread of the rotated part also
// loads the partner chunk (GPT-NeoX layout; the thread that owns it sits rotary_dim / 16 lanes away, so the second load hits the cache), computes the pair and
// keeps its half.  V is copied.  k / v and the caches must not overlap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_rotary.h"

namespace tfa {

// ROT: 0 = plain copy, 1 = GPT-NeoX halves, 2 = GPT-J interleaved
template <typename T, bool CF32, int ROT>
__global__ __launch_bounds__(256) void kvcache_append_varlen_kernel(const AppendVarlenArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) return;
  // gid = (row * Hk + hk) * cpr + c
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
  koff += (long long)hk * a.ks_h + c * 8;
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
  *reinterpret_cast<rot_u32x4*>(reinterpret_cast<unsigned short*>(a.k_cache) + koff) = kx;
  *reinterpret_cast<rot_u32x4*>(reinterpret_cast<unsigned short*>(a.v_cache) + voff) = vx;
}

template <typename T, bool CF32>
static void launch_rot(const AppendVarlenArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.interleaved) hipLaunchKernelGGL((kvcache_append_varlen_kernel<T, CF32, 2>), dim3(blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((kvcache_append_varlen_kernel<T, CF32, 1>), dim3(blocks), dim3(256), 0, stream, a);
}

hipError_t launch_kvcache_append_varlen(const AppendVarlenArgs& a, hipStream_t stream, int* grid, int* block, bool dry) {
  const long long blocks = (a.total + 255) / 256;
  if (blocks <= 0 || blocks >= (long long)0x7fffffff) return hipErrorInvalidValue;
  if (grid) *grid = (int)blocks;
  if (block) *block = 256;
  if (dry) return hipSuccess;
  (void)hipGetLastError();
  if (!a.cos) {
    hipLaunchKernelGGL((kvcache_append_varlen_kernel<__bf16, false, 0>), dim3((unsigned)blocks), dim3(256), 0, stream, a);   // a copy: the element type does not matter
  } else if (a.bf16) {
    if (a.cos_f32) launch_rot<__bf16, true>(a, (unsigned)blocks, stream);
    else launch_rot<__bf16, false>(a, (unsigned)blocks, stream);
  } else {
    if (a.cos_f32) launch_rot<_Float16, true>(a, (unsigned)blocks, stream);
    else launch_rot<_Float16, false>(a, (unsigned)blocks, stream);
  }
  return hipGetLastError();
}

}  // namespace tfa
