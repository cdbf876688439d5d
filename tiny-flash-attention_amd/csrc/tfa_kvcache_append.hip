// tfa_kvcache_append.hip — in-place append of this step's keys and values to a K/V cache (include/tfa.h: tfa_kvcache_append; the
// first launch of tfa_fwd_kvcache when k_new / v_new are given).  A pure copy: every thread moves one 16-byte chunk of one new K row and
// the same chunk of the V row to key position cache_seqlens[b] + t of sequence b, through the block table when the cache is paged.
// The position is read on the device (the host never reads cache_seqlens) and checked against the capacity; a paged row whose block-table
// entry is not a page of the cache is dropped too: nothing is ever stored outside the cache tensors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_kvcache.h"

namespace tfa {

__global__ __launch_bounds__(256) void kvcache_append_kernel(const AppendArgs a) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) return;
  // gid = ((b * n_new + t) * Hk + hk) * cpr + c
  const int c = (int)(gid % a.cpr);
  long long r = gid / a.cpr;
  const int hk = (int)(r % a.Hk);
  r /= a.Hk;
  const int t = (int)(r % a.n_new);
  const int b = (int)(r / a.n_new);
  const long long pos = (long long)a.seqlens[b] + t;
  if (pos < 0 || pos >= a.capacity) return;                   // at or beyond the capacity: not written (and not attended: the length is clamped)
  long long koff, voff;
  if (a.block_table) {
    const int pidx = (int)(pos / a.page_size);
    const int page = a.block_table[(long long)b * a.bt_stride + pidx];
    if (page < 0 || page >= a.num_pages) return;              // not a page of this cache
    const long long row = pos - (long long)pidx * a.page_size;
    koff = (long long)page * a.ks_b + row * a.ks_n;
    voff = (long long)page * a.vs_b + row * a.vs_n;
  } else {
    koff = (long long)b * a.ks_b + pos * a.ks_n;
    voff = (long long)b * a.vs_b + pos * a.vs_n;
  }
  koff += (long long)hk * a.ks_h + c * 8;
  voff += (long long)hk * a.vs_h + c * 8;
  const long long kn = (long long)b * a.kn_b + (long long)t * a.kn_n + (long long)hk * a.kn_h + c * 8;
  const long long vn = (long long)b * a.vn_b + (long long)t * a.vn_n + (long long)hk * a.vn_h + c * 8;
  const u32x4 kx = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(a.k_new) + kn);
  const u32x4 vx = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(a.v_new) + vn);
  *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(a.k_cache) + koff) = kx;
  *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(a.v_cache) + voff) = vx;
}

hipError_t launch_kvcache_append(const AppendArgs& a, hipStream_t stream) {
  const long long blocks = (a.total + 255) / 256;
  if (blocks <= 0 || blocks >= (long long)0x7fffffff) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(kvcache_append_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace tfa
