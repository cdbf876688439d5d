// tfa_kvcache_append_fp8.hip — in-place append of this step's keys and values to an e4m3 K/V cache (include/tfa.h: tfa_kvcache_append_fp8; the first launch of
// tfa_fwd_kvcache_fp8 when k_new / v_new are given).  tfa_kvcache_append.hip with a quantisation in the middle: every thread reads one 16-byte chunk (8 elements) of one new K
// row and of the V row, divides by the (sequence, K/V head)'s descale in fp32 (a true division: no fast-math in this build), clamps into the finite e4m3 range — the
// conversion does not saturate: without the clamp everything above 448 would become NaN — converts with round-to-nearest-even and stores 8 bytes.  A NaN stays NaN.
// (tfa_quantise8.h: the arithmetic, shared with the packed append.)
// Positions, capacity and page checks are the 16-bit append's: nothing is ever stored outside the cache tensors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_kvcache.h"
#include "tfa_quantise8.h"

namespace tfa {

template <typename T>
__global__ __launch_bounds__(256) void kvcache_append_fp8_kernel(const Append8Args a) {
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
  koff += (long long)hk * a.ks_h + c * 8;                     // (cache strides: bytes)
  voff += (long long)hk * a.vs_h + c * 8;
  const long long kn = (long long)b * a.kn_b + (long long)t * a.kn_n + (long long)hk * a.kn_h + c * 8;
  const long long vn = (long long)b * a.vn_b + (long long)t * a.vn_n + (long long)hk * a.vn_h + c * 8;
  const float kd = a.k_descale ? a.k_descale[(long long)b * a.kd_b + (long long)hk * a.kd_h] : 1.f;
  const float vd = a.v_descale ? a.v_descale[(long long)b * a.vd_b + (long long)hk * a.vd_h] : 1.f;
  quantise8<T>(a.k_new, kn, kd, a.k_cache, koff);
  quantise8<T>(a.v_new, vn, vd, a.v_cache, voff);
}

hipError_t launch_kvcache_append_fp8(const Append8Args& a, hipStream_t stream) {
  const long long blocks = (a.total + 255) / 256;
  if (blocks <= 0 || blocks >= (long long)0x7fffffff) return hipErrorInvalidValue;
  (void)hipGetLastError();
  if (a.bf16) hipLaunchKernelGGL(kvcache_append_fp8_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(kvcache_append_fp8_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace tfa
