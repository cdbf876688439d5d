// tfa_quantise8.h — the e4m3 quantisation of the K/V-cache appends (include/tfa.h: tfa_kvcache_append_fp8, tfa_kvcache_append_varlen_ex), ONCE, as device
// functions both kernels call, so the 4-D and the packed append leave the same bytes:
//   byte = rne_e4m3fn(clamp(float(x) / descale, -448, 448)),  NaN stays NaN.
// The division is a true fp32 division (no fast-math in this build); the clamp sits in front of the conversion because the conversion does not saturate —
// without it everything above 448 would become NaN.  Eight 16-bit elements (one 16-byte chunk) become eight bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfa {

typedef __attribute__((ext_vector_type(2))) unsigned q8_u32x2;
template <typename T>
struct q8_vec {
  typedef __attribute__((ext_vector_type(8))) T type;
};

// eight elements in registers -> eight e4m3 bytes
template <typename T>
__device__ __forceinline__ q8_u32x2 quantise8_bytes(const typename q8_vec<T>::type x, float d) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float q = (float)x[i] / d;
    y[i] = q != q ? q : fminf(fmaxf(q, -448.f), 448.f);
  }
  q8_u32x2 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h + 0], y[4 * h + 1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h + 2], y[4 * h + 3], w, true);
    r[h] = (unsigned)w;
  }
  return r;
}

// src + off (elements of T, a 16-byte aligned chunk) -> dst + doff (bytes, 8-byte aligned)
template <typename T>
__device__ __forceinline__ void quantise8(const void* src, long long off, float d, void* dst, long long doff) {
  typedef typename q8_vec<T>::type t8;
  const t8 x = *reinterpret_cast<const t8*>(reinterpret_cast<const T*>(src) + off);
  *reinterpret_cast<q8_u32x2*>(reinterpret_cast<unsigned char*>(dst) + doff) = quantise8_bytes<T>(x, d);
}

}  // namespace tfa
