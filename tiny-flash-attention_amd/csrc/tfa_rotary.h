// tfa_rotary.h — rotary position embedding (include/tfa.h: tfa_rotary, tfa_kvcache_append_varlen, tfa_kvcache_append_varlen_ex): the pair arithmetic, ONCE, as device
// functions all kernels call (tfa_rotary.hip rotates a tensor; tfa_kvcache_append_varlen.hip and tfa_kvcache_append_varlen_ex.hip rotate K on its way into the cache,
// the latter q in place too, and must leave the same bits), the search that finds a packed row's sequence, and the launchers' arguments.
//   o1 = x1 * cos - x2 * sin,  o2 = x1 * sin + x2 * cos  in fp32, each output rounded once to the 16-bit type.
// The products and sums are spelled as one fp32 multiply and one fused multiply-add per output (no contraction left to the compiler), so the bits do not
// depend on the unit the function is inlined into; an fma rounds once where a product and a sum round twice: inside the stated bound, never outside.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfa {

typedef __attribute__((ext_vector_type(4))) unsigned rot_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned rot_u32x2;
typedef __attribute__((ext_vector_type(4))) float rot_f32x4;

// ---- the pair -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rotary_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
  o1 = __fmaf_rn(x1, c, -__fmul_rn(x2, s));
  o2 = __fmaf_rn(x1, s, __fmul_rn(x2, c));
}

// 16-bit element <-> fp32 (T = __bf16 or _Float16); the conversion back is the one rounding (to nearest even)
template <typename T>
__device__ __forceinline__ float rot_to_f32(unsigned short bits) {
  return (float)__builtin_bit_cast(T, bits);
}
template <typename T>
__device__ __forceinline__ unsigned short rot_from_f32(float f) {
  return __builtin_bit_cast(unsigned short, (T)f);
}
template <typename T>
__device__ __forceinline__ float rot_elem(const rot_u32x4& v, int i) {
  const unsigned w = v[i >> 1];
  return rot_to_f32<T>((unsigned short)((i & 1) ? (w >> 16) : (w & 0xffffu)));
}
template <typename T>
__device__ __forceinline__ void rot_set(rot_u32x4& v, int i, float lo, float hi) {   // elements 2i, 2i + 1
  v[i] = (unsigned)rot_from_f32<T>(lo) | ((unsigned)rot_from_f32<T>(hi) << 16);
}

// n (4 or 8) consecutive table values from `row` + first (elements), as fp32; tables are T or fp32 (CF32); 16-byte loads (8 bytes: four 16-bit values)
template <typename T, bool CF32, int n>
__device__ __forceinline__ void rot_table(const void* table, long long off, float* f) {
  if constexpr (CF32) {
    const float* p = reinterpret_cast<const float*>(table) + off;
#pragma unroll
    for (int q = 0; q < n / 4; ++q) {
      const rot_f32x4 w = *reinterpret_cast<const rot_f32x4*>(p + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * q + i] = w[i];
    }
  } else {
    const unsigned short* p = reinterpret_cast<const unsigned short*>(table) + off;
    if constexpr (n == 8) {
      const rot_u32x4 w = *reinterpret_cast<const rot_u32x4*>(p);
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = rot_elem<T>(w, i);
    } else {
      const rot_u32x2 w2 = *reinterpret_cast<const rot_u32x2*>(p);
      const rot_u32x4 w = {w2[0], w2[1], 0u, 0u};
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = rot_elem<T>(w, i);
    }
  }
}

// GPT-NeoX layout: chunk `a` holds x[8j .. 8j+8), chunk `b` holds x[rd/2 + 8j .. rd/2 + 8j + 8); cos / sin values 8j .. 8j+8 of the position's row.
// sign = -1 for the conjugate rotation (the backward).
template <typename T, bool CF32>
__device__ __forceinline__ void rotary_chunks_halves(const rot_u32x4& a, const rot_u32x4& b, const void* cos, const void* sin, long long toff, float sign,
                                                     rot_u32x4& oa, rot_u32x4& ob) {
  float c[8], s[8];
  rot_table<T, CF32, 8>(cos, toff, c);
  rot_table<T, CF32, 8>(sin, toff, s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float o1l, o2l, o1h, o2h;
    rotary_pair(rot_elem<T>(a, 2 * i), rot_elem<T>(b, 2 * i), c[2 * i], sign * s[2 * i], o1l, o2l);
    rotary_pair(rot_elem<T>(a, 2 * i + 1), rot_elem<T>(b, 2 * i + 1), c[2 * i + 1], sign * s[2 * i + 1], o1h, o2h);
    rot_set<T>(oa, i, o1l, o1h);
    rot_set<T>(ob, i, o2l, o2h);
  }
}

// GPT-J layout: chunk `a` holds x[8c .. 8c+8) = the pairs 4c .. 4c+4; cos / sin values 4c .. 4c+4 of the position's row
template <typename T, bool CF32>
__device__ __forceinline__ void rotary_chunk_interleaved(const rot_u32x4& a, const void* cos, const void* sin, long long toff, float sign, rot_u32x4& oa) {
  float c[4], s[4];
  rot_table<T, CF32, 4>(cos, toff, c);
  rot_table<T, CF32, 4>(sin, toff, s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float o1, o2;
    rotary_pair(rot_elem<T>(a, 2 * i), rot_elem<T>(a, 2 * i + 1), c[i], sign * s[i], o1, o2);
    rot_set<T>(oa, i, o1, o2);
  }
}

// The sequence that owns packed row `row`: b with cu[b] <= row < cu[b+1], or -1 (a row outside every sequence, or a cu_seqlens that is not monotonic —
// the answer is verified, never trusted).  Reads cu[0 .. B] only.
__device__ __forceinline__ int rot_find_sequence(const int* cu, int B, long long row) {
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)cu[mid + 1] <= row) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= B) return -1;
  return ((long long)cu[lo] <= row && row < (long long)cu[lo + 1]) ? lo : -1;
}

// ---- tfa_rotary.hip (strides in ELEMENTS; 16-bit elements, 16-byte chunks) --------------------------------------------------------------------
struct RotaryTensor {
  const void* x;
  void* out;
  long long xs_b, xs_h, xs_n;   // batch (0 in the packed form), head, row
  long long os_b, os_h, os_n;
};
struct RotaryArgs {
  RotaryTensor t[2];            // t[1]: the optional second tensor (its heads follow the first's in a row's work items)
  const void* cos;
  const void* sin;
  long long cos_stride, sin_stride;
  const int* offsets;           // device, B entries, or nullptr: `offset`
  const int* cu;                // device, B + 1 entries, or nullptr: (B, N, H, D)
  long long total;              // threads with work: rows * (H + H2) * ipr
  long long rows;               // B * N, or the packed row count
  int offset;
  int B, N, H, H2;
  int rd8;                      // rotary_dim / 8: chunks of the rotated part
  int ipr;                      // work items per (row, head): halves: rd8 / 2 pairs of chunks + the copied chunks; interleaved: D / 8 chunks
  int seqlen_ro;
  int interleaved, conjugate;
  int bf16, cos_f32;
};
hipError_t launch_rotary(const RotaryArgs& a, hipStream_t stream, int* grid, int* block, bool dry);

// ---- tfa_kvcache_append_varlen.hip ------------------------------------------------------------------------------------------------------------
struct AppendVarlenArgs {
  const void* k;                // (total_new, Hk, D) by kn_* / vn_*
  const void* v;
  void* k_cache;
  void* v_cache;
  const int* cu;                // device, B + 1 entries
  const int* seqlens;           // device, B entries
  const int* block_table;       // device (B, max_blocks) by bt_stride, or nullptr: contiguous cache
  const void* cos;              // both or neither: K is rotated at its key position
  const void* sin;
  long long cos_stride, sin_stride;
  long long bt_stride;
  long long ks_b, ks_h, ks_n;   // cache strides: batch (contiguous) or page (paged), head, row
  long long vs_b, vs_h, vs_n;
  long long kn_h, kn_n, vn_h, vn_n;
  long long total;              // threads with work: total_new * Hk * cpr
  int B, Hk, cpr;               // cpr = D / 8
  int capacity, page_size, num_pages;
  int rd8, seqlen_ro;
  int interleaved, bf16, cos_f32;
};
hipError_t launch_kvcache_append_varlen(const AppendVarlenArgs& a, hipStream_t stream, int* grid, int* block, bool dry);

// ---- tfa_kvcache_append_varlen_ex.hip: the same append into an e4m3 cache (cache strides then count bytes) and / or with q rotated in place in the launch -------
struct AppendVarlenExArgs : AppendVarlenArgs {
  const float* k_descale;       // fp8: device fp32 by (kd_b, kd_h) elements, or nullptr = 1.0
  const float* v_descale;
  long long kd_b, kd_h, vd_b, vd_h;
  void* q;                      // (total_new, H, D) by q_h / q_n (elements), rotated in place at K's positions, or nullptr
  long long q_h, q_n;
  long long q_total;            // threads with q work behind the `total` K/V ones: total_new * H * q_ipr (0 without q)
  int H, q_ipr;                 // q_ipr: work items per (row, head) — the rotated part only: rd8 / 2 pairs of chunks (halves) or rd8 chunks (interleaved)
  int fp8;                      // 1: the caches hold e4m3 bytes
};
hipError_t launch_kvcache_append_varlen_ex(const AppendVarlenExArgs& a, hipStream_t stream, int* grid, int* block, bool dry);

}  // namespace tfa
