// tfa_rotary.hip — rotary position embedding of one tensor, or of q and k in one launch (include/tfa.h: tfa_rotary).  Memory-bound: every lane moves 16-byte
// chunks — in the GPT-NeoX layout chunk j of the first half and chunk j of the second half of the rotated part (two loads, two stores), in the GPT-J layout one chunk
// of four pairs (one load, one store), a chunk behind rotary_dim is copied (skipped in place).  Work items are numbered (row, head, item), so the lanes of a wave cover
// the chunks and heads of one row before the next row and the row's cos / sin values are read once from memory and then from cache.  The position of a row is formed
// on the device: seqlen_offsets[b] + t, with b found by a binary search of cu_seqlens in the packed form; a row without a valid position is copied bit for bit.
// The thread that stores a chunk is the thread that loaded it: in place there is nothing to order.  No LDS, no trigonometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_rotary.h"

namespace tfa {

template <typename T, bool CF32, bool IL>
__global__ __launch_bounds__(256) void rotary_kernel(const RotaryArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) return;
  // gid = (row * (H + H2) + h) * ipr + item
  const int item = (int)(gid % a.ipr);
  long long r = gid / a.ipr;
  const int heads = a.H + a.H2;
  int h = (int)(r % heads);
  const long long row = r / heads;
  const int which = h >= a.H ? 1 : 0;
  if (which) h -= a.H;
  const RotaryTensor& t = a.t[which];

  // the row's sequence, its index inside it, its position
  int b;
  long long tt, xrow;
  if (a.cu) {
    b = rot_find_sequence(a.cu, a.B, row);
    tt = b >= 0 ? row - (long long)a.cu[b] : 0;
    xrow = row;                                             // packed: rows by the row stride alone (xs_b = 0)
  } else {
    b = (int)(row / a.N);
    tt = row - (long long)b * a.N;
    xrow = tt;
  }
  const int bb = a.cu ? 0 : b;
  const unsigned short* xp = reinterpret_cast<const unsigned short*>(t.x) + (long long)bb * t.xs_b + xrow * t.xs_n + (long long)h * t.xs_h;
  unsigned short* op = reinterpret_cast<unsigned short*>(t.out) + (long long)bb * t.os_b + xrow * t.os_n + (long long)h * t.os_h;
  long long pos = -1;
  if (b >= 0) pos = (long long)(a.offsets ? a.offsets[b] : a.offset) + tt;
  const bool rotate = b >= 0 && pos >= 0 && pos < a.seqlen_ro;
  const float sign = a.conjugate ? -1.f : 1.f;

  const int nrot = IL ? a.rd8 : a.rd8 / 2;                  // items of the rotated part
  if (item >= nrot) {                                       // a chunk behind rotary_dim
    if (t.x == t.out) return;
    const int c = a.rd8 + (item - nrot);
    *reinterpret_cast<rot_u32x4*>(op + c * 8) = *reinterpret_cast<const rot_u32x4*>(xp + c * 8);
    return;
  }
  if constexpr (IL) {
    const rot_u32x4 xa = *reinterpret_cast<const rot_u32x4*>(xp + item * 8);
    rot_u32x4 oa = xa;
    if (rotate) rotary_chunk_interleaved<T, CF32>(xa, (const char*)a.cos + pos * a.cos_stride * (CF32 ? 4 : 2), (const char*)a.sin + pos * a.sin_stride * (CF32 ? 4 : 2),
                                                  item * 4, sign, oa);
    else if (t.x == t.out) return;
    *reinterpret_cast<rot_u32x4*>(op + item * 8) = oa;
  } else {
    const int half = a.rd8 * 4;                             // rotary_dim / 2 elements
    const rot_u32x4 xa = *reinterpret_cast<const rot_u32x4*>(xp + item * 8);
    const rot_u32x4 xb = *reinterpret_cast<const rot_u32x4*>(xp + half + item * 8);
    rot_u32x4 oa = xa, ob = xb;
    if (rotate) rotary_chunks_halves<T, CF32>(xa, xb, (const char*)a.cos + pos * a.cos_stride * (CF32 ? 4 : 2), (const char*)a.sin + pos * a.sin_stride * (CF32 ? 4 : 2),
                                              item * 8, sign, oa, ob);
    else if (t.x == t.out) return;
    *reinterpret_cast<rot_u32x4*>(op + item * 8) = oa;
    *reinterpret_cast<rot_u32x4*>(op + half + item * 8) = ob;
  }
}

template <typename T, bool CF32>
static void launch_il(const RotaryArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.interleaved) hipLaunchKernelGGL((rotary_kernel<T, CF32, true>), dim3(blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((rotary_kernel<T, CF32, false>), dim3(blocks), dim3(256), 0, stream, a);
}

hipError_t launch_rotary(const RotaryArgs& a, hipStream_t stream, int* grid, int* block, bool dry) {
  const long long blocks = (a.total + 255) / 256;
  if (blocks <= 0 || blocks >= (long long)0x7fffffff) return hipErrorInvalidValue;
  if (grid) *grid = (int)blocks;
  if (block) *block = 256;
  if (dry) return hipSuccess;
  (void)hipGetLastError();
  if (a.bf16) {
    if (a.cos_f32) launch_il<__bf16, true>(a, (unsigned)blocks, stream);
    else launch_il<__bf16, false>(a, (unsigned)blocks, stream);
  } else {
    if (a.cos_f32) launch_il<_Float16, true>(a, (unsigned)blocks, stream);
    else launch_il<_Float16, false>(a, (unsigned)blocks, stream);
  }
  return hipGetLastError();
}

}  // namespace tfa
