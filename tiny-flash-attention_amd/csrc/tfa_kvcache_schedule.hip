// tfa_kvcache_schedule.hip — the work list of the scheduled packed-q KV-cache call (include/tfa.h: tfa_kvcache_varlen_schedule; FlashAttention-3's
// get_scheduler_metadata).  One launch of ONE workgroup on the caller's stream: nothing is read on the host, nothing is allocated.  It reads cu_seqlens_q
// (B + 1 entries), clamps every sequence's (q0_b, nq_b) exactly as the attention kernel does (tfa_fwd_kernel_dma_body.inc: decode(), the VQ branch), counts the
// sequence's own work items — nb_b = ceil(nq_b * G' / 128) blocks: nb_b items, or ceil(nb_b / 2) heavy / light pairs under causal — and writes
//   metadata[0 .. SCHED_HDR):   n_items, B, G', causal, max_seqlen_q, total_q, bound, 0
//   metadata[SCHED_HDR + 2 i ..): (b, wi) of item i, ascending b, then ascending wi; sequences without rows contribute nothing
// The offsets are a block-wide exclusive scan of the item counts through LDS, 256 sequences a stride, with a carry across strides: any B.  Rows at or beyond
// `bound` (the rows the buffer holds) are not written and n_items is clamped to it: a monotonic cu_seqlens_q never gets there (the bound is proven for it in tfa.h),
// a broken one loses items, it never writes outside the buffer.  Plain C++ stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfa_kvcache.h"

namespace tfa {

__global__ __launch_bounds__(256) void kvcache_schedule_kernel(const ScheduleArgs a) {
  __shared__ long long scan[256];
  const int tid = threadIdx.x;
  long long carry = 0;                                         // items of the strides before this one (the same value in every thread)
  for (int base = 0; base < a.B; base += 256) {
    const int b = base + tid;
    long long cnt = 0;
    if (b < a.B) {
      const int c0 = a.cu[b], c1 = a.cu[b + 1];
      const int q0 = c0 < 0 ? 0 : (c0 > a.total_q ? a.total_q : c0);
      const int room = a.total_q - q0 < a.max_q ? a.total_q - q0 : a.max_q;
      const long long d = (long long)c1 - c0;
      const int nq = d < 0 ? 0 : (d > room ? room : (int)d);
      const int nb = (nq * a.gp + 127) / 128;                  // (max_q * G' < 2^30: the host's check)
      cnt = a.causal ? (nb + 1) >> 1 : nb;
    }
    scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                  // inclusive scan, log2(256) steps
      const long long v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const long long first = carry + scan[tid] - cnt;           // exclusive prefix: this sequence's first row of the list
    const long long stride_total = scan[255];
    __syncthreads();                                           // everyone has read the scan before the next stride overwrites it
    for (long long i = 0; i < cnt && first + i < a.bound; ++i) {
      int2 row;
      row.x = b;
      row.y = (int)i;
      reinterpret_cast<int2*>(a.meta + SCHEDULE_HDR)[first + i] = row;
    }
    carry += stride_total;
  }
  if (tid == 0) {
    a.meta[0] = (int)(carry < a.bound ? carry : a.bound);
    a.meta[1] = a.B;
    a.meta[2] = a.gp;
    a.meta[3] = a.causal;
    a.meta[4] = a.max_q;
    a.meta[5] = a.total_q;
    a.meta[6] = a.bound;
    a.meta[7] = 0;
  }
}

hipError_t launch_kvcache_schedule(const ScheduleArgs& a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(kvcache_schedule_kernel, dim3(1), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace tfa
