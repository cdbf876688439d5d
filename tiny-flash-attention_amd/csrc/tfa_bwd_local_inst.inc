// tfa_bwd_local_inst.inc — the local (sliding-window) instantiations (LOCAL) of the backward's two launches — dQ (tfa_bwd_kernel.h) and the fused dK/dV
// (tfa_bwd_kv_kernel.h) — for one (TFA_T, TFA_D), fixed-length (TFA_VARLEN false) or packed variable-length (true); included by
// tfa_bwd_inst_local_<dtype>_<D>_<fx|vl>.hip, units of their own.  The causal-form, full-width instantiations only (head dims below the kernel's width read the
// missing columns as zeros, BArgs::dv); no windowed form, no dS workspace.
#include <hip/hip_runtime.h>
#include "tfa_bwd_launch.h"

namespace tfa {

template <typename Kern>
static hipError_t launch_bwd_local_kernel(Kern kern, std::atomic<unsigned long long>& mask, const BArgs& a, int grid, int block, int lds, hipStream_t stream, bool dry) {
  if (dry) return hipSuccess;
  hipError_t e = set_dyn_lds_once(mask, reinterpret_cast<const void*>(kern), lds);
  if (e != hipSuccess) return e;
  (void)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, a);
  return hipGetLastError();
}

template <typename T, int D, bool F32OUT>
static hipError_t launch_bwd_dq_local_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int lds = bwd_lds_bytes<D, BWD_DQ, false>();                  // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_local_kernel(bwd_kernel<T, D, BWD_DQ, true, F32OUT, false, 8, false, D / 32, TFA_VARLEN, true>, attr_mask, a, grid, 512, lds, stream, dry);
}

template <typename T, int D, bool F32OUT>
static hipError_t launch_bwd_kv_local_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int KG = TFA_BWD_KV_KG_OF(false);
  constexpr int lds = bwd_kv_lds_bytes<D, KG>();                          // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_local_kernel(bwd_kv_kernel<T, D, true, F32OUT, false, KG, false, D / 32, TFA_VARLEN, true>, attr_mask, a, grid, KG * 128, lds, stream, dry);
}

template <>
hipError_t launch_bwd_local<TFA_T, TFA_D, TFA_VARLEN>(const BArgs& a, bool keys, int grid, bool f32out, hipStream_t s, bool dry) {
  if (keys) return f32out ? launch_bwd_kv_local_one<TFA_T, TFA_D, true>(a, grid, s, dry) : launch_bwd_kv_local_one<TFA_T, TFA_D, false>(a, grid, s, dry);
  return f32out ? launch_bwd_dq_local_one<TFA_T, TFA_D, true>(a, grid, s, dry) : launch_bwd_dq_local_one<TFA_T, TFA_D, false>(a, grid, s, dry);
}

}  // namespace tfa
