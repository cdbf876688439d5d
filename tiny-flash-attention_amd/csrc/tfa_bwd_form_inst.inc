// tfa_bwd_form_inst.inc — the packed variable-length (TFA_VARLEN) and local (sliding-window, TFA_LOCAL) instantiations of the backward's two launches — dQ
// (tfa_bwd_kernel.h) and the fused dK/dV (tfa_bwd_kv_kernel.h) — for one (TFA_T, TFA_D); included by tfa_bwd_inst_varlen_<dtype>_<D>.hip (varlen) and
// tfa_bwd_inst_local_<dtype>_<D>_<fx|vl>.hip (local, fixed-length or varlen), units of their own.  The full-width instantiations only (head dims below the
// kernel's width read the missing columns as zeros, BArgs::dv), the local ones in the causal form only; no windowed form, no dS workspace.
// TFA_ALIBI (tfa_bwd_inst_alibi_<dtype>_<D>_<fx|vl>.hip): the ALiBi form of the local instantiations (full, causal and windowed attention with slopes).
// TFA_SOFTCAP (tfa_bwd_inst_softcap_<dtype>_<D>_<fx|vl>.hip): the soft-capping form of the local instantiations (every mask, with or without slopes).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "tfa_bwd_launch.h"
#if !defined(TFA_ALIBI)
#define TFA_ALIBI false
#endif
#if !defined(TFA_SOFTCAP)
#define TFA_SOFTCAP false
#endif

namespace tfa {

template <typename T, int D, bool CAUSAL, bool F32OUT>
static hipError_t launch_bwd_dq_form_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int lds = bwd_lds_bytes<D, BWD_DQ, false>();                  // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(bwd_kernel<T, D, BWD_DQ, CAUSAL, F32OUT, false, 8, false, D / 32, TFA_VARLEN, TFA_LOCAL, TFA_ALIBI, TFA_SOFTCAP>, attr_mask, grid, 512, lds, a, stream, dry);
}

template <typename T, int D, bool CAUSAL, bool F32OUT>
static hipError_t launch_bwd_kv_form_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int KG = TFA_BWD_KV_KG_OF(false);
  constexpr int lds = bwd_kv_lds_bytes<D, KG>();                          // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(bwd_kv_kernel<T, D, CAUSAL, F32OUT, false, KG, false, D / 32, TFA_VARLEN, TFA_LOCAL, TFA_ALIBI, TFA_SOFTCAP>, attr_mask, grid, KG * 128, lds, a, stream, dry);
}

// calls one(CAUSAL, F32OUT) as std::bool_constant pairs: the local kernels exist as the causal template only
template <typename F>
static hipError_t by_causal_f32out(bool causal, bool f32out, F one) {
  using Y = std::true_type;
  using N = std::false_type;
  if (TFA_LOCAL || causal) return f32out ? one(Y{}, Y{}) : one(Y{}, N{});
  if constexpr (TFA_LOCAL) return hipErrorInvalidValue;   // (never: a window implies the causal template)
  else return f32out ? one(N{}, Y{}) : one(N{}, N{});
}

template <>
hipError_t launch_bwd_form<TFA_T, TFA_D, TFA_VARLEN, TFA_LOCAL, TFA_ALIBI, TFA_SOFTCAP>(const BArgs& a, bool keys, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (keys)
    return by_causal_f32out(causal, f32out, [&](auto c, auto f) { return launch_bwd_kv_form_one<TFA_T, TFA_D, decltype(c)::value, decltype(f)::value>(a, grid, s, dry); });
  return by_causal_f32out(causal, f32out, [&](auto c, auto f) { return launch_bwd_dq_form_one<TFA_T, TFA_D, decltype(c)::value, decltype(f)::value>(a, grid, s, dry); });
}

}  // namespace tfa
