// tfa_bwd_form_inst.inc — the instantiations of the backward's two launches — dQ (tfa_bwd_kernel.h) and the fused dK/dV (tfa_bwd_kv_kernel.h) — in one form
// (tfa_host_util.h: TFA_FORMS) for one (TFA_T, TFA_D, TFA_FORM | TFA_FORM_VL): the units tfa_bwd_inst_varlen_<dtype>_<D> (packed variable-length) and
// tfa_bwd_inst_<local|alibi|softcap>_<dtype>_<D>_<fx|vl> (local, fixed-length or varlen), units of their own; the Makefile turns a unit's name into these defines.
// The full-width instantiations only (head dims below the kernel's width read the missing columns as zeros, BArgs::dv), the local ones in the causal form
// only; no windowed form, no dS workspace.  alibi / softcap: the ALiBi and the soft-capping (with or without slopes) form of the local instantiations, every mask.
// bias: the dense-bias form of the fixed-length local instantiations (tfa_bwd_bias; units tfa_bwd_inst_bias_<dtype>_<D>_fx).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "tfa_bwd_launch.h"
#if !defined(TFA_FORM_VL)
#define TFA_FORM_VL 0
#endif

namespace tfa {

constexpr int kForm = (TFA_FORM) | TFA_FORM_VL;   // ... and as the kernels' four template booleans
static_assert(form_legal(kForm), "not a form of the backward kernels (tfa_host_util.h: form_legal)");
constexpr bool kVarlen = (kForm & FORM_VARLEN) != 0, kLocal = (kForm & FORM_LOCAL) != 0, kAlibi = (kForm & FORM_ALIBI) != 0, kSoftcap = (kForm & FORM_SOFTCAP) != 0;
constexpr bool kBias = (kForm & FORM_BIAS) != 0;

template <typename T, int D, bool CAUSAL, bool F32OUT>
static hipError_t launch_bwd_dq_form_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int lds = bwd_lds_bytes<D, BWD_DQ, false>();                  // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(bwd_kernel<T, D, BWD_DQ, CAUSAL, F32OUT, false, 8, false, D / 32, kVarlen, kLocal, kAlibi, kSoftcap, kBias>, attr_mask, grid, 512, lds, a, stream, dry);
}

template <typename T, int D, bool CAUSAL, bool F32OUT>
static hipError_t launch_bwd_kv_form_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int KG = TFA_BWD_KV_KG_OF(false);
  constexpr int lds = bwd_kv_lds_bytes<D, KG>();                          // (the twin's layout: tfa_bwd_launch.h)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(bwd_kv_kernel<T, D, CAUSAL, F32OUT, false, KG, false, D / 32, kVarlen, kLocal, kAlibi, kSoftcap, kBias>, attr_mask, grid, KG * 128, lds, a, stream, dry);
}

// calls one(CAUSAL, F32OUT) as std::bool_constant pairs: the local kernels exist as the causal template only
template <typename F>
static hipError_t by_causal_f32out(bool causal, bool f32out, F one) {
  using Y = std::true_type;
  using N = std::false_type;
  if (kLocal || causal) return f32out ? one(Y{}, Y{}) : one(Y{}, N{});
  if constexpr (kLocal) return hipErrorInvalidValue;   // (never: a window implies the causal template)
  else return f32out ? one(N{}, Y{}) : one(N{}, N{});
}

template <>
hipError_t launch_bwd_form<TFA_T, TFA_D, kForm>(const BArgs& a, bool keys, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (keys)
    return by_causal_f32out(causal, f32out, [&](auto c, auto f) { return launch_bwd_kv_form_one<TFA_T, TFA_D, decltype(c)::value, decltype(f)::value>(a, grid, s, dry); });
  return by_causal_f32out(causal, f32out, [&](auto c, auto f) { return launch_bwd_dq_form_one<TFA_T, TFA_D, decltype(c)::value, decltype(f)::value>(a, grid, s, dry); });
}

}  // namespace tfa
