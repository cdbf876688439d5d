// tfa_fwd_form_inst.inc — the instantiations of the il8 / il4 kernels in one form (tfa_host_util.h: TFA_FORMS) for one (TFA_T, TFA_D, TFA_FORM | TFA_FORM_VL,
// TFA_CAUSAL): the units tfa_fwd_inst_varlen_<dtype>_<D>_c<0|1> (packed variable-length, VF_IL_VARLEN) and tfa_fwd_inst_<local|alibi|softcap>_<dtype>_<D>_<fx|vl>
// (local, fixed-length or varlen), units of their own so that the parallel build stays parallel; the Makefile turns a unit's name into these defines.  Only the
// MAIN instantiation of each variant exists in these forms (the one with the hand-scheduled statement; varlen, for bf16, with the max-free row reference): no
// windowed, idle-wave or narrow twin — head dims below the kernel's width run it with the missing columns read as zeros (KArgs::dv).  The local form
// (VF_IL_LOCAL) drops the causal pairing (and with it PREF2) and is always the CAUSAL template, so its units' names carry no c<0|1>: the right edge is the
// causal limit moved by win_right (a window without a right edge carries win_right >= Nq - 1).
// alibi: the ALiBi form of the local instantiations (VF_IL_ALIBI) — full, causal and windowed attention with slopes are this one kernel per (dtype, width,
// fixed / varlen), the window's missing sides carried as unbounded.
// softcap: the soft-capping form of the local instantiations (VF_IL_SOFTCAP), with or without slopes (a run-time choice of the one kernel), every mask.
// bias: the dense-bias form of the fixed-length local instantiations (VF_IL_BIAS; units tfa_fwd_inst_bias_<dtype>_<D>_fx): every mask, the bias loaded in the tile bodies.
// paged: the paged-K/V form of the plain varlen instantiations (VF_IL_PAGED; units tfa_fwd_inst_paged_<dtype>_<D>_c<0|1>): per-tile descriptors, so the
// compiler-scheduled tile bodies and the lazy row reference for both types.
#include "tfa_launch.h"
#if !defined(TFA_FORM_VL)
#define TFA_FORM_VL 0
#endif
#if !defined(TFA_CAUSAL)
#define TFA_CAUSAL true
#endif

namespace tfa {

template <>
hipError_t launch_fwd_form_c<TFA_T, TFA_D, (TFA_FORM) | TFA_FORM_VL, TFA_CAUSAL>(const KArgs& a, bool f32out, int variant, hipStream_t s, LaunchGeom* g, bool dry) {
  constexpr int F = (TFA_FORM) | TFA_FORM_VL;
  static_assert(form_legal(F, TFA_CAUSAL), "not a form of the il kernels (tfa_host_util.h: form_legal)");
  constexpr bool LOCAL = (F & FORM_LOCAL) != 0;
  constexpr int FORM = ((F & FORM_VARLEN) ? VF_IL_VARLEN : 0) | (LOCAL ? VF_IL_LOCAL : 0) | ((F & FORM_ALIBI) ? VF_IL_ALIBI : 0) | ((F & FORM_SOFTCAP) ? VF_IL_SOFTCAP : 0) |
                       ((F & FORM_PAGED) ? VF_IL_PAGED : 0) | ((F & FORM_BIAS) ? VF_IL_BIAS : 0);
  constexpr int PAIR = LOCAL ? 0 : VF_PAIR;   // (the local form: one query block per work item, no causal pairs — and so no PREF2)
  constexpr int VF30 = PAIR | (LOCAL ? 0 : VF_IL_PREF2) | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_QLDS | FORM;   // variant 30's main instantiation (tfa_fwd_inst.inc)
  constexpr int VF32 = PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE | FORM;                                              // variant 32's
  switch (variant) {
    case kDefaultVariant:
      return f32out ? launch_one_il<TFA_T, TFA_D, 8, VF30, TFA_CAUSAL, true>(a, s, g, dry) : launch_one_il<TFA_T, TFA_D, 8, VF30, TFA_CAUSAL, false>(a, s, g, dry);
    case kSmallGridVariant:
      return f32out ? launch_one_il<TFA_T, TFA_D, 4, VF32, TFA_CAUSAL, true>(a, s, g, dry) : launch_one_il<TFA_T, TFA_D, 4, VF32, TFA_CAUSAL, false>(a, s, g, dry);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace tfa
