// tfa_fwd_form_inst.inc — the packed variable-length (VF_IL_VARLEN) and local (sliding-window, VF_IL_LOCAL) instantiations of the il8 / il4 kernels for one
// (TFA_T, TFA_D, TFA_VARLEN, TFA_LOCAL, TFA_CAUSAL).  Included by tfa_fwd_inst_varlen_<dtype>_<D>_c<0|1>.hip (varlen) and tfa_fwd_inst_local_<dtype>_<D>_<fx|vl>.hip
// (local, fixed-length or varlen): units of their own, so that the parallel build stays parallel.  Only the MAIN instantiation of each variant exists in these
// forms (the one with the hand-scheduled statement; varlen, for bf16, with the max-free row reference): no windowed, idle-wave or narrow twin — head dims below
// the kernel's width run it with the missing columns read as zeros (KArgs::dv).  The local form drops the causal pairing (and with it PREF2) and is always the
// CAUSAL template: the right edge is the causal limit moved by win_right (a window without a right edge carries win_right >= Nq - 1).
// TFA_ALIBI (tfa_fwd_inst_alibi_<dtype>_<D>_<fx|vl>.hip): the ALiBi form of the local instantiations (VF_IL_ALIBI) — full, causal and windowed attention with
// slopes are this one kernel per (dtype, width, fixed / varlen), the window's missing sides carried as unbounded.
// TFA_SOFTCAP (tfa_fwd_inst_softcap_<dtype>_<D>_<fx|vl>.hip): the soft-capping form of the local instantiations (VF_IL_SOFTCAP), with or without slopes (a run-time
// choice of the one kernel: TFA_ALIBI stays false), every mask.
#include "tfa_launch.h"
#if !defined(TFA_ALIBI)
#define TFA_ALIBI false
#endif
#if !defined(TFA_SOFTCAP)
#define TFA_SOFTCAP false
#endif

namespace tfa {

template <>
hipError_t launch_fwd_form_c<TFA_T, TFA_D, TFA_VARLEN, TFA_LOCAL, TFA_CAUSAL, TFA_ALIBI, TFA_SOFTCAP>(const KArgs& a, bool f32out, int variant, hipStream_t s, LaunchGeom* g, bool dry) {
  static_assert(TFA_CAUSAL || !TFA_LOCAL, "the local kernels are the causal template");
  static_assert(TFA_LOCAL || !TFA_ALIBI, "the ALiBi kernels are a form of the local ones");
  static_assert(!TFA_SOFTCAP || (TFA_LOCAL && !TFA_ALIBI), "the softcap kernels are a form of the local ones; their slopes are a run-time choice");
  constexpr int FORM = (TFA_VARLEN ? VF_IL_VARLEN : 0) | (TFA_LOCAL ? VF_IL_LOCAL : 0) | (TFA_ALIBI ? VF_IL_ALIBI : 0) | (TFA_SOFTCAP ? VF_IL_SOFTCAP : 0);
  constexpr int PAIR = TFA_LOCAL ? 0 : VF_PAIR;   // (the local form: one query block per work item, no causal pairs — and so no PREF2)
  constexpr int VF30 = PAIR | (TFA_LOCAL ? 0 : VF_IL_PREF2) | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_QLDS | FORM;   // variant 30's main instantiation (tfa_fwd_inst.inc)
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
