// tfa_fwd_local_inst.inc — the local (sliding-window) instantiations (VF_IL_LOCAL) of the il8 / il4 kernels for one (TFA_T, TFA_D), fixed-length
// (TFA_VARLEN 0) or packed variable-length (TFA_VARLEN 1).  Included by tfa_fwd_inst_local_<dtype>_<D>_<fx|vl>.hip: units of their own, so that the
// parallel build stays parallel.  The form of the main instantiation of variants 30 and 32 without the causal pairing (and so without PREF2), full width
// only: head dims below the kernel's width run it with the missing columns read as zeros (KArgs::dv).  Always the CAUSAL template: the right edge is the
// causal limit moved by win_right (a window without a right edge carries win_right >= Nq - 1).
#include "tfa_launch.h"

namespace tfa {

template <typename T, int D, int NW, int VF, bool F32OUT>
static hipError_t launch_one_il_local(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = il_lds_bytes<D, NW, VF>();
  auto kern = fwd_kernel_il<T, D, NW, true, F32OUT, VF>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, NW * 64, lds, a, stream, geom, dry);
}

template <>
hipError_t launch_fwd_local_c<TFA_T, TFA_D, TFA_VARLEN>(const KArgs& a, bool f32out, int variant, hipStream_t s, LaunchGeom* g, bool dry) {
  constexpr int VL = VF_IL_LOCAL | (TFA_VARLEN ? VF_IL_VARLEN : 0);
  constexpr int VF30 = VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_QLDS | VL;   // variant 30's main instantiation less the pairing (tfa_fwd_inst.inc)
  constexpr int VF32 = VF_IL_EPI | VF_IL_EPI_INPLACE | VL;              // variant 32's
  switch (variant) {
    case kDefaultVariant:
      return f32out ? launch_one_il_local<TFA_T, TFA_D, 8, VF30, true>(a, s, g, dry) : launch_one_il_local<TFA_T, TFA_D, 8, VF30, false>(a, s, g, dry);
    case kSmallGridVariant:
      return f32out ? launch_one_il_local<TFA_T, TFA_D, 4, VF32, true>(a, s, g, dry) : launch_one_il_local<TFA_T, TFA_D, 4, VF32, false>(a, s, g, dry);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace tfa
