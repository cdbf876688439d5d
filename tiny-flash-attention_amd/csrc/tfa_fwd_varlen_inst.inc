// tfa_fwd_varlen_inst.inc — the packed variable-length instantiations (VF_IL_VARLEN) of the il8 / il4 kernels for one (TFA_T, TFA_D, TFA_CAUSAL).
// Included by tfa_fwd_inst_varlen_<dtype>_<D>_c<0|1>.hip: units of their own, so that the parallel build stays parallel.  Only the MAIN instantiation of
// each variant exists in varlen form (the one with the hand-scheduled statement and, for bf16, the max-free row reference): no windowed, idle-wave or
// narrow twin — head dims below the kernel's width run it with the missing columns read as zeros (KArgs::dv).
#include "tfa_launch.h"

namespace tfa {

template <typename T, int D, int NW, int VF, bool CAUSAL, bool F32OUT>
static hipError_t launch_one_il_varlen(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = il_lds_bytes<D, NW, VF>();   // (the twin's layout: tfa_launch.h)
  auto kern = fwd_kernel_il<T, D, NW, CAUSAL, F32OUT, VF | VF_IL_VARLEN>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, NW * 64, lds, a, stream, geom, dry);
}

template <>
hipError_t launch_fwd_varlen_c<TFA_T, TFA_D, TFA_CAUSAL>(const KArgs& a, bool f32out, int variant, hipStream_t s, LaunchGeom* g, bool dry) {
  constexpr int VF30 = VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_PREF2 | VF_IL_QLDS;   // variant 30's main instantiation (tfa_fwd_inst.inc)
  constexpr int VF32 = VF_PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE;                           // variant 32's
  switch (variant) {
    case kDefaultVariant:
      return f32out ? launch_one_il_varlen<TFA_T, TFA_D, 8, VF30, TFA_CAUSAL, true>(a, s, g, dry) : launch_one_il_varlen<TFA_T, TFA_D, 8, VF30, TFA_CAUSAL, false>(a, s, g, dry);
    case kSmallGridVariant:
      return f32out ? launch_one_il_varlen<TFA_T, TFA_D, 4, VF32, TFA_CAUSAL, true>(a, s, g, dry) : launch_one_il_varlen<TFA_T, TFA_D, 4, VF32, TFA_CAUSAL, false>(a, s, g, dry);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace tfa
